# -*- coding: utf-8 -*-
"""BSS-eval SDR / SIR / SAR on MI355X -- host mirror of the reference's utils/bss_eval.py GPU entry point
(`bss_eval_sources_cupy`, utils/bss_eval.py:586-637, called by experiments/evaluation/eval.py:48-73).

The arithmetic runs in libams_bss.so (include/ams_bss.h: hipFFT + hipSOLVER + hand-written assembly / reduction kernels,
float64).  There is no CPU fallback: without the library or a GPU the functions raise.  Only the permutation choice over the
nsrc x nsrc criteria (a 2..6-element loop, :613-620) is host arithmetic, as in the reference.
"""
import ctypes
import itertools
import os

import numpy as np
import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.normpath(os.path.join(_HERE, '..', 'ams_hip', 'libams_bss.so'))
FLEN = 512                      # utils/bss_eval.py:608

_lib = None
_ctx = {}                       # (nsrc, nsampl, flen, device) -> (ctx pointer, workspace tensor)


class BssError(RuntimeError):
    pass


def _load():
    """libams_bss.so with both of its interfaces declared: ams_bss_* (include/ams_bss.h) and ams_bssb_* (include/ams_bss_batch.h)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise BssError('libams_bss.so not found at %s -- run __graft_entry__.build() (no CPU fallback)' % LIB_PATH)
        lib = ctypes.CDLL(LIB_PATH)
        lib.ams_bss_abi_version.restype = ctypes.c_int
        lib.ams_bss_create.restype = ctypes.c_int
        lib.ams_bss_create.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_int, ctypes.c_int, ctypes.c_int]
        lib.ams_bss_destroy.restype = None
        lib.ams_bss_destroy.argtypes = [ctypes.c_void_p]
        lib.ams_bss_workspace_bytes.restype = ctypes.c_size_t
        lib.ams_bss_workspace_bytes.argtypes = [ctypes.c_void_p]
        lib.ams_bss_eval_pairs.restype = ctypes.c_int
        lib.ams_bss_eval_pairs.argtypes = [ctypes.c_void_p] * 5 + [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]
        lib.ams_bssb_abi_version.restype = ctypes.c_int
        lib.ams_bssb_create.restype = ctypes.c_int
        lib.ams_bssb_create.argtypes = [ctypes.POINTER(ctypes.c_void_p)] + [ctypes.c_int] * 5
        lib.ams_bssb_destroy.restype = None
        lib.ams_bssb_destroy.argtypes = [ctypes.c_void_p]
        lib.ams_bssb_workspace_bytes.restype = ctypes.c_size_t
        lib.ams_bssb_workspace_bytes.argtypes = [ctypes.c_void_p]
        lib.ams_bssb_eval.restype = ctypes.c_int
        lib.ams_bssb_eval.argtypes = [ctypes.c_void_p, ctypes.c_int] + [ctypes.c_void_p] * 5 + [ctypes.c_size_t, ctypes.c_void_p]
        lib.ams_bssb_potrf.restype = ctypes.c_int
        lib.ams_bssb_potrf.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_long, ctypes.c_int, ctypes.c_void_p,
                                       ctypes.c_void_p]
        if lib.ams_bss_abi_version() != 1:
            raise BssError('libams_bss.so ABI version mismatch')
        if lib.ams_bssb_abi_version() != 1:
            raise BssError('libams_bss.so batch ABI version mismatch')
        _lib = lib
    return _lib


def _load_batch():
    """The same library, under the name the batched path, tools/bss_bench.py and the tests use."""
    return _load()


def _context(nsrc, nsampl, flen, device):
    key = (nsrc, nsampl, flen, str(device))
    if key not in _ctx:
        lib = _load()
        p = ctypes.c_void_p()
        st = lib.ams_bss_create(ctypes.byref(p), nsrc, nsampl, flen)
        if st != 0:
            raise BssError('ams_bss_create failed: %d' % st)
        nb = lib.ams_bss_workspace_bytes(p)
        ws = torch.empty((nb + 7) // 8, dtype=torch.float64, device=device)
        _ctx[key] = (p, ws, nb)
    return _ctx[key]


def bss_eval_pairs(reference_sources, estimated_sources, flen=FLEN):
    """[nsrc, nsampl] x2 (array-like or tensors) -> (sdr, sir, sar) numpy float64 [nsrc(jest), nsrc(jtrue)] pair matrices."""
    if not torch.cuda.is_available():
        raise BssError('bss_eval needs a GPU (there is no CPU fallback)')
    dev = reference_sources.device if torch.is_tensor(reference_sources) and reference_sources.is_cuda else torch.device('cuda')
    ref = torch.as_tensor(reference_sources).to(device=dev, dtype=torch.float64)
    est = torch.as_tensor(estimated_sources).to(device=dev, dtype=torch.float64)
    nsampl = est.shape[-1]
    ref = ref.reshape(-1, nsampl).contiguous()
    est = est.reshape(-1, nsampl).contiguous()
    nsrc = est.shape[0]
    if ref.shape != est.shape:
        raise BssError('reference and estimated sources must have the same shape, got %s and %s' % (tuple(ref.shape), tuple(est.shape)))
    p, ws, nb = _context(nsrc, nsampl, flen, dev)
    crit = torch.empty((3, nsrc, nsrc), dtype=torch.float64, device=dev)
    info = torch.zeros(1, dtype=torch.int32, device=dev)
    st = _load().ams_bss_eval_pairs(p, ref.data_ptr(), est.data_ptr(), crit.data_ptr(), info.data_ptr(), ws.data_ptr(), nb,
                                    torch.cuda.current_stream().cuda_stream)
    if st != 0:
        raise BssError('ams_bss_eval_pairs failed: %d' % st)
    c = crit.cpu().numpy()
    return c[0], c[1], c[2]


def bss_eval_sources_cupy(reference_sources, estimated_sources, compute_permutation=True, nsrc=2):
    """Same contract as the reference function of this name (utils/bss_eval.py:586-637): returns
    (sdr, sir, sar, perm) with estimated source perm[j] matched to true source j by best mean SIR."""
    sdr, sir, sar = bss_eval_pairs(np.asarray(reference_sources).reshape(nsrc, -1) if not torch.is_tensor(reference_sources)
                                   else reference_sources.reshape(nsrc, -1),
                                   np.asarray(estimated_sources).reshape(nsrc, -1) if not torch.is_tensor(estimated_sources)
                                   else estimated_sources.reshape(nsrc, -1))
    return _select_permutation(sdr, sir, sar, compute_permutation)


# the reference exposes the same metric under two names (numpy and cupy back ends); both map to the HIP path here
bss_eval_sources = bss_eval_sources_cupy


# ---------------------------------------------------------------------------------------------------------------------------
# Batched path (include/ams_bss_batch.h): U utterances x K sets of estimates in one library call.  The Gram matrices of an
# utterance are assembled and factorised once (the library's own batched MFMA-f64 Cholesky) and shared by its K sets.
MAX_UTT = 64                    # utterances per library call; larger batches are processed in slices of this size

_bctx = {}                      # (max_utt, nsets, nsrc, nsampl, flen, device) -> (ctx pointer, workspace tensor, bytes)


def _batch_context(max_utt, nsets, nsrc, nsampl, flen, device):
    key = (max_utt, nsets, nsrc, nsampl, flen, str(device))
    if key not in _bctx:
        lib = _load_batch()
        p = ctypes.c_void_p()
        st = lib.ams_bssb_create(ctypes.byref(p), max_utt, nsets, nsrc, nsampl, flen)
        if st != 0:
            raise BssError('ams_bssb_create failed: %d' % st)
        nb = lib.ams_bssb_workspace_bytes(p)
        ws = torch.empty((nb + 7) // 8, dtype=torch.float64, device=device)
        _bctx[key] = (p, ws, nb)
    return _bctx[key]


def _shape_of(x):
    return tuple(x.shape) if hasattr(x, 'shape') else tuple(np.shape(x))


def bss_eval_pairs_batch(reference_sources, estimated_sources, flen=FLEN, max_utt=MAX_UTT):
    """refs [U, S, L], ests [U, S, L] or [U, K, S, L] (array-like or tensors; device tensors are read in place)
    -> (crit, info): numpy float64 [U, K, 3, S, S] with crit[u, k] = the (sdr, sir, sar) pair matrices [jest, jtrue] of
    bss_eval_pairs(refs[u], ests[u, k]), and int32 [U], non-zero where a Gram matrix of the utterance was not positive
    definite (a silent reference; that utterance's criteria are NaN, the others are unaffected)."""
    rs, es = _shape_of(reference_sources), _shape_of(estimated_sources)
    if len(rs) != 3 or len(es) not in (3, 4):
        raise BssError('expected references [U, S, L] and estimates [U, S, L] or [U, K, S, L], got %s and %s' % (rs, es))
    if len(es) == 3:
        es = (es[0], 1) + es[1:]
    U, K, S, L = es
    if (U, S, L) != rs or min(U, K, S, L) < 1:
        raise BssError('references %s and estimates %s do not match' % (rs, _shape_of(estimated_sources)))
    if max_utt < 1 or flen < 1:
        raise BssError('max_utt and flen must be positive')
    if not torch.cuda.is_available():
        raise BssError('bss_eval needs a GPU (there is no CPU fallback)')
    dev = reference_sources.device if torch.is_tensor(reference_sources) and reference_sources.is_cuda else torch.device('cuda')
    ref = torch.as_tensor(reference_sources).to(device=dev, dtype=torch.float64).contiguous()
    est = torch.as_tensor(estimated_sources).to(device=dev, dtype=torch.float64).reshape(U, K, S, L).contiguous()
    mu = min(max_utt, U)
    p, ws, nb = _batch_context(mu, K, S, L, flen, dev)
    crit = torch.empty((U, K, 3, S, S), dtype=torch.float64, device=dev)
    info = torch.zeros(U, dtype=torch.int32, device=dev)
    lib = _load_batch()
    stream = torch.cuda.current_stream().cuda_stream
    for u0 in range(0, U, mu):
        nu = min(mu, U - u0)
        st = lib.ams_bssb_eval(p, nu, ref[u0:].data_ptr(), est[u0:].data_ptr(), crit[u0:].data_ptr(), info[u0:].data_ptr(),
                               ws.data_ptr(), nb, stream)
        if st != 0:
            raise BssError('ams_bssb_eval failed: %d' % st)
    return crit.cpu().numpy(), info.cpu().numpy()


def _select_permutation(sdr, sir, sar, compute_permutation=True):
    """[S, S] pair matrices -> (sdr, sir, sar [S], perm [S]); the rule of the reference's bss_eval_sources_cupy (:613-620): best
    mean SIR, the first maximum wins."""
    nsrc = sir.shape[0]
    dum = np.arange(nsrc)
    if not compute_permutation:
        return sdr[dum, dum], sir[dum, dum], sar[dum, dum], dum
    perms = list(itertools.permutations(list(range(nsrc))))
    mean_sir = np.empty(len(perms))
    for i, perm in enumerate(perms):
        mean_sir[i] = np.mean(sir[list(perm), dum])
    popt = perms[int(np.argmax(mean_sir))]
    idx = (list(popt), dum)
    return sdr[idx], sir[idx], sar[idx], np.asarray(popt)


def _select_all(crit, compute_permutation):
    """crit [U, K, 3, S, S] -> (sdr, sir, sar [U, K, S] float64, perm [U, K, S] int): _select_permutation per (unit, set)."""
    U, K, _, S, _ = crit.shape
    sdr, sir, sar = (np.empty((U, K, S)) for _ in range(3))
    perm = np.empty((U, K, S), dtype=np.int64)
    for u in range(U):
        for k in range(K):
            sdr[u, k], sir[u, k], sar[u, k], perm[u, k] = _select_permutation(crit[u, k, 0], crit[u, k, 1], crit[u, k, 2],
                                                                              compute_permutation)
    return sdr, sir, sar, perm


def bss_eval_sources_batch(reference_sources, estimated_sources, compute_permutation=True, flen=FLEN, max_utt=MAX_UTT):
    """refs [U, S, L], ests [U, S, L] or [U, K, S, L] -> (sdr, sir, sar [U, K, S] float64, perm [U, K, S] int): per utterance and
    set what bss_eval_sources_cupy returns, from ONE library call per slice of max_utt utterances."""
    crit, _ = bss_eval_pairs_batch(reference_sources, estimated_sources, flen=flen, max_utt=max_utt)
    return _select_all(crit, compute_permutation)


def potrf_batch(a):
    """[M, n, n] symmetric positive definite (tensor or array-like) -> (factors [M, n, n] numpy, info [M]) through
    ams_bssb_potrf -- the batched Cholesky of the batched path on its own (tests, tools/bss_bench.py).  The lower triangle of
    factors[m] is the Cholesky factor; the strict upper triangle is the input's, untouched."""
    if not torch.cuda.is_available():
        raise BssError('bss_eval needs a GPU (there is no CPU fallback)')
    if len(_shape_of(a)) != 3 or _shape_of(a)[1] != _shape_of(a)[2]:
        raise BssError('expected [M, n, n], got %s' % (_shape_of(a),))
    # a symmetric matrix reads the same row-major and column-major; the factor comes back transposed
    t = torch.as_tensor(a).to(device='cuda', dtype=torch.float64).contiguous().clone()
    M, n, _ = t.shape
    info = torch.empty(M, dtype=torch.int32, device=t.device)
    st = _load_batch().ams_bssb_potrf(t.data_ptr(), n, n, n * n, M, info.data_ptr(), torch.cuda.current_stream().cuda_stream)
    if st != 0:
        raise BssError('ams_bssb_potrf failed: %d' % st)
    return t.transpose(1, 2).cpu().numpy(), info.cpu().numpy()


# ---------------------------------------------------------------------------------------------------------------------------
# Ragged path (include/ams_bss_ragged.h, libams_bss_ragged.so): R recordings of ANY lengths x K sets of estimates in one library
# call -- no context, no FFT plan, a launch count that depends on (S, K, flen) only.  The correlations and projections run in the
# time domain (float64 MFMA); the Gram matrices go through the batched Cholesky of the batched path.
RAGGED_LIB_PATH = os.path.normpath(os.path.join(_HERE, '..', 'ams_hip', 'libams_bss_ragged.so'))
RAGGED_ABI_VERSION = 1
RAGGED_CAP_BYTES = 4 << 30      # workspace of one library call; larger sets are scored in groups of consecutive recordings
RAGGED_MAX_FLEN = 1024          # include/ams_bss_ragged.h: AMS_BSSR_MAX_FLEN
RAGGED_MAX_SETS = 64
RAGGED_MAX_REC = 65535          # recordings per library call

_rlib = None
_rlayouts = {}                  # (lengths, flen) -> _RaggedLayout, the last few layouts (tables uploaded once per layout and device)


def _load_ragged():
    global _rlib
    if _rlib is None:
        if not os.path.exists(RAGGED_LIB_PATH):
            raise BssError('libams_bss_ragged.so not found at %s -- run __graft_entry__.build() (no CPU fallback)' % RAGGED_LIB_PATH)
        lib = ctypes.CDLL(RAGGED_LIB_PATH)
        vp, ci, cl = ctypes.c_void_p, ctypes.c_int, ctypes.c_long
        lib.ams_bssr_abi_version.restype = ci
        lib.ams_bssr_block.restype = ci
        lib.ams_bssr_blocks.restype = cl
        lib.ams_bssr_blocks.argtypes = [vp, ci, ci]
        lib.ams_bssr_tables.restype = ci
        lib.ams_bssr_tables.argtypes = [vp, ci, ci, vp, vp]
        lib.ams_bssr_launches.restype = ci
        lib.ams_bssr_launches.argtypes = [ci, ci, ci]
        lib.ams_bssr_workspace_bytes.restype = ctypes.c_size_t
        lib.ams_bssr_workspace_bytes.argtypes = [ci, ci, ci, ci, cl]
        lib.ams_bssr_eval.restype = ci
        lib.ams_bssr_eval.argtypes = [vp] * 5 + [ci] * 4 + [cl, vp, vp, vp, ctypes.c_size_t, vp]
        if lib.ams_bssr_abi_version() != RAGGED_ABI_VERSION:
            raise BssError('libams_bss_ragged.so ABI version mismatch: the library is %d, this binding is %d'
                           % (lib.ams_bssr_abi_version(), RAGGED_ABI_VERSION))
        _rlib = lib
    return _rlib


def ragged_block():
    """AMS_BSSR_BLOCK: the samples per block of the ragged path's summation order."""
    return int(_load_ragged().ams_bssr_block())


class _RaggedLayout(object):
    """Where R recordings lie (host, numpy; the names are the header's): L [R]; l_off, b_off [R + 1] int64; tab [Btot, 2] int32.
    tables(device) uploads them as ONE buffer, once per device."""

    def __init__(self, lengths, flen):
        lib = _load_ragged()
        self.L = np.asarray(lengths, np.int64).reshape(-1)
        self.R, self.flen = int(self.L.size), int(flen)
        self.l_off = np.concatenate([[0], np.cumsum(self.L)]).astype(np.int64)
        vp = ctypes.c_void_p
        bt = lib.ams_bssr_blocks(self.l_off.ctypes.data_as(vp), self.R, self.flen)
        if bt < 1:
            raise BssError('ragged bss_eval: %d recordings of %d samples in all with flen %d are outside what one call takes'
                           % (self.R, int(self.l_off[-1]), self.flen))
        self.Btot = int(bt)
        self.b_off = np.zeros(self.R + 1, np.int64)
        self.tab = np.zeros((self.Btot, 2), np.int32)
        st = lib.ams_bssr_tables(self.l_off.ctypes.data_as(vp), self.R, self.flen, self.b_off.ctypes.data_as(vp), self.tab.ctypes.data_as(vp))
        if st != 0:
            raise BssError('ams_bssr_tables failed: %d' % st)
        self._dev = {}

    def tables(self, device):
        key = str(torch.device(device))
        if key not in self._dev:
            n = self.R + 1
            host = np.zeros(2 * n + self.Btot, np.int64)
            host[:n], host[n:2 * n] = self.l_off, self.b_off
            host[2 * n:].view(np.int32)[:] = self.tab.reshape(-1)
            buf = torch.from_numpy(host).to(device)
            self._dev[key] = (buf[:n], buf[n:2 * n], buf[2 * n:].view(torch.int32))
        return self._dev[key]


def _ragged_layout(lengths, flen):
    key = (tuple(int(v) for v in lengths), int(flen))
    lay = _rlayouts.pop(key, None)
    if lay is None:
        lay = _RaggedLayout(key[0], flen)
        while len(_rlayouts) >= 8:
            _rlayouts.pop(next(iter(_rlayouts)))
    _rlayouts[key] = lay                      # (most recently used last)
    return lay


def bss_eval_pairs_ragged_packed(ref, est, lengths, nsets, nsrc, flen=FLEN, ws=None):
    """ONE library call on packed float64 device tensors (the layout of include/ams_bss_ragged.h): ref holds recording r's [S, L_r]
    at S l_off[r], est its [K, S, L_r] at K S l_off[r].  -> (crit [R, K, 3, S, S], info [R]) device tensors, nothing synchronised.
    ws: a workspace tensor to use instead of a fresh one (its byte size is passed on as it is)."""
    lay = _ragged_layout(lengths, flen)
    total = int(lay.l_off[-1])
    if not (torch.is_tensor(ref) and torch.is_tensor(est) and ref.is_cuda and est.is_cuda and ref.dtype == est.dtype == torch.float64
            and ref.is_contiguous() and est.is_contiguous() and ref.numel() == nsrc * total and est.numel() == nsets * nsrc * total):
        raise BssError('ragged bss_eval: packed float64 device tensors of %d and %d elements expected' % (nsrc * total, nsets * nsrc * total))
    lib, dev = _load_ragged(), ref.device
    nb = lib.ams_bssr_workspace_bytes(lay.R, nsets, nsrc, flen, lay.Btot)
    if nb == 0:
        raise BssError('ragged bss_eval: (R, K, S, flen) = (%d, %d, %d, %d) is outside the library\'s domain' % (lay.R, nsets, nsrc, flen))
    if ws is None:
        ws = torch.empty((nb + 7) // 8, dtype=torch.float64, device=dev)
    l_off, b_off, tab = lay.tables(dev)
    crit = torch.empty((lay.R, nsets, 3, nsrc, nsrc), dtype=torch.float64, device=dev)
    info = torch.zeros(lay.R, dtype=torch.int32, device=dev)
    st = lib.ams_bssr_eval(ref.data_ptr(), est.data_ptr(), l_off.data_ptr(), b_off.data_ptr(), tab.data_ptr(), lay.R, nsets, nsrc, flen,
                           lay.Btot, crit.data_ptr(), info.data_ptr(), ws.data_ptr(), ws.numel() * ws.element_size(),
                           torch.cuda.current_stream().cuda_stream)
    if st != 0:
        raise BssError('ams_bssr_eval failed: %d' % st)
    return crit, info


def _ragged_shapes(refs, ests, flen):
    """The refusals of the ragged path, made before the library or the device is touched -> (R, K, S, lengths)."""
    if not isinstance(refs, (list, tuple)) or not isinstance(ests, (list, tuple)):
        raise BssError('ragged bss_eval: references and estimates are lists, one entry per recording')
    if len(refs) < 1 or len(ests) < 1:
        raise BssError('ragged bss_eval: empty list of recordings')
    if len(refs) != len(ests):
        raise BssError('ragged bss_eval: %d references and %d estimates' % (len(refs), len(ests)))
    if int(flen) < 1 or int(flen) > RAGGED_MAX_FLEN:
        raise BssError('ragged bss_eval: flen must be in 1 .. %d, got %d' % (RAGGED_MAX_FLEN, flen))
    S = K = None
    lengths = []
    for r, (a, b) in enumerate(zip(refs, ests)):
        rs, es = _shape_of(a), _shape_of(b)
        if len(rs) != 2 or len(es) not in (2, 3):
            raise BssError('ragged bss_eval: recording %d: expected a reference [S, L] and estimates [S, L] or [K, S, L], got %s and %s'
                           % (r, rs, es))
        if len(es) == 2:
            es = (1,) + es
        if min(rs) < 1 or min(es) < 1:
            raise BssError('ragged bss_eval: recording %d is empty: %s and %s' % (r, rs, es))
        if S is None:
            S, K = rs[0], es[0]
        if rs[0] != S or es[1] != S:
            raise BssError('ragged bss_eval: recording %d has %d references and %d estimates per set, the first recording has %d'
                           % (r, rs[0], es[1], S))
        if es[0] != K:
            raise BssError('ragged bss_eval: recording %d has %d sets of estimates, the first recording has %d' % (r, es[0], K))
        if es[2] != rs[1]:
            raise BssError('ragged bss_eval: recording %d: the reference has %d samples, its estimates %d' % (r, rs[1], es[2]))
        lengths.append(int(rs[1]))
    if S > 6:
        raise BssError('ragged bss_eval: at most 6 sources, got %d' % S)
    if K > RAGGED_MAX_SETS:
        raise BssError('ragged bss_eval: at most %d sets of estimates, got %d' % (RAGGED_MAX_SETS, K))
    return len(refs), K, S, lengths


def _ragged_groups(lengths, K, S, flen, cap_bytes):
    """Consecutive recordings whose workspace stays under cap_bytes -> [(first, last + 1)]."""
    lib, B = _load_ragged(), ragged_block()
    blocks = [(L + flen - 1 + B - 1) // B for L in lengths]
    groups, r0, bt = [], 0, 0
    for r, nb in enumerate(blocks):
        alone = lib.ams_bssr_workspace_bytes(1, K, S, flen, nb)
        if alone > cap_bytes:
            raise BssError('ragged bss_eval: recording %d (%d samples, %d sources, %d sets, flen %d) needs a workspace of %d bytes, '
                           'the cap is %d' % (r, lengths[r], S, K, flen, alone, cap_bytes))
        if r > r0 and (lib.ams_bssr_workspace_bytes(r - r0 + 1, K, S, flen, bt + nb) > cap_bytes or r - r0 >= RAGGED_MAX_REC):
            groups.append((r0, r))
            r0, bt = r, 0
        bt += nb
    groups.append((r0, len(lengths)))
    return groups


def bss_eval_pairs_ragged(refs, ests, flen=FLEN, cap_bytes=None):
    """refs: a list of [S, L_r]; ests: a list of [S, L_r] or [K, S, L_r] (array-like or tensors, one K and one S for all recordings;
    device tensors are packed on the device) -> (crit, info): numpy float64 [R, K, 3, S, S] with crit[r, k] = the (sdr, sir, sar)
    pair matrices [jest, jtrue] of bss_eval_pairs(refs[r], ests[r][k]), and int32 [R], non-zero where a Gram matrix of the
    recording was not positive definite (that recording's criteria are NaN, the others are unaffected).  One library call per
    group of consecutive recordings whose workspace stays under cap_bytes (default RAGGED_CAP_BYTES); no result depends on the
    grouping; a single recording above the cap is refused."""
    R, K, S, lengths = _ragged_shapes(refs, ests, flen)
    cap = RAGGED_CAP_BYTES if cap_bytes is None else int(cap_bytes)
    if not torch.cuda.is_available():
        raise BssError('bss_eval needs a GPU (there is no CPU fallback)')
    flen = int(flen)
    groups = _ragged_groups(lengths, K, S, flen, cap)
    dev = next((x.device for x in list(refs) + list(ests) if torch.is_tensor(x) and x.is_cuda), torch.device('cuda'))
    crit, info = np.empty((R, K, 3, S, S)), np.empty(R, np.int32)
    for r0, r1 in groups:
        off = np.concatenate([[0], np.cumsum(lengths[r0:r1])])
        ref = torch.empty(S * int(off[-1]), dtype=torch.float64, device=dev)
        est = torch.empty(K * S * int(off[-1]), dtype=torch.float64, device=dev)
        for i, r in enumerate(range(r0, r1)):
            ref[S * off[i]:S * off[i + 1]].copy_(torch.as_tensor(refs[r]).reshape(-1))
            est[K * S * off[i]:K * S * off[i + 1]].copy_(torch.as_tensor(ests[r]).reshape(-1))
        c, f = bss_eval_pairs_ragged_packed(ref, est, lengths[r0:r1], K, S, flen)
        crit[r0:r1], info[r0:r1] = c.cpu().numpy(), f.cpu().numpy()
    return crit, info


def bss_eval_sources_ragged(refs, ests, compute_permutation=True, flen=FLEN, cap_bytes=None):
    """As bss_eval_pairs_ragged -> (sdr, sir, sar [R, K, S] float64, perm [R, K, S] int): per recording and set what
    bss_eval_sources_cupy returns."""
    crit, _ = bss_eval_pairs_ragged(refs, ests, flen=flen, cap_bytes=cap_bytes)
    return _select_all(crit, compute_permutation)


# ---------------------------------------------------------------------------------------------------------------------------
# Scale-invariant SDR with rectangular matching (include/ams_sisdr.h, libams_sisdr.so; host side: ams_hip/sisdr.py): recordings of
# ANY lengths whose numbers of references and of estimated tracks are free per recording and per set -- what BSS-eval above cannot
# take.  Two launches per library call whatever R is.  The definition is this project's own (the reference project has no
# counterpart); its float64 restatement is tests/sisdr_ref.py.
def si_sdr_ragged(refs, ests, mixtures, zero_mean=True, cap_bytes=None):
    """refs[r]: [Sr_r, L_r]; ests[r]: one [Se, L_r] array or a list of K of them (one K for all recordings, 1 .. 8; Sr and Se in 1 .. 6
    and free per recording and set); mixtures[r]: [L_r].  float32 numpy arrays or tensors; device tensors are packed on the device.
    -> a dictionary of numpy arrays with leading axes [R, K]:
        pair [R, K, 6, 6] (estimate, reference) si_sdr in dB, NaN outside [Se, Sr];  match_ref [R, K, 6]: the estimate of every
        reference, match_est [R, K, 6]: the reference of every estimate, -1 for a missed reference, a spurious estimate or padding;
        si_sdr, si_sdri [R, K, 6] per reference (NaN where unmatched; si_sdri = si_sdr - base);  missed, spurious [R, K];
        base [R, 6] = si_sdr(mixture, reference);  info [R]: bit 0 = a silent reference (no matching, leave it out of every mean).
    One library call per group of consecutive recordings that stays under cap_bytes (default ams_hip.sisdr.CAP_BYTES); no result
    depends on the grouping or on the other recordings; a single recording above the cap is refused.  No CPU fallback."""
    from ams_hip import sisdr
    try:
        return sisdr.si_sdr_ragged(refs, ests, mixtures, zero_mean=zero_mean, cap_bytes=cap_bytes)
    except sisdr.SisdrError as e:
        raise BssError(str(e))
