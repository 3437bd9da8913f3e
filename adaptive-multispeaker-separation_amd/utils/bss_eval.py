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
        if lib.ams_bss_abi_version() != 1:
            raise BssError('libams_bss.so ABI version mismatch')
        _lib = lib
    return _lib


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


# the reference exposes the same metric under two names (numpy and cupy back ends); both map to the HIP path here
bss_eval_sources = bss_eval_sources_cupy


# ---------------------------------------------------------------------------------------------------------------------------
# Batched path (include/ams_bss_batch.h): U utterances x K sets of estimates in one library call.  The Gram matrices of an
# utterance are assembled and factorised once (the library's own batched MFMA-f64 Cholesky) and shared by its K sets.
MAX_UTT = 64                    # utterances per library call; larger batches are processed in slices of this size

_blib = None
_bctx = {}                      # (max_utt, nsets, nsrc, nsampl, flen, device) -> (ctx pointer, workspace tensor, bytes)


def _load_batch():
    global _blib
    if _blib is None:
        if not os.path.exists(LIB_PATH):
            raise BssError('libams_bss.so not found at %s -- run __graft_entry__.build() (no CPU fallback)' % LIB_PATH)
        lib = ctypes.CDLL(LIB_PATH)
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
        if lib.ams_bssb_abi_version() != 1:
            raise BssError('libams_bss.so batch ABI version mismatch')
        _blib = lib
    return _blib


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
    """[S, S] pair matrices -> (sdr, sir, sar [S], perm [S]); the rule of bss_eval_sources_cupy: best mean SIR, the first
    maximum wins."""
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


def bss_eval_sources_batch(reference_sources, estimated_sources, compute_permutation=True, flen=FLEN, max_utt=MAX_UTT):
    """refs [U, S, L], ests [U, S, L] or [U, K, S, L] -> (sdr, sir, sar [U, K, S] float64, perm [U, K, S] int): per utterance and
    set what bss_eval_sources_cupy returns, from ONE library call per slice of max_utt utterances."""
    crit, _ = bss_eval_pairs_batch(reference_sources, estimated_sources, flen=flen, max_utt=max_utt)
    U, K, _, S, _ = crit.shape
    sdr, sir, sar = (np.empty((U, K, S)) for _ in range(3))
    perm = np.empty((U, K, S), dtype=np.int64)
    for u in range(U):
        for k in range(K):
            sdr[u, k], sir[u, k], sar[u, k], perm[u, k] = _select_permutation(crit[u, k, 0], crit[u, k, 1], crit[u, k, 2],
                                                                              compute_permutation)
    return sdr, sir, sar, perm


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
