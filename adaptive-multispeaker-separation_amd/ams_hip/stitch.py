"""Whole recordings: ctypes binding of libams_stitch.so (include/ams_stitch.h) and its tensor-level wrappers.

    mix = chunks(x, L, H)                      # [C, L]: overlapping chunks of a recording x [N], zero-padded
    est = model.infer_chunks(mix)              # [C, S, L]: every chunk separated on its own, outputs in arbitrary order
    out, trk, Q = stitch(est, N, H)            # [S, N]: outputs tracked across the chunk borders and cross-faded

Every function enqueues hand-written HIP kernels on torch's current stream; torch provides device memory and the stream, nothing
else.  There is no CPU path and no host synchronisation -- except the first call for an overlap length and device, which uploads
the cross-fade table (kept from then on).  The definitions are in DESIGN.md 4.7 and in the header.
"""
import ctypes
import os

import numpy as np
import torch

from ._lib import AmsError, check, parse_header

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, 'libams_stitch.so')
HEADER_PATH = os.path.normpath(os.path.join(_HERE, '..', '..', 'include', 'ams_stitch.h'))
ABI_VERSION = 1            # include/ams_stitch.h: ams_stitch_abi_version()
MAX_SPEAKERS = 6

_vp = ctypes.c_void_p
_lib = None
_W_HEAD = {}               # (V, device) -> the cross-fade table on the device


def load():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise AmsError('libams_stitch.so not found at %s -- the HIP extension is required (no CPU fallback); '
                       'run __graft_entry__.build()' % LIB_PATH)
    lib = ctypes.CDLL(LIB_PATH)             # (torch is imported above: one HIP runtime in the process, see _lib.load)
    for name, (ret, argtypes) in parse_header(HEADER_PATH).items():
        try:
            fn = getattr(lib, name)
        except AttributeError:
            raise AmsError('libams_stitch.so does not export %s (declared in include/ams_stitch.h)' % name)
        fn.restype = ret
        fn.argtypes = argtypes
    if lib.ams_stitch_abi_version() != ABI_VERSION:
        raise AmsError('libams_stitch.so ABI version mismatch: the library is %d, this binding is %d -- rebuild (make -C csrc)'
                       % (lib.ams_stitch_abi_version(), ABI_VERSION))
    _lib = lib
    return lib


def _p(t):
    return _vp(t.data_ptr())


def _s():
    return _vp(torch.cuda.current_stream().cuda_stream)


def _chk(dtype, *ts):
    for t in ts:
        if not torch.is_tensor(t) or not t.is_cuda:
            raise AmsError('ams_hip.stitch needs device tensors (there is no CPU fallback)')
        if t.dtype != dtype or not t.is_contiguous():
            raise AmsError('ams_hip.stitch needs contiguous %s tensors, got %s %s' % (dtype, t.dtype, tuple(t.stride())))


def default_hop(L):
    return L // 2


def check_geometry(L, H):
    """The limits of include/ams_stitch.h on the chunk length and the hop, as a ValueError before anything is built or launched."""
    if not (2 <= L <= 1 << 30):
        raise ValueError('chunk length %d: must be in 2 .. 2^30' % L)
    if not ((L + 1) // 2 <= H <= L - 1):
        raise ValueError('hop %d: must be in ceil(L / 2) .. L - 1 = %d .. %d for chunks of %d samples (no sample may lie in more than '
                         'two chunks)' % (H, (L + 1) // 2, L - 1, L))


def nb_chunks(N, L, H):
    """C = 1 + max(0, ceil((N - L) / H)): the chunks of L samples, H apart, that cover N samples."""
    if N < 1:
        raise ValueError('a recording needs at least one sample, got %d' % N)
    check_geometry(L, H)
    return 1 + max(0, -((L - N) // H))


def w_head_table(V):
    """float32((v + 0.5) / V), v < V: computed in float64 and rounded once (the kernel forms w_tail = 1 - w_head itself)."""
    return ((np.arange(V, dtype=np.float64) + 0.5) / V).astype(np.float32)


def _w_head(V, device):
    key = (V, str(device))
    if key not in _W_HEAD:
        _W_HEAD[key] = torch.from_numpy(w_head_table(V)).to(device)
    return _W_HEAD[key]


def chunks(x, L, H=None):
    """x [N] -> mix [C, L]: mix[c, l] = x[c H + l], zero past the end of the recording."""
    H = default_hop(L) if H is None else H
    _chk(torch.float32, x)
    if x.dim() != 1:
        raise AmsError('chunks: a recording is a 1-D tensor, got %s' % (tuple(x.shape),))
    N = x.shape[0]
    C = nb_chunks(N, L, H)
    mix = torch.empty((C, L), dtype=torch.float32, device=x.device)
    check(load().ams_stitch_chunks(_p(x), N, _p(mix), C, L, H, _s()), 'ams_stitch_chunks')
    return mix


def border_stats(est, H):
    """est [C, S, L], C >= 2 -> Q [C - 1, S, S]: Q[c, i, j] = sum_v (est[c, i, H + v] - est[c + 1, j, v])^2 over the overlap."""
    _chk(torch.float32, est)
    if est.dim() != 3 or est.shape[0] < 2:
        raise AmsError('border_stats: est must be [C, S, L] with C >= 2, got %s' % (tuple(est.shape),))
    C, S, L = est.shape
    lib = load()
    nbytes = lib.ams_stitch_workspace_bytes(C, S, L, H)
    ws = torch.empty(max(nbytes // 4, 1), dtype=torch.float32, device=est.device)
    Q = torch.empty((C - 1, S, S), dtype=torch.float32, device=est.device)
    check(lib.ams_stitch_stats(_p(est), _p(Q), C, S, L, H, _p(ws), ws.numel() * 4, _s()), 'ams_stitch_stats')
    return Q


def tracks(Q, S):
    """Q [C - 1, S, S] -> (rel [C - 1, S], trk [C, S]) int32: the cheapest permutation at every border, and its composition from
    chunk 0 on (track k is what chunk 0 called source k)."""
    from .functional import _perm_table32
    _chk(torch.float32, Q)
    if Q.dim() != 3 or Q.shape[0] < 1 or tuple(Q.shape[1:]) != (S, S):
        raise AmsError('tracks: Q must be [C - 1, %d, %d] with C >= 2, got %s' % (S, S, tuple(Q.shape)))
    if not 1 <= S <= MAX_SPEAKERS:
        raise AmsError('tracks: 1 .. %d sources, got %d' % (MAX_SPEAKERS, S))
    C = Q.shape[0] + 1
    perms = _perm_table32(S, Q.device)
    rel = torch.empty((C - 1, S), dtype=torch.int32, device=Q.device)
    trk = torch.empty((C, S), dtype=torch.int32, device=Q.device)
    check(load().ams_stitch_tracks(_p(Q), _p(perms), _p(rel), _p(trk), C, S, perms.shape[0], _s()), 'ams_stitch_tracks')
    return rel, trk


def overlap_add(est, trk, N, H):
    """est [C, S, L], trk [C, S] int32 -> out [S, N]: the tracked outputs cross-faded over the overlaps (bit-exact f32 contract)."""
    _chk(torch.float32, est)
    _chk(torch.int32, trk)
    if est.dim() != 3 or tuple(trk.shape) != tuple(est.shape[:2]):
        raise AmsError('overlap_add: est [C, S, L] and trk [C, S], got %s and %s' % (tuple(est.shape), tuple(trk.shape)))
    C, S, L = est.shape
    check_geometry(L, H)
    w = _w_head(L - H, est.device)
    out = torch.empty((S, N), dtype=torch.float32, device=est.device)
    check(load().ams_stitch_ola(_p(est), _p(trk), _p(w), _p(out), N, C, S, L, H, _s()), 'ams_stitch_ola')
    return out


def stitch(est, N, H=None):
    """est [C, S, L] (the model's output for the chunks of a recording of N samples) -> (out [S, N], trk [C, S], Q [C - 1, S, S]).
    Everything stays on the device; nothing synchronises with the host once the cross-fade table of this overlap length is cached
    (_w_head: the first call uploads it)."""
    _chk(torch.float32, est)
    if est.dim() != 3:
        raise AmsError('stitch: est must be [C, S, L], got %s' % (tuple(est.shape),))
    C, S, L = est.shape
    H = default_hop(L) if H is None else H
    if C != nb_chunks(N, L, H):
        raise AmsError('stitch: %d chunks of %d samples, %d apart, do not make a recording of %d samples (that takes %d)'
                       % (C, L, H, N, nb_chunks(N, L, H)))
    if C == 1:
        trk = torch.arange(S, dtype=torch.int32, device=est.device).reshape(1, S)
        Q = torch.empty((0, S, S), dtype=torch.float32, device=est.device)
    else:
        Q = border_stats(est, H)
        trk = tracks(Q, S)[1]
    return overlap_add(est, trk, N, H), trk, Q
