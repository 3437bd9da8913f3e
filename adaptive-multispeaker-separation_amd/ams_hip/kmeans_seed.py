"""k-means++ (D^2) seeding of every segment of a ragged point set: ctypes binding of libams_kmeans_seed.so (include/ams_kmeans_seed.h) and
its tensor-level wrapper.

    seeds = seed_plusplus(xn, seg, C, tries, draws, w=None)        # int32 [R tries, C] on the device

xn [Ptot, E] holds the ALREADY normalised points of the segments one after the other (what ams_hip.kmeans_ragged clusters with
normalize_input=False), seg is a kmeans_ragged.Segments (or the sizes P_r), draws a HOST uint64 array [R tries, C]: the one random number
every step of every try consumes.  Row r tries + t of the result holds the C seeds of try t of segment r, relative to the segment: what
kmeans_ragged, kmeans_ragged_soft and spk_count.count_clusters take as init_idx once it is copied to the host.  The sampling weights are
integers (DESIGN.md 4.14 and the header), so the seeds are a function of the inputs alone; the restatement is tests/kmeans_seed_ref.py.
2 C launches whatever the number of segments, nothing synchronised with the host.  Hand-written HIP kernels on torch's current stream,
torch for device memory and the stream only, no CPU path.
"""
import ctypes
import os

import numpy as np
import torch

from . import kmeans_ragged as Kr
from . import ops
from ._lib import AmsError, check, parse_header

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, 'libams_kmeans_seed.so')
HEADER_PATH = os.path.normpath(os.path.join(_HERE, '..', '..', 'include', 'ams_kmeans_seed.h'))
ABI_VERSION = 1            # include/ams_kmeans_seed.h: ams_kms_abi_version()
PAIRS = frozenset((E, C) for E in (40, 8) for C in (1, 2, 3, 4, 5, 6))

_vp = ctypes.c_void_p
_lib = None
LAUNCHES = 0               # kernel launches made through this module so far (a step is two: the weighing and the pick)


def load():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise AmsError('libams_kmeans_seed.so not found at %s -- the HIP extension is required (no CPU fallback); '
                       'run __graft_entry__.build()' % LIB_PATH)
    lib = ctypes.CDLL(LIB_PATH)             # (torch is imported above: one HIP runtime in the process, see _lib.load)
    for name, (ret, argtypes) in parse_header(HEADER_PATH).items():
        try:
            fn = getattr(lib, name)
        except AttributeError:
            raise AmsError('libams_kmeans_seed.so does not export %s (declared in include/ams_kmeans_seed.h)' % name)
        fn.restype = ret
        fn.argtypes = argtypes
    if lib.ams_kms_abi_version() != ABI_VERSION:
        raise AmsError('libams_kmeans_seed.so ABI version mismatch: the library is %d, this binding is %d -- rebuild (make -C csrc)'
                       % (lib.ams_kms_abi_version(), ABI_VERSION))
    _lib = lib
    return lib


def _p(t):
    return _vp(t.data_ptr()) if t is not None else _vp(0)


def _s():
    return _vp(torch.cuda.current_stream().cuda_stream)


def _launch(status, what, n):
    global LAUNCHES
    check(status, what)
    LAUNCHES += n


def check_domain(E, C):
    """ValueError for an (embedding size, clusters) pair the library has no kernel for -- before anything is launched."""
    if (int(E), int(C)) not in PAIRS:
        raise ValueError('k-means++ seeding takes (embedding_size, clusters) in %s, got (%d, %d)' % (ops._pairs_text(PAIRS), E, C))


def check_draws(draws, R, tries, C):
    """draws (host) -> contiguous uint64 [R tries, C]; ValueError for another dtype or shape."""
    if torch.is_tensor(draws):
        raise ValueError('k-means++ seeding: draws are a HOST uint64 array of shape [R tries, C] = %s, got a tensor' % ((R * tries, C),))
    d = np.asarray(draws)
    if d.dtype != np.uint64 or d.shape != (R * tries, C):
        raise ValueError('k-means++ seeding: draws must be uint64 of shape [R tries, C] = %s, got %s %s' % ((R * tries, C), d.dtype, d.shape))
    return np.ascontiguousarray(d)


def check_sizes(seg, C):
    """ValueError that names the recording for a segment of fewer than C points: its seeds could not be distinct."""
    small = np.flatnonzero(seg.P < int(C))
    if small.size:
        r = int(small[0])
        raise ValueError('k-means++ seeding: recording %d has %d points, fewer than the %d seeds to choose' % (r, seg.P[r], C))


def _checked(xn, p_off, C, tries, draws, w):
    C, tries = int(C), int(tries)
    seg = Kr.segments(p_off)
    if tries < 1:
        raise ValueError('k-means++ seeding: tries >= 1, got %d' % tries)
    if not torch.is_tensor(xn) or xn.dim() != 2:
        raise ValueError('k-means++ seeding: the points are a [Ptot, E] tensor, got %s' % (tuple(xn.shape) if torch.is_tensor(xn) else type(xn).__name__,))
    E = int(xn.shape[1])
    check_domain(E, C)
    if xn.shape[0] != seg.Ptot:
        raise ValueError('k-means++ seeding: %d points for segments of %d points in all' % (xn.shape[0], seg.Ptot))
    if w is not None and (not torch.is_tensor(w) or tuple(w.shape) != (seg.Ptot,)):
        raise ValueError('k-means++ seeding: the weights are a [Ptot] = [%d] tensor' % seg.Ptot)
    d = check_draws(draws, seg.R, tries, C)
    check_sizes(seg, C)
    ops._chk(xn, w)
    return seg, E, C, tries, d


def seed_plusplus(xn, p_off, C, tries, draws, w=None, steps=None):
    """xn [Ptot, E] float32 on the device, already normalised; p_off: a Segments or the sizes P_r; draws: HOST uint64 [R tries, C];
    w [Ptot] or None -> seeds int32 [R tries, C] on the device.  2 C launches, no host synchronisation (the draws are uploaded).
    steps: None, or a callable called as steps(c) after step c is enqueued -- the steps then go one entry point each (tools/seed_bench.py
    times them so); the seeds are the same."""
    seg, E, C, tries, d = _checked(xn, p_off, C, tries, draws, w)
    lib, dev = load(), xn.device
    t = seg.tables(dev)
    du = torch.from_numpy(d.view(np.int64)).to(dev)               # (the bits of the uint64 draws)
    nb = lib.ams_kms_workspace_bytes(seg.R, tries, seg.Gtot, E, C)
    ws = torch.empty((nb + 7) // 8, dtype=torch.int64, device=dev)
    seeds = torch.empty((seg.R * tries, C), dtype=torch.int32, device=dev)
    head = (_p(xn), _p(w), _p(t['tab']), _p(t['p_off']), _p(t['g_off']), _p(du), seg.R, tries, seg.Gtot, E, C)
    if steps is None:
        _launch(lib.ams_kms_seed(*head, _p(ws), nb, _p(seeds), _s()), 'ams_kms_seed', 2 * C)
    else:
        for c in range(C):
            _launch(lib.ams_kms_step(*head, c, _p(ws), nb, _p(seeds), _s()), 'ams_kms_step', 2)
            steps(c)
    return seeds
