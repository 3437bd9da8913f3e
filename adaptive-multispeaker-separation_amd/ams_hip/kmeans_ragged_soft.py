"""Soft k-means over segments of different numbers of points: ctypes binding of libams_kmeans_ragged_soft.so
(include/ams_kmeans_ragged_soft.h) and its tensor-level wrapper.

    seg = kmeans_ragged.segments([P_0, P_1, ...])    # the layout, the work table and the one-buffer upload of the hard ragged k-means
    cent, masks, best = kmeans_ragged_soft(x, seg, init_idx, C, tries, iterations, beta)

x [Ptot, E] holds the segments one after the other; every segment is clustered on its own with the soft assignment
softmax_c(-beta w |x - c|^2) (oracle/kmeans.py with beta), in iterations + 4 launches whatever the number of segments, and comes out bit
for bit as the same call gives it alone: the summation order is restarted at each segment (the header).  Like every soft
mode it is tolerance-tested against float64, not bit-specified against the oracle.  Hand-written HIP kernels on torch's current stream,
torch for device memory and the stream only, no CPU path.
"""
import ctypes
import math
import os

import torch

from . import ops
from ._lib import AmsError, check, parse_header
from .kmeans_ragged import PAIRS, Segments, check_seeds, segments      # noqa: F401  (the layout is shared)

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, 'libams_kmeans_ragged_soft.so')
HEADER_PATH = os.path.normpath(os.path.join(_HERE, '..', '..', 'include', 'ams_kmeans_ragged_soft.h'))
ABI_VERSION = 1            # include/ams_kmeans_ragged_soft.h: ams_kmrs_abi_version()

_vp = ctypes.c_void_p
_lib = None
LAUNCHES = 0               # kernel launches made through this module so far (every launching entry point of the library is one launch)


def load():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise AmsError('libams_kmeans_ragged_soft.so not found at %s -- the HIP extension is required (no CPU fallback); '
                       'run __graft_entry__.build()' % LIB_PATH)
    lib = ctypes.CDLL(LIB_PATH)             # (torch is imported above: one HIP runtime in the process, see _lib.load)
    for name, (ret, argtypes) in parse_header(HEADER_PATH).items():
        try:
            fn = getattr(lib, name)
        except AttributeError:
            raise AmsError('libams_kmeans_ragged_soft.so does not export %s (declared in include/ams_kmeans_ragged_soft.h)' % name)
        fn.restype = ret
        fn.argtypes = argtypes
    if lib.ams_kmrs_abi_version() != ABI_VERSION:
        raise AmsError('libams_kmeans_ragged_soft.so ABI version mismatch: the library is %d, this binding is %d -- rebuild (make -C csrc)'
                       % (lib.ams_kmrs_abi_version(), ABI_VERSION))
    _lib = lib
    return lib


def _p(t):
    return _vp(t.data_ptr()) if t is not None else _vp(0)


def _s():
    return _vp(torch.cuda.current_stream().cuda_stream)


def _launch(status, what):
    global LAUNCHES
    check(status, what)
    LAUNCHES += 1


def check_domain(E, C, beta):
    """ValueError for an (embedding size, clusters) pair the library has no kernel for, or a beta that is no finite number >= 0 -- before
    anything is launched."""
    if (int(E), int(C)) not in PAIRS:
        raise ValueError('ragged soft k-means takes (embedding_size, clusters) in %s, got (%d, %d)' % (ops._pairs_text(PAIRS), E, C))
    try:
        b = float('nan') if beta is None or isinstance(beta, bool) else float(beta)
    except (TypeError, ValueError):
        b = float('nan')
    if not math.isfinite(b) or b < 0:
        raise ValueError('ragged soft k-means takes a finite beta >= 0 (the hard assignment is ams_hip.kmeans_ragged), got %r' % (beta,))


def _check_points(x, seg, w):
    if not torch.is_tensor(x) or x.dim() != 2:
        raise ValueError('ragged soft k-means: the points are a [Ptot, E] tensor, got %s' % (tuple(x.shape) if torch.is_tensor(x) else type(x).__name__,))
    if x.shape[0] != seg.Ptot:
        raise ValueError('ragged soft k-means: %d points for segments of %d points in all' % (x.shape[0], seg.Ptot))
    if w is not None and (not torch.is_tensor(w) or tuple(w.shape) != (seg.Ptot,)):
        raise ValueError('ragged soft k-means: the weights are a [Ptot] = [%d] tensor' % seg.Ptot)


def _every_try(x, p_off, init_idx, C, tries, iterations, beta, w, normalize_input):
    """The checks and the init, iterate and inertia launches -> (xn, seg, centroids [R tries, C, E], inertia [R tries])."""
    C, tries, iterations = int(C), int(tries), int(iterations)
    seg = segments(p_off)
    if tries < 1 or iterations < 0:
        raise ValueError('ragged soft k-means: tries >= 1 and iterations >= 0, got %d and %d' % (tries, iterations))
    _check_points(x, seg, w)
    E = int(x.shape[1])
    check_domain(E, C, beta)
    idx = check_seeds(init_idx, seg, tries, C)
    ops._chk(x, w)
    lib, dev, beta = load(), x.device, float(beta)
    xn = ops.kmeans_normalize(x) if normalize_input else x
    t = seg.tables(dev)
    idx = torch.from_numpy(idx).to(dev)
    R, RT = seg.R, seg.R * tries
    nb = lib.ams_kmrs_workspace_bytes(R, tries, seg.Gtot, E, C)
    ws = ops._ws(nb, xn)
    # row tickets of the in-launch finish: the persistent zeroed words ops.kmeans_run uses (per device and stream; every pass leaves them zero)
    key = (dev.index, torch.cuda.current_stream().cuda_stream)
    tk = ops._KM_TICKETS.get(key)
    if tk is None or tk.numel() < RT:
        tk = ops._KM_TICKETS[key] = torch.zeros(max(RT, 1024), dtype=torch.int32, device=dev)
    tabs = (_p(t['tab']), _p(t['p_off']), _p(t['g_off']))
    cent = torch.empty((RT, C, E), dtype=torch.float32, device=dev)
    _launch(lib.ams_kmrs_init(_p(xn), _p(t['p_off']), _p(idx), _p(cent), R, tries, E, C, _s()), 'ams_kmrs_init')
    for _ in range(iterations):
        nxt = torch.empty_like(cent)
        _launch(lib.ams_kmrs_iterate(_p(xn), _p(w), *tabs, _p(cent), _p(nxt), R, tries, seg.Gtot, E, C, beta, _p(ws), nb, _p(tk), _s()),
                'ams_kmrs_iterate')
        cent = nxt
    inertia = torch.empty(RT, dtype=torch.float32, device=dev)
    _launch(lib.ams_kmrs_inertia(_p(xn), _p(w), *tabs, _p(cent), _p(inertia), R, tries, seg.Gtot, E, C, beta, _p(ws), nb, _p(tk), _s()),
            'ams_kmrs_inertia')
    return xn, seg, cent, inertia


def kmeans_ragged_soft_tries(x, p_off, init_idx, C, tries, iterations, beta, w=None, normalize_input=True):
    """The arguments of kmeans_ragged_soft -> (centroids [R tries, C, E], inertia [R tries]) of EVERY try: the run without its select and
    masks launches (iterations + 2 launches)."""
    return _every_try(x, p_off, init_idx, C, tries, iterations, beta, w, normalize_input)[2:]


def masks_ragged(xn, p_off, centroids, beta, w=None, out=None):
    """The masks launch alone: xn [Ptot, E] ALREADY normalised, centroids [R, C, E] (one set per segment), w as ams_kmrs_masks takes it
    (None: the assign_at_end labels; the run's weights otherwise) -> masks float32 [Ptot, C]: softmax_c(-beta w |x - c|^2) of every
    point (written to `out`, a contiguous float32 tensor of Ptot C elements, if given)."""
    seg = segments(p_off)
    _check_points(xn, seg, w)
    E = int(xn.shape[1])
    if not torch.is_tensor(centroids) or centroids.dim() != 3 or centroids.shape[0] != seg.R or centroids.shape[2] != E:
        raise ValueError('ragged soft k-means: the centroids are a [R, C, E] = [%d, C, %d] tensor' % (seg.R, E))
    C = int(centroids.shape[1])
    check_domain(E, C, beta)
    if out is not None and (not torch.is_tensor(out) or out.dtype != torch.float32 or out.numel() != seg.Ptot * C or not out.is_contiguous()
                            or out.device != xn.device):
        raise ValueError('ragged soft k-means: `out` is a contiguous float32 tensor of Ptot C = %d elements on the device of the points'
                         % (seg.Ptot * C))
    ops._chk(xn, w, centroids)
    t = seg.tables(xn.device)
    masks = torch.empty((seg.Ptot, C), dtype=torch.float32, device=xn.device) if out is None else out
    _launch(load().ams_kmrs_masks(_p(xn), _p(w), _p(t['tab']), _p(t['p_off']), _p(t['g_off']), _p(centroids), float(beta), _p(masks), seg.R,
                                  seg.Gtot, E, C, _s()), 'ams_kmrs_masks')
    return masks


def kmeans_ragged_soft(x, p_off, init_idx, C, tries, iterations, beta, w=None, assign_at_end=True, normalize_input=True, want_inertia=False,
                       out=None):
    """x [Ptot, E] float32 on the device, p_off: a Segments or the sizes P_r, init_idx: HOST integers [R tries, C] relative to each segment,
    beta >= 0, w [Ptot] or None -> (centroids [R, C, E], masks float32 [Ptot, C], best int32 [R]) (and inertia [R tries] with
    want_inertia; the masks are written to `out` if given).  iterations + 4 launches after the normalisation, no host synchronisation."""
    xn, seg, cent, inertia = _every_try(x, p_off, init_idx, C, tries, iterations, beta, w, normalize_input)
    C, tries, R, E, dev = int(C), int(tries), seg.R, int(x.shape[1]), x.device
    best = torch.empty(R, dtype=torch.int32, device=dev)
    sel = torch.empty((R, C, E), dtype=torch.float32, device=dev)
    _launch(load().ams_kmrs_select(_p(inertia), _p(cent), _p(best), _p(sel), R, tries, E, C, _s()), 'ams_kmrs_select')
    # at the end: the labels without the silence weights (the reference's assign_at_end); else those of the chosen try with the run's
    # weights, recomputed from its centroids (no [tries, Ptot, C] buffer is kept)
    masks = masks_ragged(xn, seg, sel, beta, None if assign_at_end else w, out=out)
    return (sel, masks, best, inertia) if want_inertia else (sel, masks, best)
