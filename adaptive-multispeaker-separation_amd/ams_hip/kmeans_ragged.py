"""Hard k-means over segments of different numbers of points: ctypes binding of libams_kmeans_ragged.so (include/ams_kmeans_ragged.h)
and its tensor-level wrapper.

    seg = segments([P_0, P_1, ...])                  # host only: p_off, g_off and the work table (segment, chunk, column)
    seg = segments_of_layout(lay, TF)                # ... for the chunk stream of stitch_batch.layout: P_r = C_r TF
    cent, labels, best = kmeans_ragged(x, seg, init_idx, C, tries, iterations)

x [Ptot, E] holds the segments one after the other; every segment is clustered on its own, bit for bit as ops.kmeans_run clusters it as a
batch of one (and as oracle/kmeans.py does), in iterations + 4 launches whatever the number of segments: the tables that tell a workgroup
which segment it works on are built on the host and uploaded as ONE buffer per layout and device.  Hand-written HIP kernels on torch's
current stream, torch for device memory and the stream only, no CPU path.  Definitions: DESIGN.md 4.10 and the header.
"""
import ctypes
import os

import numpy as np
import torch

from . import ops
from ._lib import AmsError, check, parse_header

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, 'libams_kmeans_ragged.so')
HEADER_PATH = os.path.normpath(os.path.join(_HERE, '..', '..', 'include', 'ams_kmeans_ragged.h'))
ABI_VERSION = 1            # include/ams_kmeans_ragged.h: ams_kmr_abi_version()
CHUNK = 8192               # points per chunk of the summation order
PAIRS = frozenset((E, C) for E in (40, 8) for C in (2, 3, 4, 5, 6))

_vp = ctypes.c_void_p
_lib = None
LAUNCHES = 0               # kernel launches made through this module so far (every launching entry point of the library is one launch)


def load():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise AmsError('libams_kmeans_ragged.so not found at %s -- the HIP extension is required (no CPU fallback); '
                       'run __graft_entry__.build()' % LIB_PATH)
    lib = ctypes.CDLL(LIB_PATH)             # (torch is imported above: one HIP runtime in the process, see _lib.load)
    for name, (ret, argtypes) in parse_header(HEADER_PATH).items():
        try:
            fn = getattr(lib, name)
        except AttributeError:
            raise AmsError('libams_kmeans_ragged.so does not export %s (declared in include/ams_kmeans_ragged.h)' % name)
        fn.restype = ret
        fn.argtypes = argtypes
    if lib.ams_kmr_abi_version() != ABI_VERSION:
        raise AmsError('libams_kmeans_ragged.so ABI version mismatch: the library is %d, this binding is %d -- rebuild (make -C csrc)'
                       % (lib.ams_kmr_abi_version(), ABI_VERSION))
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


def check_domain(E, C):
    """ValueError for an (embedding size, clusters) pair the library has no kernel for -- before anything is launched."""
    if (int(E), int(C)) not in PAIRS:
        raise ValueError('ragged k-means takes (embedding_size, clusters) in %s, got (%d, %d)' % (ops._pairs_text(PAIRS), E, C))


class Segments(object):
    """Where R segments lie (numpy, host only; the names are the header's):
        R, Ptot, Gtot, Pmax            ints
        P [R]; p_off, g_off [R + 1]    int64
        tab [4 Gtot, 4]                int32: (segment, chunk, column, 0)
    g_off and tab are filled by the library (ams_kmr_tables).  tables(device) uploads them as one buffer, once per device."""

    def __init__(self, sizes):
        P = np.asarray([int(v) for v in sizes], np.int64).reshape(-1)
        if P.size < 1:
            raise ValueError('segments: at least one segment')
        if P.min() < 1:
            raise ValueError('segments: a segment needs at least one point, got sizes %s' % (P[P < 1].tolist(),))
        self.R, self.P = int(P.size), P
        self.p_off = np.concatenate([[0], np.cumsum(P)]).astype(np.int64)
        self.Ptot, self.Pmax = int(self.p_off[-1]), int(P.max())
        lib = load()
        G = lib.ams_kmr_chunks(self.p_off.ctypes.data_as(_vp), self.R)
        if G < 1:
            raise ValueError('segments: %d segments of %d points in all are more than the work table holds' % (self.R, self.Ptot))
        self.Gtot = int(G)
        self.g_off = np.zeros(self.R + 1, np.int64)
        self.tab = np.zeros((4 * self.Gtot, 4), np.int32)
        check(lib.ams_kmr_tables(self.p_off.ctypes.data_as(_vp), self.R, self.g_off.ctypes.data_as(_vp), self.tab.ctypes.data_as(_vp)),
              'ams_kmr_tables')
        self._dev = {}

    def tables(self, device):
        """{'p_off', 'g_off', 'tab'}: device views of ONE uploaded buffer (the int64 tables first, the int32 table behind them)."""
        key = str(torch.device(device))
        if key not in self._dev:
            n = self.R + 1
            host = np.zeros(2 * n + 8 * self.Gtot, np.int64)
            host[:n], host[n:2 * n] = self.p_off, self.g_off
            host[2 * n:].view(np.int32)[:] = self.tab.reshape(-1)
            buf = torch.from_numpy(host).to(device)
            self._dev[key] = {'p_off': buf[:n], 'g_off': buf[n:2 * n], 'tab': buf[2 * n:].view(torch.int32).view(4 * self.Gtot, 4)}
        return self._dev[key]

    def rows(self, r):
        """The points of segment r as a slice."""
        return slice(int(self.p_off[r]), int(self.p_off[r + 1]))


def segments(sizes):
    return sizes if isinstance(sizes, Segments) else Segments(sizes)


def segments_of_layout(lay, TF):
    """The segments of the chunk stream of a stitch_batch.Layout: recording r is C_r chunks of TF points, p_off = TF c_off."""
    seg = Segments(int(TF) * lay.C)
    assert np.array_equal(seg.p_off, int(TF) * lay.c_off)
    return seg


def check_seeds(init_idx, seg, tries, C):
    """init_idx (host) -> int32 [R tries, C], checked: row r tries + t holds C distinct indices in 0 .. P_r - 1.  A bad row is a ValueError
    that names the recording -- never an out-of-range read on the device."""
    if torch.is_tensor(init_idx):
        init_idx = init_idx.detach().cpu().numpy()
    idx = np.asarray(init_idx)
    if idx.dtype.kind not in 'iu' or idx.shape != (seg.R * tries, C):
        raise ValueError('ragged k-means: init_idx must be integers of shape [R tries, C] = %s, got %s %s'
                         % ((seg.R * tries, C), idx.dtype, idx.shape))
    idx = idx.astype(np.int64)
    limit = np.repeat(seg.P, tries)[:, None]
    bad = ((idx < 0) | (idx >= limit)).any(axis=1)
    if bad.any():
        row = int(np.flatnonzero(bad)[0])
        raise ValueError('ragged k-means: recording %d, try %d: seed indices %s outside 0 .. %d (the recording has %d points)'
                         % (row // tries, row % tries, idx[row].tolist(), seg.P[row // tries] - 1, seg.P[row // tries]))
    srt = np.sort(idx, axis=1)
    rep = (srt[:, 1:] == srt[:, :-1]).any(axis=1)
    if rep.any():
        row = int(np.flatnonzero(rep)[0])
        raise ValueError('ragged k-means: recording %d, try %d: seed indices %s are not distinct' % (row // tries, row % tries, idx[row].tolist()))
    return np.ascontiguousarray(idx, dtype=np.int32)


def _every_try(x, p_off, init_idx, C, tries, iterations, w, normalize_input):
    """The checks and the init, iterate and inertia launches of kmeans_ragged -> (xn, seg, centroids [R tries, C, E], inertia [R tries])."""
    C, tries, iterations = int(C), int(tries), int(iterations)
    seg = segments(p_off)
    if tries < 1 or iterations < 0:
        raise ValueError('ragged k-means: tries >= 1 and iterations >= 0, got %d and %d' % (tries, iterations))
    if not torch.is_tensor(x) or x.dim() != 2:
        raise ValueError('ragged k-means: the points are a [Ptot, E] tensor, got %s' % (tuple(x.shape) if torch.is_tensor(x) else type(x).__name__,))
    E = int(x.shape[1])
    check_domain(E, C)
    if x.shape[0] != seg.Ptot:
        raise ValueError('ragged k-means: %d points for segments of %d points in all' % (x.shape[0], seg.Ptot))
    if w is not None and (not torch.is_tensor(w) or tuple(w.shape) != (seg.Ptot,)):
        raise ValueError('ragged k-means: the weights are a [Ptot] = [%d] tensor' % seg.Ptot)
    idx = check_seeds(init_idx, seg, tries, C)
    ops._chk(x, w)
    lib, dev = load(), x.device
    xn = ops.kmeans_normalize(x) if normalize_input else x
    t = seg.tables(dev)
    idx = torch.from_numpy(idx).to(dev)
    R, RT = seg.R, seg.R * tries
    nb = lib.ams_kmr_workspace_bytes(R, tries, seg.Gtot, E, C)
    ws = ops._ws(nb, xn)
    # row tickets of the in-launch finish: the persistent zeroed words ops.kmeans_run uses (per device and stream; every pass leaves them zero)
    key = (dev.index, torch.cuda.current_stream().cuda_stream)
    tk = ops._KM_TICKETS.get(key)
    if tk is None or tk.numel() < RT:
        tk = ops._KM_TICKETS[key] = torch.zeros(max(RT, 1024), dtype=torch.int32, device=dev)
    tabs = (_p(t['tab']), _p(t['p_off']), _p(t['g_off']))
    cent = torch.empty((RT, C, E), dtype=torch.float32, device=dev)
    _launch(lib.ams_kmr_init(_p(xn), _p(t['p_off']), _p(idx), _p(cent), R, tries, E, C, _s()), 'ams_kmr_init')
    for _ in range(iterations):
        nxt = torch.empty_like(cent)
        _launch(lib.ams_kmr_iterate(_p(xn), _p(w), *tabs, _p(cent), _p(nxt), R, tries, seg.Gtot, seg.Pmax, E, C, _p(ws), nb, _p(tk), _s()),
                'ams_kmr_iterate')
        cent = nxt
    inertia = torch.empty(RT, dtype=torch.float32, device=dev)
    _launch(lib.ams_kmr_inertia(_p(xn), _p(w), *tabs, _p(cent), _p(inertia), R, tries, seg.Gtot, seg.Pmax, E, C, _p(ws), nb, _p(tk), _s()),
            'ams_kmr_inertia')
    return xn, seg, cent, inertia


def kmeans_ragged_tries(x, p_off, init_idx, C, tries, iterations, w=None, normalize_input=True):
    """The arguments of kmeans_ragged -> (centroids [R tries, C, E], inertia [R tries]) of EVERY try: the run without its select and
    labels launches (iterations + 2 launches), for a caller that picks the try itself (ams_hip/spk_count.py)."""
    return _every_try(x, p_off, init_idx, C, tries, iterations, w, normalize_input)[2:]


def labels_ragged(xn, p_off, centroids, w=None, out=None):
    """The labels launch alone: xn [Ptot, E] ALREADY normalised, centroids [R, C, E] (one set per segment), w as ams_kmr_labels takes it
    (None: the assign_at_end re-assignment; the run's weights otherwise) -> labels int32 [Ptot] (written to `out` if given)."""
    seg = segments(p_off)
    if not torch.is_tensor(xn) or xn.dim() != 2 or xn.shape[0] != seg.Ptot:
        raise ValueError('ragged k-means: the points are a [Ptot, E] = [%d, E] tensor' % seg.Ptot)
    E = int(xn.shape[1])
    if not torch.is_tensor(centroids) or centroids.dim() != 3 or centroids.shape[0] != seg.R or centroids.shape[2] != E:
        raise ValueError('ragged k-means: the centroids are a [R, C, E] = [%d, C, %d] tensor' % (seg.R, E))
    C = int(centroids.shape[1])
    check_domain(E, C)
    if w is not None and (not torch.is_tensor(w) or tuple(w.shape) != (seg.Ptot,)):
        raise ValueError('ragged k-means: the weights are a [Ptot] = [%d] tensor' % seg.Ptot)
    ops._chk(xn, w, centroids)
    t = seg.tables(xn.device)
    labels = torch.empty(seg.Ptot, dtype=torch.int32, device=xn.device) if out is None else out
    _launch(load().ams_kmr_labels(_p(xn), _p(w), _p(t['tab']), _p(t['p_off']), _p(t['g_off']), _p(centroids), _p(labels), seg.R, seg.Gtot, E, C,
                                  _s()), 'ams_kmr_labels')
    return labels


def kmeans_ragged(x, p_off, init_idx, C, tries, iterations, w=None, assign_at_end=True, normalize_input=True, want_inertia=False):
    """x [Ptot, E] float32 on the device, p_off: a Segments or the sizes P_r, init_idx: HOST integers [R tries, C] relative to each segment
    (they are drawn on the host anyway), w [Ptot] or None -> (centroids [R, C, E], labels int32 [Ptot], best int32 [R]) (and
    inertia [R tries] with want_inertia).  iterations + 4 launches after the normalisation, no host synchronisation."""
    xn, seg, cent, inertia = _every_try(x, p_off, init_idx, C, tries, iterations, w, normalize_input)
    C, tries, R, E, dev = int(C), int(tries), seg.R, int(x.shape[1]), x.device
    best = torch.empty(R, dtype=torch.int32, device=dev)
    sel = torch.empty((R, C, E), dtype=torch.float32, device=dev)
    _launch(load().ams_kmr_select(_p(inertia), _p(cent), _p(best), _p(sel), R, tries, E, C, _s()), 'ams_kmr_select')
    # at the end: re-assigned without the silence weights (the reference's assign_at_end); else the chosen try's own last assignment
    labels = labels_ragged(xn, seg, sel, None if assign_at_end else w)
    return (sel, labels, best, inertia) if want_inertia else (sel, labels, best)
