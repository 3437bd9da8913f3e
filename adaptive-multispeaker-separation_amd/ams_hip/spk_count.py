"""Choosing the number of clusters of every segment of a ragged point set: ctypes binding of libams_spk_count.so
(include/ams_spk_count.h) and its tensor-level wrapper.

    res = count_clusters(x, seg, init_idx, lo, hi, tries, iterations, min_score=None)
    res['count'] [R], res['labels'] [Ptot], res['centroids'] [R, hi, E], res['scores'] [R, ncand], res['tries'] [R, ncand]

For every candidate number of clusters C in max(lo, 2) .. hi the ragged hard k-means (ams_hip/kmeans_ragged.py) runs with the first C
columns of the seed rows; ONE sweep over the points scores all candidates of all segments by the simplified silhouette in float64
(ams_spkc_score), one small launch picks the count per segment (ams_spkc_choose), and the labels are those of ams_kmr_labels on the
chosen candidate's centroids.  The number of launches does not depend on the number of segments; nothing is synchronised with the host.
Hand-written HIP kernels on torch's current stream, torch for device memory and the stream only, no CPU path.  Definitions: DESIGN.md
4.11 and the header; the float64 restatement is tests/speaker_count_ref.py.
"""
import ctypes
import os

import numpy as np
import torch

from . import kmeans_ragged as Kr
from . import ops
from ._lib import AmsError, check, parse_header

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, 'libams_spk_count.so')
HEADER_PATH = os.path.normpath(os.path.join(_HERE, '..', '..', 'include', 'ams_spk_count.h'))
ABI_VERSION = 1            # include/ams_spk_count.h: ams_spkc_abi_version()

_vp = ctypes.c_void_p
_lib = None
LAUNCHES = 0               # kernel launches made through this module so far (ams_spkc_score is two, the other entry points one each)


def load():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise AmsError('libams_spk_count.so not found at %s -- the HIP extension is required (no CPU fallback); '
                       'run __graft_entry__.build()' % LIB_PATH)
    lib = ctypes.CDLL(LIB_PATH)             # (torch is imported above: one HIP runtime in the process, see _lib.load)
    for name, (ret, argtypes) in parse_header(HEADER_PATH).items():
        try:
            fn = getattr(lib, name)
        except AttributeError:
            raise AmsError('libams_spk_count.so does not export %s (declared in include/ams_spk_count.h)' % name)
        fn.restype = ret
        fn.argtypes = argtypes
    if lib.ams_spkc_abi_version() != ABI_VERSION:
        raise AmsError('libams_spk_count.so ABI version mismatch: the library is %d, this binding is %d -- rebuild (make -C csrc)'
                       % (lib.ams_spkc_abi_version(), ABI_VERSION))
    _lib = lib
    return lib


def _p(t):
    return _vp(t.data_ptr()) if t is not None else _vp(0)


def _s():
    return _vp(torch.cuda.current_stream().cuda_stream)


def _launch(status, what, n=1):
    global LAUNCHES
    check(status, what)
    LAUNCHES += n


def parse_speakers(speakers, S):
    """'auto' -> (2, S); (lo, hi) or 'LO:HI' -> (lo, hi) as ints.  ValueError for anything else."""
    if isinstance(speakers, str):
        if speakers == 'auto':
            return 2, int(S)
        parts = speakers.split(':')
        if len(parts) != 2 or not all(p.strip().lstrip('-').isdigit() for p in parts):
            raise ValueError("speakers: 'auto' or LO:HI, got %r" % (speakers,))
        return int(parts[0]), int(parts[1])
    try:
        lo, hi = speakers
        if int(lo) != lo or int(hi) != hi:
            raise TypeError
    except (TypeError, ValueError):
        raise ValueError("speakers: 'auto' or a pair (lo, hi) of integers, got %r" % (speakers,))
    return int(lo), int(hi)


def check_range(lo, hi, S, min_score, E=None):
    """The refusals of a range of counts, before anything is uploaded: 1 <= lo <= hi <= S (the model's number of mask columns), lo == 1
    only with a min_score, every candidate (E, C) a pair the kernels exist for.  Returns (c_lo, ncand), c_lo = max(lo, 2)."""
    lo, hi, S = int(lo), int(hi), int(S)
    if lo < 1:
        raise ValueError('speakers: lo >= 1, got (%d, %d)' % (lo, hi))
    if lo > hi:
        raise ValueError('speakers: lo <= hi, got (%d, %d)' % (lo, hi))
    if hi > S:
        raise ValueError('speakers: hi = %d is above the %d tracks the model was built for' % (hi, S))
    if lo == 1 and min_score is None:
        raise ValueError('speakers: lo == 1 needs a min_score (the score below which a recording counts as one speaker): '
                         'none is built in, the criterion has not been measured on a trained model')
    if min_score is not None and not np.isfinite(float(min_score)):
        raise ValueError('min_score: a finite number, got %r' % (min_score,))
    c_lo = max(lo, 2)
    if hi < 2:
        raise ValueError('speakers: hi >= 2 (a range of (1, 1) has no candidate to score), got (%d, %d)' % (lo, hi))
    if E is not None:
        for C in range(c_lo, hi + 1):
            Kr.check_domain(E, C)
    return c_lo, hi - c_lo + 1


def score(xn, p_off, cents, inertias, c_lo, tries, w=None):
    """xn [Ptot, E] normalised points, cents[k] [R tries, c_lo + k, E] and inertias[k] [R tries] of every try of candidate k (what
    kmeans_ragged_tries returns), w [Ptot] or None -> (score float64 [R, ncand], tries int32 [R, ncand], sel: a list of [R, c_lo + k, E]).
    Two launches."""
    seg = Kr.segments(p_off)
    c_lo, tries, ncand = int(c_lo), int(tries), len(cents)
    c_hi = c_lo + ncand - 1
    if not torch.is_tensor(xn) or xn.dim() != 2 or xn.shape[0] != seg.Ptot:
        raise ValueError('cluster scores: the points are a [Ptot, E] = [%d, E] tensor' % seg.Ptot)
    E = int(xn.shape[1])
    if ncand < 1 or len(inertias) != ncand or tries < 1:
        raise ValueError('cluster scores: one centroid set and one inertia row per candidate, tries >= 1')
    for k in range(ncand):
        Kr.check_domain(E, c_lo + k)
        if tuple(cents[k].shape) != (seg.R * tries, c_lo + k, E) or tuple(inertias[k].shape) != (seg.R * tries,):
            raise ValueError('cluster scores: candidate %d: centroids [%d, %d, %d] and inertia [%d], got %s and %s'
                             % (c_lo + k, seg.R * tries, c_lo + k, E, seg.R * tries, tuple(cents[k].shape), tuple(inertias[k].shape)))
    if w is not None and (not torch.is_tensor(w) or tuple(w.shape) != (seg.Ptot,)):
        raise ValueError('cluster scores: the weights are a [Ptot] = [%d] tensor' % seg.Ptot)
    ops._chk(xn, w, *cents)
    ops._chk(*inertias)
    lib, dev = load(), xn.device
    t = seg.tables(dev)
    cent_all = torch.cat([c.reshape(-1) for c in cents])
    inertia_all = torch.cat([i.reshape(-1) for i in inertias])
    nb = lib.ams_spkc_workspace_bytes(seg.R, seg.Gtot, E, c_lo, c_hi)
    ws = torch.empty((nb + 7) // 8, dtype=torch.float64, device=dev)
    sc = torch.empty((seg.R, ncand), dtype=torch.float64, device=dev)
    tr = torch.empty((seg.R, ncand), dtype=torch.int32, device=dev)
    sizes = [seg.R * (c_lo + k) * E for k in range(ncand)]
    sel_all = torch.empty(sum(sizes), dtype=torch.float32, device=dev)
    _launch(lib.ams_spkc_score(_p(xn), _p(w), _p(t['tab']), _p(t['p_off']), _p(t['g_off']), _p(cent_all), _p(inertia_all), seg.R, tries,
                               seg.Gtot, E, c_lo, c_hi, _p(ws), nb, _p(sc), _p(tr), _p(sel_all), _s()), 'ams_spkc_score', 2)
    sel = [v.view(seg.R, c_lo + k, E) for k, v in enumerate(torch.split(sel_all, sizes))]
    return sc, tr, sel


def choose(sc, sel, lo, c_lo, min_score=None):
    """score [R, ncand], sel as score() returns it -> (count int32 [R], cand int32 [R], centroids [R, c_hi, E]: rows >= count zero).
    One launch."""
    R, ncand = sc.shape
    c_hi, E = int(c_lo) + ncand - 1, int(sel[0].shape[2])
    dev = sc.device
    sel_all = torch.cat([v.reshape(-1) for v in sel])
    count = torch.empty(R, dtype=torch.int32, device=dev)
    cand = torch.empty(R, dtype=torch.int32, device=dev)
    chosen = torch.empty((R, c_hi, E), dtype=torch.float32, device=dev)
    ms = None if min_score is None else ctypes.c_double(float(min_score))
    _launch(load().ams_spkc_choose(_p(sc), _p(sel_all), R, E, int(lo), int(c_lo), c_hi, None if ms is None else ctypes.addressof(ms),
                                   _p(count), _p(cand), _p(chosen), _s()), 'ams_spkc_choose')
    return count, cand, chosen


def merge_labels(labels_all, cand, p_off, c_lo):
    """labels_all int32 [ncand, Ptot] (row k: ams_kmr_labels on candidate k's selected centroids), cand [R] -> labels int32 [Ptot]: every
    segment's are those of its chosen candidate, 0 for candidate -1 (one cluster).  One launch."""
    seg = Kr.segments(p_off)
    ncand = int(labels_all.shape[0])
    t = seg.tables(labels_all.device)
    labels = torch.empty(seg.Ptot, dtype=torch.int32, device=labels_all.device)
    _launch(load().ams_spkc_labels(_p(labels_all), _p(cand), _p(t['tab']), _p(t['p_off']), seg.R, seg.Gtot, seg.Ptot, int(c_lo),
                                   int(c_lo) + ncand - 1, _p(labels), _s()), 'ams_spkc_labels')
    return labels


def count_clusters(x, p_off, init_idx, lo, hi, tries, iterations, w=None, assign_at_end=True, normalize_input=True, min_score=None):
    """x [Ptot, E] float32 on the device, p_off: a Segments or the sizes P_r, init_idx: HOST integers [R tries, >= hi] relative to each
    segment (candidate C takes the first C columns), w [Ptot] or None ->
        {'count' int32 [R], 'cand' int32 [R] (count - max(lo, 2), or -1 for one cluster), 'scores' float64 [R, ncand],
         'tries' int32 [R, ncand], 'centroids' [R, hi, E] (rows >= count zero), 'labels' int32 [Ptot], 'c_lo',
         'sel': per candidate the selected centroids [R, C, E]}
    ncand (iterations + 3) + 4 launches after the normalisation, no host synchronisation."""
    seg = Kr.segments(p_off)
    lo, hi, tries = int(lo), int(hi), int(tries)
    if not torch.is_tensor(x) or x.dim() != 2:
        raise ValueError('cluster count: the points are a [Ptot, E] tensor')
    c_lo, ncand = check_range(lo, hi, hi, min_score, int(x.shape[1]))
    idx = init_idx.detach().cpu().numpy() if torch.is_tensor(init_idx) else np.asarray(init_idx)
    if idx.ndim != 2 or idx.shape[0] != seg.R * tries or idx.shape[1] < hi:
        raise ValueError('cluster count: init_idx must be integers of shape [R tries, >= hi] = [%d, >= %d], got %s'
                         % (seg.R * tries, hi, idx.shape))
    seeds = [Kr.check_seeds(np.ascontiguousarray(idx[:, :c_lo + k]), seg, tries, c_lo + k) for k in range(ncand)]      # all before a launch
    ops._chk(x, w)
    xn = ops.kmeans_normalize(x) if normalize_input else x
    cents, inertias = [], []
    for k in range(ncand):
        c, i = Kr.kmeans_ragged_tries(xn, seg, seeds[k], c_lo + k, tries, iterations, w=w, normalize_input=False)
        cents.append(c)
        inertias.append(i)
    return count_from_tries(xn, seg, cents, inertias, lo, tries, w=w, assign_at_end=assign_at_end, min_score=min_score)


def count_from_tries(xn, p_off, cents, inertias, lo, tries, w=None, assign_at_end=True, min_score=None):
    """The second half of count_clusters, on every try's centroids and inertias of every candidate max(lo, 2) + k as
    kmeans_ragged_tries returns them: score, choose, the labels of every candidate and their merge.  ncand + 4 launches."""
    seg = Kr.segments(p_off)
    c_lo, ncand = max(int(lo), 2), len(cents)
    sc, tr, sel = score(xn, seg, cents, inertias, c_lo, tries, w)
    count, cand, chosen = choose(sc, sel, lo, c_lo, min_score)
    labels_all = torch.empty((ncand, seg.Ptot), dtype=torch.int32, device=xn.device)
    for k in range(ncand):
        Kr.labels_ragged(xn, seg, sel[k], None if assign_at_end else w, out=labels_all[k])
    labels = merge_labels(labels_all, cand, seg, c_lo)
    return {'count': count, 'cand': cand, 'scores': sc, 'tries': tr, 'centroids': chosen, 'labels': labels, 'c_lo': c_lo, 'sel': sel}
