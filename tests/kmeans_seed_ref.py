"""The restatement of the k-means++ (D^2) seeding of include/ams_kmeans_seed.h for ONE segment, in numpy: the distance
is oracle.kmeans.sqdist, the sampling weights are integers and every sum is a Python / np.uint64 integer, so nothing here depends on an
order of addition.  A plain helper module: no tests, no fixtures."""
import numpy as np

from oracle import kmeans as OK

SHIFT = 20                      # quant(v) = trunc(min(v, 2048) 2^20)
CAP = np.float32(2048.0)


def quant(v):
    """float32 [L] -> uint64 [L]: 0 for a NaN or v <= 0, else the truncation of min(v, 2048) 2^20 (exact: a power of two)."""
    v = np.asarray(v, np.float32)
    ok = v > 0                                  # (False for a NaN)
    with np.errstate(invalid='ignore'):
        s = np.where(ok, np.minimum(v, CAP), np.float32(0)) * np.float32(1 << SHIFT)
    return s.astype(np.uint64)


def weights(x, chosen, w=None):
    """q [L] uint64 of the step that follows the seeds `chosen` (step 0: none)."""
    L = x.shape[0]
    if not len(chosen):
        return quant(np.ones(L, np.float32) if w is None else w)
    ww = np.ones(L, np.float32) if w is None else np.asarray(w, np.float32)
    with np.errstate(invalid='ignore', over='ignore'):
        d = OK.sqdist(x, x[np.asarray(chosen, np.int64)], ww)     # [L, c]: point i to seed s under the weight of point i
    return np.stack([quant(d[:, j]) for j in range(d.shape[1])], axis=1).min(axis=1)


def pick(q, u, chosen):
    """The seed for the weights q, the draw u (0 .. 2^64 - 1) and the seeds chosen so far."""
    cum = np.cumsum(q.astype(np.uint64), dtype=np.uint64)
    total = int(cum[-1])
    if total == 0:
        used = set(int(s) for s in chosen)
        return min(i for i in range(len(chosen) + 1) if i not in used)
    target = (int(u) * total) >> 64
    return int(np.searchsorted(cum, np.uint64(target), side='right'))       # the smallest i with cum[i] > target


def seed_try(x, u, w=None):
    """x [L, E] float32 (normalised), u [C] draws -> the C seeds of one try."""
    chosen = []
    for c in range(len(u)):
        chosen.append(pick(weights(x, chosen, w), u[c], chosen))
    return chosen


def seed_segment(x, draws, w=None):
    """x [L, E] float32, draws uint64 [tries, C], w [L] or None -> seeds int32 [tries, C]."""
    x = np.ascontiguousarray(x, np.float32)
    draws = np.asarray(draws)
    assert draws.dtype == np.uint64 and draws.ndim == 2 and x.shape[0] >= draws.shape[1]
    return np.array([seed_try(x, [int(v) for v in row], w) for row in draws], np.int32).reshape(draws.shape)


def seed_segments(x, sizes, draws, w=None):
    """The segments of x [Ptot, E] one after the other, draws [R tries, C] -> seeds int32 [R tries, C]."""
    R = len(sizes)
    tries = draws.shape[0] // R
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    return np.concatenate([seed_segment(x[off[r]:off[r + 1]], draws[r * tries:(r + 1) * tries], None if w is None else w[off[r]:off[r + 1]])
                           for r in range(R)])
