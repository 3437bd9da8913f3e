"""The float64 reference of the ragged soft k-means tests and their input recipe (a plain helper module: no tests, no fixtures).

soft_reference restates, per try, what oracle/kmeans.py::kmeans(X[None], idx, C, tries, iterations, beta=...) computes for ONE segment as
a batch of one, from the oracle's own functions (l2_normalize_rows, labels_soft, update_soft, inertia_soft) in the dtype asked for, and
keeps what the oracle's return value drops: the centroids and the inertia of EVERY try.  tests/test_kmeans_ragged_soft_host.py holds it
equal to the oracle."""
import numpy as np

from oracle import kmeans as okm

SEGS = [37, 64, 197, 3000, 8192, 8193, 16384 + 130]     # below a slab, a slab, ragged, a short chunk, one chunk to the point, one over, three chunks
TRIES, ITERS = 5, 3
_SEG, _REF = {}, {}


def segment(P, E, C):
    """One segment's blobs, ten rows of seeds, a 0/1 mask and real weights, all drawn in float64 from RandomState(P + 7 E + C) in this
    order; made once.  -> (X float64 [P, E], idx int32 [10, C], {'mask': w, 'real': w} float64 [P])."""
    key = (P, E, C)
    if key not in _SEG:
        rng = np.random.RandomState(P + 7 * E + C)
        centers = rng.randn(C, E) * 1.5
        X = centers[rng.randint(0, C, P)] + rng.randn(P, E) * 0.8
        idx = np.stack([rng.choice(P, C, replace=False) for _ in range(10)]).astype(np.int32)
        mask = (rng.rand(P) > 0.25).astype(np.float64)
        real = rng.uniform(0.05, 1.7, P)
        _SEG[key] = (X, idx, {'mask': mask, 'real': real, 'zero': np.zeros(P)})
    return _SEG[key]


def weights(P, E, C, kind):
    return None if kind is None else segment(P, E, C)[2][kind]


class Ref(object):
    """cents [tries, C, E], inertia [tries], best, gap = (second lowest inertia - lowest) / lowest, xn, w (ones without weights), beta"""

    def masks(self, t, assign_at_end):
        """The soft labels [P, C] of try t's centroids: without the weights (assign_at_end) or with the run's."""
        return okm.labels_soft(self.xn, self.cents[t], np.ones_like(self.w) if assign_at_end else self.w, self.beta)


def soft_reference(X, idx, C, tries, iterations, beta, w=None, dtype=np.float64):
    """X [P, E] and w [P] (or None) as the DEVICE gets them (float32 values), computed in `dtype`."""
    X = np.asarray(X).astype(dtype)
    r = Ref()
    r.beta = beta
    r.xn = okm.l2_normalize_rows(X)
    r.w = np.ones(X.shape[0], dtype) if w is None else np.asarray(w).astype(dtype)
    r.cents = np.zeros((tries, C, X.shape[1]), dtype)
    r.inertia = np.zeros(tries, dtype)
    for t in range(tries):
        cent = r.xn[idx[t]]
        lab = okm.labels_soft(r.xn, cent, r.w, beta)
        for _ in range(iterations):
            cent = okm.update_soft(r.xn, r.w, lab)
            lab = okm.labels_soft(r.xn, cent, r.w, beta)
        r.cents[t] = cent
        r.inertia[t] = okm.inertia_soft(r.xn, cent, r.w, beta)
    r.best = int(np.argmin(r.inertia))
    srt = np.sort(r.inertia)
    r.gap = float((srt[1] - srt[0]) / srt[0]) if tries > 1 else float('inf')
    return r


def reference(P, E, C, beta, kind, dtype=np.float64, tries=TRIES, iterations=ITERS):
    """soft_reference on the recipe's segment, its first `tries` seed rows and its weights of `kind` (None | 'mask' | 'real' | 'zero'),
    all cast to float32 first, as the device gets them; computed once and never modified."""
    key = (P, E, C, beta, kind, np.dtype(dtype).name, tries, iterations)
    if key not in _REF:
        X, idx, _ = segment(P, E, C)
        w = weights(P, E, C, kind)
        _REF[key] = soft_reference(X.astype(np.float32), idx[:tries], C, tries, iterations, beta, None if w is None else w.astype(np.float32), dtype)
    return _REF[key]
