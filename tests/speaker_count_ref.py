"""Numpy float64 restatement of the choice of the number of speakers per recording (include/ams_spk_count.h), in the
manner of tests/stitch_ref.py: the definition the kernels of libams_spk_count.so and ams_hip/spk_count.py are tested against.  Test
infrastructure only.

Per recording: normalised float32 points x [P, E], weights w [P] (None: ones), a range lo <= hi.  Candidates C = max(lo, 2) .. hi; for
each the hard k-means of oracle/kmeans.py with the first C columns of the seed rows [tries, >= hi]; the try of a candidate is the FIRST
one with the smallest FINITE inertia (pick_try); its score is the simplified silhouette (score); the count is the candidate with the
largest score, the first maximum (choose).
"""
import numpy as np

from oracle import kmeans as okm


def planted(count, P, E, seed, noise=0.1):
    """The planted family: `count` centres on the unit sphere, P points = a centre + noise N(0, I) / sqrt(E), renormalised; float32."""
    rng = np.random.RandomState(seed)
    centres = rng.randn(count, E)
    centres /= np.linalg.norm(centres, axis=1, keepdims=True)
    x = centres[rng.randint(0, count, P)] + noise * rng.randn(P, E) / np.sqrt(E)
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    return x.astype(np.float32)


def draw_seeds(P, tries, hi, seed):
    """[tries, hi] distinct point indices per row."""
    rng = np.random.RandomState(seed)
    return np.stack([rng.choice(P, hi, replace=False) for _ in range(tries)]).astype(np.int32)


def every_try(x, w, seeds, C, iterations):
    """oracle/kmeans.py's hard k-means on ALREADY normalised points for every seed row: (centroids [tries, C, E], inertia [tries]),
    float32."""
    x = np.asarray(x, np.float32)
    w = np.ones(x.shape[0], np.float32) if w is None else np.asarray(w, np.float32)
    cents, inert = [], []
    for row in np.asarray(seeds)[:, :C]:
        cent = x[row]
        lab = okm.labels_hard(x, cent, w)
        for _ in range(iterations):
            cent = okm.update_hard(x, w, lab, C)
            lab = okm.labels_hard(x, cent, w)
        cents.append(cent)
        with np.errstate(invalid='ignore'):
            inert.append(okm.inertia_hard(x, cent, w))
    return np.stack(cents), np.asarray(inert, np.float32)


def pick_try(inertia):
    """The first try with the smallest finite inertia; -1 if no try is finite."""
    best = -1
    for t, v in enumerate(np.asarray(inertia)):
        if np.isfinite(v) and (best < 0 or v < inertia[best]):
            best = t
    return best


def select_try(inertia):
    """kmeans_ragged's own selection: np.argmin, which takes the first NaN."""
    return int(np.argmin(np.asarray(inertia)))


def score(x, w, cent):
    """sum w s / sum w, s = (d2 - d1) / d2 with d1 <= d2 the two smallest distances sqrt(sum_e (x_e - c_e)^2), s = 0 where d2 == 0.
    float64 on the float32 inputs; -inf where sum w == 0."""
    x = np.asarray(x, np.float32).astype(np.float64)
    cent = np.asarray(cent, np.float32).astype(np.float64)
    w = np.ones(x.shape[0]) if w is None else np.asarray(w, np.float32).astype(np.float64)
    if w.sum() == 0:
        return -np.inf
    total = 0.0
    for a in range(0, x.shape[0], 4096):
        diff = x[a:a + 4096, None, :] - cent[None]
        d = np.sort(np.sqrt((diff * diff).sum(axis=2)), axis=1)
        d1, d2 = d[:, 0], d[:, 1]
        s = np.where(d2 == 0, 0.0, (d2 - d1) / np.where(d2 == 0, 1.0, d2))
        total += float((w[a:a + 4096] * s).sum())
    return total / float(w.sum())


def scores_of(x, w, cents, inertias):
    """cents[k] [tries, C_k, E], inertias[k] [tries] -> (scores [ncand] float64, tries [ncand]); a disqualified candidate: -inf, -1."""
    sc, tr = [], []
    for cent, inertia in zip(cents, inertias):
        t = pick_try(inertia)
        tr.append(t)
        sc.append(-np.inf if t < 0 else score(x, w, cent[t]))
    return np.asarray(sc, np.float64), np.asarray(tr, np.int32)


def choose(scores, lo, min_score=None):
    """-> (count, candidate): the first maximum; count 1 (candidate -1) if lo == 1 and the best score is below min_score or every
    candidate is disqualified; max(lo, 2) (candidate 0) if lo >= 2 and every candidate is disqualified."""
    if lo == 1 and min_score is None:
        raise ValueError('lo == 1 needs a min_score')
    c_lo = max(lo, 2)
    scores = np.asarray(scores, np.float64)
    k = int(np.argmax(scores))
    if scores[k] == -np.inf:
        return (1, -1) if lo == 1 else (c_lo, 0)
    if lo == 1 and scores[k] < min_score:
        return 1, -1
    return c_lo + k, k


def margin(scores):
    """The best score minus the runner-up's (inf with one candidate or a disqualified runner-up)."""
    s = np.sort(np.asarray(scores, np.float64))[::-1]
    return np.inf if s.size < 2 or s[1] == -np.inf else float(s[0] - s[1])


def count(x, w, seeds, lo, hi, iterations, min_score=None, cents=None, inertias=None):
    """The whole definition for one recording -> dict(count, cand, scores, tries, centroids [hi, E] (rows >= count zero), sel).  cents /
    inertias: every try of every candidate if they are at hand (the device's), else oracle/kmeans.py's."""
    c_lo = max(lo, 2)
    if cents is None:
        runs = [every_try(x, w, seeds, C, iterations) for C in range(c_lo, hi + 1)]
        cents, inertias = [r[0] for r in runs], [r[1] for r in runs]
    sc, tr = scores_of(x, w, cents, inertias)
    n, cd = choose(sc, lo, min_score)
    sel = [cent[t if t >= 0 else select_try(inertia)] for cent, inertia, t in zip(cents, inertias, tr)]
    chosen = np.zeros((hi, np.asarray(x).shape[1]), np.float32)
    if cd >= 0:
        chosen[:n] = sel[cd]
    return {'count': n, 'cand': cd, 'scores': sc, 'tries': tr, 'centroids': chosen, 'sel': sel}
