"""numpy restatement of the whole-recording stitcher (include/ams_stitch.h) and a generator of test material.

The reference project has no counterpart of this feature: the GPU tests compare libams_stitch.so with THIS module.  A plain helper
module like tests/fenced.py: no pytest hooks, no fixtures.

    nb_chunks, chunks                 the chunk arithmetic and the zero-padded gather
    border_stats                      Q in float64
    search                            the border permutations with the tie and NaN rules, and the margin of every border
    tracks                            the composition of the border permutations
    overlap_add                       the cross-fade in float32 with exactly the contract's arithmetic
    material                          S random sources, chunked, every chunk's sources permuted, a little noise per chunk
"""
from itertools import permutations

import numpy as np


def nb_chunks(N, L, H):
    assert N >= 1 and 2 <= L and (L + 1) // 2 <= H <= L - 1
    return 1 + max(0, -((L - N) // H))


def chunks(x, L, H):
    """x [N] -> [C, L]: chunk c starts at c H; zero past the end."""
    x = np.asarray(x)
    N = x.shape[0]
    C = nb_chunks(N, L, H)
    pad = np.zeros((C - 1) * H + L, x.dtype)
    pad[:N] = x
    return np.stack([pad[c * H:c * H + L] for c in range(C)])


def border_stats(est, H):
    """est [C, S, L] -> Q [C - 1, S, S] float64: Q[c, i, j] = sum_v (est[c, i, H + v] - est[c + 1, j, v])^2."""
    est = np.asarray(est, np.float64)
    C, S, L = est.shape
    V = L - H
    tail, head = est[:-1, :, H:], est[1:, :, :V]
    d = tail[:, :, None, :] - head[:, None, :, :]
    return (d * d).sum(axis=-1)


def perm_table(S):
    return np.array(list(permutations(range(S))), np.int32)


def search(Q):
    """Q [C - 1, S, S] -> (rel [C - 1, S] int32, margin [C - 1]).  The cost of permutation p is sum_s Q[c, s, p(s)], added in s order
    in Q's precision; costs are compared with <, the lowest index wins among equals, a NaN cost never wins, all NaN -> index 0.
    margin = (second - best) / second over the non-NaN costs: 1 where there is one permutation only, 0 where that is not defined
    (fewer than two non-NaN costs, or a second-best cost that is not positive)."""
    Q = np.asarray(Q)
    nb, S, _ = Q.shape
    perms = perm_table(S)
    rel = np.zeros((nb, S), np.int32)
    margin = np.zeros(nb)
    for c in range(nb):
        cost = np.zeros(len(perms), Q.dtype)
        with np.errstate(invalid='ignore', over='ignore'):
            for s in range(S):
                cost = (cost + Q[c, s, perms[:, s]]).astype(Q.dtype)
        best = -1
        for p in range(len(perms)):
            if cost[p] != cost[p]:
                continue
            if best < 0 or cost[p] < cost[best]:
                best = p
        rel[c] = perms[max(best, 0)]
        valid = np.sort(cost[~np.isnan(cost)].astype(np.float64))
        if len(perms) == 1:
            margin[c] = 1.0
        elif len(valid) >= 2 and valid[1] > 0 and np.isfinite(valid[1]):
            margin[c] = (valid[1] - valid[0]) / valid[1]
    return rel, margin


def tracks(rel):
    """rel [C - 1, S] -> trk [C, S]: trk[0, k] = k, trk[c + 1, k] = rel[c][trk[c, k]]."""
    rel = np.asarray(rel)
    nb, S = rel.shape
    trk = np.zeros((nb + 1, S), np.int32)
    trk[0] = np.arange(S)
    for c in range(nb):
        trk[c + 1] = rel[c][trk[c]]
    return trk


def w_head(V):
    return ((np.arange(V, dtype=np.float64) + 0.5) / V).astype(np.float32)


def overlap_add(est, trk, N, H):
    """est [C, S, L] float32, trk [C, S] -> out [S, N] float32: fl(w_tail * tail) + fl(w_head * head) on the overlaps with
    w_tail = fl(1 - w_head), a copy elsewhere.  Every operation is a float32 numpy operation: one rounding each, no FMA."""
    est = np.asarray(est, np.float32)
    C, S, L = est.shape
    V = L - H
    assert C == nb_chunks(N, L, H)
    wh = w_head(V)
    wt = (np.float32(1.0) - wh).astype(np.float32)
    n = np.arange(N, dtype=np.int64)
    c1 = np.minimum(n // H, C - 1)
    p = n - c1 * H
    fade = (c1 > 0) & (p < V)
    out = np.empty((S, N), np.float32)
    c0 = np.maximum(c1 - 1, 0)
    pf = np.where(fade, p, 0)
    for k in range(S):
        cur = est[c1, trk[c1, k], p]
        with np.errstate(invalid='ignore'):
            a = (wt[pf] * est[c0, trk[c0, k], H + pf]).astype(np.float32)
            b = (wh[pf] * cur).astype(np.float32)
            out[k] = np.where(fade, (a + b).astype(np.float32), cur)
    return out


def material(seed, S, L, H, N, noise=1e-3):
    """(src [S, N], est [C, S, L], perm [C, S], truth [C, S]).  est[c, perm[c, s]] = chunk c of source s (+ noise * randn): perm[c] is
    where chunk c put each source, so truth[c, k] = perm[c][inverse(perm[0])[k]] is the output of chunk c that continues output k of
    chunk 0 -- what tracks() must return."""
    rng = np.random.RandomState(seed)
    src = rng.randn(S, N).astype(np.float32)
    C = nb_chunks(N, L, H)
    cut = np.stack([chunks(src[s], L, H) for s in range(S)], axis=1)          # [C, S, L]
    est = np.empty_like(cut)
    perm = np.zeros((C, S), np.int32)
    for c in range(C):
        perm[c] = rng.permutation(S)
        est[c, perm[c]] = cut[c]
    if noise:
        est = (est + np.float32(noise) * rng.randn(C, S, L).astype(np.float32)).astype(np.float32)
    inv0 = np.argsort(perm[0])
    truth = perm[:, inv0].astype(np.int32)
    return src, est, perm, truth
