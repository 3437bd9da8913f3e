"""Numpy restatement of the ragged BSS-eval's definition (include/ams_bss_ragged.h) -- test infrastructure only.

oracle/bss_eval.py's arithmetic without the FFT: linear correlations by lag, time cut into blocks of AMS_BSSR_BLOCK samples with the
block partials added in block order, the Gram layout of gram_kernel / rhs_kernel, FIR projections, the five sums per block.  It ties
the time-domain definition to the pinned oracle on the CPU; the order of the additions INSIDE a block is numpy's, not the kernels'.
"""
import numpy as np

BLOCK = 4096        # include/ams_bss_ragged.h: AMS_BSSR_BLOCK


def nblocks(L, flen, block=BLOCK):
    return (L + flen - 1 + block - 1) // block


def corr(x, y, flen, block=BLOCK):
    """u(x, y)[m] = sum_t x[t] y[t + m], m = 0 .. flen - 1; samples outside 0 .. L - 1 are zero; one partial per block of t."""
    L = x.shape[0]
    yp = np.concatenate([y, np.zeros(flen + block)])
    xp = np.concatenate([x, np.zeros(flen + block)])
    out = np.zeros(flen)
    for b in range(nblocks(L, flen, block)):
        t0 = b * block
        part = np.array([np.dot(xp[t0:t0 + block], yp[t0 + m:t0 + block + m]) for m in range(flen)])
        out = out + part
    return out


def gram(refs, flen, block=BLOCK):
    """G [S F, S F]: block (i, j) element [a, b] = rr_ij[b - a], rr_ij[m] = sum_t ref_i[t + m] ref_j[t]; every ordered pair once."""
    S = refs.shape[0]
    u = [[corr(refs[a], refs[b], flen, block) for b in range(S)] for a in range(S)]          # u[a][b] = u(ref_a, ref_b)
    k = np.arange(flen)
    d = k[None, :] - k[:, None]                                                              # b - a
    G = np.empty((S * flen, S * flen))
    for i in range(S):
        for j in range(S):
            G[i * flen:(i + 1) * flen, j * flen:(j + 1) * flen] = np.where(d >= 0, u[j][i][np.abs(d)], u[i][j][np.abs(d)])
    return G


def fir(c, x, n):
    """P[t] = sum_k c[k] x[t - k], t = 0 .. n - 1."""
    return np.convolve(c, x)[:n]


def bss_eval_pairs(refs, ests, flen, block=BLOCK):
    """refs [S, L], ests [K, S, L] -> (crit [K, 3, S, S] with crit[k][c][jest][jtrue], info)."""
    refs, ests = np.asarray(refs, np.float64), np.asarray(ests, np.float64)
    S, L = refs.shape
    ests = ests.reshape(-1, S, L)
    K = ests.shape[0]
    rows = ests.reshape(K * S, L)
    Lp = L + flen - 1
    G = gram(refs, flen, block)
    crit = np.full((K, 3, S, S), np.nan)
    try:
        np.linalg.cholesky(G)
        for j in range(S):
            np.linalg.cholesky(G[j * flen:(j + 1) * flen, j * flen:(j + 1) * flen])
    except np.linalg.LinAlgError:
        return crit, 1
    D = np.stack([np.concatenate([corr(refs[i], rows[e], flen, block) for i in range(S)]) for e in range(K * S)])      # Df[e][i F + k]
    Cf = np.linalg.solve(G, D.T).T
    pad = np.zeros(flen - 1)
    for e in range(K * S):
        pf = sum(fir(Cf[e, i * flen:(i + 1) * flen], refs[i], Lp) for i in range(S))
        ev = np.concatenate([rows[e], pad])
        for j in range(S):
            blk = slice(j * flen, (j + 1) * flen)
            cj = np.linalg.solve(G[blk, blk], D[e, blk])
            pj = fir(cj, refs[j], Lp)
            s_true = np.concatenate([refs[j], pad])
            e_spat = pj - s_true
            e_interf = pf - s_true - e_spat
            e_artif = -s_true - e_spat - e_interf + ev
            s_filt = s_true + e_spat
            terms = [s_filt ** 2, (e_interf + e_artif) ** 2, e_interf ** 2, (s_filt + e_interf) ** 2, e_artif ** 2]
            s = np.zeros(5)
            for b in range(nblocks(L, flen, block)):                                         # one row of five per block, added in order
                s = s + np.array([t[b * block:(b + 1) * block].sum() for t in terms])
            db = lambda num, den: 10.0 * np.log10(num / (den + 1e-12))                       # noqa: E731
            crit[e // S, :, e % S, j] = db(s[0], s[1]), db(s[0], s[2]), db(s[3], s[4])
    return crit, 0
