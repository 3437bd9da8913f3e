"""The definition of the ragged SI-SDR scoring (include/ams_sisdr.h) restated in numpy float64 -- test infrastructure only.
The reference project has no counterpart: parity of libams_sisdr.so is against this file.

    si_sdr(e, s)                       one estimate against one reference
    score(refs, sets, mixture)         one recording: refs [Sr, L], sets: a list of K arrays [Se_k, L], mixture [L]
    score_many(refs, ests, mixtures)   the outputs of utils.bss_eval.si_sdr_ragged, recording by recording
    gap(pair, Se, Sr)                  best minus second-best assignment, in mean dB over the pairs

The arithmetic is the direct one: means removed from the signals, then inner products."""
import itertools

import numpy as np

MAXS = 6


def centred(x, zero_mean=True):
    x = np.asarray(x, np.float64)
    return x - x.mean(axis=-1, keepdims=True) if zero_mean else x


def si_sdr_centred(e, s):
    g, ee, ss = float(np.dot(e, s)), float(np.dot(e, e)), float(np.dot(s, s))
    if not ss > 0.0:
        return np.nan                               # a silent reference
    if not ee > 0.0:
        return -np.inf                              # a silent estimate
    den = ss * ee - g * g
    if den <= 0.0:
        return np.inf if g != 0.0 else -np.inf
    if g == 0.0:
        return -np.inf
    return 10.0 * np.log10(g * g / den)


def si_sdr(e, s, zero_mean=True):
    return si_sdr_centred(centred(e, zero_mean), centred(s, zero_mean))


def candidates(Se, Sr):
    """The assignments in the order they are tried: the estimate of every reference if Se >= Sr, else the reference of every estimate."""
    return list(itertools.permutations(range(Se), Sr)) if Se >= Sr else list(itertools.permutations(range(Sr), Se))


def values(pair, Se, Sr):
    """The sum of si_sdr over the pairs of every candidate, added from 0.0 in tuple order."""
    out = []
    for t in candidates(Se, Sr):
        v = 0.0
        for q, w in enumerate(t):
            v = v + (pair[w, q] if Se >= Sr else pair[q, w])
        out.append(v)
    return out


def match(pair, Se, Sr):
    """pair [6, 6] (estimate, reference) -> (match_ref [6], match_est [6]): the first candidate leads, a later one takes the lead only
    with a value that compares greater (so a NaN never does)."""
    cand, vals = candidates(Se, Sr), values(pair, Se, Sr)
    best = 0
    for c in range(1, len(cand)):
        if vals[c] > vals[best]:
            best = c
    mr, me = np.full(MAXS, -1, np.int32), np.full(MAXS, -1, np.int32)
    for q, w in enumerate(cand[best]):
        if Se >= Sr:
            mr[q], me[w] = w, q
        else:
            me[q], mr[w] = w, q
    return mr, me


def gap(pair, Se, Sr):
    """Best minus second-best candidate value over min(Se, Sr) pairs (dB in mean); inf with one candidate."""
    v = sorted(values(pair, Se, Sr), reverse=True)
    return np.inf if len(v) < 2 else (v[0] - v[1]) / min(Se, Sr)


def score(refs, sets, mixture, zero_mean=True):
    refs = centred(refs, zero_mean)
    Sr = refs.shape[0]
    x = centred(mixture, zero_mean)
    base = np.full(MAXS, np.nan)
    info = 0
    for j in range(Sr):
        base[j] = si_sdr_centred(x, refs[j])
        if not float(np.dot(refs[j], refs[j])) > 0.0:
            info |= 1
    K = len(sets)
    out = dict(pair=np.full((K, MAXS, MAXS), np.nan), match_ref=np.full((K, MAXS), -1, np.int32), match_est=np.full((K, MAXS), -1, np.int32),
               si_sdr=np.full((K, MAXS), np.nan), si_sdri=np.full((K, MAXS), np.nan), missed=np.zeros(K, np.int32),
               spurious=np.zeros(K, np.int32), base=base, info=np.int32(info))
    for k, est in enumerate(sets):
        est = centred(est, zero_mean)
        Se = est.shape[0]
        for i in range(Se):
            for j in range(Sr):
                out['pair'][k, i, j] = si_sdr_centred(est[i], refs[j])
        if info:
            continue                                # no matching, left out of every mean
        mr, me = match(out['pair'][k], Se, Sr)
        out['match_ref'][k], out['match_est'][k] = mr, me
        for j in range(Sr):
            if mr[j] >= 0:
                out['si_sdr'][k, j] = out['pair'][k, mr[j], j]
                with np.errstate(invalid='ignore'):
                    out['si_sdri'][k, j] = out['si_sdr'][k, j] - base[j]
        n = min(Se, Sr)
        out['missed'][k], out['spurious'][k] = Sr - n, Se - n
    return out


def score_many(refs, ests, mixtures, zero_mean=True):
    """The outputs with leading axes [R, K]; ests[r]: one [Se, L] array or a list of K of them."""
    per = [score(r, e if isinstance(e, (list, tuple)) else [e], m, zero_mean) for r, e, m in zip(refs, ests, mixtures)]
    return {key: np.stack([p[key] for p in per]) for key in per[0]}
