"""Ragged SI-SDR scoring: one call over recordings of different lengths against a loop of the same arithmetic in torch: one JSON line.

R = 256 recordings of 4 .. 12 s at 8 kHz drawn (RandomState(7)) from 16 distinct values, Sr = Se = 2 true sources and tracks, K = 2 sets
of estimates, the signals by the mix construction of tests/bss_common.py (RandomState(9)) plus a DC offset, float32 on the device.
    (a) loop_ms     for r: the Gram products of the centred rows in torch float64 on the device, the pair table from them, the matching
                    on the host -- what a user of the tree could write without the library
    (b) ragged_ms   utils.bss_eval.si_sdr_ragged(refs, ests, mixtures)                      ONE library call, two launches
The results of (a) and (b) are compared first (1e-6 dB on the pair tables, the matchings equal).  Then (a) and (b) are timed in
alternating blocks in one process, warm (an untimed call of each first), every call between two device synchronisations; medians of
--reps.  Expected: ragged_ms / loop_ms < 1 (exit status 1 otherwise).
Also recorded: the two kernels of one call alone (torch.profiler, a call of its own) against the bytes they must read over the HBM
peak DESIGN.md 4 uses (8.0 TB/s) -- the packed float32 rows once, the block partials written and read once -- and against the float64
rate DESIGN.md 4.11 uses (39.3 T fused multiply-adds per second) on the multiply-adds of the definition: (Sr + 2) nrows + nrows per
sample.

usage: python tools/sisdr_bench.py [--reps 5] [--recordings 256] [--no-profile]"""
import argparse
import contextlib
import itertools
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, 'adaptive-multispeaker-separation_amd')
for _p in (ROOT, PKG):
    if _p not in sys.path:
        sys.path.insert(0, _p)

S, K = 2, 2
HBM_BYTES_PER_S, F64_FMA_PER_S = 8.0e12, 39.3e12
TOL_DB = 1e-6


def _mix(rng, nsrc, L):                                       # as tests/bss_common.py
    s = rng.randn(nsrc, L)
    for i in range(nsrc):
        s[i] = np.convolve(s[i], rng.randn(8 + 3 * i), mode='same')
    a = rng.randn(nsrc, nsrc) * 0.3 + np.eye(nsrc)
    est = a.dot(s) + 0.05 * rng.randn(nsrc, L)
    return s, est


def _timed_ms(fn):
    import torch
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3


def _kernel_ms(fn, names):
    """Device time of the kernels whose names contain one of `names`, from one profiled call; None where the profiler gives none."""
    import torch
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        out = {n: 0.0 for n in names}
        for ev in prof.events():
            for n in names:
                if n in ev.name:
                    out[n] += float(getattr(ev, 'device_time', 0.0) or getattr(ev, 'cuda_time', 0.0)) / 1e3
        return {n: (round(v, 4) if v > 0 else None) for n, v in out.items()}
    except Exception as e:                                    # the measurement is optional; the comparison and the timing are not
        print('profiler unavailable: %r' % (e,), file=sys.stderr)
        return {n: None for n in names}


def _loop_one(ref, est, x):
    """One recording in torch float64: pair [K, Se, Sr] and base [Sr] on the device."""
    import torch
    Sr = ref.shape[0]
    rows = torch.cat([ref, x[None]] + list(est)).double()
    rows = rows - rows.mean(dim=1, keepdim=True)
    g = rows[:Sr] @ rows.t()                                  # [Sr, nrows]
    sq = (rows * rows).sum(dim=1)
    ss = sq[:Sr, None]
    g2 = g * g
    db = 10.0 * torch.log10(g2 / (ss * sq[None] - g2))        # [Sr, nrows]
    return db[:, Sr + 1:].t().reshape(K, -1, Sr), db[:, Sr]


def _match(pair):
    """pair [Se, Sr] with Se == Sr -> the estimate of every reference: the first maximum over itertools.permutations."""
    n = pair.shape[0]
    best, bv = None, None
    for t in itertools.permutations(range(n)):
        v = sum(pair[t[j], j] for j in range(n))
        if best is None or v > bv:
            best, bv = t, v
    return list(best)


def run(reps, R, profile_kernels):
    import torch
    from ams_hip import sisdr
    from utils import bss_eval as hb
    values = np.random.RandomState(7).randint(32000, 96001, size=16)
    lengths = values[np.random.RandomState(8).randint(0, 16, size=R)].tolist()
    rng = np.random.RandomState(9)
    refs, ests, mixes = [], [], []
    for L in lengths:
        r, e = _mix(rng, S, L)
        dc = lambda n: 0.5 * rng.randn(n, 1)                  # noqa: E731
        refs.append(torch.from_numpy(np.asarray(r + dc(S), np.float32)).cuda())
        ests.append([torch.from_numpy(np.asarray(v + dc(S), np.float32)).cuda() for v in (e[::-1], e + 0.2 * rng.randn(S, L))])
        mixes.append(torch.from_numpy(np.asarray(r.sum(axis=0) + 0.05 * rng.randn(L) + 0.5 * rng.randn(), np.float32)).cuda())

    def loop():
        out = [_loop_one(r, e, x) for r, e, x in zip(refs, ests, mixes)]
        pair = torch.stack([p for p, _ in out]).cpu().numpy()  # [R, K, Se, Sr]
        base = torch.stack([b for _, b in out]).cpu().numpy()
        return pair, base, [[_match(pair[r, k]) for k in range(K)] for r in range(R)]

    ragged = lambda: hb.si_sdr_ragged(refs, ests, mixes)      # noqa: E731
    # the same results first (and the warm-up call of each)
    got = ragged()
    pair, base, match = loop()
    if got['info'].any():
        raise AssertionError('a reference counts as silent')
    err = max(float(np.abs(got['pair'][:, :, :S, :S] - pair).max()), float(np.abs(got['base'][:, :S] - base).max()))
    if not err < TOL_DB:
        raise AssertionError('the ragged call and the loop disagree: %.3e dB' % err)
    if got['match_ref'][:, :, :S].tolist() != match:
        raise AssertionError('the ragged call and the loop match differently')
    la, lb = [], []
    for _ in range(reps):                                     # alternating blocks
        la.append(_timed_ms(loop))
        lb.append(_timed_ms(ragged))
    loop_ms, ragged_ms = float(np.median(la)), float(np.median(lb))
    lay = sisdr.Layout([S] * R, [[S] * K] * R, lengths)
    tot = int(sum(lengths))
    nrows = S + 1 + K * S
    gram_bytes = 4 * lay.floats + 8 * lay.Btot * ((S + 2) * nrows + nrows)
    finish_bytes = 8 * lay.Btot * ((S + 2) * nrows + nrows)
    fma = tot * ((S + 2) * nrows + nrows)
    res = dict(recordings=R, distinct_lengths=len(set(lengths)), samples=tot, rows_per_recording=nrows, blocks=lay.Btot, block=sisdr.block(),
               packed_bytes=4 * lay.floats, workspace_bytes=lay.workspace_bytes(), launches_per_call=2, max_db_difference=err,
               loop_ms=round(loop_ms, 3), ragged_ms=round(ragged_ms, 3), ragged_over_loop=round(ragged_ms / loop_ms, 4),
               loop_ms_all=[round(v, 2) for v in la], ragged_ms_all=[round(v, 2) for v in lb],
               gram_hbm_ms=round(gram_bytes / HBM_BYTES_PER_S * 1e3, 4), gram_f64_ms=round(fma / F64_FMA_PER_S * 1e3, 4),
               finish_hbm_ms=round(finish_bytes / HBM_BYTES_PER_S * 1e3, 5))
    if profile_kernels:
        x = sisdr.pack(lay, [p for r, e, m in zip(refs, ests, mixes) for p in [r, m] + e], refs[0].device)
        k = _kernel_ms(lambda: sisdr.eval_packed(x, lay), ('sisdr_gram_kernel', 'sisdr_finish_kernel'))
        res.update(gram_kernel_ms=k['sisdr_gram_kernel'], finish_kernel_ms=k['sisdr_finish_kernel'])
        if k['sisdr_gram_kernel']:
            res.update(gram_over_hbm=round(k['sisdr_gram_kernel'] / (gram_bytes / HBM_BYTES_PER_S * 1e3), 2),
                       gram_over_f64=round(k['sisdr_gram_kernel'] / (fma / F64_FMA_PER_S * 1e3), 2))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--recordings', type=int, default=256)
    ap.add_argument('--no-profile', action='store_true', help='skip the profiled call (the kernels alone)')
    args = ap.parse_args()
    with contextlib.redirect_stdout(sys.stderr):
        r = run(args.reps, args.recordings, not args.no_profile)
    ok = r['ragged_ms'] < r['loop_ms']
    print(json.dumps(dict(bench='sisdr', references=S, tracks=S, nsets=K, reps=args.reps, expected='ragged_ms / loop_ms < 1', ok=ok, **r)),
          flush=True)
    return 0 if ok else 1


if __name__ == '__main__':
    sys.exit(main())
