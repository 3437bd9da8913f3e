"""Ragged BSS-eval: one call over recordings of different lengths against the loop of batched calls: one JSON line.

R = 256 recordings, S = 2 sources, K = 2 sets of estimates, flen = 512: lengths of 4 .. 12 s at 8 kHz drawn (RandomState(7)) from 16
distinct values, the signals by the mix construction of tests/bss_common.py (RandomState(9)), float64 on the device.
    (a) loop_ms     for r: utils.bss_eval.bss_eval_pairs_batch(ref_r[None], est_r[None])     the existing code: one cached context
                    (four hipFFT plans and a workspace) per distinct length -- 16 here, created during warm-up
    (b) ragged_ms   utils.bss_eval.bss_eval_pairs_ragged(refs, ests)                         ONE library call, no plan
The results of (a) and (b) are compared first under the project's dB rule (1e-6 dB below 100 dB, "stays above" above).  Then (a) and (b)
are timed in alternating blocks in one process, warm (an untimed call of each first), every call between two device synchronisations;
medians of --reps.  Required: ragged_ms / loop_ms < 1 (exit status 1 otherwise).
Also recorded: the correlation and the projection kernel of one ragged call alone (torch.profiler, a call of its own) against the
float64 matrix rate of the board (78.6 TFLOP/s, the data-sheet figure DESIGN.md 6b uses) on the multiply-adds of the definition:
(S^2 + K S^2) F sum L_r for the correlations, 2 K S^2 F sum (L_r + F - 1) for the projections.

usage: python tools/score_bench.py [--reps 5] [--recordings 256] [--no-profile]"""
import argparse
import contextlib
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

S, K, F = 2, 2, 512
F64_MATRIX_TFLOPS = 78.6
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


def _db_error(got, ref):
    small = ref < 100.0
    err = float(np.abs(got[small] - ref[small]).max(initial=0.0))
    return err, bool(err < TOL_DB and (got[~small] > 100.0).all())


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
        return {n: (round(v, 3) if v > 0 else None) for n, v in out.items()}
    except Exception as e:                                    # the measurement is optional; the comparison and the timing are not
        print('profiler unavailable: %r' % (e,), file=sys.stderr)
        return {n: None for n in names}


def run(reps, R, profile_kernels):
    import torch
    from utils import bss_eval as hb
    values = np.random.RandomState(7).randint(32000, 96001, size=16)
    lengths = values[np.random.RandomState(8).randint(0, 16, size=R)].tolist()
    rng = np.random.RandomState(9)
    refs, ests = [], []
    for L in lengths:
        r, e = _mix(rng, S, L)
        refs.append(torch.from_numpy(r).cuda())
        ests.append(torch.from_numpy(np.stack([e[::-1]] + [e + 0.2 * k * rng.randn(S, L) for k in range(1, K)])).cuda())
    loop = lambda: [hb.bss_eval_pairs_batch(r[None], e[None]) for r, e in zip(refs, ests)]          # noqa: E731
    ragged = lambda: hb.bss_eval_pairs_ragged(refs, ests)                                           # noqa: E731
    # the same results first (and the warm-up call of each: the loop's contexts are created here)
    crit, info = ragged()
    ref = loop()
    want = np.concatenate([c for c, _ in ref])
    if info.any() or any(i.any() for _, i in ref):
        raise AssertionError('a Gram matrix was not positive definite')
    err, same = _db_error(crit, want)
    if not same:
        raise AssertionError('the ragged call and the loop of batched calls disagree: %.3e dB' % err)
    del ref
    la, lb = [], []
    for _ in range(reps):                                     # alternating blocks
        la.append(_timed_ms(loop))
        lb.append(_timed_ms(ragged))
    loop_ms, ragged_ms = float(np.median(la)), float(np.median(lb))
    lib = hb._load_ragged()
    lay = hb._ragged_layout(lengths, F)
    tot = int(sum(lengths))
    corr_gflop = 2e-9 * (S * S + K * S * S) * F * tot
    proj_gflop = 2e-9 * 2 * K * S * S * F * (tot + R * (F - 1))
    res = dict(recordings=R, distinct_lengths=len(set(lengths)), samples=tot, blocks=lay.Btot, block=hb.ragged_block(),
               workspace_bytes=int(lib.ams_bssr_workspace_bytes(R, K, S, F, lay.Btot)), loop_contexts=len(hb._bctx),
               ragged_launches=int(lib.ams_bssr_launches(S, K, F)), max_db_difference=err,
               loop_ms=round(loop_ms, 3), ragged_ms=round(ragged_ms, 3), ragged_over_loop=round(ragged_ms / loop_ms, 4),
               loop_ms_all=[round(v, 2) for v in la], ragged_ms_all=[round(v, 2) for v in lb],
               corr_gflop=round(corr_gflop, 2), proj_gflop=round(proj_gflop, 2),
               corr_bound_ms=round(corr_gflop / F64_MATRIX_TFLOPS, 3), proj_bound_ms=round(proj_gflop / F64_MATRIX_TFLOPS, 3))
    if profile_kernels:
        k = _kernel_ms(ragged, ('bssr_corr_kernel', 'bssr_proj_kernel', 'potrf_', 'solve_'))
        res.update(corr_kernel_ms=k['bssr_corr_kernel'], proj_kernel_ms=k['bssr_proj_kernel'], potrf_kernels_ms=k['potrf_'],
                   solve_kernels_ms=k['solve_'])
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
    print(json.dumps(dict(bench='score', nsrc=S, nsets=K, flen=F, reps=args.reps, required='ragged_ms / loop_ms < 1', ok=ok, **r)), flush=True)
    return 0 if ok else 1


if __name__ == '__main__':
    sys.exit(main())
