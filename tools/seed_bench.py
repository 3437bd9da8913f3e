"""k-means++ (D^2) seeding of the recording-level k-means (ams_hip/kmeans_seed.py) against the uniform seeds of the model:
one JSON line.

The workload of tools/cluster_bench.py and tools/count_bench.py: R = 256 recordings of RandomState(7).randint(32000, 96001) samples (1483
chunks of L = 20480, H = 10240), TF = 20480 points per chunk, E = 40, 10 iterations, no silence weights; the planted family of
tools/count_bench.py with 2 .. 6 clusters per recording.  Everything is timed afresh in this run on the same points, warm, every call
between two device synchronisations; medians of --reps.
    (a) seed_ms            seed_plusplus alone for C = 2 and C = 6 at 10 tries (the upload of the draws included), and step_ms: the
                           steps of C = 6 one entry point each (the weighing and the pick of step c), synchronised after every step
    (b) kmeans2_ms         kmeans_ragged at C = 2, 10 tries x 10 iterations, from uniform ('model') seeds and from k-means++ seeds: the
                           seeding and the copy of the seeds to the host included
    (c) counted_ms         spk_count.count_clusters, candidates 2 .. 6, from uniform seeds at 10 tries and from k-means++ seeds (made once
                           for C = 6, the host copy included) at 10 and at 3 tries; for each of the three
        non_finite_share   the share of tries (all candidates) that ended with a non-finite inertia
        planted_found      the share of recordings whose planted count was chosen
        inertia_ratio      the mean over the recordings of (the smallest finite inertia of the candidate with the planted count) /
                           (the same of the 10-try run from uniform seeds); recordings without a finite try on either side are left out
No threshold: the exit status is 0 whenever the run completes.  How k-means++ seeds behave on a trained model's embeddings is not
measured here.

usage: python tools/seed_bench.py [--reps 3] [--recordings 256]"""
import argparse
import contextlib
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, 'adaptive-multispeaker-separation_amd')
for _p in (ROOT, PKG):
    if _p not in sys.path:
        sys.path.insert(0, _p)

L, H, TF, E, TRIES, FEW, ITERS, LO, HI = 20480, 10240, 20480, 40, 10, 3, 10, 2, 6


def _timed_ms(fn):
    import torch
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3


def _median_ms(fn, reps):
    fn()                                                           # warm
    return round(float(np.median([_timed_ms(fn) for _ in range(reps)])), 3)


def _u64(rng, shape):
    return (rng.randint(0, 1 << 32, size=shape).astype(np.uint64) << np.uint64(32)) | rng.randint(0, 1 << 32, size=shape).astype(np.uint64)


def run(reps, lengths):
    import torch
    from ams_hip import kmeans_ragged as kr
    from ams_hip import kmeans_seed as ks
    from ams_hip import ops
    from ams_hip import spk_count as sc
    from ams_hip import stitch_batch as sb
    lay = sb.layout(lengths, L, H, 2)
    seg = kr.segments_of_layout(lay, TF)
    gen = torch.Generator(device='cuda').manual_seed(11)
    planted = [2 + r % (HI - 1) for r in range(seg.R)]
    xn = torch.empty((seg.Ptot, E), dtype=torch.float32, device='cuda')
    for r in range(seg.R):
        rows = seg.rows(r)
        n = rows.stop - rows.start
        cen = torch.nn.functional.normalize(torch.randn(planted[r], E, device='cuda', generator=gen), dim=1)
        pick = torch.randint(0, planted[r], (n,), device='cuda', generator=gen)
        xn[rows] = cen[pick] + 0.1 / np.sqrt(E) * torch.randn(n, E, device='cuda', generator=gen)
    xn = ops.kmeans_normalize(xn)
    rng = np.random.RandomState(13)
    uniform = np.concatenate([np.stack([rng.choice(int(p), HI, replace=False) for _ in range(TRIES)]) for p in seg.P]).astype(np.int32)
    draws = _u64(rng, (seg.R * TRIES, HI))
    few = np.ascontiguousarray(draws.reshape(seg.R, TRIES, HI)[:, :FEW].reshape(-1, HI))        # the first 3 tries of every recording
    cands = list(range(LO, HI + 1))

    def plus(C, d, tries):
        return ks.seed_plusplus(xn, seg, C, tries, np.ascontiguousarray(d[:, :C])).cpu().numpy()      # (the host copy synchronises)

    # (a)
    out = dict(recordings=seg.R, chunks=lay.Ctot, points=seg.Ptot, point_bytes=seg.Ptot * E * 4, candidates=cands)
    n0 = ks.LAUNCHES
    plus(HI, draws, TRIES)
    out['seed_launches_c6'] = ks.LAUNCHES - n0
    out['seed_ms'] = {'c2': _median_ms(lambda: plus(2, draws, TRIES), reps), 'c6': _median_ms(lambda: plus(HI, draws, TRIES), reps)}
    steps = []
    for _ in range(reps):
        stamps = []

        def stamp(c):
            torch.cuda.synchronize()
            stamps.append(time.perf_counter())
        torch.cuda.synchronize()
        stamps.append(time.perf_counter())
        ks.seed_plusplus(xn, seg, HI, TRIES, draws, steps=stamp)
        steps.append(np.diff(stamps) * 1e3)
    out['step_ms'] = [round(float(v), 3) for v in np.median(np.stack(steps), axis=0)]
    # (b)
    u2 = np.ascontiguousarray(uniform[:, :2])
    out['kmeans2_ms'] = {
        'model': _median_ms(lambda: kr.kmeans_ragged(xn, seg, u2, 2, TRIES, ITERS, normalize_input=False), reps),
        'plusplus': _median_ms(lambda: kr.kmeans_ragged(xn, seg, plus(2, draws, TRIES), 2, TRIES, ITERS, normalize_input=False), reps)}
    # (c)
    kinds = (('model_10', lambda: uniform, TRIES), ('plusplus_10', lambda: plus(HI, draws, TRIES), TRIES),
             ('plusplus_3', lambda: plus(HI, few, FEW), FEW))
    out['counted_ms'] = {name: _median_ms(lambda: sc.count_clusters(xn, seg, seeds(), LO, HI, tries, ITERS, normalize_input=False), reps)
                         for name, seeds, tries in kinds}
    best, quality = {}, {}
    for name, seeds, tries in kinds:
        idx = seeds()
        runs = [kr.kmeans_ragged_tries(xn, seg, np.ascontiguousarray(idx[:, :C]), C, tries, ITERS, normalize_input=False) for C in cands]
        res = sc.count_from_tries(xn, seg, [r[0] for r in runs], [r[1] for r in runs], LO, tries)
        inert = torch.stack([r[1].view(seg.R, tries) for r in runs]).cpu().numpy()               # [candidate, R, tries]
        fin = np.where(np.isfinite(inert), inert, np.inf).min(axis=2)                            # [candidate, R]
        best[name] = np.array([fin[planted[r] - LO, r] for r in range(seg.R)])
        quality[name] = dict(non_finite_share=round(float((~np.isfinite(inert)).mean()), 5),
                             planted_found=round(float(np.mean(np.array(res['count'].tolist()) == np.array(planted))), 4))
        del runs, res
    for name in best:
        ok = np.isfinite(best[name]) & np.isfinite(best['model_10']) & (best['model_10'] > 0)
        quality[name]['inertia_ratio'] = round(float(np.mean(best[name][ok] / best['model_10'][ok])), 5) if ok.any() else None
        quality[name]['inertia_recordings'] = int(ok.sum())
    out['quality'] = quality
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--recordings', type=int, default=256)
    args = ap.parse_args()
    os.environ.setdefault('AMS_LOG_DIR', tempfile.mkdtemp(prefix='ams_sdb_log_'))    # (before config is imported)
    lengths = np.random.RandomState(7).randint(32000, 96001, size=args.recordings)
    with contextlib.redirect_stdout(sys.stderr):
        r = run(args.reps, lengths)
    print(json.dumps(dict(bench='seed', embedding_size=E, tries=TRIES, few_tries=FEW, iterations=ITERS, points_per_chunk=TF, chunk_size=L,
                          hop=H, reps=args.reps, **r)), flush=True)
    return 0


if __name__ == '__main__':
    sys.exit(main())
