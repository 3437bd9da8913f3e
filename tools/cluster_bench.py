"""Recording-level clustering: one ragged k-means call against one call per recording, and separate_recordings in both modes: one JSON line.

The workload of tools/stitch_many_bench.py: R = 256 recordings of RandomState(7).randint(32000, 96001) samples (4 .. 12 s at 8 kHz; 1483
chunks of L = 20480, H = 10240), TF = 20480 points per chunk, so recording r is a segment of C_r * 20480 points; E = 40, C = 2, 10 tries,
10 iterations, no silence weights, labels re-assigned at the end.
    (a) loop_ms     for r: ops.kmeans_run(xn_r[None], idx_r, ...)        b = 1 per recording, 14 launches each
    (b) ragged_ms   kmeans_ragged(xn, segments, idx, ...)                ONE call: 14 launches in all
on the same normalised points and the same seeds (the results are compared first: every label, centroid and chosen try equal).  (a) and
(b) are timed in alternating blocks in one process, warm (two untimed calls of each), every call between two device synchronisations;
medians of --reps.  Required: ragged_ms / loop_ms < 1 (exit status 1 otherwise).
    (c) chunk_ms / recording_ms   model.separate_recordings(xs) with clustering='chunk' / 'recording' on the front_DPCL inference model of
        tools/stitch_many_bench.py (batch 64, --kmeans_seeding fast); the model passes of each are counted.

usage: python tools/cluster_bench.py [--reps 5] [--model-reps 3] [--recordings 256] [--no-model]"""
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

S, L, H, B, TF, E, TRIES, ITERS = 2, 20480, 10240, 64, 20480, 40, 10, 10


def _timed_ms(fn):
    import torch
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3


def run_kmeans(reps, lengths):
    import torch
    from ams_hip import kmeans_ragged as kr
    from ams_hip import ops
    from ams_hip import stitch_batch as sb
    lay = sb.layout(lengths, L, H, S)
    seg = kr.segments_of_layout(lay, TF)
    gen = torch.Generator(device='cuda').manual_seed(11)
    # two blobs per recording on the unit sphere: centres c0, c1 drawn per recording, points around them
    xn = torch.empty((seg.Ptot, E), dtype=torch.float32, device='cuda')
    for r in range(seg.R):
        rows = seg.rows(r)
        n = rows.stop - rows.start
        cen = torch.randn(2, E, device='cuda', generator=gen) * 1.5
        pick = (torch.rand(n, device='cuda', generator=gen) < 0.5).long()
        xn[rows] = cen[pick] + torch.randn(n, E, device='cuda', generator=gen)
    xn = ops.kmeans_normalize(xn)
    rng = np.random.RandomState(13)
    idx = np.concatenate([np.stack([rng.choice(int(p), S, replace=False) for _ in range(TRIES)]) for p in seg.P]).astype(np.int32)
    per = [(xn[seg.rows(r)][None], torch.from_numpy(idx[r * TRIES:(r + 1) * TRIES]).cuda()) for r in range(seg.R)]
    loop = lambda: [ops.kmeans_run(x, i, S, TRIES, ITERS)[:3] for x, i in per]
    ragged = lambda: kr.kmeans_ragged(xn, seg, idx, S, TRIES, ITERS, normalize_input=False)
    # the same results first (and the first warm-up call of each)
    n0 = kr.LAUNCHES
    cent, lab, best = ragged()
    launches = kr.LAUNCHES - n0
    ref = loop()
    torch.cuda.synchronize()
    for r, (c1, l1, b1) in enumerate(ref):
        if not (torch.equal(cent[r], c1[0]) and torch.equal(lab[seg.rows(r)], l1[0]) and int(best[r]) == int(b1[0])):
            raise AssertionError('recording %d: the ragged call and ops.kmeans_run disagree' % r)
    del ref
    loop()
    ragged()
    la, lb = [], []
    for _ in range(reps):                                         # alternating blocks
        la.append(_timed_ms(loop))
        lb.append(_timed_ms(ragged))
    loop_ms, ragged_ms = float(np.median(la)), float(np.median(lb))
    return dict(recordings=seg.R, chunks=lay.Ctot, points=seg.Ptot, chunks_of_8192=seg.Gtot, point_bytes=seg.Ptot * E * 4,
                loop_launches=seg.R * (ITERS + 4), ragged_launches=launches, loop_ms=round(loop_ms, 3), ragged_ms=round(ragged_ms, 3),
                ragged_over_loop=round(ragged_ms / loop_ms, 4), loop_ms_all=[round(v, 2) for v in la], ragged_ms_all=[round(v, 2) for v in lb])


def run_model(reps, lengths):
    import torch
    from tools.stitch_many_bench import _model, _passes
    gen = torch.Generator(device='cuda').manual_seed(7)
    xs = [0.1 * torch.randn(int(n), device='cuda', generator=gen) for n in lengths]
    tr, model, seeding = _model()
    chunk = lambda: model.separate_recordings(xs)
    rec = lambda: model.separate_recordings(xs, clustering='recording')
    with tr.graph.as_default():
        chunk_passes, rec_passes = _passes(model, chunk), _passes(model, rec)       # (the first warm-up call of each)
        outs = rec()
        if not all(bool(torch.isfinite(o).all()) for o in outs):
            raise FloatingPointError("separate_recordings(clustering='recording') returned non-finite samples")
        del outs
        chunk()
        ca, cb = [], []
        for _ in range(reps):
            ca.append(_timed_ms(chunk))
            cb.append(_timed_ms(rec))
    return dict(chunk_passes=chunk_passes, recording_passes=rec_passes, chunk_ms=round(float(np.median(ca)), 3),
                recording_ms=round(float(np.median(cb)), 3), recording_over_chunk=round(float(np.median(cb) / np.median(ca)), 4),
                model='front_DPCL inference, batch %d' % B, kmeans_seeding=seeding)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--model-reps', type=int, default=3)
    ap.add_argument('--recordings', type=int, default=256)
    ap.add_argument('--no-model', action='store_true', help='(a) and (b) only')
    args = ap.parse_args()
    os.environ.setdefault('AMS_LOG_DIR', tempfile.mkdtemp(prefix='ams_clb_log_'))    # (before config is imported)
    lengths = np.random.RandomState(7).randint(32000, 96001, size=args.recordings)
    with contextlib.redirect_stdout(sys.stderr):
        import torch
        r = run_kmeans(args.reps, lengths)
        torch.cuda.empty_cache()
        if not args.no_model:
            r.update(run_model(args.model_reps, lengths))
    ok = r['ragged_ms'] < r['loop_ms']
    print(json.dumps(dict(bench='cluster', embedding_size=E, clusters=S, tries=TRIES, iterations=ITERS, points_per_chunk=TF, chunk_size=L,
                          hop=H, reps=args.reps, required='ragged_ms / loop_ms < 1', ok=ok, **r)), flush=True)
    return 0 if ok else 1


if __name__ == '__main__':
    sys.exit(main())
