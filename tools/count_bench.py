"""Choosing the number of speakers per recording: one counted call against the existing pieces in a loop per recording: one JSON line.

The workload of tools/cluster_bench.py: R = 256 recordings of RandomState(7).randint(32000, 96001) samples (1483 chunks of L = 20480,
H = 10240), TF = 20480 points per chunk, E = 40, 10 tries, 10 iterations, no silence weights, labels re-assigned at the end.  The
points are the planted family of tests/speaker_count_ref.py with 2 .. 6 clusters per recording; candidates 2 .. 6.
    (a) loop_ms      for r: for C in 2 .. 6: ops.kmeans_run(xn_r[None], idx_r[:, :C], C, ...), the simplified silhouette of its centroids
                     in torch float64 on the device (differences first); the count by argmax and the labels by index, no host
                     synchronisation inside the loop
    (b) counted_ms   spk_count.count_clusters(xn, segments, idx, 2, 6, ...)   ONE call
on the same normalised points and seeds.  The results are compared first: counts and labels equal, scores within 1e-9, on the
recordings without a non-finite try (ops.kmeans_run picks such a try, the counted call skips it; their number is reported).  (a) and (b)
are timed in alternating blocks in one process, warm, every call between two device synchronisations; medians of --reps.
Required: counted_ms / loop_ms < 1 (exit status 1 otherwise).
    (c) sweep_ms     ams_spkc_score alone (the sweep and its finish) on the tries of (b), against
                     hbm_ms: the packed points once at the 6.29 TB/s a float4 copy reaches on this part, and
                     f64_ms: 2 P (2 + .. + 6) E float64 vector instructions (a subtraction and a fused multiply-add per component and
                     centroid) at the 78.6 TFLOP/s of the public specification (39.3 T fused multiply-adds a second)
    (d) auto_ms / recording_ms   model.separate_recordings(xs, clustering='recording') with speakers='auto' / without, on the front_DPCL
                     inference model of tools/stitch_many_bench.py built with S = 3 (batch 64, --kmeans_seeding fast)

usage: python tools/count_bench.py [--reps 3] [--model-reps 3] [--recordings 256] [--no-model]"""
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

L, H, B, TF, E, TRIES, ITERS, LO, HI, S_MODEL = 20480, 10240, 64, 20480, 40, 10, 10, 2, 6, 3
HBM_BYTES_PER_S, F64_INSTR_PER_S = 6.29e12, 39.3e12


def _timed_ms(fn):
    import torch
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3


def _score64(x, cent):
    """The simplified silhouette of x [P, E] against cent [C, E] in float64, differences first."""
    d = _distances64(x, cent)
    two = d.topk(2, dim=1, largest=False).values
    d1, d2 = two[:, 0], two[:, 1]
    return ((d2 - d1) / d2).nan_to_num(0.0).sum() / x.shape[0]


def _distances64(x, cent):
    import torch
    x64, c64 = x.double(), cent.double()
    return torch.stack([((x64 - c64[c]) ** 2).sum(dim=1) for c in range(c64.shape[0])], dim=1).sqrt()


def run_counts(reps, lengths):
    import torch
    from ams_hip import kmeans_ragged as kr
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
    idx = np.concatenate([np.stack([rng.choice(int(p), HI, replace=False) for _ in range(TRIES)]) for p in seg.P]).astype(np.int32)
    cands = list(range(LO, HI + 1))
    per = [(xn[seg.rows(r)], [torch.from_numpy(np.ascontiguousarray(idx[r * TRIES:(r + 1) * TRIES, :C])).cuda() for C in cands])
           for r in range(seg.R)]

    def loop():
        out = []
        for x, seeds in per:
            scores, labs = [], []
            for C, sd in zip(cands, seeds):
                cent, lab, _, _ = ops.kmeans_run(x[None], sd, C, TRIES, ITERS)
                scores.append(_score64(x, cent[0]))
                labs.append(lab[0])
            scores = torch.stack(scores)
            k = scores.nan_to_num(float('-inf')).argmax()       # (a NaN try picked by ops.kmeans_run: the candidate is out)
            out.append((scores, k, torch.stack(labs).index_select(0, k[None])[0]))
        return out

    counted = lambda: sc.count_clusters(xn, seg, idx, LO, HI, TRIES, ITERS, normalize_input=False)
    # the same results first (and the first warm-up call of each)
    n0 = kr.LAUNCHES + sc.LAUNCHES
    res = counted()
    launches = kr.LAUNCHES + sc.LAUNCHES - n0
    ref = loop()
    torch.cuda.synchronize()
    runs = [kr.kmeans_ragged_tries(xn, seg, np.ascontiguousarray(idx[:, :C]), C, TRIES, ITERS, normalize_input=False) for C in cands]
    cents, inertias = [r[0] for r in runs], [r[1] for r in runs]
    # ops.kmeans_run picks a try with a NaN inertia (an empty cluster) where there is one, the counted call skips it: the two are
    # compared on the recordings whose every try of every candidate is finite
    clean = torch.stack([torch.isfinite(i).view(seg.R, TRIES).all(dim=1) for i in inertias]).all(dim=0).tolist()
    if not any(clean):
        raise AssertionError('no recording without a non-finite try: nothing to compare')
    worst = 0.0
    for r, (scores, k, lab) in enumerate(ref):
        if not clean[r]:
            continue
        worst = max(worst, float((scores - res['scores'][r]).abs().max()))
        if int(k) + LO != int(res['count'][r]) or not torch.equal(lab, res['labels'][seg.rows(r)]):
            raise AssertionError('recording %d: the counted call and the loop disagree (%d / %d)' % (r, int(res['count'][r]), int(k) + LO))
    if worst > 1e-9:
        raise AssertionError('scores differ by %.3g' % worst)
    found = sum(int(c) == p for c, p in zip(res['count'].tolist(), planted))
    del ref
    loop()
    counted()
    la, lb = [], []
    for _ in range(reps):                                         # alternating blocks
        la.append(_timed_ms(loop))
        lb.append(_timed_ms(counted))
    # (c) the sweep alone, on the tries of the counted call
    sweep = lambda: sc.score(xn, seg, cents, inertias, LO, TRIES)
    sweep()
    sweep()
    ls = [_timed_ms(sweep) for _ in range(max(reps, 5))]
    loop_ms, counted_ms, sweep_ms = float(np.median(la)), float(np.median(lb)), float(np.median(ls))
    nbytes = seg.Ptot * E * 4
    instr = 2 * seg.Ptot * sum(cands) * E
    hbm_ms, f64_ms = nbytes / HBM_BYTES_PER_S * 1e3, instr / F64_INSTR_PER_S * 1e3
    return dict(recordings=seg.R, compared_recordings=sum(clean), non_finite_tries=int(sum((~torch.isfinite(i)).sum() for i in inertias)),
                chunks=lay.Ctot, points=seg.Ptot, point_bytes=nbytes, candidates=cands, planted_counts_found=found,
                max_score_difference=worst, loop_launches_kmeans=seg.R * len(cands) * (ITERS + 4), counted_launches=launches,
                loop_ms=round(loop_ms, 3), counted_ms=round(counted_ms, 3), counted_over_loop=round(counted_ms / loop_ms, 4),
                loop_ms_all=[round(v, 2) for v in la], counted_ms_all=[round(v, 2) for v in lb],
                sweep_ms=round(sweep_ms, 3), sweep_ms_all=[round(v, 3) for v in ls], hbm_ms=round(hbm_ms, 3), f64_ms=round(f64_ms, 3),
                sweep_over_hbm=round(sweep_ms / hbm_ms, 3), sweep_over_f64=round(sweep_ms / f64_ms, 3),
                sweep_bound='float64 arithmetic' if f64_ms > hbm_ms else 'HBM read',
                sweep_share_of_bound=round(max(hbm_ms, f64_ms) / sweep_ms, 4))


def _model():
    from models.dpcl import DPCL
    from tools import bench_configs as bc
    from tools.stitch_many_bench import F
    from utils.trainer import Front_Separator_Inference
    tmp = tempfile.mkdtemp(prefix='ams_cnb_')
    tr0, tfds0, a = bc._front_dpcl_checkpoint(tmp, DPCL, 'front_DPCL', B, S_MODEL, L, F)
    with tr0.graph.as_default():
        tr0.model.create_saver()
        tr0.model.save(0)
        folder = tr0.model._dir()
    del tr0
    a.update(model_folder=folder, nb_tries=10, nb_steps=10, end_assign=True, out=False, kmeans_seeding='fast')
    for k in ('mix', 'non_mix', 'ind'):
        a.pop(k, None)
    tr = Front_Separator_Inference(DPCL, 'front_DPCL_inference', **a)
    return tr, tr.prepare_inference(), a['kmeans_seeding']


def run_model(reps, lengths):
    import torch
    from tools.stitch_many_bench import _passes
    gen = torch.Generator(device='cuda').manual_seed(7)
    xs = [0.1 * torch.randn(int(n), device='cuda', generator=gen) for n in lengths]
    tr, model, seeding = _model()
    rec = lambda: model.separate_recordings(xs, clustering='recording')
    auto = lambda: model.separate_recordings(xs, clustering='recording', speakers='auto')
    with tr.graph.as_default():
        rec_passes, auto_passes = _passes(model, rec), _passes(model, auto)         # (the first warm-up call of each)
        outs = auto()
        if not all(bool(torch.isfinite(o).all()) for o in outs):
            raise FloatingPointError("separate_recordings(speakers='auto') returned non-finite samples")
        counts = model.last_clustering['counts'].tolist()
        del outs
        rec()
        ca, cb = [], []
        for _ in range(reps):
            ca.append(_timed_ms(rec))
            cb.append(_timed_ms(auto))
    return dict(recording_passes=rec_passes, auto_passes=auto_passes, recording_ms=round(float(np.median(ca)), 3),
                auto_ms=round(float(np.median(cb)), 3), auto_over_recording=round(float(np.median(cb) / np.median(ca)), 4),
                auto_counts={str(c): counts.count(c) for c in sorted(set(counts))},
                model='front_DPCL inference, S = %d, batch %d' % (S_MODEL, B), kmeans_seeding=seeding)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--model-reps', type=int, default=3)
    ap.add_argument('--recordings', type=int, default=256)
    ap.add_argument('--no-model', action='store_true', help='(a), (b) and (c) only')
    args = ap.parse_args()
    os.environ.setdefault('AMS_LOG_DIR', tempfile.mkdtemp(prefix='ams_cnb_log_'))    # (before config is imported)
    lengths = np.random.RandomState(7).randint(32000, 96001, size=args.recordings)
    with contextlib.redirect_stdout(sys.stderr):
        import torch
        r = run_counts(args.reps, lengths)
        torch.cuda.empty_cache()
        if not args.no_model:
            r.update(run_model(args.model_reps, lengths))
    ok = r['counted_ms'] < r['loop_ms']
    print(json.dumps(dict(bench='count', embedding_size=E, tries=TRIES, iterations=ITERS, points_per_chunk=TF, chunk_size=L, hop=H,
                          reps=args.reps, required='counted_ms / loop_ms < 1', ok=ok, **r)), flush=True)
    return 0 if ok else 1


if __name__ == '__main__':
    sys.exit(main())
