"""Recording-level SOFT clustering: one ragged soft k-means call against one soft call per recording, and separate_recordings of a soft
k-means model in 'chunk' and in 'recording_soft' mode: one JSON line.

The geometry of tools/cluster_bench.py: R = 256 recordings of RandomState(7).randint(32000, 96001) samples (1483 chunks of L = 20480,
H = 10240), TF = 20480 points per chunk; E = 40, C = 2, 10 tries, 10 iterations, beta = 5, no silence weights, labels at the end.
    (a) loop_ms     for r: ops.kmeans_run(xn_r[None], idx_r, ..., beta)      b = 1 per recording, 14 launches each
    (b) ragged_ms   kmeans_ragged_soft(xn, segments, idx, ..., beta)        ONE call: 14 launches in all
on the same normalised points and the same seeds.  The results are compared first, within the tolerance of
tests/test_gpu_kmeans_ragged_soft.py: where both chose the same try the masks agree within 1e-3; where they did not, the two tries'
inertia must be within 1e-3 relative (a tie, as when the tries collapse onto one solution).  (a) and (b) are timed in alternating blocks in
one process, warm (two untimed calls of each), every call between two device synchronisations; medians of --reps.  Required:
ragged_ms / loop_ms < 1 (exit status 1 otherwise).
    pass_us                     one iteration pass of (b): (the every-try run with 10 iterations - with 0) / 10
    pass_point_tries_per_s      Ptot tries / pass time, beside batch_kernel_point_tries_per_s = 64 x 20480 / 42 us, the batch soft pass's
                                own rate: whether the table indirection and the fixed order cost anything
    (c) chunk_ms / recording_soft_ms   model.separate_recordings(xs) with clustering='chunk' / 'recording_soft' on the front_DPCL inference
        model of tools/stitch_many_bench.py built with beta_kmeans = 5 (batch 64, --kmeans_seeding fast); the model passes are counted.
With R = 1 and a short recording the ragged call has few workgroups (one per 8192 points and try) and does not fill the device: that is
not what is measured here.

usage: python tools/cluster_soft_bench.py [--reps 5] [--model-reps 3] [--recordings 256] [--no-model]"""
import argparse
import contextlib
import json
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, 'adaptive-multispeaker-separation_amd')
for _p in (ROOT, PKG):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from tools.cluster_bench import B, E, H, ITERS, L, S, TF, TRIES, _timed_ms      # noqa: E402  (one geometry, one way of timing)

BETA, TOL = 5.0, 1e-3
BATCH_RATE = 64 * 20480 / 42e-6                                   # point-tries per second of kmeans_soft_acc_kernel


def run_kmeans(reps, lengths):
    import torch
    from ams_hip import kmeans_ragged as kr
    from ams_hip import kmeans_ragged_soft as krs
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
    loop = lambda: [ops.kmeans_run(x, i, S, TRIES, ITERS, beta=BETA)[:3] for x, i in per]
    ragged = lambda: krs.kmeans_ragged_soft(xn, seg, idx, S, TRIES, ITERS, BETA, normalize_input=False, want_inertia=True)
    # the same results first (and the first warm-up call of each)
    n0 = krs.LAUNCHES
    cent, masks, best, inertia = ragged()
    launches = krs.LAUNCHES - n0
    ref = loop()
    torch.cuda.synchronize()
    inertia = inertia.view(seg.R, TRIES).cpu().numpy()
    worst, ties = 0.0, 0
    for r, (c1, m1, b1) in enumerate(ref):
        b0, b1 = int(best[r]), int(b1[0])
        if b0 == b1:
            err = float((masks[seg.rows(r)] - m1[0]).abs().max())
            worst = max(worst, err)
            if not err <= TOL:
                raise AssertionError('recording %d: the masks of the ragged call and of ops.kmeans_run differ by %.3g' % (r, err))
        else:
            ties += 1
            lo, hi = sorted((float(inertia[r, b0]), float(inertia[r, b1])))
            if not hi - lo <= TOL * lo:
                raise AssertionError('recording %d: the ragged call chose try %d, ops.kmeans_run try %d, and their inertia differs: %r'
                                     % (r, b0, b1, inertia[r].tolist()))
    del ref, cent, masks
    loop()
    ragged()
    la, lb = [], []
    for _ in range(reps):                                         # alternating blocks
        la.append(_timed_ms(loop))
        lb.append(_timed_ms(ragged))
    loop_ms, ragged_ms = float(np.median(la)), float(np.median(lb))
    # one iteration pass: the every-try run with and without its iterations
    tries_run = lambda it: krs.kmeans_ragged_soft_tries(xn, seg, idx, S, TRIES, it, BETA, normalize_input=False)
    tries_run(ITERS)
    tries_run(0)
    t10, t0 = [], []
    for _ in range(reps):
        t10.append(_timed_ms(lambda: tries_run(ITERS)))
        t0.append(_timed_ms(lambda: tries_run(0)))
    pass_ms = (float(np.median(t10)) - float(np.median(t0))) / ITERS
    return dict(recordings=seg.R, chunks=lay.Ctot, points=seg.Ptot, chunks_of_8192=seg.Gtot, point_bytes=seg.Ptot * E * 4,
                loop_launches=seg.R * (ITERS + 4), ragged_launches=launches, masks_max_difference=worst, other_try_of_a_tie=ties,
                loop_ms=round(loop_ms, 3), ragged_ms=round(ragged_ms, 3), ragged_over_loop=round(ragged_ms / loop_ms, 4),
                loop_ms_all=[round(v, 2) for v in la], ragged_ms_all=[round(v, 2) for v in lb], pass_us=round(pass_ms * 1e3, 1),
                pass_point_tries_per_s=float('%.4g' % (seg.Ptot * TRIES / (pass_ms * 1e-3))),
                batch_kernel_point_tries_per_s=float('%.4g' % BATCH_RATE))


def _soft_model():
    """The model of tools/stitch_many_bench.py::_model with a soft k-means."""
    from models.dpcl import DPCL
    from tools import bench_configs as bc
    from tools.stitch_many_bench import F
    from utils.trainer import Front_Separator_Inference
    tmp = tempfile.mkdtemp(prefix='ams_csb_')
    tr0, tfds0, a = bc._front_dpcl_checkpoint(tmp, DPCL, 'front_DPCL', B, S, L, F)
    with tr0.graph.as_default():
        tr0.model.create_saver()
        tr0.model.save(0)
        folder = tr0.model._dir()
    del tr0
    a.update(model_folder=folder, nb_tries=TRIES, nb_steps=ITERS, end_assign=True, out=False, kmeans_seeding='fast', beta_kmeans=BETA)
    for k in ('mix', 'non_mix', 'ind'):
        a.pop(k, None)
    tr = Front_Separator_Inference(DPCL, 'front_DPCL_inference', **a)
    return tr, tr.prepare_inference(), a['kmeans_seeding']


def run_model(reps, lengths):
    import torch
    from tools.stitch_many_bench import _passes
    gen = torch.Generator(device='cuda').manual_seed(7)
    xs = [0.1 * torch.randn(int(n), device='cuda', generator=gen) for n in lengths]
    tr, model, seeding = _soft_model()
    chunk = lambda: model.separate_recordings(xs)
    rec = lambda: model.separate_recordings(xs, clustering='recording_soft')
    with tr.graph.as_default():
        chunk_passes, rec_passes = _passes(model, chunk), _passes(model, rec)       # (the first warm-up call of each)
        outs = rec()
        if not all(bool(torch.isfinite(o).all()) for o in outs):
            raise FloatingPointError("separate_recordings(clustering='recording_soft') returned non-finite samples")
        del outs
        chunk()
        ca, cb = [], []
        for _ in range(reps):
            ca.append(_timed_ms(chunk))
            cb.append(_timed_ms(rec))
    return dict(chunk_passes=chunk_passes, recording_soft_passes=rec_passes, chunk_ms=round(float(np.median(ca)), 3),
                recording_soft_ms=round(float(np.median(cb)), 3), recording_soft_over_chunk=round(float(np.median(cb) / np.median(ca)), 4),
                model='front_DPCL inference, beta_kmeans %g, batch %d' % (BETA, B), kmeans_seeding=seeding)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--model-reps', type=int, default=3)
    ap.add_argument('--recordings', type=int, default=256)
    ap.add_argument('--no-model', action='store_true', help='(a) and (b) only')
    args = ap.parse_args()
    os.environ.setdefault('AMS_LOG_DIR', tempfile.mkdtemp(prefix='ams_csb_log_'))    # (before config is imported)
    lengths = np.random.RandomState(7).randint(32000, 96001, size=args.recordings)
    with contextlib.redirect_stdout(sys.stderr):
        import torch
        r = run_kmeans(args.reps, lengths)
        torch.cuda.empty_cache()
        if not args.no_model:
            r.update(run_model(args.model_reps, lengths))
    ok = r['ragged_ms'] < r['loop_ms']
    print(json.dumps(dict(bench='cluster_soft', embedding_size=E, clusters=S, tries=TRIES, iterations=ITERS, beta=BETA, points_per_chunk=TF,
                          chunk_size=L, hop=H, reps=args.reps, required='ragged_ms / loop_ms < 1', ok=ok, **r)), flush=True)
    return 0 if ok else 1


if __name__ == '__main__':
    sys.exit(main())
