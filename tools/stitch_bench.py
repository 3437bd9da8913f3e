"""Whole-recording timing: one JSON line for a one-minute recording at 8 kHz (S = 2, L = 20480, H = 10240, N = 480000, 46 chunks).

Per kernel group of ams_hip/stitch.py (chunks, border_stats, tracks, overlap_add): the median ms per call, and next to it the call's
algorithmic bytes (include/ams_stitch.h, "Bytes moved") over the HBM peak of 8.0 TB/s -- the time the bytes alone would take; these
calls move a few MB each, so launch and kernel-boundary time is what they consist of.  End to end: Network.separate_recording with the
front_DPCL inference model of tools/bench_configs.py (front -> 3 x BLSTM(600) -> hard k-means 10 x 10 with --kmeans_seeding fast -> masks -> back, batch 64;
the command line's default seeding, 'reference', draws the restarts row by row on the host and is slower per batch).
Nothing comparable exists before this feature: the numbers are reported, no threshold rests on them.

usage: python tools/stitch_bench.py [--reps 20] [--no-model]"""
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

HBM_PEAK = 8.0e12          # bytes / s, MI355X spec
S, L, H, N = 2, 20480, 10240, 480000


def _median_ms(fn, reps):
    import torch
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t) * 1e3)
    return float(np.median(out))


def kernels(reps):
    import torch
    from ams_hip import stitch
    C, V = stitch.nb_chunks(N, L, H), L - H
    x = torch.randn(N, device='cuda')
    est = torch.randn(C, S, L, device='cuda')
    Q = stitch.border_stats(est, H)
    trk = stitch.tracks(Q, S)[1]
    nslab = -(-V // 1024)
    calls = {
        'chunks': (lambda: stitch.chunks(x, L, H), 4 * (N + (C - 1) * V) + 4 * C * L),
        'border_stats': (lambda: stitch.border_stats(est, H), 8 * (C - 1) * S * V + 4 * (C - 1) * S * S * (2 * nslab + 1)),
        'tracks': (lambda: stitch.tracks(Q, S), 4 * (C - 1) * (S * S + 2 * S)),
        'overlap_add': (lambda: stitch.overlap_add(est, trk, N, H), 4 * S * (N + (C - 1) * V) + 4 * S * N),
    }
    out = {}
    for name, (fn, nbytes) in calls.items():
        for _ in range(3):
            fn()
        out[name + '_ms'] = round(_median_ms(fn, reps), 4)
        out[name + '_bytes'] = nbytes
        out[name + '_ms_at_hbm_peak'] = round(nbytes / HBM_PEAK * 1e3, 5)
    out['stitch_ms'] = round(_median_ms(lambda: stitch.stitch(est, N, H), reps), 4)
    return C, out


def end_to_end(reps):
    import torch
    from models.dpcl import DPCL
    from tools import bench_configs as bc
    from utils.trainer import Front_Separator_Inference
    tmp = tempfile.mkdtemp(prefix='ams_sb_')
    B, F = 64, 256
    tr0, tfds0, a = bc._front_dpcl_checkpoint(tmp, DPCL, 'front_DPCL', B, S, L, F)
    with tr0.graph.as_default():
        tr0.model.create_saver()
        tr0.model.save(0)
        folder = tr0.model._dir()
    del tr0
    a.update(model_folder=folder, nb_tries=10, nb_steps=10, end_assign=True, out=False, kmeans_seeding='fast')
    for k in ('mix', 'non_mix', 'ind'):
        a.pop(k, None)
    tr = Front_Separator_Inference(DPCL, 'front_DPCL_inference', **a)
    model = tr.prepare_inference()
    x = 0.1 * torch.randn(N, device='cuda')
    with tr.graph.as_default():
        for _ in range(2):
            out = model.separate_recording(x)
        ms = _median_ms(lambda: model.separate_recording(x), reps)
    if not bool(torch.isfinite(out).all()):
        raise FloatingPointError('separate_recording returned non-finite samples')
    return {'separate_recording_ms': round(ms, 3), 'model': 'front_DPCL inference, batch %d, %d filters' % (B, F), 'kmeans_seeding': a['kmeans_seeding'],
            'seconds_of_audio_per_s': round(N / 8000.0 / (ms * 1e-3), 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--no-model', action='store_true', help='the four kernel groups only')
    args = ap.parse_args()
    os.environ.setdefault('AMS_LOG_DIR', tempfile.mkdtemp(prefix='ams_sb_log_'))     # (before config is imported)
    with contextlib.redirect_stdout(sys.stderr):
        C, r = kernels(args.reps)
        if not args.no_model:
            r.update(end_to_end(max(args.reps // 4, 3)))
    print(json.dumps(dict(bench='stitch', nb_speakers=S, chunk_size=L, hop=H, samples=N, chunks=C, reps=args.reps,
                          hbm_peak_tb_s=HBM_PEAK / 1e12, **r)), flush=True)


if __name__ == '__main__':
    main()
