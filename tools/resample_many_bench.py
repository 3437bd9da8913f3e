"""The ragged resampler against one resampler call per recording: one JSON line.

The workload: R = 256 recordings whose durations are the 256 lengths of tools/stitch_many_bench.py (RandomState(7).randint(32000, 96001)
samples at 8 kHz: 4 .. 12 s), as int16 stereo frames at rates that cycle through 16000 / 44100 / 48000 / 8000 Hz; S = 2 tracks back.
    (a) in_loop    per recording: an upload and resample.from_pcm16                 what separate_recordings did before the ragged form
    (b) in_ragged  resample_ragged.to_model_rate: one upload, one table, ONE launch
    (c) out_loop   per recording: resample.resample and the cut [:, :n_out].contiguous()
    (d) out_ragged resample_ragged.from_model_rate: one table, ONE launch (the cut is n_keep)
(a) and (b) with the uploads (host frames in) and without them (device frames in); the way back has no data upload, (d) includes its
table upload.  The same four at R = 1 (the first recording).  End to end with the front_DPCL inference model of tools/bench_configs.py
(--kmeans_seeding fast, batch 64): the loop of one separate_recordings call per distinct rate that
experiments/evaluation/separate_many.py makes without --one_stream, against ONE call with fs=[...].

Medians of --reps ALTERNATED repetitions (a, b, c, d, a, b, ...), each host-timed between two device synchronisations, after two warm-up
rounds; `spread` is [min, max] of the same repetitions.  Beside the times: the kernel launches of each form and the call's algorithmic
bytes over the 8.0 TB/s peak.  `ragged_wins`: (a) + (c) exceeds (b) + (d), with the uploads, at R = 256, by more than the widest
spread (max - min) of the four.  No threshold: the line says which way it went.

usage: python tools/resample_many_bench.py [--reps 10] [--recordings 256] [--no_model]"""
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

S, L, H, B = 2, 20480, 10240, 64
RATES = (16000, 44100, 48000, 8000)
FS = 8000
PEAK = 8.0e12                                                      # bytes per second


def _alternated(fns, reps, warm=2):
    """{name: (median ms, [min, max])} of reps rounds in which every function runs once, in turn."""
    import torch
    times = {k: [] for k in fns}
    for i in range(warm + reps):
        for k, fn in fns.items():
            torch.cuda.synchronize()
            t = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if i >= warm:
                times[k].append((time.perf_counter() - t) * 1e3)
    return {k: (round(float(np.median(v)), 4), [round(min(v), 4), round(max(v), 4)]) for k, v in times.items()}


def _workload(R):
    lengths = np.random.RandomState(7).randint(32000, 96001, size=256)[:R]
    rates = [RATES[r % 4] for r in range(R)]
    rng = np.random.RandomState(8)
    frames = [rng.randint(-9000, 9000, size=(int(n) * fs // FS, 2)).astype(np.int16) for n, fs in zip(lengths, rates)]
    return frames, rates


def resampler(R, reps):
    import torch
    from ams_hip import resample as Rs
    from ams_hip import resample_ragged as Rr
    from ams_hip import stitch_batch as sb
    frames, rates = _workload(R)
    dev = [torch.from_numpy(f).cuda() for f in frames]
    N = [f.shape[0] for f in frames]
    lay = sb.layout(Rr.model_lengths(N, rates, FS), L, H, S)
    gen = torch.Generator(device='cuda').manual_seed(9)
    out = 0.1 * torch.randn(lay.out_total, device='cuda', generator=gen)
    views = [out[int(o):int(o) + S * int(n)].view(S, int(n)) for o, n in zip(lay.out_off, lay.n)]

    def in_loop(up):
        ys = []
        for f, d, fs in zip(frames, dev, rates):
            x = torch.from_numpy(np.array(f)).cuda().contiguous() if up else d
            ys.append(Rs.from_pcm16(x, fs, FS))
        return ys

    def out_loop():
        res = []
        for v, n, fs in zip(views, N, rates):
            if fs == FS:
                res.append(v)
                continue
            y = Rs.resample(v.contiguous(), FS, fs)
            res.append(y[:, :n].contiguous() if n < y.shape[1] else y)
        return res
    in_ragged = lambda up: Rr.to_model_rate(frames if up else dev, rates, lay=lay, fs_model=FS)      # noqa: E731
    out_ragged = lambda: Rr.from_model_rate(out, lay, S, rates, N, fs_model=FS)                     # noqa: E731
    # the two forms agree, bit for bit, before anything is timed
    xp = in_ragged(True)[0]
    assert torch.equal(xp, sb.pack(in_loop(False), lay)) and torch.equal(xp, in_ragged(False)[0])
    for a, b in zip(out_loop(), out_ragged()):
        assert torch.equal(a, b)
    n0 = Rr.LAUNCHES
    in_ragged(True)
    out_ragged()
    ragged_launches = Rr.LAUNCHES - n0
    t = _alternated({'in_loop_upload': lambda: in_loop(True), 'in_ragged_upload': lambda: in_ragged(True),
                     'in_loop': lambda: in_loop(False), 'in_ragged': lambda: in_ragged(False),
                     'out_loop': out_loop, 'out_ragged': out_ragged}, reps)
    back = [r for r in range(R) if rates[r] != FS]
    bytes_in = sum(2 * 2 * n for n in N) + 4 * int(lay.n.sum())
    bytes_out = sum(4 * S * int(lay.n[r]) + 4 * S * N[r] for r in back)
    res = dict(recordings=R, frames=int(sum(N)), seconds_of_audio=round(sum(n / fs for n, fs in zip(N, rates)), 1),
               launches=dict(in_loop=R, in_ragged=1, out_loop='%d resample + %d cut' % (len(back), len(back)), out_ragged=1,
                             ragged_counted=ragged_launches),
               bytes_in=bytes_in, bytes_out=bytes_out, in_at_peak_ms=round(bytes_in / PEAK * 1e3, 4), out_at_peak_ms=round(bytes_out / PEAK * 1e3, 4))
    for k, (med, spread) in t.items():
        res[k + '_ms'], res[k + '_spread'] = med, spread
    loop, ragged = t['in_loop_upload'][0] + t['out_loop'][0], t['in_ragged_upload'][0] + t['out_ragged'][0]
    widest = max(t[k][1][1] - t[k][1][0] for k in ('in_loop_upload', 'out_loop', 'in_ragged_upload', 'out_ragged'))
    res.update(loop_ms=round(loop, 4), ragged_ms=round(ragged, 4), widest_spread_ms=round(widest, 4), ragged_wins=bool(loop - ragged > widest))
    return res


def end_to_end(R, reps):
    import torch
    from tools.stitch_many_bench import _model, _passes
    frames, rates = _workload(R)
    tr, model, seeding = _model()
    by_rate = lambda: [model.separate_recordings([frames[i] for i in range(R) if rates[i] == fs], fs=fs)      # noqa: E731
                       for fs in sorted(set(rates))]
    one = lambda: model.separate_recordings(frames, fs=rates)                                                # noqa: E731
    with tr.graph.as_default():
        p_loop, p_one = _passes(model, by_rate), _passes(model, one)
        if not all(bool(torch.isfinite(o).all()) for o in one()):
            raise FloatingPointError('separate_recordings returned non-finite samples')
        t = _alternated({'by_rate': by_rate, 'one_call': one}, reps, warm=1)
    return dict(model='front_DPCL inference, batch %d' % B, kmeans_seeding=seeding, by_rate_calls=len(set(rates)), by_rate_passes=p_loop,
                one_call_passes=p_one, by_rate_ms=t['by_rate'][0], by_rate_spread=t['by_rate'][1], one_call_ms=t['one_call'][0],
                one_call_spread=t['one_call'][1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--recordings', type=int, default=256)
    ap.add_argument('--no_model', action='store_true', help='the resampler alone, without the end-to-end part')
    args = ap.parse_args()
    os.environ.setdefault('AMS_LOG_DIR', tempfile.mkdtemp(prefix='ams_rmb_log_'))    # (before config is imported)
    with contextlib.redirect_stdout(sys.stderr):
        many, single = resampler(args.recordings, args.reps), resampler(1, args.reps)
        e2e = None if args.no_model else end_to_end(args.recordings, min(args.reps, 5))
    print(json.dumps(dict(bench='resample_many', nb_speakers=S, chunk_size=L, hop=H, rates=list(RATES), reps=args.reps, peak_tb_s=PEAK / 1e12,
                          many=many, one=single, end_to_end=e2e, ragged_wins=many['ragged_wins'])), flush=True)
    return 0


if __name__ == '__main__':
    sys.exit(main())
