"""Times the two input paths of the record datasets (data/dataset.py) on a synthetic record set written to a temporary directory:
the host pipeline (decode -> shuffle -> chunk -> zip -> numpy sum -> batch -> three uploads) and the device-resident path
(data/resident.py: pool uploaded once, a pass planned as an index table, one ams_mix_gather launch per batch).

  python tools/data_bench.py [--batch 64] [--speakers 2] [--chunk 20480] [--utterances 60] [--normalize] [--passes 2]

One JSON line:
  host_ms_per_batch       wall clock of a whole host-path pass over its batches, uploads included (device synchronised at the end)
  resident_ms_per_batch   the same for the resident path over `--passes` reshuffled passes, each pass's planning and table upload included
  plan_ms_per_pass        the planning + table upload share of that
  kernel_us               one gather launch, from a captured graph of 50 launches over different batches and output buffers
  kernel_gbps, of_hbm     (2 S + 1) B L 4 bytes over kernel_us; against 5.9 TB/s, the rate amsgrad_kernel reaches
  load_s, pool_bytes      one-time read + normalise + upload of the split, and the size of the device pool
The synthetic pool is tens of MB and stays in the 256 MiB last-level cache: the kernel's reads are served from there, its writes go to
fresh buffers.  At ~26 MB per launch the kernel is of the order of a launch's fixed cost; the figure is reported, not tuned.
"""
import argparse
import json
import os
import shutil
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'adaptive-multispeaker-separation_amd'))

import numpy as np  # noqa: E402
import torch  # noqa: E402

RATE = 5.9e12


def write_records(folder, utterances, L, seed=0):
    from data import tfrecord
    rng = np.random.RandomState(seed)
    for g, base in (('M', 0), ('F', 1000)):
        items = [((0.05 * rng.randn(rng.randint(3 * L, 8 * L))).astype(np.float32), base + i // 2) for i in range(utterances)]
        tfrecord.write_audio_records(os.path.join(folder, 'train_%s.tfrecords' % g), items)


def run_pass(ds, L):
    """All batches of one pass through TFDataset._next; returns (batches, seconds), device synchronised."""
    from ams_hip.graph import Run
    t0 = time.perf_counter()
    ds.initialize(ds.TRAIN)
    n = 0
    while True:
        try:
            ds._next(Run({ds.handle: ds.TRAIN, ds.chunk_size: L}, new_pass=False))
        except StopIteration:
            break
        n += 1
    torch.cuda.synchronize()
    return n, time.perf_counter() - t0


def kernel_time(ds, L, launches=50, replays=20):
    from ams_hip import load
    import ctypes
    vp = ctypes.c_void_p
    rec, plan = ds._plan(ds.TRAIN, L, 0)
    B, S = ds.batch_size, ds.S
    full = [k for k in range(plan.nb_batches) if plan.batch(k)[1] == B]
    outs = [(torch.empty(B * L + B * S * L, device=rec.pool.device), torch.empty((B, S), dtype=torch.int32, device=rec.pool.device))
            for _ in range(launches)]
    lib = load()
    side = torch.cuda.Stream()

    def enqueue():
        st = vp(torch.cuda.current_stream().cuda_stream)
        for i, (flat, ind) in enumerate(outs):
            first = plan.batch(full[i % len(full)])[0]
            rc = lib.ams_mix_gather(vp(rec.pool.data_ptr()), vp(rec.utt_off_dev.data_ptr()), vp(plan.table_dev.data_ptr()),
                                    vp(plan.keys_dev.data_ptr()), first, vp(flat.data_ptr()), vp(flat.data_ptr() + 4 * B * L),
                                    vp(ind.data_ptr()), B, S, L, st)
            assert rc == 0, rc
    with torch.cuda.stream(side):
        enqueue()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        enqueue()
    g.replay()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(replays):
        g.replay()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / (replays * launches)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=64)
    ap.add_argument('--speakers', type=int, default=2)
    ap.add_argument('--chunk', type=int, default=20480)
    ap.add_argument('--utterances', type=int, default=60, help='per gender file')
    ap.add_argument('--normalize', action='store_true')
    ap.add_argument('--passes', type=int, default=2)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('data_bench needs the GPU: it times uploads and a kernel')
    from ams_hip.graph import Graph
    from data.dataset import TFDataset
    B, S, L = args.batch, args.speakers, args.chunk
    tmp = tempfile.mkdtemp(prefix='ams_data_bench_')
    try:
        write_records(tmp, args.utterances, L)
        os.environ['AMS_DATA_DIR'] = tmp
        kw = dict(batch_size=B, nb_speakers=S, chunk_size=L, dataset='records', dataset_normalize=args.normalize)
        with Graph().as_default():
            host, res = TFDataset(resident=False, **kw), TFDataset(resident=True, **kw)
        torch.zeros(1, device='cuda')
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res._plan(res.TRAIN, L, 0)                               # loads the pool (and plans epoch 0)
        torch.cuda.synchronize()
        load_s = time.perf_counter() - t0
        rec = res._pools[res.TRAIN]
        run_pass(res, L)                                         # warm-up: code object, allocator
        n_res = t_res = t_plan = 0
        for _ in range(args.passes):
            epoch = res._epochs[res.TRAIN] + 1
            t0 = time.perf_counter()
            res._plan(res.TRAIN, L, epoch)                       # what the pass below will ask for first: timed here and inside it
            torch.cuda.synchronize()
            t_plan += time.perf_counter() - t0
            res._plans.clear()
            n, t = run_pass(res, L)
            n_res, t_res = n_res + n, t_res + t
        n_host, t_host = run_pass(host, L)
        us = kernel_time(res, L)
        nbytes = (2 * S + 1) * B * L * 4
        print(json.dumps(dict(B=B, S=S, L=L, normalize=bool(args.normalize), batches_per_pass=n_host,
                              host_ms_per_batch=round(1e3 * t_host / max(n_host, 1), 3),
                              resident_ms_per_batch=round(1e3 * t_res / max(n_res, 1), 4),
                              plan_ms_per_pass=round(1e3 * t_plan / args.passes, 3),
                              kernel_us=round(us, 2), kernel_mbytes=round(nbytes / 1e6, 2), kernel_gbps=round(nbytes / us / 1e3, 1),
                              of_hbm=round(nbytes / (us * 1e-6) / RATE, 3), load_s=round(load_s, 3), pool_bytes=rec.pool_bytes)))
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == '__main__':
    main()
