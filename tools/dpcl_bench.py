"""The fused l2-normalise + DPCL loss kernels alone at the B = 64 step's shape (64 x 20480 points x 40, S = 2): us per launch and
algorithmic GB/s, the streamed backward (default) against the register-fed one (AMS_DPCL_STREAM=0) IN ONE PROCESS.

    python tools/dpcl_bench.py [--launches 200] [--runs 2] [--sets 3] [--out FILE]

The switch is read once per library image, so the register-fed arm runs from a second image of the same library file (a copy under
another name, loaded with the switch set).  Every launch is timed with its own pair of events; the launches rotate over `--sets`
independent U / dU sets (3 x 420 MB: no launch finds its U in the 256 MB Infinity Cache).  Reported: the median launch of each run, and
the median of the runs.  (AMS_HIP_LIB selects a variant library for the default arm.)"""
import argparse
import ctypes
import os
import shutil
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'adaptive-multispeaker-separation_amd')]
from ams_hip import _lib, ops  # noqa: E402


def second_image(tmp):
    """The library once more under another name, with AMS_DPCL_STREAM=0 in force when it first reads its environment."""
    path = os.path.join(tmp, 'libams_hip_register_arm.so')
    shutil.copy(_lib.LIB_PATH, path)
    lib = ctypes.CDLL(path)
    for name, (ret, argtypes) in _lib.parse_header().items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = ret, argtypes
    return lib


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--launches', type=int, default=200)
    ap.add_argument('--runs', type=int, default=2)
    ap.add_argument('--sets', type=int, default=3)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    B, TF, E, S = 64, 20480, 40, 2
    g = torch.Generator(device='cuda').manual_seed(0)
    Us = [torch.randn(B, TF, E, device='cuda', generator=g) for _ in range(a.sets)]
    dUs = [torch.empty_like(u) for u in Us]
    Y = torch.zeros(B, TF, S, device='cuda')
    Y[..., 0] = (torch.rand(B, TF, device='cuda', generator=g) > 0.5).float()
    Y[..., 1] = 1 - Y[..., 0]
    up = torch.ones(1, device='cuda')
    fw = [ops.dpcl_loss_fwd_u(u, Y) for u in Us]                 # (out, inv, None, ws) per set
    lib_new = ops.load()
    geo = (ctypes.c_int * 5)()
    assert lib_new.ams_dpcl_stream_geometry(geo) == 1, 'unset AMS_DPCL_STREAM: the default arm is the streamed one'
    p, s = ops._p, ops._s
    with tempfile.TemporaryDirectory(prefix='ams_dpcl_') as tmp:
        os.environ['AMS_DPCL_STREAM'] = '0'
        lib_old = second_image(tmp)
        assert lib_old.ams_dpcl_stream_geometry(geo) == 0
        del os.environ['AMS_DPCL_STREAM']

        def bwd(lib):
            def f(k):
                st = lib.ams_dpcl_loss_bwd_u(p(Us[k]), p(Y), p(fw[k][1]), p(up), p(dUs[k]), B, TF, E, S, p(fw[k][3]), s())
                assert st == 0, st
            return f

        def gram(k):
            ops.dpcl_loss_fwd_u(Us[k], Y)

        def run(fn):
            for i in range(20):
                fn(i % a.sets)
            torch.cuda.synchronize()
            ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(a.launches)]
            for i, (e0, e1) in enumerate(ev):
                e0.record()
                fn(i % a.sets)
                e1.record()
            torch.cuda.synchronize()
            return float(np.median([e0.elapsed_time(e1) * 1e3 for e0, e1 in ev]))

        # bits first: both arms on the same inputs and workspace
        bwd(lib_old)(0)
        ref = dUs[0].clone()
        dUs[0].fill_(float('nan'))
        bwd(lib_new)(0)
        torch.cuda.synchronize()
        same = bool(torch.equal(ref.view(torch.int32), dUs[0].view(torch.int32)))
        rows = []
        arms = [('dpcl_bwd_u  register-fed (AMS_DPCL_STREAM=0)', bwd(lib_old), 4.0 * B * TF * (2 * E + S + 1)),
                ('dpcl_bwd_u  streamed (default)', bwd(lib_new), 4.0 * B * TF * (2 * E + S + 1)),
                ('dpcl_gram_u (one arm)', gram, 4.0 * B * TF * (E + S + 1))]
        meds = {name: [] for name, _, _ in arms}
        for _ in range(a.runs):                                  # the arms alternate inside every run
            for name, fn, _ in arms:
                meds[name].append(run(fn))
        for name, _, nbytes in arms:
            m = float(np.median(meds[name]))
            rows.append('%-48s %s  median %7.1f us  %6.0f GB/s' % (name, ' '.join('%7.1f' % v for v in meds[name]), m, nbytes / m * 1e-3))
    head = ['shape B %d TF %d E %d S %d; %d launches per run over %d U / dU sets, per-launch events; us per launch: runs, median of runs'
            % (B, TF, E, S, a.launches, a.sets),
            'streamed geometry: %d points per workgroup, depth %d, %d workgroups per CU; dU bit-equal between the arms: %s'
            % (geo[0], geo[1], geo[2], same)]
    text = '\n'.join(head + rows)
    print(text)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
