"""Micro-benchmark: forward products from pre-split fp16 operand images (csrc/gemm_ps.hip) beside the in-product fp16x3 form
(csrc/gemm.hip), at the benchmark's forward shapes; pack launches timed separately.

    python tools/gemm_ps_bench.py [--reps 200]

--dx: the backward dX products in the image form instead (include/ams.h: ams_gemm_ps_a_f32), launch + slab reduce as the step runs them, the
two step shapes by default, for whichever plan the process's AMS_GEMM_DX_TILE gives (unset: the model; 256 / 320):

    python tools/gemm_ps_bench.py --dx                                     # the library of this tree
    AMS_GEMM_DX_TILE=256 python tools/gemm_ps_bench.py --dx                # the 128 x 256 tile and its slab rule
    python tools/gemm_ps_bench.py --dx --lib /path/to/other/libams_hip.so  # another build's kernels (the parent commit's) on the same operands

Operands and the weight image come from this tree's library (the image bytes are the same in every build); --lib only supplies
ams_gemm_ps_a_workspace_bytes / ams_gemm_ps_a_f32, loaded beside it.  One JSON line per shape: the plan (when the library has
ams_gemm_ps_a_plan) and, over --reps launches with events around each, min / median / p90 / max in microseconds.
"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'adaptive-multispeaker-separation_amd')]
from ams_hip import ops  # noqa: E402

SHAPES = [('dense fwd  x.W', 5120, 10240, 600), ('proj l2,3  x.Wx', 5120, 2400, 600), ('proj l1    x.Wx', 5120, 2400, 256),
          ('cfg5 dense', 10240, 20480, 600), ('square 4096', 4096, 4096, 4096)]


def timed(fn, reps, warm):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3


def main_dx(a):
    lib = ops.load()
    if a.lib:
        lib = ctypes.CDLL(a.lib)
        lib.ams_gemm_ps_a_workspace_bytes.restype = ctypes.c_size_t
        lib.ams_gemm_ps_a_workspace_bytes.argtypes = [ctypes.c_int] * 3
        lib.ams_gemm_ps_a_f32.restype = ctypes.c_int32
        lib.ams_gemm_ps_a_f32.argtypes = ([ctypes.c_int] * 3 + [ctypes.c_void_p, ctypes.c_long, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_long] +
                                          [ctypes.c_void_p] * 3 + [ctypes.c_size_t, ctypes.c_void_p])
    has_plan = hasattr(lib, 'ams_gemm_ps_a_plan')
    if a.lib and has_plan:
        lib.ams_gemm_ps_a_plan.restype = ctypes.c_int32
        lib.ams_gemm_ps_a_plan.argtypes = [ctypes.c_int] * 3 + [ctypes.c_size_t] + [ctypes.c_void_p] * 3
    for shape in a.shapes.split(','):
        M, N, K = (int(v) for v in shape.split('x'))
        rng = np.random.RandomState(M + N + K)
        dU = torch.from_numpy((rng.randn(M, K) * np.exp(rng.randn(M, K))).astype(np.float32)).cuda()
        W = torch.from_numpy((rng.randn(N, K) * 0.05).astype(np.float32)).cuda()
        am = (ops.absmax(dU), ops.absmax(W))
        img = ops.ps_pack_rows(W, am[1])
        nb = lib.ams_gemm_ps_a_workspace_bytes(M, N, K)
        ws = torch.empty(max(nb, 16) // 4, dtype=torch.float32, device='cuda')
        out = torch.empty((M, N), dtype=torch.float32, device='cuda')
        plan = None
        if has_plan:
            t, s, k = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
            ops.check(lib.ams_gemm_ps_a_plan(M, N, K, nb, ctypes.byref(t), ctypes.byref(s), ctypes.byref(k)), 'ams_gemm_ps_a_plan')
            plan = dict(tile_n=t.value, splits=s.value, kps=k.value)

        def run():
            ops.check(lib.ams_gemm_ps_a_f32(M, N, K, ops._p(dU), K, ops._p(img), ops._p(out), N, ops._p(am[0]), ops._p(am[1]), ops._p(ws), nb,
                                            ops._s()), 'ams_gemm_ps_a_f32')
        for _ in range(a.warm):
            run()
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(a.reps)]
        for b, e in ev:
            b.record()
            run()
            e.record()
        torch.cuda.synchronize()
        us = np.sort(np.array([b.elapsed_time(e) * 1e3 for b, e in ev]))
        ref = dU[:64].double() @ W.double().t()
        err = float((out[:64].double() - ref).abs().max() / ref.abs().max())
        print(json.dumps(dict(shape=[M, N, K], lib=a.lib or 'own', dx_tile_env=os.environ.get('AMS_GEMM_DX_TILE'), plan=plan,
                              ws_bytes=int(nb), us_min=round(float(us[0]), 1), us_median=round(float(np.median(us)), 1),
                              us_p90=round(float(us[int(0.9 * len(us))]), 1), us_max=round(float(us[-1]), 1), reps=a.reps,
                              rel_err_rows0_63=err)), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=200)
    ap.add_argument('--warm', type=int, default=100)
    ap.add_argument('--only', default='')
    ap.add_argument('--dx', action='store_true')
    ap.add_argument('--shapes', default='5120x600x10240,5120x600x2400')
    ap.add_argument('--lib', default=None)
    a = ap.parse_args()
    if a.dx:
        return main_dx(a)
    rng = np.random.RandomState(0)
    for label, M, N, K in SHAPES:
        if a.only and a.only not in label:
            continue
        A = torch.from_numpy(rng.rand(M, K).astype(np.float32) * 2 - 1).cuda()
        W = torch.from_numpy((rng.randn(K, N) * 0.05).astype(np.float32)).cuda()
        bias = torch.zeros(N, device='cuda')
        out = torch.empty(M, N, device='cuda')
        am = (ops.absmax(A), ops.absmax(W))
        ai, bi = ops.ps_pack_rows(A, am[0]), ops.ps_pack_cols(W, am[1])
        t_ps = timed(lambda: ops.gemm_ps(ai, bi, K, am, bias=bias, out=out), a.reps, a.warm)
        t_g = timed(lambda: ops.gemm(A, W, bias=bias, out=out, amax=am), a.reps, a.warm)
        t_pr = timed(lambda: ops.ps_pack_rows(A, am[0], img=ai), a.reps, a.warm)
        t_pc = timed(lambda: ops.ps_pack_cols(W, am[1], img=bi), a.reps, a.warm)
        fl = 2.0 * M * N * K
        print('%-18s M=%5d N=%5d K=%4d  pre-split %7.1f us (%6.1f TF f32-eq, %.3f of the 16-bit pipe)   in-product %7.1f us (%6.1f TF)   '
              'pack rows %5.1f us  pack cols %5.1f us' % (label, M, N, K, t_ps, fl / t_ps * 1e-6, 3 * fl / t_ps * 1e-6 / 2500.0, t_g,
                                                          fl / t_g * 1e-6, t_pr, t_pc), flush=True)


if __name__ == '__main__':
    main()
