"""Times the dilated conv2d stack (--add_dilated, csrc/conv2d.hip) layer by layer -- forward, dX, dW -- in each arithmetic class.
TFLOP/s are f32-equivalent with all taps counted (padding included); 'of_f16x3_peak' is the fraction of the fp16x3 rate, 2500/3 TFLOP/s.

  python tools/dilated_bench.py [--batch 64] [--iters 5] [--classes f16x3,bf16x6,f32] [--out rows.json]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'adaptive-multispeaker-separation_amd'))

import numpy as np  # noqa: E402
import torch  # noqa: E402

SPECS = [((1, 7), (1, 1), 128), ((7, 1), (1, 1), 128)] + [((5, 5), (r, 1), 128) for r in (4, 8, 16, 32)] + \
        [((5, 5), (r, r), 128) for r in (1, 2, 4, 8, 16, 32)] + [((5, 5), (1, 1), 4)]
F16X3_PEAK = 2500.0 / 3


def _time(fn, iters):
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def bench_layers(B, T, F, iters, classes):
    from ams_hip import ops, _lib
    lib = _lib.load()
    d = torch.device('cuda')
    rng = np.random.RandomState(0)
    rows = []
    old = lib.ams_gemm_get_arith()
    try:
        for cls in classes:
            lib.ams_gemm_set_arith(0 if cls == 'f32' else 1)
            tot = {'fwd': 0.0, 'dX': 0.0, 'dW': 0.0}
            cin = 1
            for l, ((kh, kw), rate, cout) in enumerate(SPECS):
                lim = np.sqrt(6.0 / (kh * kw * (cin + cout)))
                w = torch.from_numpy(rng.uniform(-lim, lim, (kh, kw, cin, cout)).astype(np.float32)).to(d)
                b = torch.zeros(cout, device=d)
                x = torch.rand(B, T, F, cin, device=d)
                dy = torch.randn(B, T, F, cout, device=d)
                bx, bw, bd = ops.absmax(x), ops.absmax(w), ops.absmax(dy)
                am = (lambda p, q: (p, q)) if cls == 'f16x3' else (lambda p, q: None)
                flop = 2.0 * B * T * F * kh * kw * cin * cout
                r = {'class': cls, 'layer': l + 1, 'kernel': [kh, kw], 'rate': list(rate), 'cin': cin, 'cout': cout}
                r['fwd_ms'] = _time(lambda: ops.dilated_conv2d_fwd(x, w, b, rate, amax=am(bx, bw)), iters)
                r['dW_ms'] = _time(lambda: ops.dilated_conv2d_bwd_filter(x, dy, w, rate, amax=am(bx, bd)), iters)
                if l > 0:
                    r['dX_ms'] = _time(lambda: ops.dilated_conv2d_bwd_data(dy, w, x, rate, amax=am(bd, bw)), iters)
                for k in ('fwd', 'dX', 'dW'):
                    if k + '_ms' in r:
                        tf = flop / (r[k + '_ms'] * 1e-3) / 1e12
                        r[k + '_tflops'] = round(tf, 1)
                        r[k + '_of_f16x3_peak'] = round(tf / F16X3_PEAK, 3)
                        tot[k] += r[k + '_ms']
                        r[k + '_ms'] = round(r[k + '_ms'], 3)
                rows.append(r)
                print(json.dumps(r), flush=True)
                del x, dy, w
                cin = cout
            s = {'class': cls, 'stack_fwd_ms': round(tot['fwd'], 2), 'stack_bwd_ms': round(tot['dX'] + tot['dW'], 2),
                 'stack_fwd_bwd_ms': round(sum(tot.values()), 2)}
            rows.append(s)
            print(json.dumps(s), flush=True)
    finally:
        lib.ams_gemm_set_arith(old)
    return rows


def main():
    p = argparse.ArgumentParser()
    p.add_argument('--batch', type=int, default=64)
    p.add_argument('--T', type=int, default=79)
    p.add_argument('--F', type=int, default=257)
    p.add_argument('--iters', type=int, default=5)
    p.add_argument('--classes', default='f16x3,bf16x6,f32')
    p.add_argument('--out', default=None)
    a = p.parse_args()
    rows = bench_layers(a.batch, a.T, a.F, a.iters, a.classes.split(','))
    if a.out:
        with open(a.out, 'w') as f:
            json.dump(rows, f, indent=1)


if __name__ == '__main__':
    main()
