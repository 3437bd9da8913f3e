"""Times the deep-attractor reconstruction loss of L41ModelV2 (csrc/danet.hip) at the bench shape -- B = 64, T*F = 79 * 257, E = 40,
S = 2 -- against its HBM traffic bound and against a torch composition of the same term, and the STFT_L41V2 training step under
hipGraph replay against the STFT_L41 step (the difference is the cost of the reconstruction chain inside a step).

  python tools/danet_bench.py --mode kernels [--iters 50]          one JSON line per launch group, then the torch composition
  python tools/danet_bench.py --mode step [--steps 200] [--rounds 3]   STFT_L41 / STFT_L41V2 replayed steps, alternating

Bytes are the algorithmic HBM bytes of each group (V once per reading pass, dV once -- twice when it is added to the gradient that is
already there --, g / y / x small); 'of_hbm' is that bound at 6.3 TB/s over the measured time.
"""
import argparse
import json
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'adaptive-multispeaker-separation_amd'))

import torch  # noqa: E402

HBM = 6.3e12


def _time(fn, iters):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def _row(name, ms, nbytes, **kw):
    r = dict(name=name, ms=round(ms, 4), mbytes=round(nbytes / 1e6, 1), bound_ms=round(nbytes / HBM * 1e3, 4),
             of_hbm=round(nbytes / HBM * 1e3 / ms, 3), **kw)
    print(json.dumps(r), flush=True)
    return r


def bench_kernels(B, T, Fq, E, S, iters, silence):
    from ams_hip import functional as F, ops as K
    d = torch.device('cuda')
    TF = T * Fq
    torch.manual_seed(0)
    v = torch.randn(B, TF, E, device=d) * 0.3
    lab = torch.randint(0, S, (B, TF), device=d)
    y = torch.nn.functional.one_hot(lab, S).float() * 2.0 - 1.0
    xin = torch.rand(B, TF, device=d)
    xnm = torch.rand(B, S, TF, device=d)                                  # the rows the STFT writes
    xs, thr = (xin, 2.0) if silence else (None, None)
    up = torch.ones(1, device=d)
    fV, fS, f1 = 4.0 * B * TF * E, 4.0 * B * TF * S, 4.0 * B * TF
    rows = []
    rows.append(_row('forward, cost only (attractor pass + reconstruction pass)', _time(
        lambda: K.danet_recon_fwd(v, y, xin, xnm, xs, thr, want_grad=False), iters), 2 * fV + 2 * fS + f1 * (1 + (2 if silence else 0))))
    cost, attr, g, dattr = K.danet_recon_fwd(v, y, xin, xnm, xs, thr)
    rows.append(_row('forward of a training step (+ g, dA)', _time(
        lambda: K.danet_recon_fwd(v, y, xin, xnm, xs, thr), iters), 2 * fV + 3 * fS + f1 * (1 + (2 if silence else 0))))
    rows.append(_row('backward, written', _time(
        lambda: K.danet_recon_bwd(y, g, attr, dattr, up, xs, thr), iters), fV + 2 * fS + (f1 * 2 if silence else 0)))
    demb = torch.zeros(B, TF, E, device=d)
    rows.append(_row('backward, added to the gradient in place', _time(
        lambda: K.danet_recon_bwd(y, g, attr, dattr, up, xs, thr, into=demb), iters), 2 * fV + 2 * fS + (f1 * 2 if silence else 0)))

    def separate_form():                                                  # what two autograd nodes would do: write, torch add, measure the bound
        dv = K.danet_recon_bwd(y, g, attr, dattr, up, xs, thr)
        demb.add_(dv)
        K.absmax(demb)
    rows.append(_row('backward, written + torch add_ + absmax pass (the unfolded form)', _time(separate_form, iters),
                     5 * fV + 2 * fS + (f1 * 2 if silence else 0)))

    vg = v.clone().requires_grad_()

    def hip_chain():
        vg.grad = None
        F.danet_recon_loss(vg, y, xin, xnm, xs, thr).backward()
    t_hip = _time(hip_chain, iters)
    rows.append(_row('HIP chain: forward + backward through autograd', t_hip, 3 * fV + 5 * fS + f1))

    xnm_t = xnm.permute(0, 2, 1)                                          # [B,TF,S] view, as the separator holds it

    def torch_chain():
        vg.grad = None
        m = (y + 1.0) * 0.5
        if silence:
            ax = xs.abs()
            m = m * (torch.log10(ax.amax(1, keepdim=True) / ax) < thr).float().unsqueeze(-1)
        den = 1e-12 + m.sum(1)
        A = torch.einsum('bpe,bps->bes', vg, m) / den.unsqueeze(1)
        a = torch.sigmoid(torch.einsum('bes,bpe->bps', A, vg))
        ((xnm_t - xin.unsqueeze(-1) * a) ** 2).mean(1).mean(-1).mean().backward()
    t_torch = _time(torch_chain, iters)
    rows.append(_row('torch composition (einsum + sigmoid, float32): forward + backward', t_torch, 3 * fV + 5 * fS + f1,
                     hip_over_torch=round(t_hip / t_torch, 3)))
    hip_chain()
    gh = vg.grad.clone()
    torch_chain()
    err = float((gh - vg.grad).abs().max() / vg.grad.abs().max())
    print(json.dumps({'name': 'HIP against torch gradient, max relative to the largest entry', 'value': err}), flush=True)
    if not t_hip <= t_torch:
        raise SystemExit('the HIP chain (%.4f ms) is slower than the torch composition (%.4f ms)' % (t_hip, t_torch))
    return rows


def bench_step(steps, warmup, rounds, B):
    from tools import bench_configs as BC
    from models.L41 import L41Model
    from models.SC_V2 import L41ModelV2
    from utils.trainer import STFT_Separator_Trainer
    os.environ.setdefault('AMS_LOG_DIR', tempfile.mkdtemp(prefix='ams_db_log_'))
    L, S = 20480, 2
    built = {}
    for name, cls, typ in (('STFT_L41', L41Model, 'STFT_L41'), ('STFT_L41V2', L41ModelV2, 'STFT_DANet_SCE')):
        a = BC._args(window_size=512, hop_size=256, chunk_size=L, batch_size=B, nb_speakers=S, layer_size=600, nb_layers=3,
                     embedding_size=40, model_folder=None, learning_rate=1e-3, pretraining=False, tot_speakers=251, hip_graph=True)
        for k in ('filters', 'max_pool', 'type'):
            a.pop(k)
        tr = STFT_Separator_Trainer(cls, typ, **a)
        dist, tfds = tr.prepare()
        BC._time_train(tr, tfds, L, 5, max(warmup, 4))                     # capture, and let the step choose its product form
        built[name] = (tr, tfds)
    out = []
    for r in range(rounds):
        for name in ('STFT_L41', 'STFT_L41V2'):
            tr, tfds = built[name]
            dt, c = BC._time_train(tr, tfds, L, steps, 2)
            row = {'round': r, 'name': name + '_graph', 'ms_per_step': round(dt * 1e3, 4), 'cost': float('%.6g' % c)}
            print(json.dumps(row), flush=True)
            out.append(row)
    med = {n: sorted(x['ms_per_step'] for x in out if x['name'] == n + '_graph')[rounds // 2] for n in built}
    print(json.dumps({'name': 'median', 'STFT_L41_ms': med['STFT_L41'], 'STFT_L41V2_ms': med['STFT_L41V2'],
                      'reconstruction_chain_ms': round(med['STFT_L41V2'] - med['STFT_L41'], 4)}), flush=True)
    return out


def main():
    p = argparse.ArgumentParser()
    p.add_argument('--mode', choices=['kernels', 'step'], default='kernels')
    p.add_argument('--batch', type=int, default=64)
    p.add_argument('--T', type=int, default=79)
    p.add_argument('--F', type=int, default=257)
    p.add_argument('--E', type=int, default=40)
    p.add_argument('--S', type=int, default=2)
    p.add_argument('--iters', type=int, default=50)
    p.add_argument('--silence', action='store_true')
    p.add_argument('--steps', type=int, default=200)
    p.add_argument('--warmup', type=int, default=4)
    p.add_argument('--rounds', type=int, default=3)
    a = p.parse_args()
    if a.mode == 'kernels':
        bench_kernels(a.batch, a.T, a.F, a.E, a.S, a.iters, a.silence)
    else:
        bench_step(a.steps, a.warmup, a.rounds, a.batch)


if __name__ == '__main__':
    main()
