"""BSS-eval timing.  Default: the per-utterance call against the numpy oracle (one line of text, as before).
--batch U: U utterances (nsrc = 2, L = 20480) scored (a) by the per-utterance loop of experiments/evaluation/eval.py -- 2 U calls
of bss_eval_sources_cupy -- and (b) by one bss_eval_sources_batch call with two sets of estimates; one JSON line.  --once: one
batched call and nothing else (the run to put under rocprofv3 --kernel-trace --stats)."""
import sys, os, time
R=os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, R); sys.path.insert(0, R+'/adaptive-multispeaker-separation_amd')
import numpy as np, torch
from utils import bss_eval as hb
from oracle import bss_eval as ob


def single():
    rng=np.random.RandomState(0); S,L=2,20480
    s=rng.randn(S,L); est=s[::-1]+0.3*rng.randn(S,L)
    st=torch.tensor(s,device='cuda'); et=torch.tensor(est,device='cuda')
    for _ in range(3): hb.bss_eval_pairs(st,et)
    torch.cuda.synchronize(); t=time.time(); n=20
    for _ in range(n): hb.bss_eval_pairs(st,et)
    torch.cuda.synchronize(); g=(time.time()-t)/n
    t=time.time(); ob.bss_eval_sources(s,est); c=time.time()-t
    print('gpu ms per call (4 pairs, S=2, L=20480):', g*1e3, ' oracle numpy s:', c)


def _median_ms(fn, reps):
    out = []
    for _ in range(reps):
        torch.cuda.synchronize(); t = time.perf_counter()
        fn()
        torch.cuda.synchronize(); out.append((time.perf_counter() - t) * 1e3)
    return float(np.median(out))


def batch(U, reps, once):
    import json
    rng = np.random.RandomState(0); S, L = 2, 20480
    nm = rng.randn(U, S, L)
    for u in range(U):
        for k in range(S):
            nm[u, k] = np.convolve(nm[u, k], rng.randn(12), mode='same')
    refs = torch.tensor(nm, device='cuda')
    mix = refs.sum(1, keepdim=True).expand(-1, S, -1)
    sep = refs + 0.05 * torch.tensor(rng.randn(U, S, L), device='cuda')
    sets = torch.stack([mix, sep], dim=1).contiguous()                  # [U, 2, S, L]

    def batched():
        return hb.bss_eval_sources_batch(refs, sets)

    def loop():
        out = []
        for u in range(U):
            out.append((hb.bss_eval_sources_cupy(refs[u], mix[u], nsrc=S), hb.bss_eval_sources_cupy(refs[u], sep[u], nsrc=S)))
        return out
    if once:
        batched(); torch.cuda.synchronize()
        return
    b = batched(); a = loop()                                           # warm: plans, contexts, workspaces
    worst = max(np.abs(b[c][u, k] - a[u][k][c]).max() for u in range(U) for k in range(2) for c in range(2))      # sdr, sir
    t_loop = _median_ms(loop, reps)
    t_batch = _median_ms(batched, reps)
    # the factorisation kernels alone: the U + U*S matrices of one call, N^3 / 3 flop each
    N, F = S * hb.FLEN, hb.FLEN
    g = torch.randn(U, N, N + 8, device='cuda', dtype=torch.float64)
    big = g @ g.transpose(1, 2) / N + torch.eye(N, device='cuda', dtype=torch.float64)
    small = big[:, :F, :F].repeat(S, 1, 1).contiguous()
    lib = hb._load_batch()
    info = torch.empty(U * S, dtype=torch.int32, device='cuda')
    stream = torch.cuda.current_stream().cuda_stream

    def potrf():
        x, y = big.clone(), small.clone()
        torch.cuda.synchronize(); t = time.perf_counter()
        lib.ams_bssb_potrf(x.data_ptr(), N, N, N * N, U, info.data_ptr(), stream)
        lib.ams_bssb_potrf(y.data_ptr(), F, F, F * F, U * S, info.data_ptr(), stream)
        torch.cuda.synchronize()
        return (time.perf_counter() - t) * 1e3
    potrf()
    t_potrf = float(np.median([potrf() for _ in range(reps)]))
    flop = U * (N ** 3 / 3.0) + U * S * (F ** 3 / 3.0)
    print(json.dumps({'bench': 'bss_batch', 'utterances': U, 'nsrc': S, 'nsampl': L, 'flen': hb.FLEN, 'sets': 2, 'reps': reps,
                      'loop_ms': round(t_loop, 3), 'loop_calls': 2 * U, 'batched_ms': round(t_batch, 3),
                      'ratio_batched_over_loop': round(t_batch / t_loop, 4), 'max_abs_db_diff_sdr_sir': float(worst),
                      'potrf_ms': round(t_potrf, 3), 'potrf_f64_tflops': round(flop / (t_potrf * 1e-3) / 1e12, 3)}))


if __name__ == '__main__':
    import argparse
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=0, help='utterances per batch; 0: the per-utterance timing')
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--once', action='store_true', help='with --batch: one batched call only (for a kernel trace)')
    a = ap.parse_args()
    if a.batch > 0:
        batch(a.batch, a.reps, a.once)
    else:
        single()
