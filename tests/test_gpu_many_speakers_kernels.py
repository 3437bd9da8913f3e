"""GPU: the kernels that serve five and six speakers -- the pair table and the parallel permutation search of the PIT costs, the L41
loss, the deep-clustering loss, hard k-means (bit for bit) and soft k-means (forward and backward) -- against the same oracles, with
the same tolerances, as their S = 2, 3 tests in test_gpu_kernels2.py / test_gpu_kmeans_soft.py."""
import numpy as np
import pytest

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

from oracle import dense as odense, dpcl as odpcl, l41 as ol41, losses as olosses, kmeans as okm
from tests import test_gpu_kmeans_soft as ksoft

TOL = 2e-5                                       # tests/test_gpu_kernels2.py


def dev(x, dtype=np.float32):
    return torch.from_numpy(np.ascontiguousarray(x, dtype=dtype)).cuda()


def host(t):
    torch.cuda.synchronize()
    return t.detach().cpu().numpy().astype(np.float64)


def rel(a, b):
    b = np.asarray(b, np.float64)
    return np.abs(np.asarray(a, np.float64) - b).max() / max(np.abs(b).max(), 1e-30)


@pytest.fixture(scope='module')
def F():
    from ams_hip import functional as f
    return f


@pytest.fixture(scope='module')
def ops():
    from ams_hip import ops as o
    return o


def search(F, ops, xn, est, cl, cs, mode=1):
    """pbest of the PIT search, straight from the entry point the costs go through."""
    S = est.shape[1]
    st = F.pair_stats(dev(xn), dev(est), None)
    out, pbest, _ = ops.pair_combine_fwd(st['table'].detach(), None, F._perm_table32(S, st['table'].device), S, mode, cl, cs)
    torch.cuda.synchronize()
    return out, pbest.cpu().numpy()


@pytest.mark.parametrize('S', [5, 6])
def test_pair_stats_and_costs(F, ops, S):
    """The body of test_gpu_kernels2.py::test_pair_stats_and_costs at B = 5, L = 4099 (two 4096-sample chunks, the second of three
    samples).  Best and second-best permutation differ by 8.5e-5 (S = 5) / 9.5e-4 (S = 6) relative for these inputs, against a float32
    evaluation error of 2e-7: the search must return the oracle's permutation for every utterance."""
    rng = np.random.RandomState(S)
    B, L = 5, 4099
    xn, bk = rng.randn(B, S, L) * 0.1, rng.randn(B, S, L) * 0.1
    xm = xn.sum(1)
    for kind in ('l2', 'sdr', 'l2+sdr'):
        bt = dev(bk).requires_grad_()
        p = F.pretrain_cost(dev(xm), dev(xn), bt)
        loss = p[0] if kind == 'l2' else p[1] if kind == 'sdr' else p[0] + p[1]
        lo, l2, sdr = olosses.pretrain_cost(xm, xn, bk, kind)
        assert abs(float(loss) - lo) < TOL * max(1.0, abs(lo))
        imp, _ = olosses.sdr_improvement(xm, xn, bk)
        assert abs(float(p[2]) - imp) < 1e-4 * max(1.0, abs(imp))
        loss.backward()
        assert rel(host(bt.grad), olosses.pretrain_cost_bwd(xn, bk, kind)) < 5 * TOL
    # PIT cost of the fine-tune recipes (0.5 sum_l, mean_s, min_perm, mean_b) + sub-gradient
    bt = dev(bk).requires_grad_()
    c = F.pit_l2(dev(xn), bt, 'sum', 'mean', 0.5)
    c_ref, best = olosses.cost_finetuning(xn, bk)
    assert abs(float(c) - c_ref) < TOL * max(1.0, abs(c_ref))
    c.backward()
    assert rel(host(bt.grad), olosses.pit_l2_bwd(xn, bk, best, 'sum', 'mean', 0.5)) < 5 * TOL
    _, pbest = search(F, ops, xn, bk, 0.5, 1.0 / S)
    assert np.array_equal(pbest, best), (pbest, best)
    # Adapt.cost non-pretraining branch, including the cross-batch SDR broadcast (quirk C-3)
    bt = dev(bk).requires_grad_()
    p = F.pit_cost_adapt(dev(xm), dev(xn), bt)
    lo, l2, sdr = olosses.pit_cost_adapt(xm, xn, bk, 'sdr+l2')
    assert abs(float(p[0]) - l2) < TOL * max(1.0, abs(l2)) and abs(float(p[1]) - sdr) < 1e-4 * max(1.0, abs(sdr))
    imp_ref, _ = olosses.sdr_improvement(xm, xn[:, None], bk, True)
    assert abs(float(p[2]) - imp_ref) < 1e-3 * max(1.0, abs(imp_ref))
    # gradient of the quirky sdr term vs torch autograd on the CPU restatement
    bt2 = torch.from_numpy(bk).requires_grad_()
    t_ = torch.from_numpy(xn)
    tn, an = (t_ ** 2).sum(-1), (bt2 ** 2).sum(-1)
    ts2 = ((t_[:, None] * bt2[None]).sum(-1)) ** 2
    sdr_t = (tn[:, None] * an[None]) / (ts2 + 1e-12)
    sdr_t.min(1)[0].sum(-1).mean().backward()
    p[1].backward()
    assert rel(host(bt.grad), bt2.grad.numpy()) < 1e-3
    # the l2 term of the same branch (mode 2 of the search): gradient through the selected permutation
    bt = dev(bk).requires_grad_()
    F.pit_cost_adapt(dev(xm), dev(xn), bt, want_imp=False)[0].backward()
    assert rel(host(bt.grad), olosses.pit_l2_bwd(xn, bk, best, 'mean', 'sum', 1.0)) < 5 * TOL


def planted(S, B, L, rng):
    """t, est with est[b, p_b(s)] = 0.6 t[b, s] + 0.5 noise; p_b = the first, the last and random rows of the permutation table."""
    P = olosses.perms(S)
    t, noise = rng.randn(B, S, L), rng.randn(B, S, L)
    pidx = np.concatenate([[0, len(P) - 1], rng.randint(0, len(P), max(B - 2, 0))])[:B]
    est = np.empty_like(t)
    for b in range(B):
        est[b, P[pidx[b]]] = 0.6 * t[b] + 0.5 * noise[b]
    return t, est, pidx


@pytest.mark.parametrize('L', [517, 4099])
@pytest.mark.parametrize('S', [5, 6])
def test_planted_permutations_are_found(F, ops, S, L):
    """The planted permutation wins by a wide margin (the runner-up costs at least 0.8 more, relative: checked on the CPU for these
    draws), so index for index: pbest == planted."""
    B = 5
    t, est, pidx = planted(S, B, L, np.random.RandomState(100 * S + 7))
    c_ref, best = olosses.cost_finetuning(t, est)
    assert np.array_equal(best, pidx)
    et = dev(est).requires_grad_()
    c = F.pit_l2(dev(t), et, 'sum', 'mean', 0.5)
    assert abs(float(c) - c_ref) < TOL * max(1.0, abs(c_ref))
    c.backward()
    assert rel(host(et.grad), olosses.pit_l2_bwd(t, est, pidx, 'sum', 'mean', 0.5)) < 5 * TOL
    _, pbest = search(F, ops, t, est, 0.5, 1.0 / S)
    assert np.array_equal(pbest, pidx), (pbest, pidx)


@pytest.mark.parametrize('B,S,L', [(5, 6, 517), (1, 6, 517), (260, 5, 67), (3, 5, 300)])
def test_equal_costs_keep_the_lowest_permutation_index(F, ops, B, S, L):
    """Two estimate rows of an utterance bitwise equal: the permutations that differ in which of the two they give to which target cost
    the same, bit for bit (float32 on the device, float64 in the oracle); np.argmin and the search keep the lower index."""
    rng = np.random.RandomState(1000 * S + B)
    P = olosses.perms(S)
    t, est, _ = planted(S, B, L, rng)
    pairs = np.stack([rng.choice(S, 2, replace=False) for _ in range(B)])
    tied = np.arange(B) % 3 != 1                                    # (B = 1: its only utterance)
    for b in np.nonzero(tied)[0]:
        est[b, pairs[b, 1]] = est[b, pairs[b, 0]]
    est = est.astype(np.float32).astype(np.float64)                  # the rows the device sees, bit for bit
    t = t.astype(np.float32).astype(np.float64)
    c_ref, best = olosses.cost_finetuning(t, est)
    lookup = {tuple(p): i for i, p in enumerate(P)}
    for b in np.nonzero(tied)[0]:
        p = P[best[b]].copy()
        i, j = pairs[b]
        swap = np.where(p == i, j, np.where(p == j, i, p))
        assert lookup[tuple(swap)] > best[b]                         # the tie is there and the oracle kept its lower end
    out, pbest = search(F, ops, t, est, 0.5, 1.0 / S)
    assert np.array_equal(pbest, best), np.nonzero(pbest != best)
    assert abs(float(out[0]) - c_ref) < TOL * max(1.0, abs(c_ref))


def _l41_case(S, rng, B=3, T=4, Fq=70, E=40, NS=23):
    spk = rng.randn(NS, E)
    I = np.stack([rng.choice(NS, S, replace=False) for _ in range(B)]).astype(np.int32)
    lab = rng.randint(0, S, (B, T, Fq))
    y = np.where(np.eye(S)[lab] > 0, 1.0, -1.0)
    y[0, 0, :5] = -1.0                                              # bins with no dominant speaker: argmax -> 0
    return spk, I, y


@pytest.mark.parametrize('from_u', [False, True])
@pytest.mark.parametrize('normalize', [True, False])
@pytest.mark.parametrize('S', [5, 6])
def test_l41_loss(F, S, normalize, from_u):
    l41_loss_case(F, 6 + S, 40, S, normalize, from_u)


def l41_loss_case(F, seed, E, S, normalize, from_u, upload=None):
    """The body of test_l41_loss (E = 40, seed 6 + S there); the other embedding sizes: tests/test_gpu_dispatch_arms.py.  upload: the
    caller's dev (a fenced one)."""
    dev = upload or globals()['dev']
    rng = np.random.RandomState(seed)
    B, T, Fq = 3, 4, 70                                             # 280 bins per utterance: two blocks, the second of 24
    spk, I, y = _l41_case(S, rng, E=E)
    if from_u:
        u = rng.randn(B, T, Fq * E) * np.exp(rng.randn(B, T, 1))
        u[0, 0, :E] = 0.0                                           # the epsilon clamp
        emb, inv = odense.l2norm_fwd(u, E)
    else:
        u = emb = rng.randn(B, T, Fq, E) * 0.3
    c_ref = ol41.l41_cost(emb, y, spk, I, normalize)
    de, ds = ol41.l41_cost_bwd(emb, y, spk, I, normalize)
    if from_u:
        de = odense.l2norm_bwd(emb, inv, de.reshape(emb.shape)).reshape(u.shape)
    ut, st = dev(u).requires_grad_(), dev(spk).requires_grad_()
    c = F.l41_loss(ut, dev(y), st, dev(I, np.int32), normalize, from_u=from_u)
    assert abs(float(c) - c_ref) < TOL * max(1.0, abs(c_ref))
    c.backward()
    assert rel(host(ut.grad), de) < 5 * TOL and rel(host(st.grad), ds) < 5 * TOL


@pytest.mark.parametrize('from_u', [False, True])
@pytest.mark.parametrize('method,K', [('k-nearest', 6), ('random', 16)])
def test_l41_loss_negative_sampling_five_speakers(F, method, K, from_u):
    l41_negative_sampling_case(F, 60 + K, 40, 5, method, K, from_u)


def l41_negative_sampling_case(F, seed, E, S, method, K, from_u, upload=None):
    """The body of test_l41_loss_negative_sampling_five_speakers (E = 40, S = 5, seed 60 + K there)."""
    dev = upload or globals()['dev']
    rate, normalize = 0.3, True
    rng = np.random.RandomState(seed)
    B, T, Fq, NS = 3, 4, 70, 23
    spk, I, y = _l41_case(S, rng, E=E)
    if from_u:
        u = rng.randn(B, T, Fq * E) * np.exp(rng.randn(B, T, 1))
        emb, inv = odense.l2norm_fwd(u, E)
    else:
        u = emb = rng.randn(B, T, Fq, E) * 0.3
    ut, st = dev(u).requires_grad_(), dev(spk).requires_grad_()
    if method == 'k-nearest':
        idx_ref = ol41.knearest_indices(spk, I, K, normalize)
        idx = F.l41_knearest(st, dev(I, np.int32), K, normalize)
        assert idx.shape == (B, S, K)
        assert np.array_equal(np.sort(idx.cpu().numpy(), axis=2), np.sort(idx_ref, axis=2))
    else:
        idx_ref = ol41.random_indices(I, NS, K, np.random.RandomState(3))
        idx = dev(idx_ref, np.int32)
    c = F.l41_loss(ut, dev(y), st, dev(I, np.int32), normalize, neg_idx=idx, ns_rate=rate, from_u=from_u)
    c_ref = ol41.l41_cost(emb, y, spk, I, normalize, idx_ref, rate)
    assert abs(float(c) - c_ref) < TOL * max(1.0, abs(c_ref))
    assert abs(c_ref - ol41.l41_cost(emb, y, spk, I, normalize)) > 1e-3               # the term is really there
    c.backward()
    de, ds = ol41.l41_cost_bwd(emb, y, spk, I, normalize, idx_ref, rate)
    if from_u:
        de = odense.l2norm_bwd(emb, inv, de.reshape(emb.shape)).reshape(u.shape)
    assert rel(host(ut.grad), de) < 5 * TOL and rel(host(st.grad), ds) < 5 * TOL


@pytest.mark.parametrize('E', [40, 8])
@pytest.mark.parametrize('S', [5, 6])
def test_dpcl_loss(F, S, E):
    """models/dpcl.py's entry (the network output before Normalize, fused normalise + loss) on the generic path of S > 4."""
    dpcl_loss_u_case(F, S, E, 9, 33)                                 # 297 points


def dpcl_loss_u_case(F, S, E, T, Fq, zero_row=False, upload=None):
    """The body of test_dpcl_loss at T * Fq points; zero_row: one point of u all zeros (the eps clamp, as test_gpu_kernels.py::
    test_l2norm_dpcl has it); upload: the caller's dev (a fenced one).  Other sizes: tests/test_gpu_dispatch_arms.py."""
    dev = upload or globals()['dev']
    rng = np.random.RandomState(10 * S + E)
    B = 2
    u = rng.randn(B, T, Fq * E) * np.exp(rng.randn(B, T, 1))
    if zero_row:
        u[0, 0, :E] = 0.0
    lab = rng.randint(0, S, (B, T * Fq))
    lab[0, :100] = 0                                                 # unbalanced classes
    Y = np.eye(S)[lab]
    V, inv = odense.l2norm_fwd(u.reshape(B, -1), E)
    Vf = V.reshape(B, T * Fq, E)
    c_ref, terms = odpcl.dpcl_cost(Vf, Y)
    du_ref = odense.l2norm_bwd(V, inv, odpcl.dpcl_cost_bwd(Vf, Y).reshape(V.shape)).reshape(u.shape)
    ut = dev(u).requires_grad_()
    cost, all_terms = F.dpcl_loss_u(ut, dev(Y), E)
    o = host(all_terms)
    assert abs(o[0] - c_ref) < TOL * max(1.0, abs(c_ref)), (o[0], c_ref)
    for k in range(3):
        assert abs(o[1 + k] - terms[k]) < TOL * max(1.0, abs(terms[k]))
    cost.backward(torch.ones(1, device='cuda'))
    F.OVERLAP.join()
    assert rel(host(ut.grad), du_ref) < 5 * TOL


def kmeans_hard_inputs(seed, b, L, E, C, tries, with_w):
    rng = np.random.RandomState(seed)
    centers = rng.randn(C, E).astype(np.float32) * 2.0
    lab_true = rng.randint(0, C, (b, L))
    X = (centers[lab_true] + rng.randn(b, L, E).astype(np.float32) * 0.7).astype(np.float32)
    w = (rng.rand(b, L) > 0.2).astype(np.float32) if with_w else None
    if with_w == 'real':
        w = rng.uniform(0.05, 1.7, (b, L)).astype(np.float32)
    elif with_w == 'mixed':
        w[:, ::3] = rng.uniform(0.05, 1.7, (b, L))[:, ::3].astype(np.float32)
    idx = np.stack([rng.choice(L, C, replace=False) for _ in range(b * tries)]).astype(np.int32)
    return X, w, idx


@pytest.mark.parametrize('b,L,E,C,tries,with_w,end,seed,best_expected',
                         [(2, 8449, 40, 5, 2, False, True, 13453, [1, 0]), (2, 4100, 40, 6, 3, True, False, 10109, [2, 0]),
                          (2, 2500, 8, 5, 1, 'real', True, 7500, [0, 0]), (1, 8449, 40, 6, 2, 'mixed', True, 14449, [1])])
def test_kmeans_hard_bit_exact(F, ops, b, L, E, C, tries, with_w, end, seed, best_expected):
    """The body of test_gpu_kernels2.py::test_kmeans_hard_bit_exact (same order of random draws) for five and six clusters.  L = 8449 is
    one full 8192-point chunk plus a second of one slab and one point.  The seeds are ones for which the oracle uses every cluster
    (others meet the reference's empty-cluster NaN)."""
    kmeans_hard_case(F, ops, b, L, E, C, tries, with_w, end, seed, best_expected)


def kmeans_hard_case(F, ops, b, L, E, C, tries, with_w, end, seed, best_expected, upload=None):
    """The body of test_kmeans_hard_bit_exact; upload: the caller's dev (a fenced one).  Other (E, C): tests/test_gpu_dispatch_arms.py."""
    dev = upload or globals()['dev']
    X, w, idx = kmeans_hard_inputs(seed, b, L, E, C, tries, with_w)
    cent_ref, lab_ref, best_ref = okm.kmeans(X, idx, C, tries, 4, beta=None, notsilent=w, assign_at_end=end)
    assert np.isfinite(cent_ref).all()
    assert list(best_ref) == best_expected
    xn = ops.kmeans_normalize(dev(X))
    assert np.array_equal(host(xn).astype(np.float32), okm.l2_normalize_rows(X))
    cent, lab, best = F.kmeans(dev(X), dev(idx, np.int32), C, tries, 4, None, dev(w) if with_w else None, end)
    torch.cuda.synchronize()
    assert np.array_equal(best.cpu().numpy(), best_ref)
    assert np.array_equal(cent.cpu().numpy(), cent_ref)
    assert np.array_equal(lab.cpu().numpy(), lab_ref)


@pytest.mark.parametrize('b,L,E,C,tries,iters,with_w,end', [(2, 3000, 40, 5, 2, 3, True, True), (2, 2500, 8, 6, 1, 4, True, False)])
def test_soft_kmeans_backward(b, L, E, C, tries, iters, with_w, end, monkeypatch):
    """test_gpu_kmeans_soft.py::test_soft_kmeans_backward -- forward and backward against float64 autograd of torch_soft_kmeans -- at
    five and six clusters: its body, its assertions."""
    ksoft.test_soft_kmeans_backward(b, L, E, C, tries, iters, with_w, end, monkeypatch)
