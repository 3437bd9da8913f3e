"""GPU: batched BSS-eval (include/ams_bss_batch.h through utils/bss_eval.py) against the pinned reference vectors, the numpy
oracle and the per-utterance path, plus the properties the batch must keep: a result depends on its utterance's data only, a
silent reference poisons its own utterance only, slicing changes nothing, and the f64 MFMA lane map is the right one.

dB rule (tests/test_bss_golden.py, unchanged): 1e-6 dB where the expected value is below 100 dB, "stays above 100 dB" above."""
import numpy as np
import pytest

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

from oracle import bss_eval as obss
from tests.bss_common import G, close_db as _close_db, cupy_db as _cupy_db, mix as _mix, oracle as _oracle


def _batch(seed, U, K, nsrc, L):
    rng = np.random.RandomState(seed)
    refs, ests = np.empty((U, nsrc, L)), np.empty((U, K, nsrc, L))
    for u in range(U):
        refs[u], e = _mix(rng, nsrc, L)
        ests[u, 0] = e[::-1]                                  # permuted
        for k in range(1, K):
            ests[u, k] = e + 0.2 * k * rng.randn(nsrc, L)
    return refs, ests


@pytest.mark.parametrize('names', [('n2_L20480', 'n2_mixture_as_estimate'), ('n2_L3000', 'n2_near_silent_estimate'),
                                   ('n3_L3000',), ('n3_L20480',)])
def test_pinned_vectors(names):
    from utils import bss_eval as hb
    refs = np.stack([G[n + '/ref'] for n in names])
    ests = np.stack([G[n + '/est'] for n in names])
    crit, info = hb.bss_eval_pairs_batch(refs, ests)
    assert crit.shape == (len(names), 1, 3) + refs.shape[1:2] * 2 and not info.any()
    for u, n in enumerate(names):
        ref_c = _cupy_db(n)
        for k in range(3):
            _close_db(crit[u, 0, k], ref_c[k])
    perm = hb.bss_eval_sources_batch(refs, ests)[3]
    for u, n in enumerate(names):
        assert np.array_equal(perm[u, 0], G[n + '/perm'])


def test_pinned_vectors_cover_the_file():
    """Every case of the golden file is in the parametrisation above."""
    cases = sorted({k.split('/')[0] for k in G.files if k.startswith('n')})
    assert cases == sorted(['n2_L20480', 'n2_mixture_as_estimate', 'n2_L3000', 'n2_near_silent_estimate', 'n3_L3000', 'n3_L20480'])
    assert G['n2_L20480/ref'].shape == G['n2_mixture_as_estimate/ref'].shape
    assert G['n2_L3000/ref'].shape == G['n2_near_silent_estimate/ref'].shape


@pytest.mark.parametrize('nsrc,L', [(2, 2500), (3, 2500), (2, 20480), (3, 20480)])
def test_against_oracle_and_per_utterance_path(nsrc, L):
    from utils import bss_eval as hb
    U, K = 5, 2
    refs, ests = _batch(100 * nsrc + L, U, K, nsrc, L)
    crit, info = hb.bss_eval_pairs_batch(refs, ests)
    assert not info.any()
    want, wperm = _oracle(refs, ests, obss.FLEN)
    _close_db(crit, want)
    single = np.stack([np.stack([np.stack(hb.bss_eval_pairs(refs[u], ests[u, k])) for k in range(K)]) for u in range(U)])
    _close_db(crit, single, 2e-6)
    out = hb.bss_eval_sources_batch(refs, ests)
    assert np.array_equal(out[3], wperm)
    dum = np.arange(nsrc)
    for u in range(U):
        for k in range(K):
            for c in range(3):
                _close_db(out[c][u, k], want[u, k, c][wperm[u, k], dum])
            assert np.array_equal(hb.bss_eval_sources_cupy(refs[u], ests[u, k], nsrc=nsrc)[3], out[3][u, k])


@pytest.mark.parametrize('flen', [100, 37])
def test_edge_tiles(flen):
    """Orders that are not multiples of the 16 / 32 / 64 tiles: flen = 100 -> 200 and 100; flen = 37 -> 74 and 37."""
    from utils import bss_eval as hb
    refs, ests = _batch(flen, 3, 2, 2, 1500)
    crit, info = hb.bss_eval_pairs_batch(refs, ests, flen=flen)
    assert not info.any()
    _close_db(crit, _oracle(refs, ests, flen)[0])


def _spd(rng, n):
    a = rng.randn(n, n + 8)
    m = a.dot(a.T) / n + np.eye(n) * 0.1
    return (m + m.T) / 2                                      # exactly symmetric


@pytest.mark.parametrize('n', [100, 512])
def test_potrf_depends_on_its_matrix_only(n):
    from utils import bss_eval as hb
    rng = np.random.RandomState(n)
    mats = np.stack([_spd(rng, n) for _ in range(7)])
    alone, info = hb.potrf_batch(mats[3:4])
    assert info.tolist() == [0]
    want = np.linalg.cholesky(mats[3])
    assert np.abs(np.tril(alone[0]) - want).max() < 1e-10 * np.abs(want).max() * n
    assert np.array_equal(np.triu(alone[0], 1), np.triu(mats[3], 1))        # the strict upper triangle is untouched
    for pos in range(7):                                       # at any position of a batch of 7
        order = [i for i in range(7) if i != 3]
        order.insert(pos, 3)
        f, info = hb.potrf_batch(mats[order])
        assert not info.any()
        assert np.array_equal(np.tril(f[pos]), np.tril(alone[0])), pos
    bad = mats.copy()                                          # next to a matrix that fails (a numerical condition, not a fault)
    piv = n // 2 + 3
    bad[2, piv, piv] = -1.0
    f, info = hb.potrf_batch(bad)
    assert info.tolist() == [0, 0, piv + 1, 0, 0, 0, 0]
    assert np.array_equal(np.tril(f[3]), np.tril(alone[0]))
    assert np.isnan(f[2][piv, piv]) and np.isnan(np.tril(f[2])[n - 1, piv:]).all()
    assert np.isfinite(np.tril(f[[0, 1, 3, 4, 5, 6]])).all()


def test_end_to_end_repeatable_and_batch_independent():
    from utils import bss_eval as hb
    refs, ests = _batch(77, 7, 2, 2, 4000)
    a, _ = hb.bss_eval_pairs_batch(refs, ests)
    b, _ = hb.bss_eval_pairs_batch(refs, ests)
    assert np.array_equal(a, b)                                # two successive identical calls: bitwise
    for u in (0, 3, 6):
        solo, info = hb.bss_eval_pairs_batch(refs[u:u + 1], ests[u:u + 1])
        assert not info.any()
        _close_db(a[u], solo[0])


def test_silent_reference_poisons_its_own_utterance_only():
    from utils import bss_eval as hb
    refs, ests = _batch(5, 4, 2, 2, 3000)
    refs[2, 1] = 0.0                                           # Gram matrix of utterance 2 is singular
    crit, info = hb.bss_eval_pairs_batch(refs, ests)
    assert info[2] != 0 and not info[[0, 1, 3]].any()
    assert np.isnan(crit[2]).all()
    for u in (0, 1, 3):
        assert np.isfinite(crit[u]).all()
        solo, sinfo = hb.bss_eval_pairs_batch(refs[u:u + 1], ests[u:u + 1])
        assert not sinfo.any()
        _close_db(crit[u], solo[0])


def test_slicing_equals_unsliced():
    from utils import bss_eval as hb
    mu = 3
    U = 2 * mu + 3
    refs, ests = _batch(21, U, 2, 2, 2000)
    whole, wi = hb.bss_eval_pairs_batch(refs, ests, flen=64, max_utt=U)
    sliced, si = hb.bss_eval_pairs_batch(refs, ests, flen=64, max_utt=mu)
    assert not wi.any() and not si.any()
    _close_db(sliced, whole)
    t = torch.tensor(refs, dtype=torch.float64, device='cuda')
    e = torch.tensor(ests, dtype=torch.float64, device='cuda')
    again, _ = hb.bss_eval_pairs_batch(t, e, flen=64, max_utt=mu)        # device tensors are read in place
    assert np.array_equal(again, sliced)


@pytest.mark.parametrize('n', [16, 64, 200, 512, 1024])
def test_mfma_layout_on_exact_integer_factor(n):
    """A = L L^T with a dense integer L (diagonal n, entries below it from {-1, 0, 1}): A is exact in float64 and well
    conditioned, so the factor must come back as L to rounding (bound 1e-9 * n; float64 rounding is of the order n * 2^-53
    relative).  One element put in the wrong row by the f32 lane map is an error of order 1 or more."""
    from utils import bss_eval as hb
    rng = np.random.RandomState(n)
    L = np.tril(rng.randint(-1, 2, size=(n, n)).astype(np.float64), -1) + n * np.eye(n)
    A = L.dot(L.T)
    assert np.array_equal(A, A.T) and np.abs(A).max() < 2 ** 52
    f, info = hb.potrf_batch(np.stack([A, A]))
    assert info.tolist() == [0, 0]
    err = np.abs(np.tril(f[0]) - L).max()
    print('n = %d: max |factor - L| = %.3e (bound %.3e)' % (n, err, 1e-9 * n))
    assert err <= 1e-9 * n
    assert np.array_equal(f[0], f[1])


def test_evaluate_batched_on_device_tensors():
    """The B = 3 case of tests/test_gpu_bss_eval.py::test_eval_loop_accumulates_improvement through both loops."""
    from experiments.evaluation.eval import evaluate, evaluate_batched
    rng = np.random.RandomState(9)
    B, S, L = 3, 2, 4096
    nm = rng.randn(B, S, L)
    for b in range(B):
        for k in range(S):
            nm[b, k] = np.convolve(nm[b, k], rng.randn(12), mode='same')
    mix = nm.sum(1)
    sep = nm + 0.05 * rng.randn(B, S, L)
    t = lambda a: torch.tensor(a, dtype=torch.float32, device='cuda')     # noqa: E731
    means, arr = evaluate([(t(mix), t(nm), t(sep))], nsrc=S, verbose=False)
    means_b, arr_b = evaluate_batched([(t(mix), t(nm), t(sep))], nsrc=S, verbose=False)
    assert arr_b.shape == arr.shape == (B, 2, S)
    _close_db(arr_b, arr, 2e-6)
    assert np.abs(np.array(means_b) - np.array(means)).max() < 2e-6
