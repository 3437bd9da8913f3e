"""GPU: every instantiated (E, S / C) arm of the embedding losses and of the k-means runs at least once, and the nearest pairs outside
each table are refused as a status, not a fault.

The losses and the k-means are instantiated per embedding size E and per speaker / cluster count (csrc/kmeans.hip, kmeans_soft.hip,
l41.hip, danet.hip, dpcl.hip); include/ams.h states the tables, --embedding_size and --nb_speakers reach every arm.  The arms differ
in vector width, LDS row pitch and thread ownership (E = 20: five float4 per point; L41: thread tid < S * E owns an output), which is
the kind of code that is wrong at one size only -- and the neighbouring modules run E = 40 and a few E = 8 cases.

ACCEPTED SIDE.  Every case is the BODY of the test that covers the family at E = 40, imported, with that test's oracle and tolerance:
  hard k-means   test_gpu_many_speakers_kernels.kmeans_hard_case        oracle.kmeans.kmeans, array_equal on centroids, labels, best
  soft forward   test_gpu_kernels2.kmeans_soft_forward_case             oracle.kmeans.kmeans, 1e-4 / 1e-3
  soft backward  test_gpu_kmeans_soft.soft_kmeans_backward_case         float64 autograd of torch_soft_kmeans, 1e-3
  L41            test_gpu_many_speakers_kernels.l41_loss_case / l41_negative_sampling_case      oracle.l41, TOL / 5 TOL
  DANet          test_gpu_danet.reconstruction_case                     tests/danet_ref.py, TOL / 5 TOL
  DPCL           test_gpu_many_speakers_kernels.dpcl_loss_u_case, test_gpu_kernels.test_l2norm_dpcl (and its forward part,
                 l2norm_dpcl_forward_case)                              oracle.dpcl + oracle.dense, TOL / 5 TOL
No tolerance is new.  Shapes are the smallest that reach every loop of an arm: k-means L = 8449 (one 8192-point chunk and a ragged
second one) and L = 197 (one partial chunk), b = 2; L41 and DANet B = 3 x 280 bins (two blocks, the second of 24); DPCL TF = 2561 and 77.

SEEDS.  The k-means and k-nearest cases carry seeds chosen ON THE CPU, from the references alone, so that the comparison is not a
coin toss in float32 (the conditions and the margins found are in HISTORY.md):
  * hard: the float32 oracle uses every cluster in every pass of every try and in the end assignment (an empty cluster is the
    reference's NaN centroid); `best` is part of the row and asserted against the oracle before anything runs on the device;
  * soft, forward and backward: every cluster keeps a soft mass of at least one point in every pass, and with two tries the best
    try's inertia is below the other's by at least 1e-3 relative;
  * L41 k-nearest: the K-th and (K+1)-th neighbour products differ by at least 1e-4 of the largest product.
No case is skipped or tolerated.

REFUSED SIDE.  The nearest pairs outside each table go to the entry points themselves (through ops.check, as ams_hip.ops calls them)
with every output and the workspace holding a sentinel: AmsError carrying AMS_E_INVALID_ARG, the sentinel still in every word, no
sticky error raised -- and the device answers the synchronize that follows.

The tables below are copied from include/ams.h; ams_hip/ops.py states them once for the host side (refusal at construction,
tests/test_dispatch_tables_host.py) and test_host_tables_are_these asserts that the two are the same."""
import numpy as np
import pytest

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

from tests import test_gpu_danet as DA
from tests import test_gpu_kernels as K1
from tests import test_gpu_kernels2 as K2
from tests import test_gpu_kmeans_soft as KS
from tests import test_gpu_many_speakers_kernels as MS

# ---- the tables (include/ams.h)
# "ams_kmeans_iterate / ams_kmeans_assign: (E, C) in {40, 8} x {2 .. 6} or {20} x {2, 3}": hard (beta < 0) and soft forward (beta >= 0)
HARD_KMEANS = sorted([(E, C) for E in (40, 8) for C in (2, 3, 4, 5, 6)] + [(20, 2), (20, 3)], reverse=True)
SOFT_FORWARD = list(HARD_KMEANS)
# "ams_kmeans_soft_bwd: (40, 2 .. 6), (8, 2 | 3 | 5 | 6), (20, 2)"
SOFT_BACKWARD = sorted([(40, C) for C in (2, 3, 4, 5, 6)] + [(8, 2), (8, 3), (8, 5), (8, 6), (20, 2)], reverse=True)
# "1 <= S <= 6 (ABI 9; was 4), E in {3, 4, 8, 16, 20, 32, 40}: all four entry points" (L41); the DANet reconstruction: the same E, S <= 4;
# ams_dpcl_loss_bwd: the same E
LOSS_E = (3, 4, 8, 16, 20, 32, 40)
L41 = [(E, S) for E in LOSS_E for S in (1, 2, 3, 4, 5, 6)]
DANET = [(E, S) for E in LOSS_E for S in (1, 2, 3, 4)]
# the deep-clustering loss: 1 <= S <= 8 and E + S <= 64 (four 16-wide tiles of the augmented Gram); its normalised-input backward: LOSS_E
DPCL_MAX_S, DPCL_MAX_E_PLUS_S, DPCL_BWD_E = 8, 64, LOSS_E

SENTINEL = -12345.5


def dev(x, dtype=np.float32):
    return torch.from_numpy(np.ascontiguousarray(x, dtype=dtype)).cuda()


@pytest.fixture(scope='module')
def F():
    from ams_hip import functional as f
    return f


@pytest.fixture(scope='module')
def ops():
    from ams_hip import ops as o
    return o


def test_host_tables_are_these(ops):
    assert sorted(ops.KMEANS_PAIRS, reverse=True) == HARD_KMEANS and sorted(ops.KMEANS_SOFT_FWD_PAIRS, reverse=True) == SOFT_FORWARD
    assert sorted(ops.KMEANS_SOFT_BWD_PAIRS, reverse=True) == SOFT_BACKWARD
    assert tuple(ops.LOSS_E) == LOSS_E
    assert [(E, S) for E in LOSS_E for S in range(1, 12) if ops.l41_in_domain(E, S)] == L41
    assert [(E, S) for E in LOSS_E for S in range(1, 12) if ops.danet_in_domain(E, S)] == DANET
    assert not any(ops.l41_in_domain(E, 2) or ops.danet_in_domain(E, 2) for E in range(1, 80) if E not in LOSS_E)
    assert (ops.DPCL_MAX_S, ops.DPCL_MAX_E_PLUS_S) == (DPCL_MAX_S, DPCL_MAX_E_PLUS_S)
    assert all(ops.dpcl_in_domain(E, S) == (S <= DPCL_MAX_S and E + S <= DPCL_MAX_E_PLUS_S) for E in range(1, 70) for S in range(1, 11))


# ----------------------------------------------------------------------------------------------------------------- hard k-means
# (E, C, L, tries, with_w, end, seed, best_expected): per pair with and without silence weights x one and three tries at L = 8449, and
# three weighted tries at L = 197.  (40, 2) with three tries stays on kmeans_pass_kernel: the five-tries kernel needs tries % 5 == 0.
HARD_CASES = [
    (40, 6, 8449, 1, False, True, 40610, [0, 0]), (40, 6, 8449, 3, True, False, 40631, [2, 2]),
    (40, 6, 8449, 3, False, True, 50630, [0, 1]), (40, 6, 8449, 1, True, False, 60611, [0, 0]),
    (40, 6, 197, 3, True, True, 70638, [0, 0]), (40, 5, 8449, 1, False, True, 40510, [0, 0]),
    (40, 5, 8449, 3, True, False, 40531, [1, 1]), (40, 5, 8449, 3, False, True, 50530, [1, 0]),
    (40, 5, 8449, 1, True, False, 60511, [0, 0]), (40, 5, 197, 3, True, True, 40538, [2, 1]),
    (40, 4, 8449, 1, False, True, 40410, [0, 0]), (40, 4, 8449, 3, True, False, 40431, [0, 2]),
    (40, 4, 8449, 3, False, True, 50430, [2, 1]), (40, 4, 8449, 1, True, False, 50411, [0, 0]),
    (40, 4, 197, 3, True, True, 50438, [1, 1]), (40, 3, 8449, 1, False, True, 40310, [0, 0]),
    (40, 3, 8449, 3, True, False, 40331, [0, 0]), (40, 3, 8449, 3, False, True, 40330, [0, 0]),
    (40, 3, 8449, 1, True, False, 40311, [0, 0]), (40, 3, 197, 3, True, True, 40338, [1, 2]),
    (40, 2, 8449, 1, False, True, 40210, [0, 0]), (40, 2, 8449, 3, True, False, 40231, [1, 0]),
    (40, 2, 8449, 3, False, True, 40230, [0, 0]), (40, 2, 8449, 1, True, False, 40211, [0, 0]),
    (40, 2, 197, 3, True, True, 40238, [1, 0]), (20, 3, 8449, 1, False, True, 20310, [0, 0]),
    (20, 3, 8449, 3, True, False, 20331, [1, 2]), (20, 3, 8449, 3, False, True, 30330, [0, 1]),
    (20, 3, 8449, 1, True, False, 20311, [0, 0]), (20, 3, 197, 3, True, True, 20338, [0, 1]),
    (20, 2, 8449, 1, False, True, 20210, [0, 0]), (20, 2, 8449, 3, True, False, 20231, [2, 0]),
    (20, 2, 8449, 3, False, True, 20230, [0, 0]), (20, 2, 8449, 1, True, False, 20211, [0, 0]),
    (20, 2, 197, 3, True, True, 20238, [0, 1]), (8, 6, 8449, 1, False, True, 8610, [0, 0]),
    (8, 6, 8449, 3, True, False, 8631, [0, 2]), (8, 6, 8449, 3, False, True, 8630, [2, 1]),
    (8, 6, 8449, 1, True, False, 8611, [0, 0]), (8, 6, 197, 3, True, True, 8638, [0, 2]),
    (8, 5, 8449, 1, False, True, 8510, [0, 0]), (8, 5, 8449, 3, True, False, 8531, [0, 1]),
    (8, 5, 8449, 3, False, True, 8530, [0, 1]), (8, 5, 8449, 1, True, False, 8511, [0, 0]),
    (8, 5, 197, 3, True, True, 8538, [2, 0]), (8, 4, 8449, 1, False, True, 8410, [0, 0]),
    (8, 4, 8449, 3, True, False, 8431, [2, 0]), (8, 4, 8449, 3, False, True, 8430, [0, 0]),
    (8, 4, 8449, 1, True, False, 8411, [0, 0]), (8, 4, 197, 3, True, True, 8438, [2, 0]),
    (8, 3, 8449, 1, False, True, 8310, [0, 0]), (8, 3, 8449, 3, True, False, 8331, [2, 2]),
    (8, 3, 8449, 3, False, True, 8330, [2, 0]), (8, 3, 8449, 1, True, False, 8311, [0, 0]),
    (8, 3, 197, 3, True, True, 8338, [0, 0]), (8, 2, 8449, 1, False, True, 8210, [0, 0]),
    (8, 2, 8449, 3, True, False, 8231, [0, 1]), (8, 2, 8449, 3, False, True, 8230, [0, 0]),
    (8, 2, 8449, 1, True, False, 8211, [0, 0]), (8, 2, 197, 3, True, True, 8238, [2, 2]),
]


def _hard_id(c):
    return 'E%d-C%d-L%d-tries%d-%s-%s' % (c[0], c[1], c[2], c[3], 'w' if c[4] else 'now', 'end' if c[5] else 'kept')


@pytest.mark.parametrize('E,C,L,tries,with_w,end,seed,best_expected', HARD_CASES, ids=[_hard_id(c) for c in HARD_CASES])
def test_hard_kmeans(F, ops, E, C, L, tries, with_w, end, seed, best_expected):
    MS.kmeans_hard_case(F, ops, 2, L, E, C, tries, with_w, end, seed, best_expected, upload=dev)


def test_every_hard_kmeans_pair_runs_every_combination():
    for pair in HARD_KMEANS:
        mine = [c for c in HARD_CASES if (c[0], c[1]) == pair]
        assert {(c[3], bool(c[4])) for c in mine if c[2] == 8449} == {(1, False), (1, True), (3, False), (3, True)}, pair
        assert any(c[2] == 197 for c in mine), pair
    assert {(c[0], c[1]) for c in HARD_CASES} == set(HARD_KMEANS)


# ----------------------------------------------------------------------------------------------------------------- soft k-means, forward
# (E, C, L, seed): two tries, five iterations, beta = 10, silence weights, end assignment (the body of test_kmeans_soft_forward)
SOFT_FORWARD_CASES = [
    (40, 6, 8449, 40600), (40, 6, 197, 40607), (40, 5, 8449, 40500), (40, 5, 197, 40507),
    (40, 4, 8449, 40400), (40, 4, 197, 40407), (40, 3, 8449, 40300), (40, 3, 197, 40307),
    (40, 2, 8449, 40200), (40, 2, 197, 40207), (20, 3, 8449, 20300), (20, 3, 197, 20307),
    (20, 2, 8449, 20200), (20, 2, 197, 20207), (8, 6, 8449, 8600), (8, 6, 197, 8607),
    (8, 5, 8449, 8500), (8, 5, 197, 8507), (8, 4, 8449, 8400), (8, 4, 197, 8407),
    (8, 3, 8449, 8300), (8, 3, 197, 8307), (8, 2, 8449, 8200), (8, 2, 197, 8207),
]


@pytest.mark.parametrize('E,C,L,seed', SOFT_FORWARD_CASES, ids=['E%d-C%d-L%d' % c[:3] for c in SOFT_FORWARD_CASES])
def test_soft_kmeans_forward(F, E, C, L, seed):
    K2.kmeans_soft_forward_case(F, seed, 2, L, E, C, 2, upload=dev)


# ----------------------------------------------------------------------------------------------------------------- soft k-means, backward
# (E, C, L, tries, iters, with_w, end, seed): beta = 3 (the body of test_soft_kmeans_backward)
SOFT_BACKWARD_CASES = [
    (40, 6, 8449, 2, 3, True, True, 40600), (40, 6, 197, 1, 2, False, False, 40607),
    (40, 5, 8449, 2, 3, True, True, 40500), (40, 5, 197, 1, 2, False, False, 40507),
    (40, 4, 8449, 2, 3, True, True, 40400), (40, 4, 197, 1, 2, False, False, 40407),
    (40, 3, 8449, 2, 3, True, True, 40300), (40, 3, 197, 1, 2, False, False, 40307),
    (40, 2, 8449, 2, 3, True, True, 40200), (40, 2, 197, 1, 2, False, False, 40207),
    (20, 2, 8449, 2, 3, True, True, 20200), (20, 2, 197, 1, 2, False, False, 20207),
    (8, 6, 8449, 2, 3, True, True, 8600), (8, 6, 197, 1, 2, False, False, 8607),
    (8, 5, 8449, 2, 3, True, True, 8500), (8, 5, 197, 1, 2, False, False, 8507),
    (8, 3, 8449, 2, 3, True, True, 8300), (8, 3, 197, 1, 2, False, False, 8307),
    (8, 2, 8449, 2, 3, True, True, 8200), (8, 2, 197, 1, 2, False, False, 8207),
]


@pytest.mark.parametrize('E,C,L,tries,iters,with_w,end,seed', SOFT_BACKWARD_CASES,
                         ids=['E%d-C%d-L%d' % c[:3] for c in SOFT_BACKWARD_CASES])
def test_soft_kmeans_backward(E, C, L, tries, iters, with_w, end, seed, monkeypatch):
    KS.soft_kmeans_backward_case(seed, 2, L, E, C, tries, iters, with_w, end, monkeypatch)


def test_every_soft_kmeans_pair_runs():
    assert {c[:2] for c in SOFT_FORWARD_CASES} == set(SOFT_FORWARD) and {c[:2] for c in SOFT_BACKWARD_CASES} == set(SOFT_BACKWARD)
    for cases in (SOFT_FORWARD_CASES, SOFT_BACKWARD_CASES):
        assert {c[2] for c in cases} == {8449, 197}


@pytest.mark.parametrize('E,C', sorted(set(SOFT_FORWARD) - set(SOFT_BACKWARD)))
def test_soft_kmeans_under_gradient_is_refused_before_any_launch(F, ops, monkeypatch, E, C):
    """The seam between the two tables: (8, 4) and (20, 3) run forward (test_soft_kmeans_forward has both, against the oracle) and have
    no backward kernel.  With a gradient wanted F.kmeans refuses BEFORE the forward: nothing of ops is reached."""
    from ams_hip._lib import AmsError
    assert (E, C) in ((8, 4), (20, 3))
    X, w, idx = K2.kmeans_soft_forward_inputs(7, 2, 197, E, C, 1)

    def launched(*a, **k):
        raise AssertionError('a launch was reached')
    for name in ('kmeans_run', 'kmeans_normalize', 'l2norm_fwd', 'l2norm2_fwd', 'l2norm_kmeans_normalize'):
        monkeypatch.setattr(ops, name, launched)
    for pre in (False, True):
        Xd = dev(X).requires_grad_()
        with pytest.raises(AmsError) as e:
            if pre:
                F.kmeans(launched, dev(idx, np.int32), C, 1, 3, 3.0, dev(w), True, pre_norm=lambda: Xd)
            else:
                F.kmeans(Xd, dev(idx, np.int32), C, 1, 3, 3.0, dev(w), True)
        assert 'ams_kmeans_soft_bwd' in str(e.value) and 'ams_kmeans_iterate' in str(e.value) and '(%d, %d)' % (E, C) in str(e.value)
    torch.cuda.synchronize()
    assert ops.persist_errors() == 0


# ----------------------------------------------------------------------------------------------------------------- L41
L41_FULL = [(E, S) for E in (4, 8, 16, 32) for S in (1, 2, 4, 6)]
# every (normalize, from_u) for L41_FULL; one of the four, by parity, for the other pairs of the table
L41_CASES = [(E, S, n, u) for (E, S) in L41 for n in (True, False) for u in (False, True)
             if (E, S) in L41_FULL or (n, u) == ((E + S) % 2 == 0, S % 2 == 1)]


@pytest.mark.parametrize('E,S,normalize,from_u', L41_CASES,
                         ids=['E%d-S%d-%s-%s' % (E, S, 'norm' if n else 'raw', 'u' if u else 'v') for E, S, n, u in L41_CASES])
def test_l41_loss(F, E, S, normalize, from_u):
    """Forward and backward, vector (E % 4 == 0) and 4-byte (E = 3) forms, MAXS = 4 (S <= 4) and MAXS = 6 instantiations."""
    MS.l41_loss_case(F, 100 * E + S, E, S, normalize, from_u, upload=dev)


# (E, S, method, K, seed): K = 16 with one set per utterance (NSEL = 1), and NSEL = S at NSEL * K = 32 (the limit) and 30
L41_NS_CASES = [
    (8, 4, 'k-nearest', 8, 848), (8, 4, 'random', 16, 848),
    (8, 6, 'k-nearest', 5, 865), (8, 6, 'random', 16, 865),
    (32, 4, 'k-nearest', 8, 13248), (32, 4, 'random', 16, 13248),
    (32, 6, 'k-nearest', 5, 3265), (32, 6, 'random', 16, 3265),
]


@pytest.mark.parametrize('from_u', [False, True])
@pytest.mark.parametrize('E,S,method,K,seed', L41_NS_CASES, ids=['E%d-S%d-%s-K%d' % c[:4] for c in L41_NS_CASES])
def test_l41_negative_sampling(F, E, S, method, K, seed, from_u):
    MS.l41_negative_sampling_case(F, seed, E, S, method, K, from_u, upload=dev)


# ----------------------------------------------------------------------------------------------------------------- DANet
DANET_FULL = [(E, S) for E in (3, 4, 16, 20, 32) for S in (1, 2, 4)]
DANET_CASES = [(E, S, kind) for (E, S) in DANET for kind in ('binary', 'fractional') if kind == 'binary' or (E, S) in DANET_FULL]


@pytest.mark.parametrize('E,S,kind', DANET_CASES, ids=['E%d-S%d-%s' % c for c in DANET_CASES])
def test_danet_reconstruction(F, E, S, kind):
    DA.reconstruction_case(F, 3, 4, 70, E, S, kind)


# ----------------------------------------------------------------------------------------------------------------- DPCL
# the fused form (network output before Normalize): NT = ceil((E + S) / 16) tiles; (60, 4) and (56, 8) sit at E + S = 64 exactly, (50, 2)
# and (45, 5) are NT = 4 below it, (13, 2) and (27, 3) NT = 1 and 2; 45, 13 and 27 are odd (the 4-byte staging on rows longer than a float4)
DPCL_U = [(50, 2), (60, 4), (56, 8), (45, 5), (13, 2), (27, 3)]
# the form on normalised embeddings, whose backward is instantiated per E: every E of its switch, the never-run 4, 16, 32 with two S
DPCL_V = [(E, 2) for E in DPCL_BWD_E] + [(E, 3) for E in (4, 16, 32)]
POINTS = {2561: (13, 197), 77: (7, 11)}                              # TF = T * Fq: past one 2560-point chunk by a point; below one slab


@pytest.mark.parametrize('TF', [2561, 77])
@pytest.mark.parametrize('E,S', DPCL_U, ids=['E%d-S%d' % p for p in DPCL_U])
def test_dpcl_from_the_network_output(F, E, S, TF):
    assert S <= DPCL_MAX_S and E + S <= DPCL_MAX_E_PLUS_S
    T, Fq = POINTS[TF]
    MS.dpcl_loss_u_case(F, S, E, T, Fq, zero_row=True, upload=dev)


@pytest.mark.parametrize('TF', [2561, 77])
@pytest.mark.parametrize('E,S', DPCL_V, ids=['E%d-S%d' % p for p in DPCL_V])
def test_dpcl_from_normalised_embeddings(ops, E, S, TF):
    """test_gpu_kernels.py::test_l2norm_dpcl itself (one u row of zeros; both forms of the loss, every backward) at the E of the
    ams_dpcl_loss_bwd switch."""
    K1.test_l2norm_dpcl(ops, 2, TF, E, S)


@pytest.mark.parametrize('TF', [2561, 77])
@pytest.mark.parametrize('E,S', [p for p in DPCL_U if p[0] + p[1] > 48], ids=['E%d-S%d' % p for p in DPCL_U if p[0] + p[1] > 48])
def test_dpcl_forward_on_normalised_embeddings_at_four_tiles(ops, E, S, TF):
    """dpcl_gram_kernel<4>: the forward of the un-fused form has no list of E (its backward has: DPCL_BWD_E stops at 40), so four tiles
    are reached by the forward alone -- the first part of test_l2norm_dpcl, its assertions."""
    K1.l2norm_dpcl_forward_case(ops, 2, TF, E, S)


def test_every_dpcl_tile_count_runs():
    assert {-(-(E + S) // 16) for E, S in DPCL_U} == {1, 2, 4} and {-(-(E + S) // 16) for E, S in DPCL_V} == {1, 2, 3}
    assert max(E + S for E, S in DPCL_U) == DPCL_MAX_E_PLUS_S and max(S for E, S in DPCL_U) == DPCL_MAX_S


# ----------------------------------------------------------------------------------------------------------------- the refused side
def _sent(*shape, dtype=torch.float32):
    return torch.full(shape, SENTINEL if dtype.is_floating_point else int(SENTINEL), dtype=dtype, device='cuda')


def _rand(*shape):
    return dev(np.random.RandomState(sum(shape)).randn(*shape))


def _refused(ops, call, what, outputs):
    """call() returns the entry point's status.  AMS_E_INVALID_ARG as an AmsError, every output word untouched, nothing sticky, and the
    device answers."""
    from ams_hip._lib import AmsError
    with pytest.raises(AmsError, match='%s failed: AMS_E_INVALID_ARG' % what):
        ops.check(call(), what)
    torch.cuda.synchronize()
    for o in outputs:
        assert bool((o == (SENTINEL if o.dtype.is_floating_point else int(SENTINEL))).all()), (what, tuple(o.shape))
    assert ops.persist_errors() == 0


def _ws(nbytes):
    return _sent(max(int(nbytes), 16) // 4 + 1)


@pytest.mark.parametrize('E,C', [(20, 4), (16, 2), (40, 7)])
def test_hard_kmeans_outside_the_table_is_refused(F, ops, E, C):
    from ams_hip._lib import AmsError
    assert (E, C) not in HARD_KMEANS
    lib, p, s = ops.load(), ops._p, ops._s
    b, tries, L = 2, 2, 300
    R = b * tries
    xn = ops.kmeans_normalize(_rand(b, L, E))
    cent = _rand(R, C, E)
    nb = lib.ams_kmeans_workspace_bytes(R, L, E, C)
    tk = torch.zeros(R, dtype=torch.int32, device='cuda')
    for beta in (-1.0, 10.0):                                      # hard, and the soft forward of the same two entry points
        if beta >= 0 and E == 40:
            continue                                               # (40, 7) is stopped by C <= 6 either way; once is enough
        out, den, ws = _sent(R, C, E), _sent(R, C), _ws(nb)
        _refused(ops, lambda: lib.ams_kmeans_iterate(p(xn), p(None), p(cent), p(out), p(den), b, tries, L, E, C, beta, 1, p(ws), nb, p(tk), s()),
                 'ams_kmeans_iterate', [out, den, ws])
        lab, soft, inertia = _sent(R, L, dtype=torch.int32), _sent(R, L, C), _sent(R)
        _refused(ops, lambda: lib.ams_kmeans_assign(p(xn), p(None), p(cent), p(lab if beta < 0 else None), p(soft if beta >= 0 else None),
                                                    p(inertia), b, tries, L, E, C, beta, 1, p(ws), nb, p(tk), s()),
                 'ams_kmeans_assign', [lab, soft, inertia, ws])
    assert not bool(tk.any())
    idx = dev(np.stack([np.arange(C) for _ in range(R)]), np.int32)
    with pytest.raises(AmsError, match='AMS_E_INVALID_ARG'):       # and through the wrapper the models call
        F.kmeans(_rand(b, L, E), idx, C, tries, 3, None, None, True)
    torch.cuda.synchronize()
    assert ops.persist_errors() == 0


@pytest.mark.parametrize('E,C', [(8, 4), (20, 3)])
def test_soft_kmeans_backward_outside_its_table_is_refused(ops, E, C):
    assert (E, C) in SOFT_FORWARD and (E, C) not in SOFT_BACKWARD
    lib, p, s = ops.load(), ops._p, ops._s
    b, L, n_it = 2, 300, 2
    xn = ops.kmeans_normalize(_rand(b, L, E))
    cents, dens = _rand(n_it + 1, b, C, E), _rand(n_it, b, C).abs() + 1.0
    dsel, dout = _rand(b, C, E), _rand(b, L, C)
    nb = lib.ams_kmeans_soft_bwd_workspace_bytes(b, L, E, C, n_it)
    dx, g0, ws = _sent(b, L, E), _sent(b, C, E), _ws(nb)
    _refused(ops, lambda: lib.ams_kmeans_soft_bwd(p(xn), p(None), p(None), p(cents), p(dens), p(dsel), p(dout), p(None), p(None), p(None),
                                                  p(dx), p(g0), b, L, E, C, 3.0, n_it, p(ws), nb, s()),
             'ams_kmeans_soft_bwd', [dx, g0, ws])


@pytest.mark.parametrize('E', [5, 64])
def test_l41_outside_the_table_is_refused(F, ops, E):
    from ams_hip._lib import AmsError
    assert E not in LOSS_E
    lib, p, s = ops.load(), ops._p, ops._s
    B, TF, S, K = 2, 300, 2, 4
    emb, vs, negs = _rand(B, TF, E), _rand(B, S, E), _rand(B, 1, K, E)
    y = dev(np.where(np.random.RandomState(E).rand(B, TF, S) > 0.5, 1.0, -1.0))
    up = torch.ones(1, device='cuda')
    nb, nbn = lib.ams_l41_workspace_bytes(B, TF, E, S), lib.ams_l41_ns_workspace_bytes(B, TF, E, S, 1, K)
    for from_u in (0, 1):
        cost, ws = _sent(1), _ws(nbn)
        _refused(ops, lambda: lib.ams_l41_loss_fwd(p(emb), p(y), p(vs), p(cost), B, TF, E, S, from_u, p(ws), nb, s()), 'ams_l41_loss_fwd',
                 [cost, ws])
        _refused(ops, lambda: lib.ams_l41_loss_ns_fwd(p(emb), p(y), p(vs), p(negs), p(cost), B, TF, E, S, 1, K, 0.3, from_u, p(ws), nbn, s()),
                 'ams_l41_loss_ns_fwd', [cost, ws])
        demb, dvs, dnegs, am = _sent(B, TF, E), _sent(B, S, E), _sent(B, 1, K, E), _sent(1)
        _refused(ops, lambda: lib.ams_l41_loss_bwd(p(emb), p(y), p(vs), p(up), p(demb), p(dvs), p(am), B, TF, E, S, from_u, p(ws), nb, s()),
                 'ams_l41_loss_bwd', [demb, dvs, am, ws])
        _refused(ops, lambda: lib.ams_l41_loss_ns_bwd(p(emb), p(y), p(vs), p(negs), p(up), p(demb), p(dvs), p(dnegs), p(am), B, TF, E, S, 1, K,
                                                      0.3, from_u, p(ws), nbn, s()), 'ams_l41_loss_ns_bwd', [demb, dvs, dnegs, am, ws])
    spk = _rand(11, E).requires_grad_()
    with pytest.raises(AmsError, match='AMS_E_INVALID_ARG'):
        F.l41_loss(emb.requires_grad_(), y, spk, dev(np.array([[0, 3], [5, 1]]), np.int32), False)
    torch.cuda.synchronize()
    assert ops.persist_errors() == 0


@pytest.mark.parametrize('E', [5, 64])
def test_danet_outside_the_table_is_refused(ops, E):
    assert E not in LOSS_E
    lib, p, s = ops.load(), ops._p, ops._s
    B, TF, S = 2, 300, 2
    v, x, xnm = _rand(B, TF, E), _rand(B, TF), _rand(B, TF, S)
    y = dev(np.where(np.random.RandomState(E).rand(B, TF, S) > 0.5, 1.0, -1.0))
    up = torch.ones(1, device='cuda')
    nb = lib.ams_danet_workspace_bytes(B, TF, E, S)
    cost, attr, g, dattr, ws = _sent(1), _sent(B, S, E), _sent(B, TF, S), _sent(B, S, E), _ws(nb)
    _refused(ops, lambda: lib.ams_danet_recon_fwd(p(v), p(y), p(None), 0.0, p(x), p(xnm), 0, p(cost), p(attr), p(g), p(dattr), B, TF, E, S,
                                                  p(ws), nb, s()), 'ams_danet_recon_fwd', [cost, attr, g, dattr, ws])
    dv, am = _sent(B, TF, E), _sent(1)
    gg, aa = _rand(B, TF, S), _rand(B, S, E)
    _refused(ops, lambda: lib.ams_danet_recon_bwd(p(y), p(None), 0.0, p(gg), p(aa), p(aa), p(up), p(dv), 0, p(am), B, TF, E, S, p(ws), nb, s()),
             'ams_danet_recon_bwd', [dv, am, ws])


@pytest.mark.parametrize('E,S', [(61, 4), (57, 8), (63, 2)])
def test_dpcl_past_four_tiles_is_refused(ops, E, S):
    assert E + S == DPCL_MAX_E_PLUS_S + 1
    lib, p, s = ops.load(), ops._p, ops._s
    B, TF = 2, 300
    U = _rand(B, TF, E)
    Y = dev(np.eye(S)[np.random.RandomState(E).randint(0, S, (B, TF))])
    nb, nbu = lib.ams_dpcl_workspace_bytes(B, TF, E, S), lib.ams_dpcl_u_workspace_bytes(B, TF, E, S)
    out, ws = _sent(4), _ws(max(nb, nbu))
    _refused(ops, lambda: lib.ams_dpcl_loss_fwd(p(U), p(Y), p(out), B, TF, E, S, p(ws), nb, s()), 'ams_dpcl_loss_fwd', [out, ws])
    _refused(ops, lambda: lib.ams_dpcl_u_count_labels(p(Y), B, TF, E, S, p(ws), nbu, s()), 'ams_dpcl_u_count_labels', [ws])
    inv, V = _sent(B, TF), _sent(B, TF, E)
    _refused(ops, lambda: lib.ams_dpcl_loss_fwd_u(p(U), p(Y), p(inv), p(V), p(out), B, TF, E, S, 0, p(ws), nbu, s()), 'ams_dpcl_loss_fwd_u',
             [inv, V, out, ws])
    dU, iv = _sent(B, TF, E), _rand(B, TF).abs()
    _refused(ops, lambda: lib.ams_dpcl_loss_bwd_u(p(U), p(Y), p(iv), p(None), p(dU), B, TF, E, S, p(ws), s()), 'ams_dpcl_loss_bwd_u', [dU, ws])


def test_dpcl_normalised_backward_outside_its_switch_is_refused(ops):
    E, S = 5, 2
    assert E not in DPCL_BWD_E
    lib, p, s = ops.load(), ops._p, ops._s
    B, TF = 2, 300
    V = _rand(B, TF, E)
    Y = dev(np.eye(S)[np.random.RandomState(E).randint(0, S, (B, TF))])
    ws = _ws(lib.ams_dpcl_workspace_bytes(B, TF, E, S))
    dU = _sent(B, TF, E)
    _refused(ops, lambda: lib.ams_dpcl_loss_bwd(p(V), p(Y), p(None), p(None), p(dU), B, TF, E, S, p(ws), s()), 'ams_dpcl_loss_bwd', [dU, ws])
