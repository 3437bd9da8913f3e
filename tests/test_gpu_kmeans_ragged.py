"""GPU: hard k-means over segments of different numbers of points in one call (ams_hip/kmeans_ragged.py, libams_kmeans_ragged.so,
include/ams_kmeans_ragged.h).  Every segment must come out, bit for bit, as oracle/kmeans.py gives it alone as a batch of one and as
ops.kmeans_run gives it alone -- centroids (NaN where a cluster is empty), labels and the chosen try -- whatever its neighbours in the
packed buffer are; the number of launches must not depend on the number of segments; nothing outside the outputs may be written.
Every comparison is exact: the summation order is shared by construction (chunks of 8192 points restarted at each segment)."""
import numpy as np
import pytest

from oracle import kmeans as okm

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

SEGS = [37, 64, 197, 3000, 8192, 8193, 16384 + 130]     # below a slab, a slab, ragged, one chunk to the point, one over, three chunks
ITERS = 2
_SEG, _REF = {}, {}


def _segment(P, E, C, kind, seed=0):
    """One segment's blobs (as _data of tests/test_gpu_kmeans_tries.py, spread 2.5), ten rows of seeds and its weights; made once."""
    key = (P, E, C, kind, seed)
    if key not in _SEG:
        rng = np.random.RandomState(1000 * seed + P + 7 * E + C)
        centers = rng.randn(C, E).astype(np.float32) * 1.5
        X = (centers[rng.randint(0, C, P)] + rng.randn(P, E).astype(np.float32) * 2.5).astype(np.float32)
        idx = np.stack([rng.choice(P, C, replace=False) for _ in range(10)]).astype(np.int32)
        w = None
        if kind == 'mask':
            w = (rng.rand(P) > 0.25).astype(np.float32)
        elif kind == 'real':
            w = rng.uniform(0.05, 1.7, P).astype(np.float32)
        elif kind == 'zero':
            w = np.zeros(P, np.float32)
        _SEG[key] = (X, idx, w)
    return _SEG[key]


def _oracle(P, E, C, kind, tries, end, seed=0):
    """oracle/kmeans.py::kmeans on the segment alone (b = 1).  The run is made once per (segment, tries) with assign_at_end off; with it
    on, the labels are the oracle's own re-assignment to the chosen centroids without weights (oracle/kmeans.py, the last lines of kmeans)."""
    key = (P, E, C, kind, tries, seed)
    X, _, w = _segment(P, E, C, kind, seed)
    if key not in _REF:
        _REF[key] = okm.kmeans(X[None], _segment(P, E, C, kind, seed)[1][:tries], C, tries, ITERS, beta=None,
                               notsilent=None if w is None else w[None], assign_at_end=False)
    cent, lab, best = _REF[key]
    if end:
        lab = okm.labels_hard(okm.l2_normalize_rows(X), cent[0], np.ones(P, np.float32))[None]
    return cent, lab, best


def _pack(sizes, E, C, kinds, tries, seed=0):
    parts = [_segment(P, E, C, k, seed) for P, k in zip(sizes, kinds)]
    X = np.concatenate([p[0] for p in parts])
    idx = np.concatenate([p[1][:tries] for p in parts])
    w = None
    if any(p[2] is not None for p in parts):
        w = np.concatenate([np.ones(P, np.float32) if p[2] is None else p[2] for P, p in zip(sizes, parts)])
    return X, idx, w


def _check(sizes, E, C, tries, end, kinds=None, against_run=True, oracle_on=None, dev=None, seed=0):
    """One ragged call over `sizes`; every segment against the oracle (those in oracle_on; default all) and against ops.kmeans_run."""
    from ams_hip import kmeans_ragged as kr
    from ams_hip import ops
    kinds = kinds or [None] * len(sizes)
    X, idx, w = _pack(sizes, E, C, kinds, tries, seed)
    up = dev or (lambda a, dt=np.float32: torch.from_numpy(np.ascontiguousarray(a, dt)).cuda())
    xd, wd = up(X), None if w is None else up(w)
    seg = kr.segments(sizes)
    n0 = kr.LAUNCHES
    cent, lab, best = kr.kmeans_ragged(xd, seg, idx, C, tries, ITERS, w=wd, assign_at_end=end)
    launches = kr.LAUNCHES - n0
    torch.cuda.synchronize()
    assert cent.shape == (len(sizes), C, E) and lab.shape == (sum(sizes),) and best.shape == (len(sizes),)
    cent, lab, best = cent.cpu().numpy(), lab.cpu().numpy(), best.cpu().numpy()
    for r, P in enumerate(sizes):
        if against_run:
            rows = seg.rows(r)
            xn = ops.kmeans_normalize(xd[rows].contiguous()[None])
            wr = None if wd is None else wd[rows].contiguous()[None]
            c1, l1, b1, _ = ops.kmeans_run(xn, up(idx[r * tries:(r + 1) * tries], np.int32), C, tries, ITERS, w=wr, assign_at_end=end)
            torch.cuda.synchronize()
            assert best[r] == int(b1[0]), (r, P)
            assert np.array_equal(cent[r], c1[0].cpu().numpy(), equal_nan=True), (r, P)
            assert np.array_equal(lab[rows], l1[0].cpu().numpy()), (r, P)
    # the oracle: the segments whose every point is silent last
    for r in sorted(range(len(sizes)), key=lambda q: kinds[q] == 'zero'):
        if oracle_on is not None and r not in oracle_on:
            continue
        P, rows = sizes[r], seg.rows(r)
        # (a segment without weights beside weighted ones runs with ones: x * 1 == x, the oracle's own default)
        c_ref, l_ref, b_ref = _oracle(P, E, C, kinds[r], tries, end, seed)
        if kinds[r] == 'zero':
            print('all-zero segment %d (P = %d): NaN centroid rows: ours %s, oracle %s; labels that differ: %d of %d; best %d / %d'
                  % (r, P, np.isnan(cent[r]).all(axis=1).tolist(), np.isnan(c_ref[0]).all(axis=1).tolist(),
                     int((lab[rows] != l_ref[0]).sum()), P, best[r], b_ref[0]))
        assert best[r] == b_ref[0], (r, P)
        assert np.array_equal(cent[r], c_ref[0], equal_nan=True), (r, P)
        assert np.array_equal(lab[rows], l_ref[0]), (r, P)
    return launches


@pytest.mark.parametrize('end', [True, False])
@pytest.mark.parametrize('tries', [5, 10])
@pytest.mark.parametrize('order', ['forward', 'reversed'])
def test_every_segment_is_the_oracle_and_kmeans_run_on_it_alone(order, tries, end):
    sizes = SEGS if order == 'forward' else SEGS[::-1]
    assert _check(sizes, 40, 2, tries, end) == ITERS + 4


@pytest.mark.parametrize('end', [True, False])
@pytest.mark.parametrize('tries', [5, 10])
@pytest.mark.parametrize('order', ['forward', 'reversed'])
def test_silence_weights(order, tries, end):
    """A 0/1 mask and real weights: silent points are counted in the denominators and labelled 0."""
    kinds = ['mask', 'real', 'mask', 'real', 'real', 'mask', 'real']
    sizes = SEGS
    if order == 'reversed':
        sizes, kinds = SEGS[::-1], kinds[::-1]
    _check(sizes, 40, 2, tries, end, kinds)


@pytest.mark.parametrize('end', [True, False])
@pytest.mark.parametrize('tries', [5, 10])
@pytest.mark.parametrize('order', ['forward', 'reversed'])
def test_silence_weights_with_an_all_zero_segment(order, tries, end):
    """The same with a segment whose weights are ALL zero between the others.  Every point of it is silent, all are labelled 0, cluster 1
    is empty and its centroid is 0 / 0 = NaN after the first update.  From then on an assignment compares a distance with NaN; the
    kernels take it as np.argmin in the oracle does (the first NaN wins: csrc/kmeans.hip), so the labels flip to 1, the centroids
    alternate between [0, NaN] and [NaN, 0] from one update to the next and every try's inertia is NaN.  Every segment, this one
    included, must equal ops.kmeans_run on it alone AND oracle/kmeans.py on it alone."""
    kinds = ['mask', 'real', 'mask', 'zero', 'real', 'mask', 'real']
    sizes = SEGS
    if order == 'reversed':
        sizes, kinds = SEGS[::-1], kinds[::-1]
    _check(sizes, 40, 2, tries, end, kinds)


@pytest.mark.parametrize('tries', [5, 10])
def test_one_segment(tries):
    assert _check([8192 + 257], 40, 2, tries, True) == ITERS + 4


def test_launches_do_not_depend_on_the_number_of_segments():
    sizes = [100 + (r * 617) % 601 for r in range(40)]                      # 40 segments of 100 .. 700 points
    assert min(sizes) >= 100 and max(sizes) <= 700 and len(set(sizes)) > 30
    many = _check(sizes, 40, 2, 5, True, oracle_on=(0, 17, 39))
    one = _check(sizes[:1], 40, 2, 5, True)
    assert many == one == ITERS + 4


@pytest.mark.parametrize('E,C,tries', [(8, 3, 2), (40, 6, 5)])
@pytest.mark.parametrize('kind', [None, 'mask'])
def test_other_arms(E, C, tries, kind):
    """The per-try pass (8, 3) and the grouped accumulation of five and six clusters (40, 6)."""
    _check([900, 8192 + 257], E, C, tries, True, [kind, kind])
    _check([900, 8192 + 257], E, C, tries, False, [kind, kind], against_run=False)


def _every_pair():
    from ams_hip import kmeans_ragged as kr
    return sorted(kr.PAIRS)


@pytest.mark.parametrize('end', [True, False])
@pytest.mark.parametrize('kind', [None, 'mask'])
@pytest.mark.parametrize('order', ['forward', 'reversed'])
@pytest.mark.parametrize('E,C', _every_pair())
def test_the_per_try_pass_of_every_pair(E, C, order, kind, end):
    """tries = 2: every (E, C) the library takes, (40, 2) included, runs the per-try pass -- accumulation (the grouped kernel at C = 5, 6),
    inertia and labels -- over a full chunk plus 257 points (a second chunk whose second slab has one lane), a segment shorter than a
    wave, and an exact chunk, so that the segment after it starts on a chunk edge."""
    sizes = [8449, 37, 8192]
    if order == 'reversed':
        sizes = sizes[::-1]
    assert _check(sizes, E, C, 2, end, [kind] * 3) == ITERS + 4


def test_empty_cluster_gives_the_oracles_nan():
    """Two seed indices that hold the SAME point: every point is as near to centroid 0 as to centroid 1, the tie goes to 0, cluster 1 is
    empty and its centroid is 0 / 0 after the first update.  The assignments against the NaN centroid that follow go as the oracle's
    np.argmin (the first NaN wins), so centroids, labels and the chosen try are compared in full, as for the healthy neighbour."""
    from ams_hip import kmeans_ragged as kr
    E, C, tries = 40, 2, 5
    Xa, ia, _ = _segment(700, E, C, None, seed=3)
    Xb, ib, _ = _segment(300, E, C, None, seed=3)
    Xb = Xb.copy()
    Xb[11] = Xb[5]
    ib = np.tile(np.array([[5, 11]], np.int32), (tries, 1))
    X, idx = np.concatenate([Xa, Xb]), np.concatenate([ia[:tries], ib])
    for iters in (1, ITERS):
        cent, lab, best = kr.kmeans_ragged(torch.from_numpy(X).cuda(), [700, 300], idx, C, tries, iters)
        torch.cuda.synchronize()
        ref_a = okm.kmeans(Xa[None], ia[:tries], C, tries, iters, beta=None, notsilent=None, assign_at_end=True)
        ref_b = okm.kmeans(Xb[None], ib, C, tries, iters, beta=None, notsilent=None, assign_at_end=True)
        assert np.isnan(ref_b[0][0]).all(axis=1).sum() == 1 and not np.isnan(ref_a[0]).any()
        if iters == 1:
            assert np.isnan(ref_b[0][0, 1]).all()
        for r, (ref, rows) in enumerate(((ref_a, slice(0, 700)), (ref_b, slice(700, 1000)))):
            assert np.array_equal(cent[r].cpu().numpy(), ref[0][0], equal_nan=True), (iters, r)
            assert np.array_equal(lab[rows].cpu().numpy(), ref[1][0]) and int(best[r]) == ref[2][0], (iters, r)


@pytest.mark.parametrize('E,C,tries,kinds', [(40, 2, 5, None), (40, 2, 10, ['mask', 'real', 'zero']), (8, 3, 2, None), (40, 6, 5, None),
                                             (40, 4, 2, None), (8, 5, 2, None)])
@pytest.mark.parametrize('base', [0, 4, 12])
def test_inside_fenced_buffers(E, C, tries, kinds, base):
    """Red zones around every operand, NaN-filled outputs and workspaces, the points and weights at an odd base: nothing outside the
    outputs is written (Fence.check on exit) and the results are those of the aligned run (the oracle's)."""
    from tests.fenced import Fence
    with Fence() as fence:
        _check([197, 8192 + 257, 900], E, C, tries, True, kinds, against_run=False, dev=lambda a, dt=np.float32: fence.dev(a, dt, base=base))
        fence.check()
