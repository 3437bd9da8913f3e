"""GPU: the number of clusters per segment of a ragged point set in one counted call (ams_hip/spk_count.py, libams_spk_count.so,
include/ams_spk_count.h) against the float64 restatement tests/speaker_count_ref.py.

The points are the planted family (speaker_count_ref.planted: centres on the unit sphere, noise 0.1 N(0, I) / sqrt(E), renormalised).
The k-means of every candidate is the existing ragged one (tested against oracle/kmeans.py in tests/test_gpu_kmeans_ragged.py), so the
restatement is given every try's centroids and inertias as the device produced them and restates what is new: the try of a candidate
(first smallest FINITE inertia), its score, the count, the selected centroids; the labels are compared with the existing labels pass
on the chosen candidate's centroids.

Bounds.  Scores: 1e-9 absolute (float64 sums of <= 2e5 non-negative terms in [0, 1] err by at most N 2^-53 ~ 2e-11 relative; the
per-point terms err by ~1e-14 in the difference-first form).  Tries and counts: equal; every restatement margin on these inputs is
asserted to be >= 1e-6, so a score off by 1e-9 cannot change a count."""
import numpy as np
import pytest

from tests import speaker_count_ref as ref

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

SEGS = [37, 64, 197, 3000, 8192, 8193, 16384 + 130]     # as tests/test_gpu_kmeans_ragged.py: below a slab .. three chunks
ITERS = 3
TOL = 1e-9
MARGIN = 1e-6
_SEG = {}


def _segment(P, E, hi, kind, r):
    """One segment: planted points with 2 + r % (hi - 1) clusters, ten seed rows of hi columns, its weights; made once."""
    key = (P, E, hi, kind, r)
    if key not in _SEG:
        true = 2 + r % (hi - 1)
        x = ref.planted(true, P, E, 31 * P + E + r)
        idx = ref.draw_seeds(P, 10, hi, 7 * P + E + r)
        rng = np.random.RandomState(P + 3 * r)
        w = None
        if kind == 'mask':
            w = (rng.rand(P) > 0.25).astype(np.float32)
        elif kind == 'real':
            w = rng.uniform(0.05, 1.7, P).astype(np.float32)
        elif kind == 'zero':
            w = np.zeros(P, np.float32)
        _SEG[key] = (x, idx, w, true)
    return _SEG[key]


def _pack(sizes, E, hi, kinds, tries):
    parts = [_segment(P, E, hi, k, r) for r, (P, k) in enumerate(zip(sizes, kinds))]
    X = np.concatenate([p[0] for p in parts])
    idx = np.concatenate([p[1][:tries] for p in parts])
    w = None
    if any(p[2] is not None for p in parts):
        w = np.concatenate([np.ones(P, np.float32) if p[2] is None else p[2] for P, p in zip(sizes, parts)])
    return X, idx, w, [p[3] for p in parts]


def _host(res):
    out = {k: res[k].cpu().numpy() for k in ('count', 'cand', 'scores', 'tries', 'centroids', 'labels')}
    out['sel'] = [s.cpu().numpy() for s in res['sel']]
    return out


def _against_ref(got, X, w, sizes, cents, inertias, tries, lo, hi, min_score, labels_of):
    """Every segment of one counted call against the restatement on the device's tries."""
    off = np.concatenate([[0], np.cumsum(sizes)])
    counts = []
    for r, P in enumerate(sizes):
        rows = slice(int(off[r]), int(off[r + 1]))
        want = ref.count(X[rows], None if w is None else w[rows], None, lo, hi, ITERS, min_score,
                         cents=[c[r * tries:(r + 1) * tries] for c in cents], inertias=[i[r * tries:(r + 1) * tries] for i in inertias])
        m = ref.margin(want['scores'])
        fin = np.isfinite(want['scores'])
        print('segment %d (P = %d): count %d / %d, tries %s / %s, margin %.3g, max |score - ref| %.3g'
              % (r, P, got['count'][r], want['count'], got['tries'][r].tolist(), want['tries'].tolist(), m,
                 np.abs(got['scores'][r][fin] - want['scores'][fin]).max() if fin.any() else 0.0))
        assert m >= MARGIN, (r, P, want['scores'])
        if min_score is not None and fin.any():
            assert abs(want['scores'].max() - min_score) >= MARGIN, (r, P)
        assert np.array_equal(np.isfinite(got['scores'][r]), fin) and np.all(got['scores'][r][~fin] == -np.inf), (r, P)
        assert np.all(np.abs(got['scores'][r][fin] - want['scores'][fin]) <= TOL), (r, P)
        assert np.array_equal(got['tries'][r], want['tries']), (r, P)
        assert got['count'][r] == want['count'] and got['cand'][r] == want['cand'], (r, P)
        assert np.array_equal(got['centroids'][r], want['centroids'], equal_nan=True), (r, P)
        for k in range(len(cents)):
            assert np.array_equal(got['sel'][k][r], want['sel'][k], equal_nan=True), (r, P, k)
        lab = np.zeros(P, np.int32) if want['cand'] < 0 else labels_of[want['cand']][rows]
        assert np.array_equal(got['labels'][rows], lab), (r, P)
        counts.append(want['count'])
    return counts


def _check(sizes, E, hi, tries, kinds=None, lo=2, min_score=None, end=True, poison=(), alone=True, dev=None):
    """One counted call over `sizes` against the restatement, and every segment against the call on it alone.  poison: (segment,
    candidate, tries to make NaN) entries applied to the device's inertias and centroids before the scoring half."""
    from ams_hip import kmeans_ragged as kr
    from ams_hip import spk_count as sc
    kinds = kinds or [None] * len(sizes)
    X, idx, w, true = _pack(sizes, E, hi, kinds, tries)
    up = dev or (lambda a, dt=np.float32: torch.from_numpy(np.ascontiguousarray(a, dt)).cuda())
    xd, wd = up(X), None if w is None else up(w)
    seg = kr.segments(sizes)
    c_lo = max(lo, 2)
    n0 = kr.LAUNCHES + sc.LAUNCHES
    if poison:
        runs = [kr.kmeans_ragged_tries(xd, seg, np.ascontiguousarray(idx[:, :C]), C, tries, ITERS, w=wd, normalize_input=False)
                for C in range(c_lo, hi + 1)]
        cents, inertias = [r[0] for r in runs], [r[1] for r in runs]
        for r, k, ts in poison:
            for t in ts:
                inertias[k][r * tries + t] = float('nan')
                cents[k][r * tries + t, -1] = float('nan')
        res = sc.count_from_tries(xd, seg, cents, inertias, lo, tries, w=wd, assign_at_end=end, min_score=min_score)
    else:
        res = sc.count_clusters(xd, seg, idx, lo, hi, tries, ITERS, w=wd, assign_at_end=end, normalize_input=False, min_score=min_score)
    launches = kr.LAUNCHES + sc.LAUNCHES - n0
    torch.cuda.synchronize()
    assert res['scores'].shape == (len(sizes), hi - c_lo + 1) and res['centroids'].shape == (len(sizes), hi, E)
    got = _host(res)
    if not poison:
        # the tries the call ran, again (the same launches on the same inputs: the same bits), for the restatement
        runs = [kr.kmeans_ragged_tries(xd, seg, np.ascontiguousarray(idx[:, :C]), C, tries, ITERS, w=wd, normalize_input=False)
                for C in range(c_lo, hi + 1)]
        cents, inertias = [r[0] for r in runs], [r[1] for r in runs]
    labels_of = [kr.labels_ragged(xd, seg, s, None if end else wd).cpu().numpy() for s in res['sel']]
    counts = _against_ref(got, X, w, sizes, [c.cpu().numpy() for c in cents], [i.cpu().numpy() for i in inertias], tries, lo, hi,
                          min_score, labels_of)
    # rows >= count of the packed centroids are zero
    for r, n in enumerate(counts):
        assert not got['centroids'][r, n:].any() and (n == 1 or got['labels'][seg.rows(r)].max() < n), r
    if alone and not poison:
        for r, P in enumerate(sizes):
            rows = seg.rows(r)
            one = _host(sc.count_clusters(xd[rows].contiguous(), [P], idx[r * tries:(r + 1) * tries], lo, hi, tries, ITERS,
                                          w=None if wd is None else wd[rows].contiguous(), assign_at_end=end, normalize_input=False,
                                          min_score=min_score))
            assert np.array_equal(one['scores'][0], got['scores'][r]) and np.array_equal(one['tries'][0], got['tries'][r]), (r, P)
            assert one['count'][0] == got['count'][r] and np.array_equal(one['labels'], got['labels'][rows]), (r, P)
            assert np.array_equal(one['centroids'][0], got['centroids'][r], equal_nan=True), (r, P)
    return launches, counts, true


@pytest.mark.parametrize('E,hi', [(8, 3), (40, 6)])
@pytest.mark.parametrize('tries', [5, 10])
@pytest.mark.parametrize('order', ['forward', 'reversed'])
def test_every_segment_is_the_restatement_and_the_call_on_it_alone(order, tries, E, hi):
    sizes = SEGS if order == 'forward' else SEGS[::-1]
    launches, counts, true = _check(sizes, E, hi, tries)
    ncand = hi - 1
    assert launches == ncand * (ITERS + 3) + 4
    print('planted %s, counted %s' % (true, counts))


@pytest.mark.parametrize('E,hi', [(8, 3), (40, 6)])
@pytest.mark.parametrize('end', [True, False])
@pytest.mark.parametrize('order', ['forward', 'reversed'])
def test_weights(order, end, E, hi):
    """A 0/1 mask and real weights; one segment whose weights are ALL zero: every try of every candidate has a NaN inertia and sum w is
    zero, so every candidate is disqualified, the count is lo = 2 and the labels are those of kmeans_ragged's own selection."""
    kinds = ['mask', 'real', 'mask', 'zero', 'real', None, 'real']
    sizes = SEGS
    if order == 'reversed':
        sizes, kinds = SEGS[::-1], kinds[::-1]
    _, counts, _ = _check(sizes, E, hi, 5, kinds, end=end)
    assert counts[kinds.index('zero')] == 2


def test_one_speaker_below_min_score_and_when_nothing_qualifies():
    """lo = 1: the all-zero-weight segment has no qualified candidate and counts 1 with labels 0; a min_score above every score makes
    every segment count 1; a min_score of 0.5 leaves the planted ones alone."""
    kinds = [None, 'zero', 'real']
    _, counts, _ = _check([197, 900, 8192 + 257], 40, 4, 5, kinds, lo=1, min_score=0.5)
    assert counts[1] == 1 and counts[0] >= 2 and counts[2] >= 2
    _, counts, _ = _check([197, 900, 8192 + 257], 40, 4, 5, kinds, lo=1, min_score=0.999)
    assert counts == [1, 1, 1]


@pytest.mark.parametrize('E,hi,tries', [(8, 3, 5), (40, 6, 10)])
def test_non_finite_tries(E, hi, tries):
    """Segment 1: tries 0 .. 2 of candidate 0 get a NaN inertia (and a NaN centroid row): they are skipped, the pick is a later try.
    Segment 2: EVERY try of the last candidate is NaN: it is disqualified (score -inf, try -1), it cannot be chosen, and its selected
    centroids are those of kmeans_ragged's own selection (the first NaN: try 0).  Segment 0 is untouched."""
    sizes = [900, 3000, 8192 + 257]
    poison = [(1, 0, (0, 1, 2)), (2, hi - 2, tuple(range(tries)))]
    from ams_hip import kmeans_ragged as kr
    from ams_hip import spk_count as sc
    _check(sizes, E, hi, tries, poison=poison)
    # the restatement agreed (inside _check); the same two properties by hand
    X, idx, _, _ = _pack(sizes, E, hi, [None] * 3, tries)
    xd = torch.from_numpy(X).cuda()
    runs = [kr.kmeans_ragged_tries(xd, sizes, np.ascontiguousarray(idx[:, :C]), C, tries, ITERS, normalize_input=False) for C in range(2, hi + 1)]
    cents, inertias = [r[0] for r in runs], [r[1] for r in runs]
    for r, k, ts in poison:
        for t in ts:
            inertias[k][r * tries + t] = float('nan')
    res = sc.count_from_tries(xd, sizes, cents, inertias, 2, tries)
    tr, scs = res['tries'].cpu().numpy(), res['scores'].cpu().numpy()
    assert tr[1, 0] >= 3 and np.isfinite(scs[1, 0])
    assert tr[2, hi - 2] == -1 and scs[2, hi - 2] == -np.inf and int(res['cand'][2]) != hi - 2
    assert torch.equal(res['sel'][hi - 2][2], cents[hi - 2][2 * tries])


@pytest.mark.parametrize('E,hi', [(8, 3), (40, 6)])
def test_launches_do_not_depend_on_the_number_of_segments(E, hi):
    sizes = [100 + (r * 617) % 601 for r in range(40)]                      # 40 segments of 100 .. 700 points
    many, _, _ = _check(sizes, E, hi, 5, alone=False)
    one, _, _ = _check(sizes[:1], E, hi, 5)
    assert many == one == (hi - 1) * (ITERS + 3) + 4


@pytest.mark.parametrize('E,hi,tries,kinds', [(40, 6, 5, None), (40, 6, 10, ['mask', 'real', 'zero']), (8, 3, 5, None)])
@pytest.mark.parametrize('base', [0, 4, 12])
def test_inside_fenced_buffers(E, hi, tries, kinds, base):
    """Red zones around every operand, NaN-filled outputs and workspaces, the points and weights at an odd base: nothing outside the
    outputs is written and the results are the restatement's."""
    from tests.fenced import Fence
    with Fence() as fence:
        _check([197, 8192 + 257, 900], E, hi, tries, kinds, alone=False, dev=lambda a, dt=np.float32: fence.dev(a, dt, base=base))
        fence.check()
