"""GPU: soft k-means over segments of different numbers of points in one call (ams_hip/kmeans_ragged_soft.py,
libams_kmeans_ragged_soft.so, include/ams_kmeans_ragged_soft.h).

Against float64 (tests/kmeans_soft_ragged_ref.py: the oracle's functions per try), per segment and per try, never only through the final
choice, with the tolerances the design fixes:
  * every try's centroids: max |err| <= 2 x the error ops.kmeans_run's own per-try centroids (its trace) show for the same segment, seeds
    and beta in the same run, + 1e-6 -- the two kernels share the arithmetic and differ in summation order;
  * every try's inertia: relative error <= 10 x the error of a float32 numpy run of the restatement on that segment, + 1e-6 -- the
    kernel's distance form |x|^2 - 2 <x, c> + |c|^2 cancels (about 1e-7 absolute on d^2);
  * best: the float64 choice where the float64 gap (second lowest - lowest) / lowest is >= 1e-3, else a try within 1e-3 of the minimum;
  * the returned masks within 1e-3 of the float64 labels of the try the library chose (the project's figure for the soft forward).
Independence is exact: a segment's centroids, inertia, choice and masks are bit-equal whatever its neighbours in the call are.

Measured (one run, one board; the tests print every figure): centroids within 2.9e-6 (ops.kmeans_run's own: 2.9e-6),
inertia within 8.7e-6 relative (at most 0.28 of its bound), masks within 7.9e-6."""
import numpy as np
import pytest

from tests import kmeans_soft_ragged_ref as ref

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

SEGS, TRIES, ITERS = ref.SEGS, ref.TRIES, ref.ITERS
CASES = [(8, 3, 3.0), (40, 6, 10.0), (40, 2, 5.0)]       # (E, C, beta); at (40, 2) the tries collapse onto one solution: the tie rule
GAP = 1e-3
_RUN = {}


def _up(a, dt=np.float32):
    return torch.from_numpy(np.ascontiguousarray(a, dt)).cuda()


def _pack(sizes, E, C, kinds):
    """The packed float32 points, the seeds and the weights (ones for a segment without weights beside weighted ones, or of kind 'one')."""
    X = np.concatenate([ref.segment(P, E, C)[0] for P in sizes]).astype(np.float32)
    idx = np.concatenate([ref.segment(P, E, C)[1][:TRIES] for P in sizes])
    w = None
    if any(k is not None for k in kinds):
        w = np.concatenate([np.ones(P) if k in (None, 'one') else ref.weights(P, E, C, k) for P, k in zip(sizes, kinds)]).astype(np.float32)
    return X, idx, w


def _call(sizes, E, C, beta, kinds, end, dev=_up):
    """One ragged call for every try and one full run -> numpy (cents [R, tries, C, E], inertia [R, tries], sel, masks, best) and the
    launches of the full run.  The full run's inertia and chosen centroids must be the every-try call's, to the bit."""
    from ams_hip import kmeans_ragged_soft as krs
    X, idx, w = _pack(sizes, E, C, kinds)
    xd, wd = dev(X), None if w is None else dev(w)
    seg = krs.segments(sizes)
    n0 = krs.LAUNCHES
    cents, inertia = krs.kmeans_ragged_soft_tries(xd, seg, idx, C, TRIES, ITERS, beta, w=wd)
    assert krs.LAUNCHES - n0 == ITERS + 2
    n0 = krs.LAUNCHES
    sel, masks, best, again = krs.kmeans_ragged_soft(xd, seg, idx, C, TRIES, ITERS, beta, w=wd, assign_at_end=end, want_inertia=True)
    launches = krs.LAUNCHES - n0
    torch.cuda.synchronize()
    R = len(sizes)
    assert cents.shape == (R * TRIES, C, E) and inertia.shape == (R * TRIES,) and sel.shape == (R, C, E) and best.shape == (R,)
    assert masks.shape == (sum(sizes), C) and masks.dtype == torch.float32 and best.dtype == torch.int32
    assert torch.equal(inertia, again)
    cents = cents.view(R, TRIES, C, E)
    assert torch.equal(sel, cents[torch.arange(R, device='cuda'), best.long()])
    return dict(seg=seg, cents=cents.cpu().numpy(), inertia=inertia.view(R, TRIES).cpu().numpy(), sel=sel.cpu().numpy(),
                masks=masks.cpu().numpy(), best=best.cpu().numpy(), launches=launches)


def _run_error(P, E, C, beta, kind):
    """max |err| per try of ops.kmeans_run's own final per-try centroids on the segment alone, against float64; measured once."""
    key = (P, E, C, beta, kind)
    if key not in _RUN:
        from ams_hip import ops
        X, idx, w = _pack([P], E, C, [kind])
        xn = ops.kmeans_normalize(_up(X)[None])
        _, _, _, trace = ops.kmeans_run(xn, _up(idx, np.int32), C, TRIES, ITERS, beta=beta, w=None if w is None else _up(w)[None])
        torch.cuda.synchronize()
        mine = trace[-2].cpu().numpy()                              # soft: trace = [c_0, c_1, den_0, ..., c_n, den_{n-1}]
        assert mine.shape == (TRIES, C, E)
        _RUN[key] = np.abs(mine - ref.reference(P, E, C, beta, kind).cents).max(axis=(1, 2))
    return _RUN[key]


def _check(sizes, E, C, beta, kinds, end, gap_required=False, dev=_up):
    """One call over `sizes`; every segment against float64 with the tolerances of the module doc.  Returns the call's results."""
    got = _call(sizes, E, C, beta, kinds, end, dev)
    worst = dict(cent=0.0, inertia=0.0, masks=0.0)
    for r, (P, kind) in enumerate(zip(sizes, kinds)):
        r64, r32 = ref.reference(P, E, C, beta, kind), ref.reference(P, E, C, beta, kind, np.float32)
        rows = got['seg'].rows(r)
        assert np.isfinite(got['cents'][r]).all() and np.isfinite(got['inertia'][r]).all() and np.isfinite(got['masks'][rows]).all()
        # every try's centroids
        err = np.abs(got['cents'][r] - r64.cents).max(axis=(1, 2))
        run = _run_error(P, E, C, beta, kind)
        print('P %5d (E %d, C %d, beta %g, w %s): centroid error per try %s, kmeans_run %s, ratio %.2f'
              % (P, E, C, beta, kind, ['%.1e' % v for v in err], ['%.1e' % v for v in run], float((err / np.maximum(run, 1e-12)).max())))
        assert (err <= 2 * run + 1e-6).all(), (r, P, err, run)
        # every try's inertia
        ierr = np.abs(got['inertia'][r] - r64.inertia) / r64.inertia
        i32 = float((np.abs(r32.inertia - r64.inertia) / r64.inertia).max())
        print('        inertia: relative error per try %s, float32 numpy %.1e; float64 gap %.2e' % (['%.1e' % v for v in ierr], i32, r64.gap))
        assert (ierr <= 10 * i32 + 1e-6).all(), (r, P, ierr, i32)
        # the choice
        b = int(got['best'][r])
        if gap_required:
            assert r64.gap >= GAP, (r, P, r64.gap)                 # the precondition holds: nothing is skipped silently
        if r64.gap >= GAP:
            assert b == r64.best, (r, P, b, r64.best, r64.inertia)
        else:
            assert r64.inertia[b] <= r64.inertia.min() * (1 + GAP), (r, P, b, r64.inertia)
        # what is returned: the chosen try's centroids and its labels
        assert np.abs(got['sel'][r] - r64.cents[b]).max() <= 2 * run[b] + 1e-6
        merr = float(np.abs(got['masks'][rows] - r64.masks(b, end)).max())
        print('        masks of try %d: max error %.1e' % (b, merr))
        assert merr <= 1e-3, (r, P, merr)
        assert np.abs(got['masks'][rows].sum(axis=1) - 1).max() <= 1e-6
        worst = dict(cent=max(worst['cent'], float(err.max())), inertia=max(worst['inertia'], float(ierr.max())), masks=max(worst['masks'], merr))
    print('worst over the call: centroids %.1e, inertia %.1e, masks %.1e' % (worst['cent'], worst['inertia'], worst['masks']))
    return got


@pytest.mark.parametrize('end', [True, False])
@pytest.mark.parametrize('kind', [None, 'mask', 'real'])
@pytest.mark.parametrize('E,C,beta', CASES)
def test_every_segment_and_every_try_against_float64(E, C, beta, kind, end):
    got = _check(SEGS, E, C, beta, [kind] * len(SEGS), end, gap_required=(E, C) != (40, 2))
    assert got['launches'] == ITERS + 4


@pytest.mark.parametrize('E,C,beta,kinds', [(40, 2, 5.0, ['real', None, 'mask', 'real', 'mask', 'real', 'real']),
                                            (8, 3, 3.0, [None] * 7), (40, 6, 10.0, ['mask'] * 7)])
@pytest.mark.parametrize('end', [True, False])
def test_a_segment_does_not_depend_on_its_neighbours(E, C, beta, kinds, end):
    """One call over SEGS, one over SEGS reversed and one call per segment alone: bit-equal centroids of every try, inertia, choice and
    masks for every segment."""
    fwd = _call(SEGS, E, C, beta, kinds, end)
    rev = _call(SEGS[::-1], E, C, beta, kinds[::-1], end)
    R = len(SEGS)
    for r, P in enumerate(SEGS):
        q = R - 1 - r
        rows, rrows = fwd['seg'].rows(r), rev['seg'].rows(q)
        one = _alone(P, E, C, beta, kinds[r], any(k is not None for k in kinds), end)
        for other, o, orows in ((rev, q, rrows), (one, 0, slice(0, P))):
            assert np.array_equal(fwd['cents'][r], other['cents'][o]) and np.array_equal(fwd['inertia'][r], other['inertia'][o]), (r, P)
            assert fwd['best'][r] == other['best'][o] and np.array_equal(fwd['sel'][r], other['sel'][o]), (r, P)
            assert np.array_equal(fwd['masks'][rows], other['masks'][orows]), (r, P)
        assert one['launches'] == fwd['launches'] == rev['launches'] == ITERS + 4


def _alone(P, E, C, beta, kind, weighted, end):
    """The segment in a call of its own; a segment without weights from a weighted call gets ones, as it has there."""
    return _call([P], E, C, beta, [kind or ('one' if weighted else None)], end)


def test_launches_do_not_depend_on_the_number_of_segments():
    sizes = [100 + (r * 617) % 601 for r in range(40)]              # 40 segments of 100 .. 700 points
    assert min(sizes) >= 100 and max(sizes) <= 700 and len(set(sizes)) > 30
    many = _call(sizes, 40, 2, 5.0, [None] * 40, True)
    seven = _call(SEGS, 40, 2, 5.0, [None] * 7, True)
    one = _call(sizes[:1], 40, 2, 5.0, [None], True)
    assert many['launches'] == seven['launches'] == one['launches'] == ITERS + 4
    # ... and the first of the forty is the one alone
    assert np.array_equal(many['cents'][0], one['cents'][0]) and np.array_equal(many['masks'][:sizes[0]], one['masks'])
    for r in (0, 17, 39):
        r64 = ref.reference(sizes[r], 40, 2, 5.0, None)
        assert np.abs(many['masks'][many['seg'].rows(r)] - r64.masks(int(many['best'][r]), True)).max() <= 1e-3


@pytest.mark.parametrize('end', [True, False])
@pytest.mark.parametrize('E,C,beta', [(40, 2, 5.0), (8, 3, 3.0)])
def test_a_segment_whose_weights_are_all_zero(E, C, beta, end):
    """Every point of it is silent: every label is 1 / C in every pass, the numerators are sums of x 0, so its centroids are 0, its
    inertia is the same for every try (the first is chosen), every mask is 1 / C and nothing is NaN.  Its neighbours are as they are
    without it."""
    sizes, kinds = [197, 3000, 8193, 900], ['real', 'zero', 'mask', None]
    got = _call(sizes, E, C, beta, kinds, end)
    rows = got['seg'].rows(1)
    for k in ('cents', 'inertia', 'sel', 'masks'):
        assert np.isfinite(got[k]).all(), k
    assert (got['cents'][1] == 0).all() and (got['sel'][1] == 0).all() and got['best'][1] == 0
    assert np.abs(got['masks'][rows] - 1.0 / C).max() <= 1e-6
    assert np.abs(got['inertia'][1] - C).max() <= 1e-4 * C          # sum_c (sum_l |x_l|^2 / C) / (P / C) with |x_l| = 1
    for r in (0, 2, 3):
        one = _alone(sizes[r], E, C, beta, kinds[r], True, end)
        assert np.array_equal(got['cents'][r], one['cents'][0]) and np.array_equal(got['masks'][got['seg'].rows(r)], one['masks']), r
        r64 = ref.reference(sizes[r], E, C, beta, kinds[r])
        assert np.abs(got['masks'][got['seg'].rows(r)] - r64.masks(int(got['best'][r]), end)).max() <= 1e-3


@pytest.mark.parametrize('kind', [None, 'real'])
@pytest.mark.parametrize('E,C', [(E, C) for E in (40, 8) for C in (2, 3, 4, 5, 6)])
def test_every_arm(E, C, kind):
    """All ten (E, C) pairs, with and without weights, below a chunk and one point over it."""
    _check([197, 8193], E, C, 4.0, [kind, kind], True)
    got = _call([197, 8193], E, C, 4.0, [kind, kind], False)
    for r, P in enumerate((197, 8193)):
        r64 = ref.reference(P, E, C, 4.0, kind)
        assert np.abs(got['masks'][got['seg'].rows(r)] - r64.masks(int(got['best'][r]), False)).max() <= 1e-3


@pytest.mark.parametrize('E,C,beta,kinds', [(40, 2, 5.0, ['mask', 'real', 'zero']), (8, 3, 3.0, [None] * 3), (40, 6, 10.0, ['real'] * 3)])
@pytest.mark.parametrize('base', [0, 4, 12])
def test_inside_fenced_buffers(E, C, beta, kinds, base):
    """Red zones around every operand, NaN-filled outputs and workspaces, the raw points and the weights at an odd base: nothing outside
    the outputs is written (Fence.check) and the results are those of the plain run, to the bit."""
    from tests.fenced import Fence
    sizes = [197, 8192 + 257, 900]
    plain = _call(sizes, E, C, beta, kinds, True)
    with Fence() as fence:
        got = _call(sizes, E, C, beta, kinds, True, dev=lambda a, dt=np.float32: fence.dev(a, dt, base=base))
        fence.check()
        off = _call(sizes, E, C, beta, kinds, False, dev=lambda a, dt=np.float32: fence.dev(a, dt, base=base))
        fence.check()
    for k in ('cents', 'inertia', 'sel', 'masks', 'best'):
        assert np.array_equal(got[k], plain[k]), k
    assert np.isfinite(off['masks']).all() and np.array_equal(off['cents'], plain['cents'])
    for r, (P, kind) in enumerate(zip(sizes, kinds)):
        r64 = ref.reference(P, E, C, beta, kind)
        assert np.abs(got['masks'][got['seg'].rows(r)] - r64.masks(int(got['best'][r]), True)).max() <= 1e-3
