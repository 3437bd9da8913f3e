"""GPU: k-means++ (D^2) seeding of a ragged point set -- ams_hip.kmeans_seed.seed_plusplus (include/ams_kmeans_seed.h)
against the numpy restatement tests/kmeans_seed_ref.py.  The sampling weights are integers and every sum is exact, so EVERY comparison
here is equality of int32 seeds (and, through the ragged k-means, of centroids, labels and chosen tries): no tolerance anywhere.

The base sizes [C, 255, 8192, 8193, 20000] are the smallest that have a segment of exactly C points, one below a workgroup's width, an
exact chunk, a chunk plus one point and a target that lands in a partial last chunk.  Every segment's points, draws and restated seeds
depend on its size alone and are computed once, whatever order or company the segment is tested in."""
import numpy as np
import pytest

from tests import kmeans_seed_ref as ref

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

TOP = (1 << 64) - 1
PAIRS = [(8, 2), (8, 3), (40, 4), (40, 6)]
_SEG = {}


def _u64(rng, shape):
    return (rng.randint(0, 1 << 32, size=shape).astype(np.uint64) << np.uint64(32)) | rng.randint(0, 1 << 32, size=shape).astype(np.uint64)


def _weights(kind, P, rng):
    if kind is None:
        return None
    if kind == 'mask':
        return (rng.rand(P) < 0.6).astype(np.float32)
    if kind == 'real':
        w = (2.5 * rng.rand(P)).astype(np.float32)
        w[rng.rand(P) < 0.1] = 0
        return w
    if kind == 'zero_chunk':                                       # the first whole chunk of the segment weighs nothing
        w = rng.rand(P).astype(np.float32)
        w[:8192] = 0
        return w
    assert kind == 'zero'
    return np.zeros(P, np.float32)


def _segment(P, E, C, tries, kind=None, shape='blobs'):
    """(points [P, E], draws [tries, C], weights or None, restated seeds [tries, C]) of a segment; made once per key."""
    key = (P, E, C, tries, kind, shape)
    if key not in _SEG:
        rng = np.random.RandomState(1000 + P % 997 + 31 * E + 7 * C + tries)
        if shape == 'same':
            x = np.tile(rng.randn(1, E), (P, 1))
        else:                                                      # loose blobs: distances from about 1e-2 to 2
            x = rng.randn(6, E)[rng.randint(0, 6, size=P)] + 0.2 * rng.randn(P, E)
        x = (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)
        if shape == 'same':
            x[:] = x[0]
        draws = _u64(rng, (tries, C))
        if shape == 'ends':                                        # columns and rows of all-zeros and all-ones draws
            draws[:, 0], draws[:, C - 1] = 0, TOP
            draws[0], draws[tries - 1] = 0, TOP
        if shape == 'nan':
            x[P - 300, E // 2] = np.nan
        w = _weights(kind, P, rng)
        _SEG[key] = (x, draws, w, ref.seed_segment(x, draws, w))
    return _SEG[key]


def _pack(segs):
    x = np.concatenate([s[0] for s in segs])
    d = np.concatenate([s[1] for s in segs])
    w = None if segs[0][2] is None and all(s[2] is None for s in segs) else \
        np.concatenate([np.ones(len(s[0]), np.float32) if s[2] is None else s[2] for s in segs])
    return x, d, w, np.concatenate([s[3] for s in segs])


def _up(a, dt=np.float32):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).cuda()


def _run(segs, C, tries, dev=_up, alone=True):
    """seed_plusplus on the segments together: equal to the restatement, and to the call on every segment alone."""
    from ams_hip import kmeans_seed as ks
    x, d, w, want = _pack(segs)
    sizes = [len(s[0]) for s in segs]
    got = ks.seed_plusplus(dev(x), sizes, C, tries, d, w=None if w is None else dev(w))
    assert got.dtype == torch.int32 and tuple(got.shape) == (len(segs) * tries, C) and got.is_cuda
    got = got.cpu().numpy()
    for r, s in enumerate(segs):
        rows = slice(r * tries, (r + 1) * tries)
        assert np.array_equal(got[rows], s[3]), (r, sizes[r], got[rows].tolist(), s[3].tolist())
        if alone:
            ws = None if w is None else (np.ones(sizes[r], np.float32) if s[2] is None else s[2])
            one = ks.seed_plusplus(dev(s[0]), [sizes[r]], C, tries, s[1], w=None if ws is None else dev(ws))
            assert np.array_equal(one.cpu().numpy(), got[rows]), (r, sizes[r])
    assert np.array_equal(got, want)
    return got


@pytest.mark.parametrize('tries', [1, 3, 10])
@pytest.mark.parametrize('E,C', PAIRS)
def test_base_sizes_forward_and_reversed(E, C, tries):
    segs = [_segment(P, E, C, tries) for P in (C, 255, 8192, 8193, 20000)]
    got = _run(segs, C, tries)
    assert all(len(set(row)) == C for row in got.tolist())         # distinct, and in range by the equality above
    _run(segs[::-1], C, tries, alone=False)


@pytest.mark.parametrize('E,C,tries', [(8, 3, 16), (8, 3, 17), (40, 6, 33)])
def test_more_tries_than_one_read_of_the_points_holds(E, C, tries):
    """The weighing holds the seed rows of 16 tries at a time: 16 is one read of the points, 17 and 33 are a full batch and a rest."""
    _run([_segment(P, E, C, tries) for P in (C, 8193, 700)], C, tries, alone=False)


@pytest.mark.parametrize('E,C,tries', [(8, 3, 3), (40, 4, 3), (40, 6, 10)])
def test_weights(E, C, tries):
    """A 0/1 mask, real weights, a segment whose first whole chunk is all zero (the pick passes it over) and a segment of all-zero
    weights (the fallback at every step) in one call; a point of weight 0 is drawn only by the fallback."""
    segs = [_segment(300, E, C, tries, 'mask'), _segment(8192 + 500, E, C, tries, 'zero_chunk'), _segment(700, E, C, tries, 'zero'),
            _segment(9000, E, C, tries, 'real'), _segment(8193, E, C, tries, None)]
    got = _run(segs, C, tries)
    assert bool((segs[0][2][got[:tries]] > 0).all()) and bool((segs[3][2][got[3 * tries:4 * tries]] > 0).all())
    assert int(got[tries:2 * tries].min()) >= 8192
    assert got[2 * tries:3 * tries].tolist() == [list(range(C))] * tries


@pytest.mark.parametrize('E,C,tries', [(8, 2, 3), (40, 6, 4)])
def test_draws_of_all_zeros_and_all_ones(E, C, tries):
    segs = [_segment(P, E, C, tries, kind, 'ends') for P, kind in ((C, None), (255, None), (8193, None), (20000, None))]
    _run(segs, C, tries)
    segs = [_segment(P, E, C, tries, 'real', 'ends') for P in (300, 8192, 8193 + 8192)]
    _run(segs, C, tries)


@pytest.mark.parametrize('E,C', [(8, 3), (40, 6)])
def test_identical_points_and_a_planted_nan(E, C):
    tries = 3
    same, nan = _segment(500, E, C, tries, None, 'same'), _segment(9000, E, C, tries, None, 'nan')
    got = _run([same, _segment(8193, E, C, tries), nan], C, tries)
    # identical points: step 0 samples, every later step is the fallback -- the smallest indices that are left, in order
    for row in got[:tries].tolist():
        assert row[1:] == [i for i in range(C) if i != row[0]][:C - 1]
    assert not bool((got[2 * tries:] == 9000 - 300).any())          # the NaN point is never chosen


def test_launches_do_not_depend_on_the_number_of_segments():
    from ams_hip import kmeans_seed as ks
    E, C, tries = 8, 3, 3
    segs = [_segment(P, E, C, tries) for P in (C, 255, 8192, 8193, 20000)]
    n0 = ks.LAUNCHES
    _run(segs[3:4], C, tries, alone=False)
    n1 = ks.LAUNCHES
    _run(segs, C, tries, alone=False)
    assert n1 - n0 == ks.LAUNCHES - n1 == 2 * C
    # step by step: the same seeds, the same launches
    x, d, w, want = _pack(segs)
    seen = []
    got = ks.seed_plusplus(_up(x), [len(s[0]) for s in segs], C, tries, d, steps=seen.append)
    assert seen == list(range(C)) and np.array_equal(got.cpu().numpy(), want)


@pytest.mark.parametrize('E,C', [(8, 3), (40, 4)])
def test_the_ragged_kmeans_takes_the_seeds(E, C):
    """kmeans_ragged from the device's seeds is kmeans_ragged from the restatement's: centroids, labels and chosen tries to the bit."""
    from ams_hip import kmeans_ragged as kr, kmeans_seed as ks
    tries = 3
    segs = [_segment(P, E, C, tries, 'mask') for P in (255, 8193, 3000)]
    x, d, w, want = _pack(segs)
    sizes = [len(s[0]) for s in segs]
    xd, wd = _up(x), _up(w)
    seeds = ks.seed_plusplus(xd, sizes, C, tries, d, w=wd).cpu().numpy()
    a = kr.kmeans_ragged(xd, sizes, seeds, C, tries, 3, w=wd, normalize_input=False)
    b = kr.kmeans_ragged(xd, sizes, want, C, tries, 3, w=wd, normalize_input=False)
    for u, v in zip(a, b):
        assert torch.equal(u.view(torch.int32) if u.dtype == torch.float32 else u, v.view(torch.int32) if v.dtype == torch.float32 else v)
    assert bool(torch.isfinite(a[0]).all())


@pytest.mark.parametrize('base', [0, 4, 12])
@pytest.mark.parametrize('E,C,tries', [(8, 3, 3), (40, 6, 10)])
def test_inside_fenced_buffers(E, C, tries, base):
    """The points and the weights between red zones at odd bases; the workspace and the seeds buffer are fenced allocations of the wrapper,
    so a seed word the kernels do not store is 2146992120 in the comparison, and a store outside any buffer fails fence.check()."""
    from tests.fenced import Fence
    segs = [_segment(P, E, C, tries) for P in (C, 255, 8192, 8193, 20000)]
    mixed = [_segment(300, E, C, tries, 'mask'), _segment(8192 + 500, E, C, tries, 'zero_chunk'), _segment(700, E, C, tries, 'zero')]
    with Fence() as fence:
        dev = lambda a, dt=np.float32: fence.dev(a, dt, base=base)                                 # noqa: E731
        _run(segs, C, tries, dev=dev, alone=False)
        fence.check()
        _run(mixed, C, tries, dev=dev, alone=False)
        fence.check()
