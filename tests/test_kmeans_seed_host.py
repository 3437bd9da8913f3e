"""CPU: the k-means++ (D^2) seeding of include/ams_kmeans_seed.h -- the numpy restatement (tests/kmeans_seed_ref.py) against
hand-computed cases and one planted statistical property, the header against the exports of libams_kmeans_seed.so, the library's argument
checks, which return before anything is launched, the wrapper's refusals, the refusals of recording_seeding / kmeans_seed_draws (all raised
before any device work), the pinned default draw stream of the model's KMeans, and both command-line parsers."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from tests import kmeans_seed_ref as ref

torch = pytest.importorskip('torch')

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {'ams_kms_abi_version', 'ams_kms_workspace_bytes', 'ams_kms_step', 'ams_kms_seed'}
INVALID, TOO_SMALL = -1, -2
ONE = 1 << 20                   # quant(1.0)
TOP = (1 << 64) - 1


def _line(a, E=8):
    """Points on a line: coordinate 0 is a, the others 0, so that d(i, s) = (a_i - a_s)^2 exactly for small integers."""
    x = np.zeros((len(a), E), np.float32)
    x[:, 0] = a
    return x


def _u_for(target, total):
    """The smallest draw whose target floor(u total / 2^64) is `target`."""
    u = -(-(target << 64) // total)
    assert (u * total) >> 64 == target and u <= TOP
    return u


def test_quant_is_the_definition():
    v = np.array([1.0, 0.0, -1.0, np.nan, np.inf, 3000.0, 2048.0, 2.0 ** -21, 2.0 ** -20, 1.5 + 2.0 ** -20, -np.inf], np.float32)
    want = [ONE, 0, 0, 0, 1 << 31, 1 << 31, 1 << 31, 0, 1, ONE + (ONE >> 1) + 1, 0]
    assert ref.quant(v).tolist() == want and ref.quant(v).dtype == np.uint64


def test_step_zero_ends_and_boundaries():
    x = _line([0, 1, 2, 3, 4])
    q = ref.weights(x, [])
    assert q.tolist() == [ONE] * 5
    assert ref.pick(q, 0, []) == 0 and ref.pick(q, TOP, []) == 4
    # a target exactly on the boundary behind point 0 is point 1's; one below is still point 0's
    assert ref.pick(q, _u_for(ONE, 5 * ONE), []) == 1 and ref.pick(q, _u_for(ONE, 5 * ONE) - 1, []) == 0
    # with weights: the ends are the first and the last point of positive weight, the boundary goes past a point of weight 0
    w = np.array([0, 1, 0, 2, 0], np.float32)
    q = ref.weights(x, [], w)
    assert q.tolist() == [0, ONE, 0, 2 * ONE, 0]
    assert ref.pick(q, 0, []) == 1 and ref.pick(q, TOP, []) == 3
    assert ref.pick(q, _u_for(ONE, 3 * ONE), []) == 3 and ref.pick(q, _u_for(ONE, 3 * ONE) - 1, []) == 1


def test_later_steps_by_hand():
    x = _line([0, 1, 1, 3, 0])
    q = ref.weights(x, [0])
    assert q.tolist() == [0, ONE, ONE, 9 * ONE, 0]                 # the seed and its duplicate have q = 0
    assert ref.pick(q, 0, [0]) == 1 and ref.pick(q, TOP, [0]) == 3
    assert ref.pick(q, _u_for(ONE, 11 * ONE), [0]) == 2 and ref.pick(q, _u_for(2 * ONE, 11 * ONE), [0]) == 3
    assert ref.pick(q, _u_for(2 * ONE, 11 * ONE) - 1, [0]) == 2
    # the minimum over the seeds, taken on the integers
    assert ref.weights(x, [0, 3]).tolist() == [0, ONE, ONE, 0, 0]
    # whole tries: u = 0 walks through the first points with q > 0, u = 2^64 - 1 through the last ones
    assert ref.seed_try(x, [0, 0, 0]) == [0, 1, 3] and ref.seed_try(x, [TOP, TOP, TOP]) == [4, 3, 2]
    # the weight is the weight of point i, not of the seed
    w = np.array([1, 4, 0, 1, 1], np.float32)
    assert ref.weights(x, [0], w).tolist() == [0, 4 * ONE, 0, 9 * ONE, 0]
    # distances above 2048 are capped
    far = _line([0, 100])
    assert ref.weights(far, [0]).tolist() == [0, 1 << 31]


def test_a_seed_is_never_drawn_twice_and_weightless_points_are_never_drawn():
    rng = np.random.RandomState(5)
    x = rng.randn(40, 8).astype(np.float32)
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    x[7] = x[3]                                                    # an exact duplicate
    draws = rng.randint(0, 1 << 63, size=(50, 6)).astype(np.uint64) * np.uint64(2) + rng.randint(0, 2, size=(50, 6)).astype(np.uint64)
    draws[0], draws[1] = 0, TOP
    s = ref.seed_segment(x, draws)
    assert s.dtype == np.int32 and s.shape == (50, 6) and s.min() >= 0 and s.max() < 40
    assert all(len(set(row)) == 6 for row in s.tolist())
    assert not any(3 in row and 7 in row for row in s.tolist())    # ... nor a seed's exact duplicate
    w = (rng.rand(40) < 0.5).astype(np.float32)
    w[:3], w[-3:] = 0, 0
    sw = ref.seed_segment(x, draws, w)
    assert all(len(set(row)) == 6 for row in sw.tolist()) and bool((w[sw] > 0).all())
    # real weights
    wr = rng.rand(40).astype(np.float32)
    wr[10:15] = 0
    sr = ref.seed_segment(x, draws, wr)
    assert all(len(set(row)) == 6 for row in sr.tolist()) and bool((wr[sr] > 0).all())


def test_the_fallback_takes_the_smallest_unused_index():
    same = np.tile(np.arange(8, dtype=np.float32) / 8, (6, 1))
    draws = np.array([[0, 0, 0, 0], [TOP, TOP, TOP, TOP], [TOP // 2, 5, TOP, 0]], np.uint64)
    # all points identical: step 0 samples, every later step has total == 0
    assert ref.seed_segment(same, draws).tolist() == [[0, 1, 2, 3], [5, 0, 1, 2], [2, 0, 1, 3]]
    # all weights zero: every step has total == 0
    x = np.random.RandomState(2).randn(6, 8).astype(np.float32)
    assert ref.seed_segment(x, draws, np.zeros(6, np.float32)).tolist() == [[0, 1, 2, 3]] * 3
    # weights run out: two points of positive weight, then the smallest indices that are left
    w = np.array([0, 0, 1, 0, 1, 0], np.float32)
    assert ref.seed_segment(x, draws[:2], w).tolist() == [[2, 4, 0, 1], [4, 2, 0, 1]]
    assert ref.pick(np.zeros(5, np.uint64), 12345, [1, 0, 3]) == 2


def test_a_nan_coordinate_gives_q_zero():
    x = _line([0, 1, 2, 3])
    x[2, 5] = np.nan
    assert ref.weights(x, [0]).tolist() == [0, ONE, 0, 9 * ONE]
    assert ref.weights(x, [0, 1]).tolist() == [0, 0, 0, 4 * ONE]
    assert ref.weights(x, []).tolist() == [ONE] * 4                # step 0 weighs by w alone
    for u in (0, TOP // 3, TOP):
        assert ref.pick(ref.weights(x, [0]), u, [0]) != 2
    # a NaN seed leaves nothing to sample from: the fallback
    assert ref.weights(x, [2]).tolist() == [0] * 4 and ref.seed_try(x, [_u_for(2 * ONE, 4 * ONE), 7, 7]) == [2, 0, 1]


def test_the_first_columns_of_a_seeding_are_the_seeding_of_fewer_clusters():
    rng = np.random.RandomState(9)
    x = rng.randn(300, 8).astype(np.float32)
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    w = rng.rand(300).astype(np.float32)
    draws = rng.randint(0, 1 << 62, size=(5, 6)).astype(np.uint64) * np.uint64(4)
    for ww in (None, w):
        six = ref.seed_segment(x, draws, ww)
        for C in range(1, 6):
            assert np.array_equal(ref.seed_segment(x, np.ascontiguousarray(draws[:, :C]), ww), six[:, :C])


def test_planted_blobs_every_try_takes_one_seed_per_blob():
    """Four tight blobs of 50 points around orthogonal unit vectors in E = 8, spread 0.005 per coordinate, 64 tries.  Inside a blob
    d ~ 2 x 8 x 0.005^2 = 4e-4 against 2 between blobs, so a step falls into a blob that has a seed with probability below
    150 x 4e-4 / (50 x 2) = 6e-4, 0.12 over the 192 later steps; the fixed generator seed makes it a plain assertion.  Uniform seeds hit
    four different blobs with probability 4! 50^4 / (200 199 198 197) = 0.097 per try."""
    rng = np.random.RandomState(1234)
    blob = np.arange(200) % 4
    x = np.eye(8, dtype=np.float32)[blob] + (0.005 * rng.randn(200, 8)).astype(np.float32)
    x = (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)
    draws = rng.randint(0, 1 << 32, size=(64, 4)).astype(np.uint64) << np.uint64(32) | rng.randint(0, 1 << 32, size=(64, 4)).astype(np.uint64)
    s = ref.seed_segment(x, draws)
    assert all(sorted(blob[row].tolist()) == [0, 1, 2, 3] for row in s)
    uniform = np.stack([rng.choice(200, 4, replace=False) for _ in range(64)])
    spread = sum(sorted(blob[row].tolist()) == [0, 1, 2, 3] for row in uniform)
    print('uniform seeds: %d of 64 tries take one seed per blob' % spread)
    assert spread < 32


# ---- the library and the wrapper
def _built(path):
    if not os.path.exists(path):
        import __graft_entry__
        __graft_entry__.build()
    return path


def _exports(path):
    out = subprocess.run(['nm', '-D', '--defined-only', _built(path)], capture_output=True, text=True, check=True).stdout
    return set(ln.split()[-1] for ln in out.splitlines() if ln.split() and ln.split()[-1].startswith('ams_'))


def test_header_and_exports():
    from ams_hip import _lib, kmeans_ragged as kr, kmeans_ragged_soft as krs, kmeans_seed as ks, spk_count as sc
    src = re.sub(r'/\*.*?\*/', ' ', open(os.path.join(ROOT, 'include', 'ams_kmeans_seed.h')).read(), flags=re.S)
    assert set(re.findall(r'\b(ams_\w+)\s*\(', src)) == NAMES
    assert set(_lib.parse_header(ks.HEADER_PATH)) == NAMES
    assert _exports(ks.LIB_PATH) == NAMES
    assert ctypes.CDLL(ks.LIB_PATH).ams_kms_abi_version() == 1 == ks.ABI_VERSION
    # the libraries beside it keep their exports and versions
    assert not any(n.startswith('ams_kms_') for n in _exports(_lib.LIB_PATH))
    for other in (kr, krs, sc):
        assert _exports(other.LIB_PATH) == set(_lib.parse_header(other.HEADER_PATH)), other
    assert _lib.ABI_VERSION == 10 and kr.ABI_VERSION == krs.ABI_VERSION == sc.ABI_VERSION == 1
    # the domain: the pairs of the ragged k-means and C = 1
    assert ks.PAIRS == kr.PAIRS | {(40, 1), (8, 1)}


def test_library_argument_checks_return_before_any_launch():
    from ams_hip import _lib, kmeans_seed as ks
    lib = ctypes.CDLL(_built(ks.LIB_PATH))
    for name, (ret, argtypes) in _lib.parse_header(ks.HEADER_PATH).items():
        getattr(lib, name).restype, getattr(lib, name).argtypes = ret, argtypes
    buf = (ctypes.c_char * 4096)()
    base = ctypes.addressof(buf)
    p = ctypes.c_void_p(base + (-base) % 16)                       # a host pointer: never dereferenced by a call that is refused
    ws = lib.ams_kms_workspace_bytes
    assert ws(2, 10, 5, 40, 2) == 8 * 5 * 10 and ws(1, 1, 1, 8, 1) == 8 and ws(3, 5, 7, 40, 6) == 8 * 7 * 5
    for R, tries, G, E, C in ((0, 1, 1, 40, 2), (1, 0, 1, 40, 2), (2, 1, 1, 40, 2), (1, 1, 1, 20, 2), (1, 1, 1, 40, 0), (1, 1, 1, 40, 7),
                              (1, 1, 0, 40, 2), (1, 1, 1 << 29, 40, 2)):
        assert ws(R, tries, G, E, C) == 0, (R, tries, G, E, C)
    big = 1 << 40

    def seed(xn=p, w=None, tab=p, p_off=p, g_off=p, draws=p, R=2, tries=5, G=3, E=40, C=2, wsp=p, nb=big, seeds=p):
        return lib.ams_kms_seed(xn, w, tab, p_off, g_off, draws, R, tries, G, E, C, wsp, nb, seeds, None)

    def step(c, xn=p, w=None, tab=p, p_off=p, g_off=p, draws=p, R=2, tries=5, G=3, E=40, C=2, wsp=p, nb=big, seeds=p):
        return lib.ams_kms_step(xn, w, tab, p_off, g_off, draws, R, tries, G, E, C, c, wsp, nb, seeds, None)
    bad_args = (dict(xn=None), dict(tab=None), dict(p_off=None), dict(g_off=None), dict(draws=None), dict(wsp=None), dict(seeds=None),
                dict(R=0), dict(tries=0), dict(G=1), dict(G=0), dict(E=20), dict(E=64), dict(C=0), dict(C=7))
    for bad in bad_args:
        assert seed(**bad) == INVALID, bad
        assert step(0, **bad) == INVALID, bad
    assert step(-1) == INVALID and step(2) == INVALID and step(6, C=6) == INVALID
    assert seed(nb=ws(2, 5, 3, 40, 2) - 1) == TOO_SMALL and step(1, nb=0, E=8, C=3) == TOO_SMALL


def test_the_wrapper_refuses_before_it_touches_the_device():
    """Every refusal is a ValueError raised on host tensors: nothing was uploaded (a device op on them would be an AmsError)."""
    from ams_hip import kmeans_ragged as kr, kmeans_seed as ks
    seg = kr.segments([30, 9, 50])
    x8 = torch.zeros(89, 8)
    good = np.zeros((6, 2), np.uint64)
    run = lambda x=x8, s=seg, C=2, tries=2, d=good, **k: ks.seed_plusplus(x, s, C, tries, d, **k)          # noqa: E731
    with pytest.raises(ValueError, match='embedding_size'):
        run(x=torch.zeros(89, 20))
    with pytest.raises(ValueError, match='embedding_size'):
        run(C=7, d=np.zeros((6, 7), np.uint64))
    with pytest.raises(ValueError, match='embedding_size'):
        ks.check_domain(40, 0)
    ks.check_domain(40, 1), ks.check_domain(8, 6)
    with pytest.raises(ValueError, match='tries >= 1'):
        run(tries=0)
    with pytest.raises(ValueError, match='Ptot, E'):
        run(x=torch.zeros(89))
    with pytest.raises(ValueError, match='88 points for segments of 89'):
        run(x=torch.zeros(88, 8))
    with pytest.raises(ValueError, match=r'weights are a \[Ptot\] = \[89\]'):
        run(w=torch.zeros(88))
    for bad in (good.astype(np.int64), good.astype(np.float64), good[:5], np.zeros((6, 3), np.uint64), np.zeros(12, np.uint64)):
        with pytest.raises(ValueError, match=r'uint64 of shape \[R tries, C\] = \(6, 2\)'):
            run(d=bad)
    with pytest.raises(ValueError, match='HOST uint64'):
        run(d=torch.zeros(6, 2, dtype=torch.int64))
    # a recording with fewer points than seeds is named
    with pytest.raises(ValueError, match='recording 1 has 2 points, fewer than the 3 seeds'):
        ks.seed_plusplus(torch.zeros(82, 8), [30, 2, 50], 3, 2, np.zeros((6, 3), np.uint64))
    # one table for both modules: the Segments of the ragged k-means
    assert kr.segments(seg) is seg


# ---- the public interface
class _KM(object):
    def __init__(self, beta):
        self.beta, self.nb_tries, self.nb_clusters = beta, 3, 2


def _stub(beta=None, kmeans=True):
    from models.network import Network

    class Stub(Network):
        def __init__(self):
            self.output, self.args, self.S = object(), {'chunk_size': 2048, 'batch_size': 2}, 2
            if kmeans:
                self.kmeans, self.embeddings, self.masks = _KM(beta), object(), object()
    return Stub()


def test_the_refusals_of_the_seeding_arguments_come_before_any_device_work():
    x = np.zeros(5000, np.float32)
    draws = np.zeros((3, 2), np.uint64)
    seeds = np.array([[0, 1], [2, 3], [4, 5]])
    for call in (lambda m, **k: m.separate_recording(x, **k), lambda m, **k: m.separate_recordings([x], **k)):
        for mode, beta in (('recording', None), ('recording_soft', 5.0)):
            with pytest.raises(ValueError, match="'model' or 'plusplus'"):
                call(_stub(beta), clustering=mode, recording_seeding='uniform')
            with pytest.raises(ValueError, match='cannot be given'):
                call(_stub(beta), clustering=mode, recording_seeding='plusplus', kmeans_init_indices=[seeds])
            with pytest.raises(ValueError, match="kmeans_seed_draws are the random numbers of recording_seeding='plusplus'"):
                call(_stub(beta), clustering=mode, kmeans_seed_draws=[draws])
            for bad, word in (([draws, draws], 'one uint64 .* per recording'), (draws, 'per recording'),
                              ([draws[:2]], r'kmeans_seed_draws\[0\] \(recording 0\).*\[3, 2\]'),
                              ([draws.astype(np.int64)], r'recording 0.*uint64'), ([np.zeros((3, 3), np.uint64)], r'recording 0.*\[3, 2\]'),
                              ([torch.zeros(3, 2, dtype=torch.int64)], 'recording 0.*a tensor')):
                with pytest.raises(ValueError, match=word):
                    call(_stub(beta), clustering=mode, recording_seeding='plusplus', kmeans_seed_draws=bad)
        with pytest.raises(ValueError, match="needs clustering='recording' or 'recording_soft'"):
            call(_stub(), recording_seeding='plusplus')
        with pytest.raises(ValueError, match="needs clustering='recording' or 'recording_soft'"):
            call(_stub(), clustering='chunk', recording_seeding='plusplus', kmeans_seed_draws=[draws])
        with pytest.raises(ValueError, match="kmeans_seed_draws are"):
            call(_stub(), kmeans_seed_draws=[draws])
        with pytest.raises(ValueError, match='k-means separator'):
            call(_stub(kmeans=False), clustering='recording', recording_seeding='plusplus')
    with pytest.raises(ValueError, match=r'kmeans_seed_draws\[1\] \(recording 1\)'):
        _stub().separate_recordings([x, x], clustering='recording', recording_seeding='plusplus', kmeans_seed_draws=[draws, draws[:1]])


def test_the_default_draws_are_a_pinned_stream_of_the_kmeans_object():
    """The stream of KMeans.seed_draws: splitmix64 of (42, recordings drawn for so far, try, column); it leaves numpy's
    global generator and the counter of the 'keyed' seeds alone, and an object built alike repeats it."""
    from ams_hip.kmeans_host import KMeans
    a, b = KMeans.__new__(KMeans), KMeans.__new__(KMeans)
    a._draws = b._draws = 0
    np.random.seed(7)
    state = np.random.get_state()[1].copy()
    first, second = a.seed_draws(3, 2), a.seed_draws(3, 2)
    assert first.dtype == np.uint64 and first.shape == (3, 2)
    assert first.tolist() == PINNED[0] and second.tolist() == PINNED[1]
    assert np.array_equal(b.seed_draws(3, 2), first) and np.array_equal(b.seed_draws(3, 2), second)
    assert np.array_equal(np.random.get_state()[1], state) and a._draws == 0
    # a wider draw has the narrower one as its first columns and rows
    c = KMeans.__new__(KMeans)
    assert np.array_equal(c.seed_draws(5, 6)[:3, :2], first)


PINNED = [[[3393783785292636687, 11281232758477310350], [10621533199800494636, 11375849681342327694],
           [15386984158666418093, 3056197940496316950]],
          [[13507620257981526559, 16989870959327898320], [15180151584907577179, 7960402628017220864],
           [16130246126598487018, 4638503458917340329]]]


def test_command_lines_take_the_flag():
    from experiments.evaluation import separate, separate_many
    one = ['--model_folder', 'm', '--sortofmodel', 'front_DPCL', '--input', 'a.wav', '--output_prefix', 'o']
    many = ['--model_folder', 'm', '--sortofmodel', 'front_DPCL', '--inputs', 'a.wav', '--output_dir', 'o']
    for cli, base in ((separate, one), (separate_many, many)):
        assert cli.build_parser().get_args(base).recording_seeding == 'model'
        args = cli.build_parser().get_args(base + ['--clustering', 'recording', '--recording_seeding', 'plusplus'])
        assert args.recording_seeding == 'plusplus' and separate.seeding_arg(args) == 'plusplus'
        with pytest.raises(SystemExit):
            cli.build_parser().get_args(base + ['--recording_seeding', 'greedy'])
        args = cli.build_parser().get_args(base + ['--recording_seeding', 'plusplus'])
        with pytest.raises(SystemExit):
            separate.seeding_arg(args)
        assert separate.seeding_arg(cli.build_parser().get_args(base)) == 'model'
