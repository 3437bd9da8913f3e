"""CPU: the boundary of the ragged soft k-means -- include/ams_kmeans_ragged_soft.h against the exports of libams_kmeans_ragged_soft.so
(the other libraries without its symbols), the library's argument checks, which return before anything is launched, the workspace formula,
the wrapper's refusals, the refusals of clustering='recording_soft' (all raised before any device work), both command-line parsers, and
the float64 reference of the GPU tests against oracle/kmeans.py."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

torch = pytest.importorskip('torch')

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {'ams_kmrs_abi_version', 'ams_kmrs_workspace_bytes', 'ams_kmrs_init', 'ams_kmrs_iterate', 'ams_kmrs_inertia', 'ams_kmrs_select',
         'ams_kmrs_masks'}
INVALID, TOO_SMALL = -1, -2


def _built(path):
    if not os.path.exists(path):
        import __graft_entry__
        __graft_entry__.build()
    return path


def _exports(path):
    out = subprocess.run(['nm', '-D', '--defined-only', _built(path)], capture_output=True, text=True, check=True).stdout
    return set(ln.split()[-1] for ln in out.splitlines() if ln.split() and ln.split()[-1].startswith('ams_'))


def test_header_and_exports():
    from ams_hip import _lib, kmeans_ragged as kr, kmeans_ragged_soft as krs
    src = re.sub(r'/\*.*?\*/', ' ', open(os.path.join(ROOT, 'include', 'ams_kmeans_ragged_soft.h')).read(), flags=re.S)
    assert set(re.findall(r'\b(ams_\w+)\s*\(', src)) == NAMES
    assert set(_lib.parse_header(krs.HEADER_PATH)) == NAMES
    assert _exports(krs.LIB_PATH) == NAMES
    assert ctypes.CDLL(krs.LIB_PATH).ams_kmrs_abi_version() == 1 == krs.ABI_VERSION
    # the libraries beside it keep their exports: none gained a soft ragged symbol
    for other in (_lib.LIB_PATH, kr.LIB_PATH):
        assert not any(n.startswith('ams_kmrs_') for n in _exports(other)), other
    assert _exports(kr.LIB_PATH) == set(_lib.parse_header(kr.HEADER_PATH)) and kr.ABI_VERSION == 1
    # the layout is the hard ragged k-means': one Segments class, one seed check
    assert krs.Segments is kr.Segments and krs.check_seeds is kr.check_seeds and krs.PAIRS == kr.PAIRS


def test_library_argument_checks_return_before_any_launch():
    from ams_hip import _lib, kmeans_ragged_soft as krs
    lib = ctypes.CDLL(_built(krs.LIB_PATH))
    for name, (ret, argtypes) in _lib.parse_header(krs.HEADER_PATH).items():
        getattr(lib, name).restype, getattr(lib, name).argtypes = ret, argtypes
    buf = (ctypes.c_char * 4096)()
    base = ctypes.addressof(buf)
    p = ctypes.c_void_p(base + (-base) % 16)                       # a 16-byte aligned host pointer: never dereferenced by a call that is refused
    q = ctypes.c_void_p(p.value + 64)                              # ... and a second one
    odd = ctypes.c_void_p(p.value + 4)
    # the workspace: 4 tries Gtot C (E + 1); zero outside the domain
    ws = lib.ams_kmrs_workspace_bytes
    assert ws(2, 10, 5, 40, 2) == 4 * 10 * 5 * 2 * 41 and ws(1, 1, 1, 8, 6) == 4 * 6 * 9 and ws(3, 5, 7, 40, 6) == 4 * 5 * 7 * 6 * 41
    for R, tries, G, E, C in ((0, 1, 1, 40, 2), (1, 0, 1, 40, 2), (2, 1, 1, 40, 2), (1, 1, 1, 20, 2), (1, 1, 1, 40, 1), (1, 1, 1, 40, 7),
                              (1, 1, 1, 32, 2), (1, 1, 0, 40, 2), (1, 1 << 20, 1 << 20, 40, 2)):
        assert ws(R, tries, G, E, C) == 0, (R, tries, G, E, C)
    big = 1 << 40

    def iterate(xn=p, w=None, tab=p, p_off=p, g_off=p, cin=p, cout=q, R=2, tries=5, G=3, E=40, C=2, beta=5.0, wsp=p, nb=big, tk=p):
        return lib.ams_kmrs_iterate(xn, w, tab, p_off, g_off, cin, cout, R, tries, G, E, C, beta, wsp, nb, tk, None)

    def inertia(xn=p, w=None, tab=p, p_off=p, g_off=p, cent=p, out=q, R=2, tries=5, G=3, E=40, C=2, beta=5.0, wsp=p, nb=big, tk=p):
        return lib.ams_kmrs_inertia(xn, w, tab, p_off, g_off, cent, out, R, tries, G, E, C, beta, wsp, nb, tk, None)

    def masks(xn=p, w=None, tab=p, p_off=p, g_off=p, cent=p, beta=5.0, out=q, R=2, G=3, E=40, C=2):
        return lib.ams_kmrs_masks(xn, w, tab, p_off, g_off, cent, beta, out, R, G, E, C, None)
    common = (dict(xn=None), dict(tab=None), dict(p_off=None), dict(g_off=None), dict(R=0), dict(G=1), dict(G=0), dict(E=20), dict(E=40, C=7),
              dict(E=8, C=1), dict(E=64), dict(beta=-1.0), dict(beta=-1e-30), dict(beta=float('nan')), dict(beta=float('inf')), dict(xn=odd))
    for fn in (iterate, inertia):
        for bad in common + (dict(wsp=None), dict(tk=None), dict(tries=0)):
            assert fn(**bad) == INVALID, bad
        assert fn(nb=ws(2, 5, 3, 40, 2) - 1) == TOO_SMALL and fn(nb=0, E=8, C=3, tries=2) == TOO_SMALL
    for bad in common + (dict(cent=None), dict(out=None)):
        assert masks(**bad) == INVALID, bad
    assert iterate(cin=None) == INVALID and iterate(cout=None) == INVALID and iterate(cout=p) == INVALID          # in place is refused
    assert inertia(cent=None) == INVALID and inertia(out=None) == INVALID
    assert lib.ams_kmrs_init(None, p, p, p, 1, 1, 40, 2, None) == INVALID and lib.ams_kmrs_init(p, p, p, p, 0, 1, 40, 2, None) == INVALID
    assert lib.ams_kmrs_init(p, p, p, p, 1, 0, 40, 2, None) == INVALID and lib.ams_kmrs_init(p, p, p, p, 1, 1, 20, 2, None) == INVALID
    assert lib.ams_kmrs_select(p, p, None, p, 1, 1, 40, 2, None) == INVALID and lib.ams_kmrs_select(p, p, p, p, 0, 1, 40, 2, None) == INVALID
    assert lib.ams_kmrs_select(p, p, p, p, 1, 1, 40, 9, None) == INVALID


def test_the_wrapper_refuses_before_it_touches_the_device():
    """Every refusal is a ValueError raised on host tensors: nothing was uploaded (a device op on them would be an AmsError)."""
    from ams_hip import kmeans_ragged_soft as krs
    seg = krs.segments([30, 9, 50])
    good = np.array([[0, 29], [3, 4], [0, 8], [8, 1], [49, 0], [7, 6]])
    x8 = torch.zeros(89, 8)
    run = lambda x=x8, s=seg, idx=good, C=2, tries=2, it=1, beta=5.0, **k: krs.kmeans_ragged_soft(x, s, idx, C, tries, it, beta, **k)     # noqa: E731
    with pytest.raises(ValueError, match='embedding_size'):
        run(x=torch.zeros(89, 20))
    with pytest.raises(ValueError, match='embedding_size'):
        run(C=7, idx=np.zeros((6, 7), np.int64))
    for beta in (-1.0, float('nan'), float('inf'), None, 'x'):
        with pytest.raises(ValueError, match='beta'):
            run(beta=beta)
    bad = good.copy()
    bad[2] = [0, 9]
    with pytest.raises(ValueError, match='recording 1, try 0.*outside'):
        run(idx=bad)
    bad = good.copy()
    bad[5] = [6, 6]
    with pytest.raises(ValueError, match='recording 2, try 1.*not distinct'):
        run(idx=bad)
    with pytest.raises(ValueError, match='shape'):
        run(idx=good[:5])
    with pytest.raises(ValueError, match=r'weights are a \[Ptot\] = \[89\]'):
        run(w=torch.zeros(88))
    with pytest.raises(ValueError, match=r'weights are a \[Ptot\]'):
        run(w=torch.zeros(89, 1))
    with pytest.raises(ValueError, match='88 points for segments of 89'):
        run(x=torch.zeros(88, 8))
    with pytest.raises(ValueError, match='tries >= 1'):
        run(tries=0)
    with pytest.raises(ValueError, match='Ptot, E'):
        run(x=torch.zeros(89))
    # the tries-only call and the masks launch alone check the same way
    with pytest.raises(ValueError, match='beta'):
        krs.kmeans_ragged_soft_tries(x8, seg, good, 2, 2, 1, -0.5)
    with pytest.raises(ValueError, match='centroids are a'):
        krs.masks_ragged(x8, seg, torch.zeros(2, 2, 8), 5.0)
    with pytest.raises(ValueError, match='beta'):
        krs.masks_ragged(x8, seg, torch.zeros(3, 2, 8), -1.0)
    with pytest.raises(ValueError, match='embedding_size'):
        krs.masks_ragged(torch.zeros(89, 20), seg, torch.zeros(3, 2, 20), 5.0)
    with pytest.raises(ValueError, match='weights'):
        krs.masks_ragged(x8, seg, torch.zeros(3, 2, 8), 5.0, w=torch.zeros(3))
    with pytest.raises(ValueError, match='`out`'):
        krs.masks_ragged(x8, seg, torch.zeros(3, 2, 8), 5.0, out=torch.zeros(89, 3))
    with pytest.raises(ValueError, match='`out`'):
        krs.masks_ragged(x8, seg, torch.zeros(3, 2, 8), 5.0, out=torch.zeros(89, 2, dtype=torch.float64))


class _KM(object):
    def __init__(self, beta):
        self.beta, self.nb_tries, self.nb_clusters = beta, 3, 2


def _stub(beta=5.0, kmeans=True):
    from models.network import Network

    class Stub(Network):
        def __init__(self):
            self.output, self.args, self.S = object(), {'chunk_size': 2048, 'batch_size': 2}, 2
            if kmeans:
                self.kmeans, self.embeddings, self.masks = _KM(beta), object(), object()
    return Stub()


def test_the_refusals_of_recording_soft_come_before_any_device_work():
    x = np.zeros(5000, np.float32)
    seeds = np.array([[0, 1], [2, 3], [4, 5]])
    for call in (lambda m, **k: m.separate_recording(x, **k), lambda m, **k: m.separate_recordings([x], **k)):
        with pytest.raises(ValueError, match='beta_kmeans'):
            call(_stub(beta=None), clustering='recording_soft')                 # a hard model: the message names what it lacks
        with pytest.raises(ValueError, match="needs clustering='recording'"):
            call(_stub(), clustering='recording_soft', speakers='auto')         # counting stays with the hard mode
        with pytest.raises(ValueError, match='k-means separator'):
            call(_stub(kmeans=False), clustering='recording_soft')
        for bad, word in (([seeds, seeds], 'one .* per recording'), (seeds, 'per recording'), ([seeds[:2]], r'\[3, 2\]'),
                          ([seeds.astype(np.float32)], 'integers'), ([np.zeros((3, 3), np.int64)], r'\[3, 2\]')):
            with pytest.raises(ValueError, match=word):
                call(_stub(), clustering='recording_soft', kmeans_init_indices=bad)
        # what was refused before still is, in the words the earlier tests pin; the soft refusal now names the new mode
        with pytest.raises(ValueError, match="hard assignment only.*'recording_soft'"):
            call(_stub(), clustering='recording')
        with pytest.raises(ValueError, match="'chunk' or 'recording'"):
            call(_stub(), clustering='soft')


def test_command_lines_take_the_flag():
    from experiments.evaluation import separate, separate_many
    one = ['--model_folder', 'm', '--sortofmodel', 'front_DPCL', '--input', 'a.wav', '--output_prefix', 'o']
    many = ['--model_folder', 'm', '--sortofmodel', 'front_DPCL', '--inputs', 'a.wav', '--output_dir', 'o']
    for cli, base in ((separate, one), (separate_many, many)):
        assert cli.build_parser().get_args(base).clustering == 'chunk'
        assert cli.build_parser().get_args(base + ['--clustering', 'recording_soft']).clustering == 'recording_soft'
        assert cli.build_parser().get_args(base + ['--clustering', 'recording']).clustering == 'recording'
        with pytest.raises(SystemExit):
            cli.build_parser().get_args(base + ['--clustering', 'both'])
    # --speakers stays with --clustering recording
    args = separate.build_parser().get_args(one + ['--clustering', 'recording_soft', '--speakers', 'auto'])
    with pytest.raises(SystemExit):
        separate.speakers_arg(args)


@pytest.mark.parametrize('dtype', [np.float64, np.float32])
@pytest.mark.parametrize('E,C,beta,kind', [(8, 3, 3.0, None), (8, 3, 3.0, 'real'), (40, 2, 5.0, 'mask'), (40, 6, 10.0, None)])
def test_the_reference_is_the_oracle_on_a_batch_of_one(E, C, beta, kind, dtype):
    """The per-try restatement and oracle/kmeans.py::kmeans run the same functions in the same order: equal to the bit, in either dtype,
    with assign_at_end both ways."""
    from oracle import kmeans as okm
    from tests import kmeans_soft_ragged_ref as ref
    for P in (37, 197):
        X, idx, _ = ref.segment(P, E, C)
        w = ref.weights(P, E, C, kind)
        X = X.astype(np.float32).astype(dtype)
        w = None if w is None else w.astype(np.float32).astype(dtype)
        r = ref.soft_reference(X, idx[:ref.TRIES], C, ref.TRIES, ref.ITERS, beta, w, dtype)
        same = ref.reference(P, E, C, beta, kind, dtype)
        assert np.array_equal(same.cents, r.cents) and np.array_equal(same.inertia, r.inertia)
        assert r.cents.dtype == dtype and r.inertia.shape == (ref.TRIES,) and np.isfinite(r.cents).all()
        for end in (True, False):
            cent, lab, best = okm.kmeans(X[None], idx[:ref.TRIES], C, ref.TRIES, ref.ITERS, beta=beta, notsilent=None if w is None else w[None],
                                         assign_at_end=end)
            assert best[0] == r.best and np.array_equal(cent[0], r.cents[r.best]) and np.array_equal(lab[0], r.masks(r.best, end))
            assert np.allclose(lab[0].sum(axis=1), 1.0)
