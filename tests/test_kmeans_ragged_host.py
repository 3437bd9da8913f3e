"""CPU: the boundary of the ragged k-means -- include/ams_kmeans_ragged.h against the exports of libams_kmeans_ragged.so (and
libams_hip.so without its symbols, its own exports unchanged), the work table and p_off for the chunk stream of a stitch_batch layout,
the wrapper's seed validation, the refusals of clustering='recording' (all raised before any device work) and the library's argument
checks, which return before anything is launched."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

torch = pytest.importorskip('torch')

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {'ams_kmr_abi_version', 'ams_kmr_chunks', 'ams_kmr_tables', 'ams_kmr_workspace_bytes', 'ams_kmr_init', 'ams_kmr_iterate',
         'ams_kmr_inertia', 'ams_kmr_select', 'ams_kmr_labels'}
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
    from ams_hip import _lib, kmeans_ragged as kr
    src = re.sub(r'/\*.*?\*/', ' ', open(os.path.join(ROOT, 'include', 'ams_kmeans_ragged.h')).read(), flags=re.S)
    assert set(re.findall(r'\b(ams_\w+)\s*\(', src)) == NAMES
    assert set(_lib.parse_header(kr.HEADER_PATH)) == NAMES
    assert _exports(kr.LIB_PATH) == NAMES
    assert ctypes.CDLL(kr.LIB_PATH).ams_kmr_abi_version() == 1 == kr.ABI_VERSION


def test_libams_hip_keeps_its_exports():
    """libams_hip.so exports exactly what include/ams.h declares (version 10), as before the ragged geometry of csrc/kmeans_hard.h existed, and
    none of the other libraries gained a ragged symbol."""
    from ams_hip import _lib, stitch, stitch_batch
    want = set(_lib.parse_header(_lib.HEADER_PATH))
    assert _lib.ABI_VERSION == 10 and 'ams_kmeans_iterate' in want and not any(n.startswith('ams_kmr_') for n in want)
    assert _exports(_lib.LIB_PATH) == want
    for other in (stitch.LIB_PATH, stitch_batch.LIB_PATH):
        assert not any(n.startswith('ams_kmr_') for n in _exports(other)), other
    assert 'kmr' not in open(_lib.HEADER_PATH).read()


def test_segments_of_a_layout():
    """Lengths that give 1, 1, 3 and 4 chunks of 2048 samples, 1024 apart; 4100 points per chunk: 1, 1, 2 and 3 chunks of 8192 points."""
    from ams_hip import kmeans_ragged as kr
    from ams_hip import stitch_batch as sb
    lay = sb.layout([1000, 2048, 3300, 4396], 2048, 1024, 2)
    assert lay.C.tolist() == [1, 1, 3, 4]
    TF = 4100
    seg = kr.segments_of_layout(lay, TF)
    assert (seg.R, seg.Ptot, seg.Pmax, seg.Gtot) == (4, 9 * TF, 4 * TF, 7)
    assert seg.P.tolist() == [TF, TF, 3 * TF, 4 * TF] and seg.p_off.tolist() == (TF * lay.c_off).tolist() == [0, TF, 2 * TF, 5 * TF, 9 * TF]
    assert seg.g_off.tolist() == [0, 1, 2, 4, 7] and seg.p_off.dtype == seg.g_off.dtype == np.int64 and seg.tab.dtype == np.int32
    want = [(r, g, k, 0) for r, G in enumerate([1, 1, 2, 3]) for g in range(G) for k in range(4)]
    assert seg.tab.shape == (28, 4) and [tuple(row) for row in seg.tab.tolist()] == want
    assert [(s.start, s.stop) for s in map(seg.rows, range(4))] == [(0, TF), (TF, 2 * TF), (2 * TF, 5 * TF), (5 * TF, 9 * TF)]
    # chunk borders to the point
    assert kr.segments([8192, 8193, 1]).g_off.tolist() == [0, 1, 3, 4]
    for bad in ([], [0], [5, -1]):
        with pytest.raises(ValueError):
            kr.segments(bad)


def test_seed_validation_names_the_recording():
    from ams_hip import kmeans_ragged as kr
    seg = kr.segments([30, 9, 50])
    good = np.array([[0, 29], [3, 4], [0, 8], [8, 1], [49, 0], [7, 6]])
    assert kr.check_seeds(good, seg, 2, 2).dtype == np.int32
    assert np.array_equal(kr.check_seeds(torch.from_numpy(good), seg, 2, 2), good)
    for row, val, word in ((2, [0, 9], 'recording 1, try 0'), (5, [50, 1], 'recording 2, try 1'), (0, [-1, 3], 'recording 0, try 0')):
        bad = good.copy()
        bad[row] = val
        with pytest.raises(ValueError, match=word + '.*outside'):
            kr.check_seeds(bad, seg, 2, 2)
    bad = good.copy()
    bad[3] = [4, 4]
    with pytest.raises(ValueError, match='recording 1, try 1.*not distinct'):
        kr.check_seeds(bad, seg, 2, 2)
    for shape in ((5, 2), (6, 3), (6,)):
        with pytest.raises(ValueError, match='shape'):
            kr.check_seeds(np.zeros(shape, np.int64), seg, 2, 2)
    with pytest.raises(ValueError, match='integers'):
        kr.check_seeds(good.astype(np.float32), seg, 2, 2)
    # the wrapper refuses a pair without a kernel, and bad seeds, before it touches the device
    with pytest.raises(ValueError, match='embedding_size'):
        kr.kmeans_ragged(torch.zeros(89, 20), seg, good, 2, 2, 1)
    bad = good.copy()
    bad[2] = [0, 9]
    with pytest.raises(ValueError, match='recording 1'):
        kr.kmeans_ragged(torch.zeros(89, 8), seg, bad, 2, 2, 1)


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


def test_the_refusals_of_recording_level_clustering_come_before_any_device_work():
    x = np.zeros(5000, np.float32)
    seeds = np.array([[0, 1], [2, 3], [4, 5]])
    for call in (lambda m, **k: m.separate_recording(x, **k), lambda m, **k: m.separate_recordings([x], **k)):
        with pytest.raises(ValueError, match="'chunk' or 'recording'"):
            call(_stub(), clustering='track')
        with pytest.raises(ValueError, match='hard assignment only'):
            call(_stub(beta=5.0), clustering='recording')
        with pytest.raises(ValueError, match='k-means separator'):
            call(_stub(kmeans=False), clustering='recording')
        for bad, word in (([seeds, seeds], 'one .* per recording'), (seeds, 'per recording'), ([seeds[:2]], r'\[3, 2\]'),
                          ([seeds.astype(np.float32)], 'integers'), ([np.zeros((3, 3), np.int64)], r'\[3, 2\]')):
            with pytest.raises(ValueError, match=word):
                call(_stub(), clustering='recording', kmeans_init_indices=bad)
        with pytest.raises(ValueError, match="clustering='recording'"):
            call(_stub(), kmeans_init_indices=[seeds])                      # per-recording seeds without the mode they belong to


def test_command_lines_take_the_flag():
    from experiments.evaluation import separate, separate_many
    one = ['--model_folder', 'm', '--sortofmodel', 'front_DPCL', '--input', 'a.wav', '--output_prefix', 'o']
    many = ['--model_folder', 'm', '--sortofmodel', 'front_DPCL', '--inputs', 'a.wav', '--output_dir', 'o']
    for cli, base in ((separate, one), (separate_many, many)):
        assert cli.build_parser().get_args(base).clustering == 'chunk'
        assert cli.build_parser().get_args(base + ['--clustering', 'recording']).clustering == 'recording'
        with pytest.raises(SystemExit):
            cli.build_parser().get_args(base + ['--clustering', 'both'])


def test_library_argument_checks_return_before_any_launch():
    from ams_hip import _lib, kmeans_ragged as kr
    lib = ctypes.CDLL(_built(kr.LIB_PATH))
    for name, (ret, argtypes) in _lib.parse_header(kr.HEADER_PATH).items():
        getattr(lib, name).restype, getattr(lib, name).argtypes = ret, argtypes
    buf = (ctypes.c_char * 4096)()
    p = ctypes.cast(buf, ctypes.c_void_p)                          # a host pointer: never dereferenced by a call that is refused
    off = lambda *v: np.asarray(v, np.int64).ctypes.data_as(ctypes.c_void_p)      # noqa: E731
    # the host tables
    assert lib.ams_kmr_chunks(off(0, 8192, 8193 + 8192), 2) == 3
    assert lib.ams_kmr_chunks(off(0, 5, 5), 2) == -1 and lib.ams_kmr_chunks(off(0, 5, 3), 2) == -1           # P_r < 1
    assert lib.ams_kmr_chunks(off(1, 5), 1) == -1 and lib.ams_kmr_chunks(off(0, 5), 0) == -1 and lib.ams_kmr_chunks(None, 1) == -1
    assert lib.ams_kmr_tables(off(0, 5, 5), 2, p, p) == INVALID and lib.ams_kmr_tables(off(0, 5), 1, None, p) == INVALID
    # the workspace: 4 tries 4 Gtot C (E + 1); zero outside the domain
    ws = lib.ams_kmr_workspace_bytes
    assert ws(2, 10, 5, 40, 2) == 4 * 10 * 4 * 5 * 2 * 41 and ws(1, 1, 1, 8, 6) == 4 * 4 * 6 * 9
    for R, tries, G, E, C in ((0, 1, 1, 40, 2), (1, 0, 1, 40, 2), (2, 1, 1, 40, 2), (1, 1, 1, 20, 2), (1, 1, 1, 40, 1), (1, 1, 1, 40, 7),
                              (1, 1, 1, 32, 2), (1, 1, 0, 40, 2), (1, 1 << 20, 1 << 20, 40, 2)):
        assert ws(R, tries, G, E, C) == 0, (R, tries, G, E, C)
    big = 1 << 40

    def iterate(xn=p, w=None, tab=p, p_off=p, g_off=p, cin=p, cout=p, R=2, tries=5, G=3, Pmax=9000, E=40, C=2, wsp=p, nb=big, tk=p):
        return lib.ams_kmr_iterate(xn, w, tab, p_off, g_off, cin, cout, R, tries, G, Pmax, E, C, wsp, nb, tk, None)

    def inertia(xn=p, w=None, tab=p, p_off=p, g_off=p, cent=p, out=p, R=2, tries=5, G=3, Pmax=9000, E=40, C=2, wsp=p, nb=big, tk=p):
        return lib.ams_kmr_inertia(xn, w, tab, p_off, g_off, cent, out, R, tries, G, Pmax, E, C, wsp, nb, tk, None)
    for fn in (iterate, inertia):
        for bad in (dict(xn=None), dict(tab=None), dict(p_off=None), dict(g_off=None), dict(wsp=None), dict(tk=None), dict(R=0), dict(tries=0),
                    dict(G=1), dict(G=0), dict(Pmax=0), dict(E=20), dict(E=40, C=7), dict(E=8, C=1), dict(E=64)):
            assert fn(**bad) == INVALID, bad
        assert fn(nb=ws(2, 5, 3, 40, 2) - 1) == TOO_SMALL and fn(nb=0, E=8, C=3, tries=2) == TOO_SMALL
    assert iterate(cin=None) == INVALID and iterate(cout=None) == INVALID and inertia(cent=None) == INVALID and inertia(out=None) == INVALID
    assert lib.ams_kmr_init(None, p, p, p, 1, 1, 40, 2, None) == INVALID and lib.ams_kmr_init(p, p, p, p, 0, 1, 40, 2, None) == INVALID
    assert lib.ams_kmr_init(p, p, p, p, 1, 0, 40, 2, None) == INVALID and lib.ams_kmr_init(p, p, p, p, 1, 1, 20, 2, None) == INVALID
    assert lib.ams_kmr_select(p, p, None, p, 1, 1, 40, 2, None) == INVALID and lib.ams_kmr_select(p, p, p, p, 0, 1, 40, 2, None) == INVALID
    assert lib.ams_kmr_select(p, p, p, p, 1, 1, 40, 9, None) == INVALID
    assert lib.ams_kmr_labels(p, None, p, p, p, p, None, 1, 1, 40, 2, None) == INVALID
    assert lib.ams_kmr_labels(p, None, p, p, p, p, p, 2, 1, 40, 2, None) == INVALID and lib.ams_kmr_labels(p, None, p, p, p, p, p, 1, 1, 20, 3, None) == INVALID
