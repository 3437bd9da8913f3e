"""CPU: the boundary of the speaker count -- include/ams_spk_count.h against the exports of libams_spk_count.so (and the other libraries
without its symbols, their own exports unchanged), the library's argument checks, which return before anything is launched, the
float64 restatement (tests/speaker_count_ref.py) on the planted family, the refusals of `speakers` on a model stub (all raised before
any device work) and those of both command lines."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from tests import speaker_count_ref as ref

torch = pytest.importorskip('torch')

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {'ams_spkc_abi_version', 'ams_spkc_workspace_bytes', 'ams_spkc_score', 'ams_spkc_choose', 'ams_spkc_labels'}
KMR_NAMES = {'ams_kmr_abi_version', 'ams_kmr_chunks', 'ams_kmr_tables', 'ams_kmr_workspace_bytes', 'ams_kmr_init', 'ams_kmr_iterate',
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
    from ams_hip import _lib, spk_count as sc
    src = re.sub(r'/\*.*?\*/', ' ', open(os.path.join(ROOT, 'include', 'ams_spk_count.h')).read(), flags=re.S)
    assert set(re.findall(r'\b(ams_\w+)\s*\(', src)) == NAMES
    assert set(_lib.parse_header(sc.HEADER_PATH)) == NAMES
    assert _exports(sc.LIB_PATH) == NAMES
    assert ctypes.CDLL(sc.LIB_PATH).ams_spkc_abi_version() == 1 == sc.ABI_VERSION


def test_the_other_libraries_keep_their_exports():
    from ams_hip import _lib, kmeans_ragged as kr, stitch, stitch_batch
    want = set(_lib.parse_header(_lib.HEADER_PATH))
    assert _lib.ABI_VERSION == 10 and not any(n.startswith('ams_spkc_') for n in want)
    assert _exports(_lib.LIB_PATH) == want
    assert _exports(kr.LIB_PATH) == KMR_NAMES == set(_lib.parse_header(kr.HEADER_PATH)) and kr.ABI_VERSION == 1
    for other in (stitch.LIB_PATH, stitch_batch.LIB_PATH, os.path.join(os.path.dirname(kr.LIB_PATH), 'libams_bss_ragged.so')):
        assert not any(n.startswith('ams_spkc_') for n in _exports(other)), other
    for header in (_lib.HEADER_PATH, kr.HEADER_PATH):
        assert 'spkc' not in open(header).read()


def test_library_argument_checks_return_before_any_launch():
    from ams_hip import _lib, spk_count as sc
    lib = ctypes.CDLL(_built(sc.LIB_PATH))
    for name, (ret, argtypes) in _lib.parse_header(sc.HEADER_PATH).items():
        getattr(lib, name).restype, getattr(lib, name).argtypes = ret, argtypes
    buf = (ctypes.c_char * 4096)()
    p = ctypes.cast(buf, ctypes.c_void_p)                          # a host pointer: never dereferenced by a call that is refused
    ms = ctypes.c_double(0.5)
    msp = ctypes.cast(ctypes.pointer(ms), ctypes.c_void_p)
    # the workspace: 8 Gtot (ncand + 1); zero outside the domain
    ws = lib.ams_spkc_workspace_bytes
    assert ws(2, 5, 40, 2, 6) == 8 * 5 * 6 and ws(1, 1, 8, 3, 3) == 8 * 2 and ws(3, 3, 8, 2, 3) == 8 * 3 * 3
    for R, G, E, lo, hi in ((0, 1, 40, 2, 3), (2, 1, 40, 2, 3), (1, 1, 20, 2, 3), (1, 1, 40, 1, 3), (1, 1, 40, 2, 7), (1, 1, 40, 4, 3),
                            (1, 0, 40, 2, 2), (1, 1 << 29, 40, 2, 2), (1, 1, 32, 2, 2)):
        assert ws(R, G, E, lo, hi) == 0, (R, G, E, lo, hi)
    big = 1 << 40

    def score(xn=p, w=None, tab=p, p_off=p, g_off=p, cent=p, inertia=p, R=2, tries=5, G=3, E=40, c_lo=2, c_hi=6, wsp=p, nb=big, sc_=p, tr=p,
              sel=p):
        return lib.ams_spkc_score(xn, w, tab, p_off, g_off, cent, inertia, R, tries, G, E, c_lo, c_hi, wsp, nb, sc_, tr, sel, None)
    for bad in (dict(xn=None), dict(tab=None), dict(p_off=None), dict(g_off=None), dict(cent=None), dict(inertia=None), dict(wsp=None),
                dict(sc_=None), dict(tr=None), dict(sel=None), dict(R=0), dict(tries=0), dict(G=1), dict(G=0), dict(E=20), dict(E=64),
                dict(c_lo=1), dict(c_hi=7), dict(c_lo=4, c_hi=3), dict(G=1 << 29)):
        assert score(**bad) == INVALID, bad
    assert score(nb=ws(2, 3, 40, 2, 6) - 1) == TOO_SMALL and score(nb=0, E=8, c_hi=3) == TOO_SMALL

    def choose(sc_=p, sel=p, R=2, E=40, lo=2, c_lo=2, c_hi=6, m=None, count=p, cand=p, chosen=p):
        return lib.ams_spkc_choose(sc_, sel, R, E, lo, c_lo, c_hi, m, count, cand, chosen, None)
    for bad in (dict(sc_=None), dict(sel=None), dict(count=None), dict(cand=None), dict(chosen=None), dict(R=0), dict(E=20), dict(c_hi=7),
                dict(lo=1), dict(lo=1, c_lo=3, m=msp), dict(lo=3, c_lo=2), dict(lo=0, c_lo=2), dict(c_lo=1, lo=1, m=msp)):
        assert choose(**bad) == INVALID, bad                                       # (lo = 1 without a min_score among them)

    def labels(la=p, cand=p, tab=p, p_off=p, R=2, G=3, Ptot=100, c_lo=2, c_hi=6, out=p):
        return lib.ams_spkc_labels(la, cand, tab, p_off, R, G, Ptot, c_lo, c_hi, out, None)
    for bad in (dict(la=None), dict(cand=None), dict(tab=None), dict(p_off=None), dict(out=None), dict(R=0), dict(G=1), dict(Ptot=1),
                dict(c_lo=1), dict(c_hi=7)):
        assert labels(**bad) == INVALID, bad


@pytest.mark.parametrize('true', [1, 2, 3, 4])
def test_the_restatement_counts_the_planted_family(true):
    """E = 40, 200 points, (lo, hi) = (1, 4), min_score 0.5, 10 tries of 10 iterations: the planted count comes back, and the margin is
    at least 0.05 -- between the winner and the runner-up for a planted count of 2 .. 4; for ONE planted cluster, where the count is
    decided by min_score and not between the candidates, between min_score and the best score."""
    x = ref.planted(true, 200, 40, 100 + true)
    seeds = ref.draw_seeds(200, 10, 4, 7 + true)
    res = ref.count(x, None, seeds, 1, 4, 10, min_score=0.5)
    margin = ref.margin(res['scores']) if true > 1 else 0.5 - float(res['scores'].max())
    print('planted %d: count %d, scores %s, tries %s, margin %.4f' % (true, res['count'], res['scores'].tolist(), res['tries'].tolist(), margin))
    assert res['count'] == true and res['cand'] == (true - 2 if true > 1 else -1)
    assert margin >= 0.05
    assert res['centroids'].shape == (4, 40) and not res['centroids'][true if true > 1 else 0:].any()


def test_the_restatements_rules():
    nan, inf = float('nan'), float('inf')
    assert ref.pick_try(np.array([nan, 3.0, 2.0, 2.0, inf], np.float32)) == 2 and ref.select_try(np.array([3.0, nan, 1.0])) == 1
    assert ref.pick_try(np.array([nan, inf, -inf], np.float32)) == -1
    assert ref.choose([0.3, 0.7, 0.7], 2) == (3, 1) and ref.choose([-inf, -inf], 2) == (2, 0) and ref.choose([-inf, -inf], 3) == (3, 0)
    assert ref.choose([-inf, -inf], 1, 0.5) == (1, -1) and ref.choose([0.3, 0.4], 1, 0.5) == (1, -1) and ref.choose([0.3, 0.6], 1, 0.5) == (3, 1)
    with pytest.raises(ValueError):
        ref.choose([0.3], 1)
    # a point on a centroid, two coincident centroids, zero weights
    x = np.array([[1, 0], [0, 1], [1, 0]], np.float32)
    assert ref.score(x, None, np.array([[1, 0], [0, 1]], np.float32)) == 1.0
    assert ref.score(x, None, np.array([[1, 0], [1, 0]], np.float32)) == 0.0
    assert ref.score(x, np.zeros(3, np.float32), np.array([[1, 0], [0, 1]], np.float32)) == -inf


class _KM(object):
    def __init__(self, beta):
        self.beta, self.nb_tries, self.nb_clusters = beta, 3, 4


def _stub(beta=None, enhance=False, E=40):
    from models.network import Network

    class Stub(Network):
        def __init__(self):
            self.output, self.args, self.S, self.embedding_size = object(), {'chunk_size': 2048, 'batch_size': 2}, 4, E
            self.kmeans, self.embeddings, self.masks = _KM(beta), object(), object()
            if enhance:
                self._cache_enhance = object()
    return Stub()


def test_the_refusals_of_speakers_come_before_any_device_work():
    x = np.zeros(5000, np.float32)
    for call in (lambda m, **k: m.separate_recording(x, **k), lambda m, **k: m.separate_recordings([x], **k)):
        with pytest.raises(ValueError, match="needs clustering='recording'"):
            call(_stub(), speakers='auto')
        with pytest.raises(ValueError, match="needs clustering='recording'"):
            call(_stub(), clustering='chunk', speakers=(2, 3))
        with pytest.raises(ValueError, match='hard assignment only'):
            call(_stub(beta=5.0), clustering='recording', speakers='auto')
        with pytest.raises(ValueError, match='enhance layer'):
            call(_stub(enhance=True), clustering='recording', speakers='auto')
        for bad, word in (((2, 5), 'above the 4 tracks'), ((0, 3), 'lo >= 1'), ((3, 2), 'lo <= hi'), ((1, 3), 'needs a min_score'),
                          ('1:3', 'needs a min_score'), ('two', "'auto' or LO:HI"), ((2,), 'pair'), ((2.5, 3), 'pair')):
            with pytest.raises(ValueError, match=word):
                call(_stub(), clustering='recording', speakers=bad)
        with pytest.raises(ValueError, match='embedding_size'):
            call(_stub(E=20), clustering='recording', speakers='auto')
        with pytest.raises(ValueError, match='min_score belongs'):
            call(_stub(), clustering='recording', min_score=0.5)
        with pytest.raises(ValueError, match='finite'):
            call(_stub(), clustering='recording', speakers=(1, 3), min_score=float('nan'))


def test_the_wrapper_refuses_before_it_touches_the_device():
    from ams_hip import spk_count as sc
    assert sc.parse_speakers('auto', 5) == (2, 5) and sc.parse_speakers('1:3', 5) == (1, 3) and sc.parse_speakers((2, 4), 5) == (2, 4)
    assert sc.check_range(1, 4, 4, 0.5, 40) == (2, 3) and sc.check_range(3, 3, 6, None, 8) == (3, 1)
    seeds = np.array([[0, 1, 2], [3, 4, 5]])
    with pytest.raises(ValueError, match='embedding_size'):
        sc.count_clusters(torch.zeros(30, 20), [30], seeds, 2, 3, 2, 1)
    with pytest.raises(ValueError, match='shape'):
        sc.count_clusters(torch.zeros(30, 8), [30], seeds[:, :2], 2, 3, 2, 1)
    with pytest.raises(ValueError, match='recording 0, try 1.*outside'):
        sc.count_clusters(torch.zeros(30, 8), [30], np.array([[0, 1, 2], [3, 4, 30]]), 2, 3, 2, 1)
    with pytest.raises(ValueError, match='not distinct'):
        sc.count_clusters(torch.zeros(30, 8), [30], np.array([[0, 1, 2], [3, 3, 5]]), 2, 3, 2, 1)
    with pytest.raises(ValueError, match='min_score'):
        sc.count_clusters(torch.zeros(30, 8), [30], seeds, 1, 3, 2, 1)


def test_command_lines_take_and_refuse_the_flags():
    from experiments.evaluation import separate, separate_many
    one = ['--model_folder', 'm', '--sortofmodel', 'front_DPCL', '--input', 'a.wav', '--output_prefix', 'o', '--nb_speakers', '3']
    many = ['--model_folder', 'm', '--sortofmodel', 'front_DPCL', '--inputs', 'a.wav', '--output_dir', 'o', '--nb_speakers', '3']
    rec = ['--clustering', 'recording']
    for cli, base in ((separate, one), (separate_many, many)):
        args = cli.build_parser().get_args(base)
        assert args.speakers is None and args.min_score is None and separate.speakers_arg(args) is None
        assert separate.speakers_arg(cli.build_parser().get_args(base + rec + ['--speakers', 'auto'])) == (2, 3)
        assert separate.speakers_arg(cli.build_parser().get_args(base + rec + ['--speakers', '1:2', '--min_score', '0.4'])) == (1, 2)
        for extra, word in ((['--speakers', 'auto'], '--clustering recording'), (rec + ['--speakers', '1:3'], 'min_score'),
                            (rec + ['--speakers', '2:4'], 'above the 3 tracks'), (rec + ['--speakers', 'some'], 'LO:HI'),
                            (rec + ['--speakers', '3:2'], 'lo <= hi'), (rec + ['--min_score', '0.5'], '--min_score goes with --speakers')):
            with pytest.raises(SystemExit, match=word):
                cli.main(base + extra)
        with pytest.raises(SystemExit, match='enhance layer is not built'):
            cli.main([a if a != 'front_DPCL' else 'front_enhanced_DPCL' for a in base] + rec + ['--speakers', 'auto'])
    with pytest.raises(SystemExit, match='not built'):
        separate_many.main(many + rec + ['--speakers', 'auto', '--reference_dir', 'r'])
