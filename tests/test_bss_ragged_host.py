"""CPU: the ragged BSS-eval's boundary -- include/ams_bss_ragged.h against the exports of libams_bss_ragged.so, the exports of the other
libraries, the host table builder, the launch count, the refusals of utils.bss_eval.bss_eval_pairs_ragged (made before the library or
the device is touched) and of experiments/evaluation/separate_many.py's scoring flags, and the time-domain definition
(tests/bss_ragged_ref.py) against the pinned numpy oracle under the project's dB rule."""
import ctypes
import glob
import os
import re
import subprocess
import wave

import numpy as np
import pytest

from oracle import bss_eval as obss
from tests import bss_ragged_ref as rr
from tests.bss_common import close_db as _close_db, mix as _mix

torch = pytest.importorskip('torch')

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, 'adaptive-multispeaker-separation_amd', 'ams_hip')
NAMES = {'ams_bssr_abi_version', 'ams_bssr_block', 'ams_bssr_blocks', 'ams_bssr_tables', 'ams_bssr_launches', 'ams_bssr_workspace_bytes',
         'ams_bssr_eval'}
# what libams_bss.so exports (include/ams_bss.h and include/ams_bss_batch.h); sharing csrc/bss/chol_batched.h with the ragged library must not change it
BSS_NAMES = {'ams_bss_abi_version', 'ams_bss_create', 'ams_bss_destroy', 'ams_bss_workspace_bytes', 'ams_bss_eval_pairs',
             'ams_bssb_abi_version', 'ams_bssb_create', 'ams_bssb_destroy', 'ams_bssb_workspace_bytes', 'ams_bssb_eval', 'ams_bssb_potrf'}
vp = ctypes.c_void_p


def _built():
    if not os.path.exists(os.path.join(LIBDIR, 'libams_bss_ragged.so')):
        import __graft_entry__
        __graft_entry__.build()


def _exports(path):
    out = subprocess.run(['nm', '-D', '--defined-only', path], capture_output=True, text=True, check=True).stdout
    return {ln.split()[-1] for ln in out.splitlines() if ln.split()[-1].startswith('ams_')}


def test_header_and_exports():
    _built()
    src = open(os.path.join(ROOT, 'include', 'ams_bss_ragged.h')).read()
    src = re.sub(r'/\*.*?\*/', ' ', src, flags=re.S)
    assert set(re.findall(r'\b(ams_\w+)\s*\(', src)) == NAMES
    assert _exports(os.path.join(LIBDIR, 'libams_bss_ragged.so')) == NAMES
    from utils import bss_eval as hb
    lib = hb._load_ragged()
    assert lib.ams_bssr_abi_version() == 1
    assert int(re.search(r'#define\s+AMS_BSSR_BLOCK\s+(\d+)', src).group(1)) == lib.ams_bssr_block() == hb.ragged_block() == rr.BLOCK
    assert int(re.search(r'#define\s+AMS_BSSR_MAX_FLEN\s+(\d+)', src).group(1)) == hb.RAGGED_MAX_FLEN


def test_other_libraries_keep_their_exports():
    _built()
    assert _exports(os.path.join(LIBDIR, 'libams_bss.so')) == BSS_NAMES
    libs = sorted(glob.glob(os.path.join(LIBDIR, 'libams_*.so')))
    assert len(libs) >= 7
    for path in libs:
        if os.path.basename(path) != 'libams_bss_ragged.so':
            assert not [n for n in _exports(path) if n.startswith('ams_bssr_')], path
    deps = subprocess.run(['readelf', '-d', os.path.join(LIBDIR, 'libams_bss_ragged.so')], capture_output=True, text=True, check=True).stdout
    assert 'hipfft' not in deps and 'hipsolver' not in deps


def _tables(lengths, F):
    from utils import bss_eval as hb
    lib = hb._load_ragged()
    l_off = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    R = len(lengths)
    bt = lib.ams_bssr_blocks(l_off.ctypes.data_as(vp), R, F)
    if bt < 0:
        return bt, None, None
    b_off, tab = np.full(R + 1, -7, np.int64), np.full((bt, 2), -7, np.int32)
    assert lib.ams_bssr_tables(l_off.ctypes.data_as(vp), R, F, b_off.ctypes.data_as(vp), tab.ctypes.data_as(vp)) == 0
    return bt, b_off, tab


@pytest.mark.parametrize('F', [32, 1])
def test_tables(F):
    B = rr.BLOCK
    lengths = [1, B - F, B - F + 1, B - F + 2, 3 * B + 5]
    want = [1, 1, 1, 2, 4]                                     # ceil((L + F - 1) / B)
    assert want == [rr.nblocks(L, F) for L in lengths] == [-(-(L + F - 1) // B) for L in lengths]
    bt, b_off, tab = _tables(lengths, F)
    assert bt == sum(want)
    assert b_off.tolist() == np.concatenate([[0], np.cumsum(want)]).tolist()
    assert tab.tolist() == [[r, b] for r, n in enumerate(want) for b in range(n)]
    from utils import bss_eval as hb
    lay = hb._RaggedLayout(lengths, F)
    assert (lay.Btot, lay.b_off.tolist(), lay.tab.tolist()) == (bt, b_off.tolist(), tab.tolist())
    assert hb._ragged_layout(lengths, F) is hb._ragged_layout(list(lengths), F)        # one layout (and one upload) per set of lengths


def test_tables_refusals():
    from utils import bss_eval as hb
    lib = hb._load_ragged()
    assert _tables([5, 0, 3], 4)[0] == -1                      # a recording without samples
    assert _tables([5], 0)[0] == -1 and _tables([5], hb.RAGGED_MAX_FLEN + 1)[0] == -1
    assert _tables([5], hb.RAGGED_MAX_FLEN)[0] == 1
    bad = np.array([1, 6], np.int64)                           # l_off[0] != 0
    assert lib.ams_bssr_blocks(bad.ctypes.data_as(vp), 1, 4) == -1
    assert lib.ams_bssr_blocks(None, 1, 4) == -1
    huge = np.array([0, (2 ** 31) * rr.BLOCK], np.int64)       # 2^31 rows: one more than the table holds
    assert lib.ams_bssr_blocks(huge.ctypes.data_as(vp), 1, 1) == -1
    assert lib.ams_bssr_blocks(np.array([0, (2 ** 31 - 1) * rr.BLOCK], np.int64).ctypes.data_as(vp), 1, 1) == 2 ** 31 - 1


def test_launches_and_workspace_are_functions_of_the_geometry():
    from utils import bss_eval as hb
    lib = hb._load_ragged()
    for S, K, F in ((2, 2, 512), (2, 1, 32), (6, 1, 16), (1, 1, 1), (3, 2, 20)):
        n = lib.ams_bssr_launches(S, K, F)
        assert n == 4 + (3 * -(-S * F // 32) - 2) + (3 * -(-F // 32) - 2) + 4 + 2        # no R, no length in the signature or the count
        assert lib.ams_bssr_launches(S, K + 1, F) == n
    assert lib.ams_bssr_launches(7, 1, 32) == -1 and lib.ams_bssr_launches(2, 0, 32) == -1 and lib.ams_bssr_launches(2, 1, 0) == -1
    # the bulk of the workspace: 8 ((S F)^2 + S F^2) per recording -- 12.6 MB at S = 2, 88 MB at S = 6, F = 512
    for S in (2, 6):
        one = lib.ams_bssr_workspace_bytes(1, 2, S, 512, 20)
        two = lib.ams_bssr_workspace_bytes(2, 2, S, 512, 40)
        bulk = 8 * ((S * 512) ** 2 + S * 512 ** 2)
        assert bulk < two - one < 1.25 * bulk
    assert lib.ams_bssr_workspace_bytes(0, 2, 2, 512, 1) == 0 and lib.ams_bssr_workspace_bytes(2, 2, 2, 512, 1) == 0      # Btot < R


def test_eval_refuses_bad_arguments_before_anything_is_launched():
    """-1 needs no device: NULL pointers and a geometry outside the domain are answered on the host."""
    from utils import bss_eval as hb
    lib = hb._load_ragged()
    p = 4096                                                   # never dereferenced
    ok = [p, p, p, p, p, 1, 1, 2, 32, 1, p, p, p, 1 << 30, None]
    for i, v in ((0, None), (4, None), (10, None), (12, None), (5, 0), (6, 0), (6, 65), (7, 0), (7, 7), (8, 0), (8, 1025), (9, 0), (12, p + 4)):
        a = list(ok)
        a[i] = v
        assert lib.ams_bssr_eval(*a) == -1, (i, v)
    a = list(ok)
    a[13] = lib.ams_bssr_workspace_bytes(1, 1, 2, 32, 1) - 1   # one byte short: -2, nothing launched (no device is needed to say so)
    assert lib.ams_bssr_eval(*a) == -2


def _refs(shapes, tensor):
    mk = (lambda s: torch.zeros(s, dtype=torch.float64)) if tensor else np.zeros
    return [mk(s) for s in shapes]


@pytest.mark.parametrize('rs,es,flen', [([], [], 32),                                           # empty lists
                                        ([(2, 100)], [(2, 100), (2, 100)], 32),                 # list lengths
                                        ([(2, 100), (3, 90)], [(2, 100), (3, 90)], 32),         # S differs between recordings
                                        ([(2, 100), (2, 90)], [(2, 2, 100), (3, 2, 90)], 32),   # K differs
                                        ([(2, 100), (2, 90)], [(2, 100), (2, 2, 90)], 32),      # K differs (no set axis / a set axis)
                                        ([(2, 100), (2, 90)], [(2, 100), (2, 91)], 32),         # L_r of a reference and its estimates
                                        ([(2, 100)], [(3, 100)], 32),                           # S of a reference and its estimates
                                        ([(7, 100)], [(7, 100)], 32),                           # S > 6
                                        ([(2, 100)], [(2, 100)], 0),                            # flen < 1
                                        ([(2, 100)], [(2, 100)], 2000),                         # flen above the library's
                                        ([(100,)], [(100,)], 32),                               # no source axis
                                        ([(2, 0)], [(2, 0)], 32)])                              # no samples
def test_pairs_ragged_refusals(rs, es, flen, monkeypatch):
    from utils import bss_eval as hb

    def touched(*a, **k):
        raise AssertionError('the library or the device was touched before the arguments were checked')
    for name in ('_load_ragged', '_ragged_layout', '_ragged_groups', 'bss_eval_pairs_ragged_packed', 'ragged_block'):
        monkeypatch.setattr(hb, name, touched)
    monkeypatch.setattr(torch.cuda, 'is_available', touched)
    for tensor in (False, True):
        with pytest.raises(hb.BssError):
            hb.bss_eval_pairs_ragged(_refs(rs, tensor), _refs(es, tensor), flen=flen)
        with pytest.raises(hb.BssError):
            hb.bss_eval_sources_ragged(_refs(rs, tensor), _refs(es, tensor), flen=flen)
    with pytest.raises(hb.BssError):
        hb.bss_eval_pairs_ragged(np.zeros((1, 2, 100)), np.zeros((1, 2, 100)))           # arrays, not lists


def test_pairs_ragged_raises_without_a_gpu(monkeypatch):
    from utils import bss_eval as hb

    def touched(*a, **k):
        raise AssertionError('the library was touched without a GPU')
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: False)
    monkeypatch.setattr(hb, '_load_ragged', touched)
    with pytest.raises(hb.BssError, match='GPU'):
        hb.bss_eval_pairs_ragged([np.ones((2, 100))], [np.ones((2, 100))])
    with pytest.raises(hb.BssError, match='GPU'):
        hb.bss_eval_sources_ragged([np.ones((2, 100))], [np.ones((2, 2, 100))])


def test_groups_and_the_cap():
    """Consecutive recordings under the cap; a recording above it is refused with the sizes in the message (host arithmetic only)."""
    from utils import bss_eval as hb
    lib = hb._load_ragged()
    lengths = [100, 5000, 300, 9000, 50]
    one = [lib.ams_bssr_workspace_bytes(1, 2, 2, 32, rr.nblocks(L, 32)) for L in lengths]
    assert hb._ragged_groups(lengths, 2, 2, 32, 1 << 40) == [(0, 5)]
    groups = hb._ragged_groups(lengths, 2, 2, 32, max(one))
    assert len(groups) >= 3 and groups[0][0] == 0 and groups[-1][1] == 5
    assert all(a[1] == b[0] for a, b in zip(groups, groups[1:]))
    for r0, r1 in groups:
        assert lib.ams_bssr_workspace_bytes(r1 - r0, 2, 2, 32, sum(rr.nblocks(L, 32) for L in lengths[r0:r1])) <= max(one)
    with pytest.raises(hb.BssError) as e:
        hb._ragged_groups(lengths, 2, 2, 32, max(one) - 1)
    assert 'recording 3' in str(e.value) and '9000' in str(e.value) and str(max(one)) in str(e.value) and str(max(one) - 1) in str(e.value)


def test_sources_ragged_permutation_rule(monkeypatch):
    from utils import bss_eval as hb
    R, K, S = 2, 2, 3
    crit = np.random.RandomState(3).randn(R, K, 3, S, S)
    sir = np.zeros((S, S))
    for e in range(S):
        sir[e, (e + 1) % S] = 30.0
    crit[0, 0, 1] = sir
    crit[1, 1, 1] = np.array([[5.0, 5.0, 0.0], [5.0, 5.0, 0.0], [0.0, 0.0, 9.0]])           # a tie: the identity wins
    monkeypatch.setattr(hb, 'bss_eval_pairs_ragged', lambda r, e, flen=hb.FLEN, cap_bytes=None: (crit.copy(), np.zeros(R, np.int32)))
    sdr, sir_o, sar, perm = hb.bss_eval_sources_ragged(None, None)
    assert sdr.shape == sir_o.shape == sar.shape == perm.shape == (R, K, S)
    assert perm[0, 0].tolist() == [2, 0, 1] and perm[1, 1].tolist() == [0, 1, 2]
    dum = np.arange(S)
    for r in range(R):
        for k in range(K):
            want = hb._select_permutation(crit[r, k, 0], crit[r, k, 1], crit[r, k, 2])
            assert np.array_equal(perm[r, k], want[3]) and np.array_equal(sdr[r, k], crit[r, k, 0][perm[r, k], dum])
    assert np.array_equal(hb.bss_eval_sources_ragged(None, None, compute_permutation=False)[3], np.broadcast_to(dum, (R, K, S)))


@pytest.mark.parametrize('S,K,L', [(2, 1, 100), (2, 1, 257), (2, 1, 4097), (3, 2, 1000)])
def test_time_domain_definition_against_the_oracle(S, K, L):
    """The margin the GPU cases have: the largest dB error of the time-domain restatement against the pinned FFT oracle."""
    flen = 32
    rng = np.random.RandomState(1000 * S + L)
    refs, e = _mix(rng, S, L)
    ests = np.stack([e[::-1]] + [e + 0.2 * k * rng.randn(S, L) for k in range(1, K)])
    got, info = rr.bss_eval_pairs(refs, ests, flen)
    assert info == 0
    want = np.stack([np.stack(obss.bss_eval_sources(refs, ests[k], flen=flen, return_matrices=True)[4]) for k in range(K)])
    err = _close_db(got, want)
    print('S = %d, K = %d, L = %d: largest |dB error| of the time-domain definition %.3e' % (S, K, L, err))
    # the correlations by lag are the oracle's circular ones (n >= L + F - 1), and the Gram layout is gram_kernel's
    n = obss._nfft(L, flen)
    sf = np.fft.fft(refs, n=n, axis=1)
    G = rr.gram(refs, flen)
    assert np.array_equal(G, G.T)
    k = np.arange(flen)
    for i in range(S):
        for j in range(S):
            ss = np.real(np.fft.ifft(sf[i] * np.conj(sf[j])))
            blk = ss[(k[None, :] - k[:, None]) % n]
            assert np.abs(G[i * flen:(i + 1) * flen, j * flen:(j + 1) * flen] - blk).max() < 1e-9 * np.abs(ss).max()
    # a silent reference: info != 0 and NaN criteria
    silent = refs.copy()
    silent[S - 1] = 0.0
    got, info = rr.bss_eval_pairs(silent, ests, flen)
    assert info != 0 and np.isnan(got).all()


def _write_wav(path, pcm, fs):
    with wave.open(path, 'wb') as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(fs)
        w.writeframes(np.asarray(pcm, '<i2').tobytes())


def test_separate_many_scoring_refusals(tmp_path):
    import config
    from experiments.evaluation import separate_many as cli
    pcm = np.random.RandomState(5).randint(-3000, 3000, size=1234).astype(np.int16)
    good, arr = str(tmp_path / 'good.wav'), str(tmp_path / 'arr.npy')
    _write_wav(good, pcm, config.fs)
    np.save(arr, (pcm[:900] / 32768.0).astype(np.float32))
    refd = str(tmp_path / 'refs')
    os.makedirs(refd)
    base = ['--model_folder', 'm', '--sortofmodel', 'front_DPCL', '--output_dir', str(tmp_path / 'o')]
    a = cli.build_parser().get_args(base + ['--inputs', good])
    assert a.reference_dir is None and a.score_both_clusterings is False and a.clustering == 'chunk'        # the defaults are today's

    def refused(extra, *words):
        with pytest.raises(SystemExit) as e:                       # each before a model is built: 'm' is no model folder
            cli.main(base + extra)
        for w in words:
            assert w in str(e.value), (w, str(e.value))

    refused(['--inputs', good, '--score_both_clusterings'], '--reference_dir')
    refused(['--inputs', good, '--reference_dir', refd, '--resample'], '--resample', 'not built')
    refused(['--inputs', good, '--reference_dir', refd], os.path.join(refd, 'good_0.wav'), 'missing')
    _write_wav(os.path.join(refd, 'good_0.wav'), pcm, config.fs)
    refused(['--inputs', good, '--reference_dir', refd], os.path.join(refd, 'good_1.wav'), 'missing')
    _write_wav(os.path.join(refd, 'good_1.wav'), pcm[:1233], config.fs)
    refused(['--inputs', good, '--reference_dir', refd], os.path.join(refd, 'good_1.wav'), '1233', '1234')
    _write_wav(os.path.join(refd, 'good_1.wav'), pcm, 2 * config.fs)
    refused(['--inputs', good, '--reference_dir', refd], 'good_1.wav', 'sample rate')
    _write_wav(os.path.join(refd, 'good_1.wav'), pcm, config.fs)
    refused(['--inputs', good, '--reference_dir', refd, '--nb_speakers', '3'], os.path.join(refd, 'good_2.wav'))
    np.save(os.path.join(refd, 'arr_0.npy'), np.zeros(900, np.float32))
    refused(['--inputs', good, arr, '--reference_dir', refd], os.path.join(refd, 'arr_1.npy'), 'missing')      # .npy for an .npy input
    np.save(os.path.join(refd, 'arr_1.npy'), np.zeros(901, np.float32))
    refused(['--inputs', good, arr, '--reference_dir', refd], 'arr_1.npy', '901', '900')
    recs = cli.read_all([good], False)
    refs = cli.read_references([good], recs, refd, 2)
    assert refs[0].shape == (2, 1234) and refs[0].dtype == np.float32 and np.array_equal(refs[0][0], recs[0][0])
    assert not os.path.exists(str(tmp_path / 'o'))
    # the tracks as they are written: through 16-bit PCM for a .wav, float32 for an .npy
    x = np.random.RandomState(2).randn(2, 50).astype(np.float32)
    from experiments.evaluation import separate as one
    paths = one.write_outputs(str(tmp_path / 'w'), x, False, None)
    assert np.array_equal(cli.as_written(x, False), np.stack([one.read_input(p) for p in paths]))
    assert np.array_equal(cli.as_written(x.astype(np.float64), True), x)


def test_score_layout(monkeypatch):
    """scores.json's dictionary from a stubbed library call: K = 1 + the sets, the mixture first and repeated S times, the means over
    the recordings with info == 0 only, NaN written as null."""
    from experiments.evaluation import separate_many as cli
    from utils import bss_eval as hb
    rng = np.random.RandomState(4)
    S, lengths = 2, [300, 200, 250]
    recs = [(rng.randn(L).astype(np.float32), 8000) for L in lengths]
    refs = [rng.randn(S, L).astype(np.float32) for L in lengths]
    sets = [('chunk', [rng.randn(S, L).astype(np.float32) for L in lengths]), ('recording', [rng.randn(S, L).astype(np.float32) for L in lengths])]
    crit = rng.randn(3, 3, 3, S, S)
    crit[1] = np.nan
    seen = {}

    def stub(r, e, flen=hb.FLEN, cap_bytes=None):
        seen['calls'] = seen.get('calls', 0) + 1
        seen['ests'] = e
        assert all(np.array_equal(a, b) for a, b in zip(r, refs))
        return crit.copy(), np.array([0, 5, 0], np.int32)
    monkeypatch.setattr(hb, 'bss_eval_pairs_ragged', stub)
    res = cli.score(['a.wav', 'b.wav', 'c.wav'], recs, refs, sets)
    assert seen['calls'] == 1 and [e.shape for e in seen['ests']] == [(3, S, L) for L in lengths]
    for i, e in enumerate(seen['ests']):
        assert np.array_equal(e[0], np.stack([recs[i][0]] * S)) and np.array_equal(e[1], sets[0][1][i]) and np.array_equal(e[2], sets[1][1][i])
    assert res['sets'] == ['mixture', 'chunk', 'recording'] and res['scored'] == 2
    assert [r['info'] for r in res['recordings']] == [0, 5, 0]
    assert res['recordings'][1]['sets']['chunk']['sdr'] == [None, None]
    want = hb._select_permutation(crit[2, 2, 0], crit[2, 2, 1], crit[2, 2, 2])
    got = res['recordings'][2]['sets']['recording']
    assert got['sdr'] == want[0].tolist() and got['sir'] == want[1].tolist() and got['sar'] == want[2].tolist() and got['perm'] == want[3].tolist()
    sdr = [np.mean([hb._select_permutation(crit[i, k, 0], crit[i, k, 1], crit[i, k, 2])[0] for i in (0, 2)]) for k in range(3)]
    assert abs(res['means']['chunk']['sdr'] - sdr[1]) < 1e-12 and abs(res['improvement']['recording']['sdr'] - (sdr[2] - sdr[0])) < 1e-12
    import json
    assert json.loads(json.dumps(res)) == res
