"""CPU: the whole-recording stitcher's boundary -- the chunk arithmetic, the numpy restatement (tests/stitch_ref.py) on permuted
sources, include/ams_stitch.h against the exports of libams_stitch.so, the unchanged exports of libams_hip.so, the wrappers' refusal of
CPU tensors, the command line's parsing, refusals and .wav round trip, and the kernels' resource usage when compiled for gfx950."""
import ctypes
import os
import re
import subprocess
import sys
import wave

import numpy as np
import pytest

from tests import stitch_ref as ref

torch = pytest.importorskip('torch')

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, 'adaptive-multispeaker-separation_amd')
NAMES = {'ams_stitch_abi_version', 'ams_stitch_chunks', 'ams_stitch_workspace_bytes', 'ams_stitch_stats', 'ams_stitch_tracks',
         'ams_stitch_ola'}
SHAPES = [(2, 256, 128, 700), (3, 256, 192, 1000), (6, 64, 32, 333), (2, 250, 125, 251), (5, 2052, 1028, 5000)]      # S, L, H, N


def _built(path):
    if not os.path.exists(path):
        import __graft_entry__
        __graft_entry__.build()
    return path


def test_nb_chunks_edge_cases():
    from ams_hip import stitch
    L, H = 256, 128
    for fn in (stitch.nb_chunks, ref.nb_chunks):
        assert fn(1, L, H) == 1 and fn(100, L, H) == 1             # N < L
        assert fn(L, L, H) == 1                                    # N = L
        assert fn(L + 1, L, H) == 2                                # N = L + 1
        for k in (1, 2, 7):
            assert fn(L + k * H, L, H) == 1 + k                    # N = L + k H exactly
            assert fn(L + k * H + 1, L, H) == 2 + k
        assert fn(251, 250, 125) == 2 and fn(5000, 2052, 1028) == 4 and fn(480000, 20480, 10240) == 46
    with pytest.raises(ValueError):
        stitch.nb_chunks(0, L, H)
    for bad in (127, 256, 0):                                      # a sample in three chunks; no overlap; no hop
        with pytest.raises(ValueError):
            stitch.nb_chunks(1000, L, bad)
    assert stitch.nb_chunks(1000, 251, 126) == ref.nb_chunks(1000, 251, 126) == 7     # odd L: H >= ceil(L / 2)
    with pytest.raises(ValueError):
        stitch.nb_chunks(1000, 251, 125)
    assert np.array_equal(stitch.w_head_table(5), ref.w_head(5))


@pytest.mark.parametrize('S,L,H,N', SHAPES)
def test_restatement_recovers_permuted_sources(S, L, H, N):
    src, est, perm, truth = ref.material(7 + S, S, L, H, N)
    C = ref.nb_chunks(N, L, H)
    assert est.shape == (C, S, L) and C >= 2
    rel, margin = ref.search(ref.border_stats(est, H))
    assert margin.min() >= 0.99999, margin.min()
    trk = ref.tracks(rel)
    assert np.array_equal(trk, truth)
    # without noise the stitched tracks ARE the sources (in the order chunk 0 had them), up to the cross-fade's rounding
    src, est, perm, truth = ref.material(7 + S, S, L, H, N, noise=0)
    out = ref.overlap_add(est, truth, N, H)
    want = src[np.argsort(perm[0])]
    assert out.shape == (S, N) and out.dtype == np.float32
    assert np.all(np.abs(out - want) <= 4 * 2.0 ** -24 * np.abs(want))
    n = np.arange(N)
    c1 = np.minimum(n // H, C - 1)
    copied = ~((c1 > 0) & (n - c1 * H < L - H))
    assert np.array_equal(out[:, copied], want[:, copied])


def test_restatement_tie_and_nan_rules():
    Q = np.zeros((3, 3, 3))
    Q[1] = np.nan
    Q[2] = np.array([[1.0, 1.0, 9.0], [1.0, 1.0, 9.0], [9.0, 9.0, 0.0]])       # identity and the swap of the first two tie: the identity
    rel, margin = ref.search(Q)
    assert rel.tolist() == [[0, 1, 2]] * 3
    Q = np.full((1, 2, 2), np.nan)
    Q[0, 0, 1] = Q[0, 1, 0] = 1.0                                              # the identity costs NaN: the swap wins
    assert ref.search(Q)[0].tolist() == [[1, 0]]
    assert ref.tracks(np.array([[1, 2, 0], [1, 2, 0]])).tolist() == [[0, 1, 2], [1, 2, 0], [2, 0, 1]]


def test_header_and_exports():
    src = open(os.path.join(ROOT, 'include', 'ams_stitch.h')).read()
    src = re.sub(r'/\*.*?\*/', ' ', src, flags=re.S)
    assert set(re.findall(r'\b(ams_\w+)\s*\(', src)) == NAMES
    from ams_hip import _lib, stitch
    assert set(_lib.parse_header(stitch.HEADER_PATH)) == NAMES
    path = _built(stitch.LIB_PATH)
    out = subprocess.run(['nm', '-D', '--defined-only', path], capture_output=True, text=True, check=True).stdout
    exported = set(ln.split()[-1] for ln in out.splitlines() if ln.split() and ln.split()[-1].startswith('ams_'))
    assert exported == NAMES
    lib = ctypes.CDLL(path)
    assert lib.ams_stitch_abi_version() == 1 == stitch.ABI_VERSION
    lib.ams_stitch_workspace_bytes.restype = ctypes.c_size_t
    assert lib.ams_stitch_workspace_bytes(46, 2, 20480, 10240) == 45 * 10 * 4 * 4
    assert lib.ams_stitch_workspace_bytes(3, 6, 4100, 2050) == 2 * 3 * 36 * 4
    assert lib.ams_stitch_workspace_bytes(1, 2, 256, 128) == 0 and lib.ams_stitch_workspace_bytes(3, 7, 256, 128) == 0


def test_product_library_exports_are_unchanged():
    from ams_hip import _lib
    path = _built(_lib.LIB_PATH)
    out = subprocess.run(['nm', '-D', '--defined-only', path], capture_output=True, text=True, check=True).stdout
    assert 'ams_stitch' not in out
    exported = set(ln.split()[-1] for ln in out.splitlines() if ln.split() and ln.split()[-1].startswith('ams_'))
    assert exported == set(_lib.parse_header())
    assert '#define AMS_ABI_VERSION 10' in open(_lib.HEADER_PATH).read() and _lib.ABI_VERSION == 10
    assert 'stitch' not in open(_lib.HEADER_PATH).read()


def test_wrappers_refuse_cpu_tensors():
    from ams_hip import stitch
    from ams_hip._lib import AmsError
    est = torch.zeros(3, 2, 256)
    with pytest.raises(AmsError):
        stitch.chunks(torch.zeros(700), 256, 128)
    with pytest.raises(AmsError):
        stitch.border_stats(est, 128)
    with pytest.raises(AmsError):
        stitch.tracks(torch.zeros(2, 2, 2), 2)
    with pytest.raises(AmsError):
        stitch.overlap_add(est, torch.zeros(3, 2, dtype=torch.int32), 500, 128)
    with pytest.raises(AmsError):
        stitch.stitch(est, 500, 128)


def _write_wav(path, pcm, fs, channels=1):
    with wave.open(path, 'wb') as w:
        w.setnchannels(channels)
        w.setsampwidth(2)
        w.setframerate(fs)
        w.writeframes(np.asarray(pcm, '<i2').tobytes())


def test_cli_flags_refusals_and_wav_round_trip(tmp_path):
    import config
    from experiments.evaluation import separate as cli
    a = cli.build_parser().get_args(['--model_folder', 'm', '--sortofmodel', 'front_DPCL', '--input', 'a.wav', '--output_prefix', 'o',
                                     '--hop', '12000', '--chunk_size', '20480', '--nb_speakers', '3', '--beta_kmeans', '5.0'])
    assert (a.model_folder, a.sortofmodel, a.input, a.output_prefix, a.hop, a.chunk_size, a.nb_speakers) == \
        ('m', 'front_DPCL', 'a.wav', 'o', 12000, 20480, 3)
    assert a.beta_kmeans == 5.0 and a.filters == 512 and a.layer_size == 600            # eval.py's argument groups
    assert cli.build_parser().get_args(['--model_folder', 'm', '--sortofmodel', 's', '--input', 'i', '--output_prefix', 'o']).hop is None
    with pytest.raises(SystemExit):
        cli.build_parser().get_args(['--model_folder', 'm', '--sortofmodel', 's', '--output_prefix', 'o'])      # no --input

    rng = np.random.RandomState(5)
    pcm = rng.randint(-32768, 32768, size=1234).astype(np.int16)
    pcm[:4] = (-32768, 32767, 0, -1)
    good = str(tmp_path / 'good.wav')
    _write_wav(good, pcm, config.fs)
    x = cli.read_wav(good)
    assert x.dtype == np.float32 and np.array_equal(x, pcm.astype(np.float32) / np.float32(32768.0))
    assert np.array_equal(cli.read_input(good), x)
    # symmetric clipping: -32768 comes back as -32767, everything else as it was; beyond full scale saturates
    back = str(tmp_path / 'back.wav')
    cli.write_wav(back, x)
    with wave.open(back, 'rb') as w:
        assert (w.getnchannels(), w.getsampwidth(), w.getframerate(), w.getnframes()) == (1, 2, config.fs, 1234)
        got = np.frombuffer(w.readframes(1234), '<i2')
    assert np.array_equal(got, np.maximum(pcm, -32767))
    cli.write_wav(back, np.array([2.0, -2.0, 1.0, -1.0], np.float32))
    assert (cli.read_wav(back) * 32768).tolist() == [32767.0, -32767.0, 32767.0, -32767.0]
    with pytest.raises(SystemExit) as e:                           # a non-finite sample has no int16 value: refused, not written
        cli.write_wav(str(tmp_path / 'nan.wav'), np.array([0.5, np.nan, np.inf], np.float32))
    assert 'not finite' in str(e.value) and not os.path.exists(str(tmp_path / 'nan.wav'))

    wrong = str(tmp_path / 'wrong.wav')
    _write_wav(wrong, pcm, 16000)
    with pytest.raises(SystemExit) as e:
        cli.read_wav(wrong)
    assert 'sample rate' in str(e.value) and '16000' in str(e.value) and str(config.fs) in str(e.value)
    stereo = str(tmp_path / 'stereo.wav')
    _write_wav(stereo, pcm, config.fs, channels=2)
    with pytest.raises(SystemExit) as e:
        cli.read_wav(stereo)
    assert 'channel' in str(e.value)

    npy = str(tmp_path / 'x.npy')
    np.save(npy, x)
    assert np.array_equal(cli.read_input(npy), x)
    np.save(npy, x.astype(np.float64))
    with pytest.raises(SystemExit):
        cli.read_input(npy)
    paths = cli.write_outputs(str(tmp_path / 'o'), np.stack([x, -x]), True)
    assert [os.path.basename(p) for p in paths] == ['o_0.npy', 'o_1.npy'] and np.array_equal(np.load(paths[1]), -x)
    paths = cli.write_outputs(str(tmp_path / 'o'), np.stack([x, -x]), False)
    assert [os.path.basename(p) for p in paths] == ['o_0.wav', 'o_1.wav']
    assert np.array_equal(cli.read_wav(paths[0]), np.maximum(x, np.float32(-32767.0 / 32768.0)))

    with pytest.raises(SystemExit) as e:                           # refused before the input is opened or a model is built
        cli.main(['--model_folder', 'm', '--sortofmodel', 'pretraining', '--input', 'missing.wav', '--output_prefix', 'o'])
    assert 'pretraining' in str(e.value) and 'clean sources' in str(e.value)


def test_stitch_kernels_compile_for_gfx950_without_scratch():
    """tools/kernel_resources.py on csrc/stitch/stitch.hip with the library's flags: both arms of chunks and ola, twelve variants of the
    border table (S = 1 .. 6, vector and dword arm) with their 36 running sums in registers, no scratch, no spill, no warning."""
    run = subprocess.run([sys.executable, os.path.join(ROOT, 'tools', 'kernel_resources.py'),
                          os.path.join(PKG, 'csrc', 'stitch', 'stitch.hip'), '-ffp-contract=off'],
                         capture_output=True, text=True, check=True)
    assert 'warning' not in run.stderr
    out = run.stdout.splitlines()[1:]
    names = ' '.join(out)
    for S in range(1, 7):
        for vec in ('true', 'false'):
            assert 'stats_kernel<%d, %s>' % (S, vec) in names, (S, vec)
    for k in ('chunks_kernel<true>', 'chunks_kernel<false>', 'ola_kernel<true>', 'ola_kernel<false>', 'stats_fold_kernel',
              'border_perm_kernel', 'tracks_kernel'):
        assert k in names, k
    rows = [ln.split() for ln in out if ln.strip()]
    assert len(rows) == 12 + 7
    for r in rows:
        vgpr, agpr, spill, scratch, occ, lds = r[-6:]
        assert spill == '0' and scratch == '0', r
        if 'chunks_kernel' in ' '.join(r) or 'ola_kernel' in ' '.join(r):
            assert lds == '0', r
