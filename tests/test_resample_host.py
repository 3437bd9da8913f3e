"""CPU: the resampler's boundary -- ratio and length arithmetic, the numpy filter design against scipy's firwin, the float64 restatement
(tests/resample_ref.py) against scipy.signal.resample_poly, include/ams_resample.h against the exports of libams_resample.so, the
unchanged exports of the three other libraries, the wrappers' refusal of CPU tensors, the command line's new flags and refusals, and
the kernels' resource usage when compiled for gfx950."""
import ctypes
import os
import re
import subprocess
import sys
import wave

import numpy as np
import pytest

from tests import resample_ref as ref

torch = pytest.importorskip('torch')
signal = pytest.importorskip('scipy.signal')

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, 'adaptive-multispeaker-separation_amd')
NAMES = {'ams_resample_abi_version', 'ams_resample_out_len', 'ams_resample_pcm16', 'ams_resample_f32'}
RATES = (11025, 12000, 16000, 22050, 24000, 32000, 44100, 48000, 88200, 96000)
DESIGN_PAIRS = [(1, 2), (80, 441), (441, 80), (320, 441), (80, 882)]


def _built(path):
    if not os.path.exists(path):
        import __graft_entry__
        __graft_entry__.build()
    return path


def _exports(path):
    out = subprocess.run(['nm', '-D', '--defined-only', path], capture_output=True, text=True, check=True).stdout
    return set(ln.split()[-1] for ln in out.splitlines() if ln.split() and ln.split()[-1].startswith('ams_'))


def test_ratio_and_out_len():
    from ams_hip import resample
    for fs in RATES:
        up, down = resample.ratio(fs, 8000)
        assert (up, down) == ref.ratio(fs, 8000) and resample.ratio(8000, fs) == (down, up)
        assert up * fs == down * 8000 and np.gcd(up, down) == 1 and max(up, down) <= 1024
    assert resample.ratio(44100, 8000) == (80, 441) and resample.ratio(88200, 8000) == (40, 441) and resample.ratio(16000, 8000) == (1, 2)
    assert max(max(resample.ratio(fs, 8000)) for fs in RATES) == 441
    assert resample.ratio(8000, 8000) == (1, 1) and resample.ratio(44100, 44100) == (1, 1)
    for a, b in ((22051, 8000), (8000, 22051)):
        with pytest.raises(ValueError) as e:
            resample.ratio(a, b)
        assert '22051' in str(e.value) and '8000' in str(e.value) and '1024' in str(e.value)
    assert '8000 / 22051' in str(pytest.raises(ValueError, resample.ratio, 22051, 8000).value)
    with pytest.raises(ValueError):
        resample.ratio(0, 8000)
    for fn in (resample.out_len, ref.out_len):
        assert fn(1, 1, 2) == 1 and fn(1, 80, 441) == 1 and fn(1, 441, 80) == 6 and fn(1, 2, 1) == 2          # N = 1
        assert fn(441, 80, 441) == 80 and fn(442, 80, 441) == 81 and fn(882, 80, 441) == 160                  # N up = j down, and one more
        assert fn(4, 1, 2) == 2 and fn(5, 1, 2) == 3
        assert fn(2646000, 80, 441) == 480000
    with pytest.raises(ValueError):
        resample.out_len(0, 1, 2)
    lib = ctypes.CDLL(_built(resample.LIB_PATH))
    lib.ams_resample_out_len.restype = ctypes.c_long
    lib.ams_resample_out_len.argtypes = [ctypes.c_long, ctypes.c_int, ctypes.c_int]
    for N, up, down in ((1, 1, 2), (1, 441, 80), (441, 80, 441), (442, 80, 441), (26_800_000, 80, 441), (5, 1024, 1023)):
        assert lib.ams_resample_out_len(N, up, down) == ref.out_len(N, up, down)
    for N, up, down in ((0, 1, 2), (5, 0, 1), (5, 1, 0), (5, 1025, 1), (5, 1, 1025), (5, 2, 4), (5, 441, 441), (1 << 39, 1, 1)):
        assert lib.ams_resample_out_len(N, up, down) == 0, (N, up, down)


@pytest.mark.parametrize('up,down', DESIGN_PAIRS)
def test_design_is_scipys_firwin(up, down):
    from ams_hip import resample
    m = max(up, down)
    want = signal.firwin(2 * 10 * m + 1, 1.0 / m, window=('kaiser', 5.0)) * up
    for h in (resample.design(up, down), ref.design(up, down)):
        assert h.dtype == np.float64 and h.shape == want.shape
        err = np.abs(h - want).max()
        assert err <= 1e-12 * np.abs(want).max(), err
    assert np.array_equal(resample.design(up, down), ref.design(up, down))


# 80 / 882 is not in lowest terms (resample_poly reduces it to 40 / 441, and the library refuses it: gcd(up, down) must be 1); the
# pair that stands for "a table of that size" wherever a signal is resampled is the coprime 80 / 883
@pytest.mark.parametrize('up,down', [p if p != (80, 882) else (80, 883) for p in DESIGN_PAIRS] + [(80, 882)])
def test_restatement_is_resample_poly(up, down):
    if (up, down) == (80, 882):
        x = 0.1 * np.random.RandomState(3).randn(3001)
        assert np.abs(ref.resample(x, 40, 441) - signal.resample_poly(x, 80, 882)).max() <= 1e-12
        return
    rng = np.random.RandomState(up + down)
    for N in (1, 2, 37, 3001):
        x = 0.1 * rng.randn(N)
        want = signal.resample_poly(x, up, down)
        got = ref.resample(x, up, down)
        assert got.shape == want.shape == (ref.out_len(N, up, down),)
        err = np.abs(got - want).max()
        assert err <= 1e-12 * max(1.0, np.abs(want).max()), (N, err)
        T = ref.nb_taps(N, up, down)
        assert T.min() >= 1 and T.max() <= 20 * max(up, down) // up + 1


def test_header_and_exports():
    src = open(os.path.join(ROOT, 'include', 'ams_resample.h')).read()
    src = re.sub(r'/\*.*?\*/', ' ', src, flags=re.S)
    assert set(re.findall(r'\b(ams_\w+)\s*\(', src)) == NAMES
    from ams_hip import _lib, resample
    assert set(_lib.parse_header(resample.HEADER_PATH)) == NAMES
    path = _built(resample.LIB_PATH)
    assert _exports(path) == NAMES
    assert ctypes.CDLL(path).ams_resample_abi_version() == 1 == resample.ABI_VERSION


def test_other_libraries_exports_are_unchanged():
    from ams_hip import _lib, stitch
    inc = os.path.join(ROOT, 'include')
    product = _exports(_built(_lib.LIB_PATH))
    assert product == set(_lib.parse_header()) and not any('resample' in n for n in product)
    assert '#define AMS_ABI_VERSION 10' in open(_lib.HEADER_PATH).read() and 'resample' not in open(_lib.HEADER_PATH).read()
    st = _exports(_built(stitch.LIB_PATH))
    assert st == set(_lib.parse_header(stitch.HEADER_PATH)) and len(st) == 6
    bss = _exports(_built(os.path.join(PKG, 'ams_hip', 'libams_bss.so')))
    assert bss == set(_lib.parse_header(os.path.join(inc, 'ams_bss.h'))) | set(_lib.parse_header(os.path.join(inc, 'ams_bss_batch.h')))
    assert not any('resample' in n for n in st | bss)


def test_wrappers_refuse_cpu_tensors():
    from ams_hip import resample
    from ams_hip._lib import AmsError
    with pytest.raises(AmsError):
        resample.resample(torch.zeros(100), 16000, 8000)
    with pytest.raises(AmsError):
        resample.resample(torch.zeros(2, 100), 8000, 44100)
    with pytest.raises(AmsError):
        resample.resample(torch.zeros(100), 8000, 8000)
    with pytest.raises(AmsError):
        resample.from_pcm16(torch.zeros(100, 2, dtype=torch.int16), 44100, 8000)
    with pytest.raises(AmsError):
        resample.from_pcm16(torch.zeros(100, 1, dtype=torch.int16), 8000, 8000)
    with pytest.raises(ValueError):                                  # the ratio is looked at first
        resample.resample(torch.zeros(100), 22051, 8000)


def _write_wav(path, pcm, fs, channels=1):
    with wave.open(path, 'wb') as w:
        w.setnchannels(channels)
        w.setsampwidth(2)
        w.setframerate(fs)
        w.writeframes(np.asarray(pcm, '<i2').tobytes())


def test_command_line_flags_and_refusals(tmp_path):
    import config
    from experiments.evaluation import separate as cli
    base = ['--model_folder', 'm', '--sortofmodel', 'front_DPCL', '--output_prefix', str(tmp_path / 'o')]
    a = cli.build_parser().get_args(base + ['--input', 'a.wav'])
    assert a.resample is False and a.output_rate is None and a.input_rate is None
    a = cli.build_parser().get_args(base + ['--input', 'a.wav', '--resample', '--output_rate', '8000', '--input_rate', '16000'])
    assert a.resample is True and a.output_rate == 8000 and a.input_rate == 16000

    rng = np.random.RandomState(6)
    pcm = rng.randint(-32768, 32768, size=(500, 2)).astype(np.int16)
    wrong = str(tmp_path / 'wrong.wav')
    _write_wav(wrong, pcm[:, 0], 16000)
    stereo = str(tmp_path / 'stereo.wav')
    _write_wav(stereo, pcm, config.fs, channels=2)
    # without --resample: today's refusals, with today's messages, from read_wav and from main
    with pytest.raises(SystemExit) as e:
        cli.read_wav(wrong)
    assert 'sample rate' in str(e.value) and '16000' in str(e.value) and 'nothing here resamples' in str(e.value)
    with pytest.raises(SystemExit) as e:
        cli.main(base + ['--input', wrong])
    assert 'sample rate of 16000 Hz' in str(e.value) and 'nothing here resamples' in str(e.value)
    with pytest.raises(SystemExit) as e:
        cli.main(base + ['--input', stereo])
    assert 'has 2 channels: one channel only' in str(e.value)

    three = str(tmp_path / 'three.wav')
    pcm3 = rng.randint(-32768, 32768, size=(321, 3)).astype(np.int16)
    pcm3[0] = (-32768, 32767, 0)
    _write_wav(three, pcm3, 44100, channels=3)
    got, fs = cli.read_recording(three)
    assert fs == 44100 and got.dtype == np.int16 and got.shape == (321, 3) and np.array_equal(got, pcm3)
    got, fs = cli.read_recording(wrong)
    assert fs == 16000 and got.shape == (500, 1) and np.array_equal(got[:, 0], pcm[:, 0])
    nine = str(tmp_path / 'nine.wav')
    _write_wav(nine, np.zeros((10, 9), np.int16), 16000, channels=9)
    with pytest.raises(SystemExit) as e:
        cli.read_recording(nine)
    assert 'channels' in str(e.value)
    bytes1 = str(tmp_path / 'bytes1.wav')
    with wave.open(bytes1, 'wb') as w:
        w.setnchannels(1)
        w.setsampwidth(1)
        w.setframerate(16000)
        w.writeframes(bytes(10))
    with pytest.raises(SystemExit) as e:
        cli.read_recording(bytes1)
    assert '16-bit PCM' in str(e.value)

    # refused before a model is built (the model folder does not exist): .npy needs --input_rate; a ratio outside the limits
    npy = str(tmp_path / 'x.npy')
    np.save(npy, np.zeros(100, np.float32))
    with pytest.raises(SystemExit) as e:
        cli.main(base + ['--input', npy, '--resample'])
    assert '--input_rate' in str(e.value)
    odd = str(tmp_path / 'odd.wav')
    _write_wav(odd, pcm[:, 0], 22051)
    with pytest.raises(SystemExit) as e:
        cli.main(base + ['--input', odd, '--resample'])
    assert '%d / 22051' % config.fs in str(e.value)
    with pytest.raises(SystemExit) as e:
        cli.main(base + ['--input', wrong, '--resample', '--output_rate', '22051'])
    assert '22051' in str(e.value)
    with pytest.raises(SystemExit) as e:                               # the new flags mean nothing without --resample
        cli.main(base + ['--input', wrong, '--output_rate', '16000'])
    assert '--resample' in str(e.value)


def test_resample_kernels_compile_for_gfx950_without_scratch():
    """tools/kernel_resources.py on csrc/resample/resample.hip with the library's flags: both arms for both kinds of input and the
    decode-only kernel, no scratch, no spill, no warning; LDS in the decimating arm only (16 KB)."""
    run = subprocess.run([sys.executable, os.path.join(ROOT, 'tools', 'kernel_resources.py'),
                          os.path.join(PKG, 'csrc', 'resample', 'resample.hip')], capture_output=True, text=True, check=True)
    assert 'warning' not in run.stderr
    rows = [ln.split() for ln in run.stdout.splitlines()[1:] if ln.strip()]
    names = ' '.join(' '.join(r) for r in rows)
    for k in ('decimate_kernel<Pcm16Source>', 'decimate_kernel<F32Source>', 'interpolate_kernel<Pcm16Source>',
              'interpolate_kernel<F32Source>', 'decode_kernel'):
        assert k in names, k
    assert len(rows) == 5
    for r in rows:
        vgpr, agpr, spill, scratch, occ, lds = r[-6:]
        assert spill == '0' and scratch == '0', r
        assert lds == ('16384' if 'decimate_kernel' in ' '.join(r) else '0'), r
