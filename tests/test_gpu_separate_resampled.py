"""GPU: whole recordings at another sample rate -- Network.separate_recording(x, fs=..., output_fs=...) against the public pieces put
together by hand (ams_hip.resample), the time alignment of a round trip through the kernels, and the command line's
--resample on a stereo 16 kHz file.  The model and its k-means seeding are those of tests/test_gpu_separate_recording.py."""
import os
import tempfile
import wave

import numpy as np
import pytest

from tests import resample_ref as ref

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

from tests.test_gpu_separate_recording import B, L, S, STEPS, TRIES, _front, _recording


def _n_for(fs, at_model_rate=3300):
    import config
    return at_model_rate * fs // config.fs + 1


@pytest.mark.parametrize('fs', [16000, 44100, 11025])
def test_fs_is_resample_separate_resample(fs):
    import config
    from ams_hip import resample
    tr, tfds, _ = _front(None)
    model = tr.model
    N = _n_for(fs)
    x = torch.from_numpy(_recording(N, 7)).cuda()
    with tr.graph.as_default():
        out = model.separate_recording(x, fs=fs)
        x8 = resample.resample(x, fs, config.fs)
        mid = model.separate_recording(x8)
        back = resample.resample(mid, config.fs, fs)
        at8 = model.separate_recording(x, fs=fs, output_fs=config.fs)
        from_numpy = model.separate_recording(x.cpu().numpy(), fs=fs)
    M = -(-N * config.fs // fs)
    assert x8.shape == (M,) and mid.shape == (S, M) and back.shape[1] >= N
    assert out.shape == (S, N) and out.is_contiguous() and bool(torch.isfinite(out).all()) and float(out.abs().max()) > 0
    assert torch.equal(out, back[:, :N])
    assert at8.shape == (S, M) and torch.equal(at8, mid)
    assert torch.equal(from_numpy, out)


def test_int16_frames_go_through_from_pcm16():
    import config
    from ams_hip import resample
    tr, tfds, _ = _front(None)
    model = tr.model
    N = _n_for(16000)
    rng = np.random.RandomState(8)
    pcm = rng.randint(-9000, 9000, size=(N, 2)).astype(np.int16)
    d = torch.from_numpy(pcm).cuda()
    with tr.graph.as_default():
        out = model.separate_recording(d, fs=16000)
        x8 = resample.from_pcm16(d, 16000, config.fs)
        mid = model.separate_recording(x8)
        back = resample.resample(mid, config.fs, 16000)
        from_numpy = model.separate_recording(pcm, fs=16000, output_fs=config.fs)
        same_rate = model.separate_recording(d[:3300], fs=config.fs)                   # decode and mix down only
        by_hand = model.separate_recording(resample.from_pcm16(d[:3300].contiguous(), config.fs, config.fs))
    assert out.shape == (S, N) and torch.equal(out, back[:, :N])
    assert torch.equal(from_numpy, mid)
    assert same_rate.shape == (S, 3300) and torch.equal(same_rate, by_hand)


def test_without_fs_nothing_changes():
    import config
    tr, tfds, _ = _front(None)
    x = torch.from_numpy(_recording(3300, 9)).cuda()
    with tr.graph.as_default():
        plain = tr.model.separate_recording(x)
        assert torch.equal(tr.model.separate_recording(x, fs=None), plain)
        assert torch.equal(tr.model.separate_recording(x, fs=config.fs), plain)
        assert torch.equal(tr.model.separate_recording(x, fs=config.fs, output_fs=config.fs), plain)
        with pytest.raises(ValueError, match='22051'):
            tr.model.separate_recording(x, fs=22051)
        with pytest.raises(ValueError, match='22051'):
            tr.model.separate_recording(x, fs=16000, output_fs=22051)


def test_round_trip_is_time_aligned():
    """16 kHz -> 8 kHz -> 16 kHz of 300 Hz + 1.1 kHz.  The restatement's round trip gives the signal back, sample for sample, away from
    the ends: a Kaiser window with beta 5.0 has 54 dB of stop-band attenuation (beta = 0.1102 (A - 8.7)), so a ripple of d = 2e-3 per
    stage, and two stages change a signal whose amplitudes add up to 0.5 by at most about 0.5 (2 d + images d) = 3e-3; a shift by one
    sample would change it by 0.25 * 2 pi 1100 / 16000 = 0.1.  The kernels are held to the restatement: within the second stage's
    bound plus the first stage's bound carried through the second filter."""
    from ams_hip import resample
    N = 4000
    t = np.arange(N) / 16000.0
    x = (0.25 * np.sin(2 * np.pi * 300 * t) + 0.25 * np.sin(2 * np.pi * 1100 * t)).astype(np.float32)
    r8 = ref.resample(x, 1, 2)
    r16 = ref.resample(r8, 2, 1)
    edge = 2 * 20                                                  # 2 half of the wider filter, in samples at 16 kHz
    figure = float(np.abs(r16[:N] - x)[edge:N - edge].max())
    print('restatement round trip: max |r16 - x| away from the ends = %.3g' % figure)
    assert r16.shape[0] >= N and figure <= 3e-3, figure
    d = torch.from_numpy(x).cuda()
    y8 = resample.resample(d, 16000, 8000)
    y16 = resample.resample(y8, 8000, 16000)
    assert y8.shape == r8.shape and y16.shape == r16.shape
    tol1 = ref.tolerance(x, 1, 2)
    assert np.all(np.abs(y8.cpu().numpy() - r8) <= tol1)
    tol = ref.tolerance(y8.cpu().numpy(), 2, 1) + ref.bound(tol1, 2, 1)
    err = np.abs(y16.cpu().numpy() - r16)
    print('kernels against the restatement: worst |y16 - r16| / bound = %.3f' % float((err / tol).max()))
    assert np.all(err <= tol)
    assert float(np.abs(y16.cpu().numpy()[:N] - x)[edge:N - edge].max()) <= figure + float(tol.max())


def _wav(path):
    with wave.open(path, 'rb') as w:
        meta = (w.getnchannels(), w.getsampwidth(), w.getframerate(), w.getnframes())
        return meta, np.frombuffer(w.readframes(w.getnframes()), '<i2')


def test_command_line_resamples_a_stereo_16k_file():
    from experiments.evaluation import separate as cli
    _, _, folder = _front(None)
    tmp = tempfile.mkdtemp(prefix='ams_cli_rs_')
    N = 6601
    rng = np.random.RandomState(10)
    pcm = np.clip(np.rint(0.3 * rng.randn(N, 2) * 32768), -32767, 32767).astype('<i2')
    src = os.path.join(tmp, 'mix.wav')
    with wave.open(src, 'wb') as w:
        w.setnchannels(2)
        w.setsampwidth(2)
        w.setframerate(16000)
        w.writeframes(pcm.tobytes())
    args = ['--model_folder', folder, '--sortofmodel', 'front_DPCL', '--input', src, '--chunk_size', str(L), '--batch_size', str(B),
            '--nb_speakers', str(S), '--nb_tries', str(TRIES), '--nb_steps', str(STEPS), '--no_summaries']
    paths = cli.main(args + ['--output_prefix', os.path.join(tmp, 'a'), '--resample'])
    assert paths == [os.path.join(tmp, 'a_%d.wav' % k) for k in range(S)]
    for p in paths:
        meta, got = _wav(p)
        assert meta == (1, 2, 16000, N) and np.abs(got).max() > 0
    paths = cli.main(args + ['--output_prefix', os.path.join(tmp, 'b'), '--resample', '--output_rate', '8000'])
    for p in paths:
        meta, got = _wav(p)
        assert meta == (1, 2, 8000, (N + 1) // 2) and np.abs(got).max() > 0
    with pytest.raises(SystemExit) as e:                           # without the flag: refused as before
        cli.main(args + ['--output_prefix', os.path.join(tmp, 'c')])
    assert 'has 2 channels: one channel only' in str(e.value) and not os.path.exists(os.path.join(tmp, 'c_0.wav'))
