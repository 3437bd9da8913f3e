"""GPU: many recordings through a model in one call -- Network.separate_recordings (models/network.py) on the tiny
Front_Separator_Inference of tests/test_gpu_separate_recording.py (B = 2, L = 2048), with and without resampling, the refusals, and the
command line experiments/evaluation/separate_many.py."""
import os
import tempfile
import wave

import numpy as np
import pytest

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

from tests.test_gpu_recipes import base_args
from tests.test_gpu_separate_recording import B, HOP, L, NF, S, STEPS, TRIES, W, _front, _recording

LENGTHS = [4396, 1000, 3300]    # 4 + 1 + 3 chunks: four passes of two, where one recording at a time takes 2 + 1 + 2


def _counting(model):
    """Count the model passes: every one goes through Network._eval_guarded.  Returns (calls, undo)."""
    calls, orig = [], model._eval_guarded

    def counted(*a, **k):
        calls.append(1)
        return orig(*a, **k)
    model._eval_guarded = counted
    return calls, lambda: model.__dict__.pop('_eval_guarded')


@pytest.mark.parametrize('beta', [None, 5.0])
def test_separate_recordings_is_chunks_many_infer_stitch_many(beta):
    from ams_hip import stitch_batch as sb
    tr, tfds, _ = _front(beta)
    model = tr.model
    xs = [torch.from_numpy(_recording(N, 20 + r)).cuda() for r, N in enumerate(LENGTHS)]
    with tr.graph.as_default():
        calls, undo = _counting(model)
        try:
            outs = model.separate_recordings(xs)
        finally:
            undo()
        mix, lay = sb.chunks_many(xs, L, L // 2, S)
        assert lay.C.tolist() == [4, 1, 3] and mix.shape == (8, L)
        assert len(calls) == -(-lay.Ctot // B) == 4               # ceil(Ctot / B) model passes, not one or more per recording
        est = model.infer_chunks(mix)
        parts = sb.stitch_many(est, lay)
        host = model.separate_recordings([x.cpu().numpy() for x in xs])     # numpy in: packed on the host, uploaded once
    assert isinstance(outs, list) and len(outs) == len(parts) == len(host) == 3
    for out, (want, trk, Q), again, N in zip(outs, parts, host, LENGTHS):
        assert out.shape == (S, N) and out.is_cuda and bool(torch.isfinite(out).all())
        assert torch.equal(out, want) and torch.equal(out, again)


@pytest.mark.parametrize('beta', [None, 5.0])
@pytest.mark.parametrize('N', [4396, 3300])
def test_one_recording_is_separate_recording(beta, N):
    """R = 1: every chunk sits in the batch row it has in separate_recording, so the k-means seeds coincide and the result is the same
    bit for bit (for several recordings it is not: a chunk's row is its place in the stream)."""
    tr, tfds, _ = _front(beta)
    x = torch.from_numpy(_recording(N)).cuda()
    with tr.graph.as_default():
        many = tr.model.separate_recordings([x])
        one = tr.model.separate_recording(x)
    assert len(many) == 1 and many[0].shape == (S, N) and torch.equal(many[0], one)


def test_int16_stereo_frames_at_16_khz():
    import config
    from ams_hip import resample as Rs
    from ams_hip import stitch_batch as sb
    tr, tfds, _ = _front(None)
    model = tr.model
    fs = 16000
    rng = np.random.RandomState(31)
    frames = [rng.randint(-9000, 9000, size=(N, 2)).astype(np.int16) for N in (7001, 2100, 5000)]
    with tr.graph.as_default():
        outs = model.separate_recordings(frames, fs=fs)
        low = model.separate_recordings([torch.from_numpy(f).cuda() for f in frames], fs=fs, output_fs=config.fs)
        ys = [Rs.from_pcm16(torch.from_numpy(f).cuda(), fs, config.fs) for f in frames]
        mix, lay = sb.chunks_many(ys, L, L // 2, S)
        parts = [p[0] for p in sb.stitch_many(model.infer_chunks(mix), lay)]
        for out, at8k, part, f, y in zip(outs, low, parts, frames, ys):
            N = f.shape[0]
            assert part.shape == (S, y.shape[0]) and torch.equal(at8k, part)
            want = Rs.resample(part.contiguous(), config.fs, fs)
            n_out = -((-N * fs) // fs)
            assert n_out == N <= want.shape[1]
            assert out.shape == (S, N) and torch.equal(out, want[:, :N]) and bool(torch.isfinite(out).all())


def test_refusals():
    from ams_hip import testing
    from utils.trainer import Pretrained_Inference
    tr, tfds, _ = _front(None)
    x = _recording(3000)
    with tr.graph.as_default():
        m = tr.model
        for bad, word in (([], 'empty'), ([np.zeros((2, 3000), np.float32)], 'float32'), ([x.astype(np.float64)], 'float32'),
                          ([x, np.zeros((3000, 1), np.int16)], 'one dtype'), ([x, np.zeros(0, np.float32)], 'at least one sample'),
                          (torch.from_numpy(x), 'a list'), (x, 'a list'), ([np.zeros((10, 2, 2), np.int16)], 'int16')):
            with pytest.raises(ValueError, match=word):
                m.separate_recordings(bad)
        for hop in (L // 2 - 1, L):
            with pytest.raises(ValueError, match='hop'):
                m.separate_recordings([x], hop=hop)
        with pytest.raises(ValueError):
            m.separate_recordings([x], fs=12345)                   # a ratio the resampler does not take
    tmp = tempfile.mkdtemp(prefix='ams_prec_many_')
    folder, params = testing.make_pretrained_adapt(os.path.join(tmp, 'pre'), window_size=W, filters=NF, hop_size=HOP, chunk_size=L,
                                                   batch_size=B, nb_speakers=S)
    a = base_args(**params)
    a.update(model_folder=folder, out=False)
    a.pop('type')
    pre = Pretrained_Inference(None, 'pretrained_inference', **a)
    model = pre.prepare_inference()
    with pre.graph.as_default():
        with pytest.raises(ValueError, match='clean sources'):
            model.separate_recordings([x])
    from experiments.evaluation import separate_many as cli
    with pytest.raises(SystemExit) as e:
        cli.main(['--model_folder', folder, '--sortofmodel', 'pretraining', '--inputs', 'x.wav', '--output_dir', tmp])
    assert 'pretraining' in str(e.value)


def test_command_line_turns_two_wavs_into_wavs():
    import config
    from experiments.evaluation import separate as one
    from experiments.evaluation import separate_many as cli
    _, _, folder = _front(None)
    tmp = tempfile.mkdtemp(prefix='ams_cli_many_')
    lengths = {'first': 3300, 'second': 1500}
    for r, (stem, N) in enumerate(lengths.items()):
        one.write_wav(os.path.join(tmp, stem + '.wav'), _recording(N, 40 + r))
    out_dir = os.path.join(tmp, 'out')
    paths = cli.main(['--model_folder', folder, '--sortofmodel', 'front_DPCL', '--inputs', os.path.join(tmp, 'first.wav'),
                      os.path.join(tmp, 'second.wav'), '--output_dir', out_dir, '--chunk_size', str(L), '--batch_size', str(B),
                      '--nb_speakers', str(S), '--nb_tries', str(TRIES), '--nb_steps', str(STEPS), '--hop', '1280', '--no_summaries'])
    assert paths == [os.path.join(out_dir, '%s_%d.wav' % (stem, k)) for stem in lengths for k in range(S)] and len(paths) == 2 * S
    for p in paths:
        N = lengths[os.path.basename(p).split('_')[0]]
        with wave.open(p, 'rb') as w:
            assert (w.getnchannels(), w.getsampwidth(), w.getframerate(), w.getnframes()) == (1, 2, config.fs, N)
        assert np.abs(one.read_wav(p)).max() > 0
