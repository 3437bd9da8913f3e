"""GPU: whole recordings through a model -- Network.infer_chunks / separate_recording (models/network.py) on the tiny
Front_Separator_Inference set-up of tests/test_gpu_recipes.py::test_front_separator_inference, one STFT recipe, the refusals, and the
command line (experiments/evaluation/separate.py) on a checkpoint written by testing.write_checkpoint."""
import os
import tempfile
import wave

import numpy as np
import pytest

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

from tests.test_gpu_recipes import INFER_TOL, _full_checkpoint, base_args

B, S, L, W, NF, HOP, LS, NL, E, TRIES, STEPS = 2, 2, 2048, 64, 16, 16, 12, 2, 8, 2, 3
_MODELS = {}


def _front(beta):
    """One Front_Separator_Inference per k-means flavour, shared by the tests below (built once, never modified)."""
    if beta not in _MODELS:
        from models.dpcl import DPCL
        from utils.trainer import Front_Separator_Inference
        tmp = tempfile.mkdtemp(prefix='ams_rec_')
        rng = np.random.RandomState(11)
        folder, params, P = _full_checkpoint(tmp, rng, W, NF, HOP, L, B, S, LS, NL, E, NF, NF)
        T = -(-L // HOP)
        idx = np.stack([rng.choice(T * NF, S, replace=False) for _ in range(B * TRIES)]).astype(np.int32)
        a = base_args(**params)
        a.update(model_folder=folder, nb_tries=TRIES, nb_steps=STEPS, beta_kmeans=beta, with_silence=beta is not None, end_assign=True,
                 kmeans_init_indices=idx, out=False)
        a.pop('type')
        tr = Front_Separator_Inference(DPCL, 'front_DPCL_inference', **a)
        dist, tfds = tr.prepare()
        _MODELS[beta] = (tr, tfds, folder)
    return _MODELS[beta]


def _recording(N, seed=3):
    return (0.3 * np.random.RandomState(seed).randn(N)).astype(np.float32)


@pytest.mark.parametrize('beta', [None, 5.0])
@pytest.mark.parametrize('N,C', [(4396, 4), (3300, 3)])          # two full batches; a last batch padded by repetition
def test_separate_recording_is_chunks_infer_stitch(beta, N, C):
    from ams_hip import stitch
    tr, tfds, _ = _front(beta)
    model = tr.model
    x = torch.from_numpy(_recording(N)).cuda()
    with tr.graph.as_default():
        out = model.separate_recording(x)
        mix = stitch.chunks(x, L, L // 2)
        assert mix.shape == (C, L)
        est = model.infer_chunks(mix)
        parts = stitch.stitch(est, N, L // 2)[0]
        again = model.separate_recording(x.cpu().numpy())         # numpy in, and a second call
    assert est.shape == (C, S, L)
    assert out.shape == (S, N) and bool(torch.isfinite(out).all())
    assert torch.equal(out, parts)
    assert torch.equal(out, again)
    if C % B:
        # the last batch was the last chunk and a copy of it: the copy is dropped, the chunk is what that batch gives (row 1 of the
        # batch draws other k-means seeds than row 0 -- kmeans_init_indices has a row per batch row and try -- so only row 0 compares)
        with tr.graph.as_default():
            last = model.infer_chunks(torch.cat([mix[-1:], mix[-1:]]))
        assert last.shape == (2, S, L) and torch.equal(last[0], est[-1])


@pytest.mark.parametrize('beta', [None, 5.0])
def test_short_recording_is_one_padded_chunk(beta):
    tr, tfds, _ = _front(beta)
    N = 1500
    x = torch.from_numpy(_recording(N, 4)).cuda()
    pad = torch.zeros(1, L, device='cuda')
    pad[0, :N] = x
    with tr.graph.as_default():
        out = tr.model.separate_recording(x)
        est = tr.model.infer_chunks(pad)
    assert out.shape == (S, N) and torch.equal(out, est[0, :, :N])


@pytest.mark.parametrize('beta', [None, 5.0])
def test_infer_chunks_agrees_with_infer(beta):
    """The inference output path reads neither the clean sources nor the speaker indices: zeros in their place give what the dataset's
    batch gives.  A tolerance, not bit equality: the fp16x3 operand bound of the front product is taken over all staged rows, and
    those differ (clean sources there, zeros here)."""
    tr, tfds, _ = _front(beta)
    with tr.graph.as_default():
        feed = {tfds.handle: tfds.get_handle(tfds.TEST), tfds.chunk_size: L}
        xm, xn, out = tr.model.infer(feed, 0)
        xm, out = xm.clone(), out.clone()
        est = tr.model.infer_chunks(xm)
    assert est.shape == out.shape == (B, S, L)
    err = float((est - out).norm() / out.norm())
    print('infer_chunks vs infer: relative L2 %.3g' % err)
    assert err < INFER_TOL, err


def test_stft_recipe_separates_a_recording():
    from models.dpcl import DPCL
    from utils.trainer import STFT_Separator_Inference
    tmp = tempfile.mkdtemp(prefix='ams_srec_')
    rng = np.random.RandomState(12)
    Bs, W2, hop2 = 2, 64, 32
    Fq = W2 // 2 + 1
    folder, params, P = _full_checkpoint(tmp, rng, W2, None, hop2, L, Bs, S, LS, NL, E, Fq, Fq, front=False)
    T = 1 + (L - W2) // hop2
    idx = np.stack([rng.choice(T * Fq, S, replace=False) for _ in range(Bs * TRIES)]).astype(np.int32)
    a = base_args(**params)
    a.update(model_folder=folder, nb_tries=TRIES, nb_steps=STEPS, end_assign=True, kmeans_init_indices=idx, out=False)
    a.pop('type')
    tr = STFT_Separator_Inference(DPCL, 'STFT_DPCL_inference', **a)
    model = tr.prepare_inference()                                 # no dataset behind this one
    N = 3300
    with tr.graph.as_default():
        out = model.separate_recording(_recording(N, 5))
    assert out.shape == (S, N) and bool(torch.isfinite(out).all()) and float(out.abs().max()) > 0


def test_refusals():
    from ams_hip import testing
    from utils.trainer import Pretrained_Inference
    tmp = tempfile.mkdtemp(prefix='ams_prec_')
    folder, params = testing.make_pretrained_adapt(os.path.join(tmp, 'pre'), window_size=W, filters=NF, hop_size=HOP, chunk_size=L,
                                                   batch_size=B, nb_speakers=S)
    a = base_args(**params)
    a.update(model_folder=folder, out=False)
    a.pop('type')
    tr = Pretrained_Inference(None, 'pretrained_inference', **a)
    model = tr.prepare_inference()
    with tr.graph.as_default():
        with pytest.raises(ValueError, match='clean sources'):
            model.separate_recording(_recording(3000))
        with pytest.raises(ValueError, match='clean sources'):
            model.infer_chunks(torch.zeros(2, L, device='cuda'))
    # a model built for another chunk size; a hop outside ceil(L / 2) .. L - 1
    tr, tfds, _ = _front(None)
    with tr.graph.as_default():
        with pytest.raises(ValueError, match='chunk_size'):
            tr.model.infer_chunks(torch.zeros(2, L // 2, device='cuda'))
        for hop in (L // 2 - 1, L):
            with pytest.raises(ValueError, match='hop'):
                tr.model.separate_recording(_recording(3000), hop=hop)
    from experiments.evaluation import separate as cli
    with pytest.raises(SystemExit) as e:
        cli.main(['--model_folder', folder, '--sortofmodel', 'pretraining', '--input', 'x.wav', '--output_prefix', 'o'])
    assert 'pretraining' in str(e.value)


def test_command_line_turns_a_wav_into_wavs():
    import config
    from experiments.evaluation import separate as cli
    _, _, folder = _front(None)
    tmp = tempfile.mkdtemp(prefix='ams_cli_')
    N = 3300
    src = os.path.join(tmp, 'mix.wav')
    cli.write_wav(src, _recording(N, 6))
    paths = cli.main(['--model_folder', folder, '--sortofmodel', 'front_DPCL', '--input', src, '--output_prefix', os.path.join(tmp, 'out'),
                      '--chunk_size', str(L), '--batch_size', str(B), '--nb_speakers', str(S), '--nb_tries', str(TRIES),
                      '--nb_steps', str(STEPS), '--hop', '1280', '--no_summaries'])
    assert paths == [os.path.join(tmp, 'out_%d.wav' % k) for k in range(S)]
    for p in paths:
        with wave.open(p, 'rb') as w:
            assert (w.getnchannels(), w.getsampwidth(), w.getframerate(), w.getnframes()) == (1, 2, config.fs, N)
        assert np.abs(cli.read_wav(p)).max() > 0
