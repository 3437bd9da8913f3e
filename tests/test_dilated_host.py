"""CPU: --add_dilated (reference models/network.py:445-446, 527-551) -- graph construction, variable names / order / shapes /
initial values, the first BLSTM's input width, the front path ignoring the flag, and checkpoint round trips.  No kernel is launched."""
import os
import tempfile

import numpy as np
import pytest

os.environ.setdefault('AMS_LOG_DIR', tempfile.mkdtemp(prefix='ams_log_'))

# (kernel [kh, kw], cin, cout) of dilated/Conv, dilated/Conv_1 .. dilated/Conv_12 (network.py:537-549)
SPECS = [((1, 7), 1, 128), ((7, 1), 128, 128)] + [((5, 5), 128, 128)] * 10 + [((5, 5), 128, 4)]
NAMES = ['dilated/Conv'] + ['dilated/Conv_%d' % i for i in range(1, 13)]


def _args(**kw):
    from ams_hip import testing
    a = dict(testing.ADAPT_DEFAULTS)
    a.update(testing.SEPARATOR_DEFAULTS)
    a.update(testing.ENHANCE_DEFAULTS)
    a.update(kw)
    a.pop('type', None)
    return a


def _stft(model_cls, name, W=64, hop=32, L=2048, LS=12, NL=2, E=8, **kw):
    from utils.trainer import STFT_Separator_Trainer
    a = _args(batch_size=2, nb_speakers=2, chunk_size=L, window_size=W, hop_size=hop, layer_size=LS, nb_layers=NL,
              embedding_size=E, model_folder=None, learning_rate=1e-3, add_dilated=True, **kw)
    tr = STFT_Separator_Trainer(model_cls, name, **a)
    tr.prepare()
    return tr


def _dpcl():
    from models.dpcl import DPCL
    return DPCL


def _l41():
    from models.L41 import L41Model
    return L41Model


@pytest.mark.parametrize('which', ['STFT_DPCL', 'STFT_L41'])
def test_stft_recipes_build_the_dilated_stack(which):
    W, LS = 64, 12
    Fq = W // 2 + 1
    tr = _stft(_dpcl() if which == 'STFT_DPCL' else _l41(), which, W=W, LS=LS)
    g, model = tr.graph, tr.model
    names = list(g.variables)
    want = [n + s for n in NAMES for s in ('/weights', '/biases')]
    dil = [n for n in names if n.startswith('dilated/')]
    assert dil == want                                       # creation order = tf.global_variables() order
    first_pred = min(i for i, n in enumerate(names) if n.startswith('prediction/'))
    assert max(names.index(n) for n in want) < first_pred    # created before prediction's
    for n, (kernel, cin, cout) in zip(NAMES, SPECS):
        w = g.variables[n + '/weights'].detach().cpu().numpy()
        b = g.variables[n + '/biases'].detach().cpu().numpy()
        assert w.shape == (kernel[0], kernel[1], cin, cout) and b.shape == (cout,), n
        assert not b.any(), n
        rf = kernel[0] * kernel[1]
        lim = np.sqrt(6.0 / (rf * cin + rf * cout))           # xavier_initializer(uniform=True)
        assert np.abs(w).max() <= lim and np.abs(w).max() > 0.9 * lim, n
    # BLSTM_0 reads 4 channels per frequency
    assert g.variables['prediction/forward_BLSTM_0/rnn/basic_lstm_cell/kernel'].shape == (4 * Fq + LS // 2, 4 * (LS // 2))
    assert g.variables['prediction/forward_BLSTM_1/rnn/basic_lstm_cell/kernel'].shape == (LS + LS // 2, 4 * (LS // 2))
    trainable = set(v.ams_name for v in model.trainable_variables)
    assert set(want) <= trainable
    assert g.get_tensor_by_name('dilated/output:0') is model.X


def test_stft_recipe_without_the_flag_is_unchanged():
    from utils.trainer import STFT_Separator_Trainer
    a = _args(batch_size=2, nb_speakers=2, chunk_size=2048, window_size=64, hop_size=32, layer_size=12, nb_layers=2, embedding_size=8,
              model_folder=None, learning_rate=1e-3)
    tr = STFT_Separator_Trainer(_dpcl(), 'STFT_DPCL', **a)
    tr.prepare()
    assert not any(n.startswith('dilated/') for n in tr.graph.variables)
    assert tr.graph.variables['prediction/forward_BLSTM_0/rnn/basic_lstm_cell/kernel'].shape == (33 + 6, 24)


def test_front_recipe_ignores_the_flag(tmp_path):
    from tests.smoke_step import build_front_dpcl
    trainer, tfds = build_front_dpcl(str(tmp_path), B=2, L=256, W=32, N=8, hop=8, layer_size=8, nb_layers=2, E=4, add_dilated=True)
    g = trainer.graph
    assert not any(n.startswith('dilated/') for n in g.variables)
    assert g.variables['prediction/forward_BLSTM_0/rnn/basic_lstm_cell/kernel'].shape == (8 + 4, 16)


def test_save_restore_round_trip_keeps_the_stack_bit_for_bit():
    tr = _stft(_dpcl(), 'STFT_DPCL')
    g, model = tr.graph, tr.model
    with g.as_default():
        for i, n in enumerate(NAMES):                        # non-trivial biases too
            b = g.variables[n + '/biases']
            b.data.copy_(b.new_tensor(np.arange(b.numel()) * 0.1 + i))
        before = {n: v.detach().cpu().numpy().copy() for n, v in g.variables.items() if n.startswith('dilated/')}
        assert set(before) <= set(model.saver)
        model.save(3)
        for n in before:
            g.variables[n].data.add_(1.0)
        model.restore_last_checkpoint()
        for n, v in before.items():
            assert np.array_equal(v, g.variables[n].detach().cpu().numpy()), n


def test_tf_checkpoint_writer_reader_round_trip_of_the_stack(tmp_path):
    from ams_hip import tf_checkpoint as tfc
    tr = _stft(_l41(), 'STFT_L41')
    g = tr.graph
    arrays = {n: v.detach().cpu().numpy() for n, v in g.variables.items()}
    prefix = str(tmp_path / 'model-5')
    tfc.write_bundle(prefix, arrays)
    back = tfc.read_bundle(prefix)
    for n in NAMES:
        for s in ('/weights', '/biases'):
            assert back[n + s].dtype == np.float32 and np.array_equal(back[n + s], arrays[n + s]), n + s
    # and the model restores the stack from a TF-layout folder under the graph's own names
    with open(str(tmp_path / 'checkpoint'), 'w') as f:
        f.write('model_checkpoint_path: "model-5"\n')
    with g.as_default():
        for n in NAMES:
            g.variables[n + '/weights'].data.zero_()
        tr.model.restore_model(str(tmp_path))
        for n in NAMES:
            assert np.array_equal(g.variables[n + '/weights'].detach().cpu().numpy(), arrays[n + '/weights']), n


def test_the_flag_is_saved_with_the_params():
    """Network.load takes add_dilated from the saved params: an _enhance / _finetuning / inference stage rebuilds the stack
    (tests/test_gpu_dilated_recipes.py builds one)."""
    import json
    tr = _stft(_dpcl(), 'STFT_DPCL')
    params = json.load(open(os.path.join(tr.model._dir(), 'params')))
    assert params['add_dilated'] is True
