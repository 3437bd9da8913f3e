"""CPU: the DANet-SCE separator (reference models/SC_V2.py) -- the float64 restatement of its reconstruction term against finite
differences, the host mirror's imports and entry points against the reference's scripts, and the flag pair the reference's graph
cannot build.  No kernel is launched."""
import importlib
import json
import os
import tempfile

import numpy as np
import pytest

os.environ.setdefault('AMS_LOG_DIR', tempfile.mkdtemp(prefix='ams_log_'))

from tests import danet_ref as R


def _case(kind, seed=3, B=2, T=5, Fq=4, E=3, S=2):
    rng = np.random.RandomState(seed)
    V = rng.standard_normal((B, T, Fq, E))
    X = rng.uniform(-1.0, 1.0, (B, T, Fq))
    X_nm = rng.uniform(-1.0, 1.0, (B, T, Fq, S))
    am = rng.randint(0, S, (B, T, Fq))
    y = np.where(am[..., None] == np.arange(S), 1.0, -1.0)
    mask = None
    if kind == 'fractional':
        y = y * rng.uniform(0.0, 1.0, (B, T, Fq))[..., None]                 # network.py:381-389 weights
    elif kind == 'silence':
        mask = R.silence_mask(X, 0.5)
        assert 0 < mask.sum() < mask.size
    elif kind == 'empty_speaker':
        y[0, :, :, 0], y[0, :, :, 1] = -1.0, 1.0                             # speaker 0 owns no bin of utterance 0
    return V, R.soft_masks(y, mask), X, X_nm


@pytest.mark.parametrize('kind', ['binary', 'fractional', 'silence', 'empty_speaker'])
def test_reconstruction_gradient_against_central_differences(kind):
    V, m, X, X_nm = _case(kind)
    if kind == 'empty_speaker':
        assert m[0, :, :, 0].sum() == 0.0
    dV = R.recon_cost_bwd(V, m, X, X_nm)
    num = np.zeros_like(V)
    h = 1e-6
    it = np.nditer(V, flags=['multi_index'])
    for _ in it:
        i = it.multi_index
        Vp, Vm = V.copy(), V.copy()
        Vp[i] += h
        Vm[i] -= h
        num[i] = (R.recon_cost(Vp, m, X, X_nm) - R.recon_cost(Vm, m, X, X_nm)) / (2 * h)
    # central differences in float64: truncation h^2 f''' ~ 1e-12, rounding eps / h ~ 1e-10 of the cost
    assert np.abs(dV - num).max() < 1e-8 * max(1.0, np.abs(dV).max()) + 2e-9, np.abs(dV - num).max()
    assert np.abs(dV).max() > 1e-4


def test_total_cost_is_the_sum_of_its_terms_and_uses_normalised_embeddings():
    rng = np.random.RandomState(5)
    V, m, X, X_nm = _case('binary')
    B, S, E = V.shape[0], m.shape[-1], V.shape[-1]
    y = 2.0 * m - 1.0
    spk = rng.standard_normal((7, E))
    I = np.array([[1, 4], [6, 2]])
    tot, (sc, rc), dV, dspk = R.sc_v2_cost(V, y, None, X, X_nm, spk, I)
    assert abs(tot - (sc + rc)) < 1e-15 and sc > 0 and rc > 0
    tot2, (sc2, rc2) = R.sc_v2_cost(3.0 * V, y, None, X, X_nm, spk, I, want_grads=False)
    assert abs(sc2 - sc) < 1e-12 and abs(rc2 - rc) > 1e-6              # scale-free contrastive term, scale-dependent reconstruction
    assert dspk.shape == spk.shape and dV.shape == V.shape


def test_modules_import_without_a_gpu():
    m = importlib.import_module('models.SC_V2')
    assert m.L41ModelV2.__mro__[1].__name__ == 'Separator'
    for name in ('STFT_L41V2', 'front_L41V2'):
        importlib.import_module('experiments.training.' + name)


def _cli_golden():
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'cli.json')) as f:
        return json.load(f)


def test_the_two_entry_points_are_the_reference_scripts():
    from experiments.training import _recipes as Rc
    gold = _cli_golden()['scripts']
    assert set(Rc.EXTRA_RECIPES) == {'STFT_L41V2', 'front_L41V2'} and not set(Rc.EXTRA_RECIPES) & set(Rc.RECIPES)
    assert set(gold) - set(Rc.RECIPES) - set(Rc.EXTRA_RECIPES) == {'front_focus', 'front_mm'}
    for name, (trainer, sep, typ, need_folder, has_prev, groups, pre) in Rc.EXTRA_RECIPES.items():
        g = gold[name]
        assert g['construct']['trainer'] == trainer and g['calls'] == ['train'], name
        assert g['construct']['args'] == [sep, typ], name
        assert g['construct']['kwargs'] == ({} if pre is None else {'pretraining': pre}), name
        assert g['separator_import'] == {'module': 'models.SC_V2', 'names': [sep]}, name
        assert tuple(m[len('add_'):-len('_args')] for m in g['groups']) == groups, name
        inline = {f['flags'][0]: f for f in g['inline_flags']}
        assert set(inline) == ({'--model_folder'} if need_folder is not None else set()) | ({'--model_previous'} if has_prev else set()), name
        assert inline['--model_folder'].get('required', False) == need_folder, name
        acts = {a.option_strings[0]: a for a in Rc.build_parser(name).parser._actions if a.option_strings}
        for flag, f in inline.items():
            assert acts[flag].required == f.get('required', False) and acts[flag].default == f.get('default'), (name, flag)
    assert {(v[1], v[2]) for v in Rc.EXTRA_RECIPES.values()} == {('L41ModelV2', 'STFT_DANet_SCE'), ('L41ModelV2', 'front_DANet_SCE')}


def _args(**kw):
    from ams_hip import testing
    a = dict(testing.ADAPT_DEFAULTS)
    a.update(testing.SEPARATOR_DEFAULTS)
    a.update(testing.ENHANCE_DEFAULTS)
    a.update(kw)
    a.pop('type', None)
    return a


def _stft_trainer(**kw):
    from models.SC_V2 import L41ModelV2
    from utils.trainer import STFT_Separator_Trainer
    a = _args(batch_size=2, nb_speakers=2, chunk_size=2048, window_size=64, hop_size=32, layer_size=12, nb_layers=2, embedding_size=8,
              model_folder=None, learning_rate=1e-3, **kw)
    tr = STFT_Separator_Trainer(L41ModelV2, 'STFT_DANet_SCE', **a)
    tr.prepare()
    return tr


def test_make_trainer_builds_the_v2_separator():
    from experiments.training import _recipes as Rc
    from models.SC_V2 import L41ModelV2
    tr = Rc.make_trainer('STFT_L41V2', ['--dataset', 'synthetic', '--batch_size', '2', '--chunk_size', '2048', '--window_size', '64',
                                        '--hop_size', '32', '--layer_size', '12', '--nb_layers', '2', '--embedding_size', '8'])
    assert tr.separator is L41ModelV2 and type(tr).__name__ == 'STFT_Separator_Trainer'
    assert tr.args['type'] == 'STFT_DANet_SCE'


@pytest.mark.parametrize('no_normalize', [True, False])
def test_construction_names_match_l41model(no_normalize):
    """Same variable names as L41Model (checkpoints interchange); no Normalize layer whatever --no_normalize says; the summaries."""
    tr = _stft_trainer(no_normalize=no_normalize)
    g, model = tr.graph, tr.model
    names = list(g.variables)
    assert 'speaker_centroids' in names and g.variables['speaker_centroids'].shape == (251, 8)
    assert 'prediction/W' in names and 'prediction/forward_BLSTM_1/rnn/basic_lstm_cell/kernel' in names
    assert model._embed_normalized is False
    for k in ('cost/reconstruction_loss/value', 'cost/source_contrastive_loss/value', 'cost/total', 'cost/cost'):
        assert k in g.summaries, k
    sd = np.sqrt(2.0 / 8)
    spk = g.variables['speaker_centroids'].detach().cpu().numpy()
    assert np.abs(spk).max() <= 2 * sd + 1e-6 and 0.7 * sd < spk.std() < 1.1 * sd

    from models.L41 import L41Model
    from utils.trainer import STFT_Separator_Trainer
    a = _args(batch_size=2, nb_speakers=2, chunk_size=2048, window_size=64, hop_size=32, layer_size=12, nb_layers=2, embedding_size=8,
              model_folder=None, learning_rate=1e-3)
    ref = STFT_Separator_Trainer(L41Model, 'STFT_L41', **a)
    ref.prepare()
    assert {n: tuple(v.shape) for n, v in ref.graph.variables.items()} == {n: tuple(v.shape) for n, v in g.variables.items()}


def test_add_dilated_with_silence_loss_is_refused():
    with pytest.raises(ValueError, match='add_dilated'):
        _stft_trainer(add_dilated=True, silence_loss=True)
    _stft_trainer(add_dilated=True)                       # each flag alone builds
    _stft_trainer(silence_loss=True)


def test_danet_kernels_compile_for_gfx950_without_scratch():
    """tools/kernel_resources.py on csrc/danet.hip: every kernel variant of the loss chain keeps its state in registers and LDS."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, os.path.join(root, 'tools', 'kernel_resources.py'),
                          os.path.join(root, 'adaptive-multispeaker-separation_amd', 'csrc', 'danet.hip')],
                         capture_output=True, text=True, check=True).stdout.splitlines()
    rows = [ln.split() for ln in out[1:] if 'danet_' in ln]
    names = ' '.join(ln for ln in out[1:])
    for k in ('danet_attr_kernel<40, true>', 'danet_recon_kernel<40, true, true>', 'danet_recon_kernel<8, false, true>',
              'danet_bwd_kernel<true, true>', 'danet_reduce_kernel', 'danet_xmax_kernel'):
        assert k in names, k
    assert len(rows) >= 40
    for r in rows:
        vgpr, agpr, spill, scratch, occ, lds = r[-6:]
        assert spill == '0' and scratch == '0', r
        assert int(lds) <= 64 * 1024, r                      # at least two workgroups per CU
