"""GPU: L41ModelV2 (reference models/SC_V2.py) through the recipe classes its two entry scripts build --
experiments/training/STFT_L41V2.py -> STFT_Separator_Trainer(L41ModelV2, 'STFT_DANet_SCE'), front_L41V2.py ->
Front_Separator_Trainer(L41ModelV2, 'front_DANet_SCE', pretraining=False) -- whole training steps against the float64 restatement
in tests/danet_ref.py, replay against eager launches, and a V2 checkpoint restored into the inference recipe."""
import json
import os
import tempfile

import numpy as np
import pytest

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

from oracle import kmeans as okm, optim as ooptim, step as ostep, stft as ostft
from tests import danet_ref as R
from tests.test_gpu_recipes import base_args, one_train_step, check_step, _full_checkpoint
from tests.test_gpu_replay import _compare

os.environ.setdefault('AMS_LOG_DIR', tempfile.mkdtemp(prefix='ams_log_'))


def _stft_trainer(**kw):
    from models.SC_V2 import L41ModelV2
    from utils.trainer import STFT_Separator_Trainer
    B, S, L, W, hop, LS, NL, E = 4, 2, 2048, 64, 32, 12, 2, 8                 # the sizes of tests/test_gpu_cfg4.py::test_stft_l41_step
    a = base_args(batch_size=B, nb_speakers=S, chunk_size=L, window_size=W, hop_size=hop, layer_size=LS, nb_layers=NL,
                  embedding_size=E, model_folder=None, learning_rate=1e-3)
    a.update(kw)
    a.pop('type')
    tr = STFT_Separator_Trainer(L41ModelV2, 'STFT_DANet_SCE', **a)
    dist, tfds = tr.prepare()
    return tr, tfds, (L, W, hop, NL, E)


@pytest.mark.parametrize('no_normalize', [True, False])
def test_stft_l41v2_step(no_normalize):
    """|STFT| -> 2xBLSTM -> Conv1D -> source-contrastive + reconstruction cost, AMSGrad: cost, every gradient, the update.  The
    prediction has no Normalize layer whatever --no_normalize says: both settings are held to the same restatement."""
    tr, tfds, (L, W, hop, NL, E) = _stft_trainer(no_normalize=no_normalize)
    names = sorted(v.ams_name for v in tr.model.trainable_variables)
    assert 'speaker_centroids' in names and any(n.startswith('prediction/') for n in names)
    P, cost, xm, xn, I, grads, P_new = one_train_step(tr, tfds, L)
    assert P['speaker_centroids'].shape == (251, E)
    c_ref, g_ref, V, Y, (sc, rc) = R.stft_l41v2_loss(xm, xn, I, P, W, hop, NL, E)
    print('cost %.9g ref %.9g (contrastive %.6g + reconstruction %.6g)' % (cost, c_ref, sc, rc))
    assert set(np.unique(Y)) == {-1.0, 1.0}
    assert rc > 1e-3 * c_ref                                            # the reconstruction term is visible in the total
    check_step(cost, c_ref, grads, g_ref, P, P_new, ooptim.AMSGrad(1e-3))


def test_stft_l41v2_step_with_silence_loss():
    """--silence_loss --threshold_silence_loss 1.0: the mask log10(max|X| / |X|) < 1 weights y_ab and m (SC_V2.py:50-56)."""
    tr, tfds, (L, W, hop, NL, E) = _stft_trainer(silence_loss=True, threshold_silence_loss=1.0)
    P, cost, xm, xn, I, grads, P_new = one_train_step(tr, tfds, L)
    c_ref, g_ref, V, Y, (sc, rc) = R.stft_l41v2_loss(xm, xn, I, P, W, hop, NL, E, silence_thr=1.0)
    c_plain = R.stft_l41v2_loss(xm, xn, I, P, W, hop, NL, E, want_grads=False)[0]
    X = ostft.stft_preprocessing(xm, xn, W, hop)[0]
    frac = R.silence_mask(X, 1.0).mean()
    print('cost %.9g ref %.9g (without the mask %.9g); %.3f of the bins kept' % (cost, c_ref, c_plain, frac))
    assert 0.05 < frac < 0.95 and abs(c_ref - c_plain) > 1e-3 * c_plain
    check_step(cost, c_ref, grads, g_ref, P, P_new, ooptim.AMSGrad(1e-3))


def test_summaries_carry_the_two_terms_and_validation_runs_without_a_backward():
    tr, tfds, (L, W, hop, NL, E) = _stft_trainer()
    g, model = tr.graph, tr.model
    with g.as_default():
        feed = {tfds.handle: tfds.get_handle(tfds.TRAIN), tfds.chunk_size: L}
        cost = float(model.train(feed, 0))
        s = model._summaries(model.last_run, ['cost/reconstruction_loss/value', 'cost/source_contrastive_loss/value', 'cost/total',
                                              'cost/cost'])
        tfds.initialize(tfds.VALID)                                     # an evaluation pass: cost only, nothing kept for a backward
        v = model.valid_batch({tfds.handle: tfds.get_handle(tfds.VALID), tfds.chunk_size: L}, 0)
    assert np.isfinite(v) and 0.1 * cost < v < 10 * cost
    assert s['cost/total'] == s['cost/cost'] == cost
    assert abs(s['cost/reconstruction_loss/value'] + s['cost/source_contrastive_loss/value'] - cost) < 1e-6 * cost
    assert s['cost/reconstruction_loss/value'] > 0 and s['cost/source_contrastive_loss/value'] > 0


FRONT_GAIN = 25.0


def _front_trainer(function_mask='None', previous=False, **kw):
    from ams_hip import testing
    from models.SC_V2 import L41ModelV2
    from utils.trainer import Front_Separator_Trainer
    tmp = tempfile.mkdtemp(prefix='ams_v2_')
    B, S, L, W, N, hop, LS, NL, E = 3, 3, 1024, 64, 16, 16, 12, 2, 8            # tests/test_gpu_recipes.py::test_front_l41_step
    if previous:
        # a whole earlier run (front, back, prediction, speaker table) restored through --model_previous
        folder, params, _ = _full_checkpoint(tmp, np.random.RandomState(17), W, N, hop, L, B, S, LS, NL, E, N, N, tot_speakers=251)
        params['function_mask'] = function_mask                        # Network.load takes the separator's flags from the saved params
        with open(os.path.join(folder, 'params'), 'w') as f:
            json.dump(params, f)
        a = base_args(**params)
        a.update(model_folder=folder, model_previous=folder, pretraining=False, learning_rate=1e-3)
    else:
        folder, params = testing.make_pretrained_adapt(os.path.join(tmp, 'pre'), window_size=W, filters=N, hop_size=hop, chunk_size=L,
                                                       batch_size=B, nb_speakers=S)
        a = base_args(**params)
        a.update(layer_size=LS, nb_layers=NL, embedding_size=E, model_folder=folder, model_previous=None, pretraining=False,
                 learning_rate=1e-3, function_mask=function_mask)
    a.update(kw)
    a.pop('type')
    tr = Front_Separator_Trainer(L41ModelV2, 'front_DANet_SCE', **a)
    dist, tfds = tr.prepare()
    # the freshly initialised front emits |X| ~ 1e-2, which leaves the reconstruction cost at 1e-4 of the contrastive one: scale the
    # (frozen) analysis filters so that both terms and both gradients are visible in what check_step compares
    tr.graph.variables['front/bases/bases'].data.mul_(FRONT_GAIN)
    return tr, tfds, (L, hop, NL, E)


@pytest.mark.parametrize('previous', [True, False])
def test_front_l41v2_step(previous):
    """front_L41V2, S = 3: signed front representation in X_input / X_non_mix; only prediction/* and the speaker table train."""
    tr, tfds, (L, hop, NL, E) = _front_trainer(previous=previous)
    names = sorted(v.ams_name for v in tr.model.trainable_variables)
    assert 'speaker_centroids' in names and not any(n.startswith(('front/', 'back/')) for n in names)
    P, cost, xm, xn, I, grads, P_new = one_train_step(tr, tfds, L)
    c_ref, g_ref, V, Y, (sc, rc) = R.front_l41v2_loss(xm, xn, I, P, hop, NL, E)
    print('cost %.9g ref %.9g (contrastive %.6g + reconstruction %.6g)' % (cost, c_ref, sc, rc))
    assert rc > 1e-2 * c_ref
    check_step(cost, c_ref, grads, g_ref, P, P_new, ooptim.AMSGrad(1e-3))


def test_front_l41v2_step_with_function_mask_sqrt():
    """--function_mask sqrt: the base class hands over y sqrt(|X| / max|X|) (network.py:381-389), so m = (y + 1) / 2 is a general float
    weight in the attractor sums and in the backward."""
    tr, tfds, (L, hop, NL, E) = _front_trainer(function_mask='sqrt')
    P, cost, xm, xn, I, grads, P_new = one_train_step(tr, tfds, L)
    c_ref, g_ref, V, Y, (sc, rc) = R.front_l41v2_loss(xm, xn, I, P, hop, NL, E, function_mask='sqrt')
    c_plain = R.front_l41v2_loss(xm, xn, I, P, hop, NL, E, want_grads=False)[0]
    print('cost %.9g ref %.9g (unweighted masks %.9g)' % (cost, c_ref, c_plain))
    assert len(np.unique(np.round(Y, 6))) > 10 and abs(c_ref - c_plain) > 1e-3 * c_plain
    check_step(cost, c_ref, grads, g_ref, P, P_new, ooptim.AMSGrad(1e-3))


def test_stft_l41v2_replay_matches_eager():
    """--hip_graph: the loss chain holds no host synchronisation; the captured step replays with the costs and weights of eager launches."""
    def make(graph):
        tr, tfds, (L, W, hop, NL, E) = _stft_trainer(batch_size=3, pretraining=False, tot_speakers=251, hip_graph=graph, no_summaries=True,
                                                     silence_loss=True, threshold_silence_loss=1.0)
        return tr, tfds, L
    _compare(make)


def test_front_l41v2_replay_matches_eager():
    def make(graph):
        tr, tfds, (L, hop, NL, E) = _front_trainer(function_mask='linear', tot_speakers=251, hip_graph=graph, no_summaries=True)
        return tr, tfds, L
    _compare(make)


def test_replay_on_one_batch_repeats_the_eager_costs():
    """Several steps on ONE batch (synthetic_batches = 1), replayed against eager: the same costs step by step."""
    costs = {}
    for graph in (False, True):
        import utils.ops
        utils.ops.rng.seed(42)
        torch.manual_seed(0)
        tr, tfds, (L, W, hop, NL, E) = _stft_trainer(batch_size=3, hip_graph=graph, no_summaries=True, synthetic_batches=1, synthetic_pool=1)
        with tr.graph.as_default():
            feed = {tfds.handle: tfds.get_handle(tfds.TRAIN), tfds.chunk_size: L}
            tfds.initialize(tfds.TRAIN)
            costs[graph] = [float(tr.model.train(feed, i)) for i in range(5)]
        torch.cuda.synchronize()
    print(costs)
    assert np.all(np.isfinite(costs[False])) and np.allclose(costs[False], costs[True], rtol=1e-5, atol=0), costs
    assert costs[False][-1] < costs[False][0]                           # one batch, five AMSGrad steps: the cost goes down


def test_v2_checkpoint_restores_into_the_inference_recipe():
    """A checkpoint written after a V2 training step -> STFT_Separator_Inference(L41ModelV2, 'inference'): the hard k-means masks equal
    the oracle's on its own float64 embeddings (no Normalize layer; k-means normalises its input), seeds injected.  A bin whose two
    distances tie within float32 rounding may fall either way: such bins are skipped -- at most 1e-4 of all bins -- and counted."""
    from models.SC_V2 import L41ModelV2
    from utils.trainer import STFT_Separator_Inference
    tr, tfds, (L, W, hop, NL, E) = _stft_trainer(batch_size=2)
    S, B, tries, steps = 2, 2, 2, 3
    one_train_step(tr, tfds, L)
    with tr.graph.as_default():
        tr.model.create_saver()
        tr.model.save(0)
        folder = tr.model._dir()
        trained = {n: v.detach().cpu().numpy().copy() for n, v in tr.graph.variables.items()}
    params = json.load(open(os.path.join(folder, 'params')))
    del tr
    Fq = W // 2 + 1
    T = 1 + (L - W) // hop
    rng = np.random.RandomState(25)         # float64 alone (oracle step, oracle k-means) leaves a smallest relative gap of 1.1e-4 here
    idx = np.stack([rng.choice(T * Fq, S, replace=False) for _ in range(B * tries)]).astype(np.int32)
    a = base_args(**params)
    a.update(model_folder=folder, nb_tries=tries, nb_steps=steps, end_assign=True, kmeans_init_indices=idx, out=False)
    a.pop('type')
    inf = STFT_Separator_Inference(L41ModelV2, 'inference', **a)
    dist, tfds = inf.prepare()
    g, model = inf.graph, inf.model
    with g.as_default():
        for n, v in trained.items():                                    # the restore brought the trained values back, bit for bit
            assert np.array_equal(g.variables[n].detach().cpu().numpy(), v), n
        feed = {tfds.handle: tfds.get_handle(tfds.TEST), tfds.chunk_size: L}
        xm, xn, masks, out = model._eval_guarded(feed, lambda run: [model.x_mix.value(run), model.x_non_mix.value(run),
                                                                    model.masks.value(run), model.output.value(run)])
    torch.cuda.synchronize()
    assert out.shape == (B, S, (T - 1) * hop + W) and bool(torch.isfinite(out).all())
    P64 = {k: v.astype(np.float64) for k, v in trained.items()}
    X = ostft.stft_preprocessing(xm.cpu().numpy().astype(np.float64), xn.cpu().numpy().astype(np.float64), W, hop)[0]
    V, _ = ostep.prediction_fwd(X, P64, NL, E, normalize=False)
    emb = V.reshape(B, T * Fq, E)
    cent, labels, best = okm.kmeans(emb, idx, S, tries, steps, assign_at_end=True)
    x0 = okm.l2_normalize_rows(emb)
    d = np.stack([np.sqrt(okm.sqdist(x0[i], cent[i], np.ones(T * Fq))) for i in range(B)])          # [B, TF, S]
    ds = np.sort(d, axis=2)
    tie = (ds[:, :, 1] - ds[:, :, 0]) < 1e-5 * ds[:, :, 1]              # float32 embeddings carry ~1e-6 relative error through the stack
    got = masks.cpu().numpy().reshape(B, T * Fq, S)
    ref = okm.masks_from_labels(labels, S, None)
    skipped = int(tie.sum())
    print('bins whose two distances tie within float32 rounding: %d of %d skipped' % (skipped, tie.size))
    assert skipped <= 1e-4 * tie.size
    assert set(np.unique(got)) == {0.0, 1.0} and 0.02 < ref[..., 0].mean() < 0.98
    assert np.array_equal(got[~tie], ref[~tie])
