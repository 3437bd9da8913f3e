"""GPU: whole recipes at five speakers through the reference-API mirror (utils/trainer.py) against the oracle -- one training step of
each family, inference with hard k-means, eager == replayed, and the scoring of a five-source output.  Sizes, helpers and tolerances
are those of tests/test_gpu_recipes.py (imported, not restated)."""
import os
import tempfile

import numpy as np
import pytest

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

from oracle import step as ostep, recipes as orec, optim as ooptim
from tests import test_gpu_recipes as rc
from tests import test_gpu_replay as rp
from tests import test_gpu_bss_batch as bb

os.environ.setdefault('AMS_LOG_DIR', tempfile.mkdtemp(prefix='ams_log_'))

S = 5


@pytest.mark.parametrize('loss,separation', [('sdr+l2', 'mask')])
def test_pretraining_step(loss, separation):
    """experiments.training.pretraining: the identity-paired costs (mode 0 of the pair costs) from the 6-wide pair table."""
    from utils.trainer import Adapt_Pretrainer
    B, L, W, N, hop = 3, 1024, 64, 16, 16
    a = rc.base_args(batch_size=B, nb_speakers=S, chunk_size=L, window_size=W, filters=N, hop_size=hop, loss=loss, separation=separation,
                     overlap_coef=1.0, optimizer='Adam', learning_rate=1e-3, pretraining=True)
    a.pop('type')
    tr = Adapt_Pretrainer(**a)
    dist, tfds = tr.prepare()
    P, cost, xm, xn, I, grads, P_new = rc.one_train_step(tr, tfds, L)
    assert xn.shape == (B, S, L)
    c_ref, g_ref, back = orec.pretrain_loss(xm, xn, P, hop, loss, separation, 1.0)
    rc.check_step(cost, c_ref, grads, g_ref, P, P_new, ooptim.AMSGrad(1e-3))


def test_stft_dpcl_step():
    """experiments.training.STFT_DPCL: the deep-clustering loss on its generic path (S > 4)."""
    from models.dpcl import DPCL
    from utils.trainer import STFT_Separator_Trainer
    B, L, W, hop, LS, NL, E = 4, 2048, 64, 32, 12, 2, 8
    a = rc.base_args(batch_size=B, nb_speakers=S, chunk_size=L, window_size=W, hop_size=hop, layer_size=LS, nb_layers=NL,
                     embedding_size=E, model_folder=None, learning_rate=1e-3)
    a.pop('type')
    tr = STFT_Separator_Trainer(DPCL, 'STFT_DPCL', **a)
    dist, tfds = tr.prepare()
    P, cost, xm, xn, I, grads, P_new = rc.one_train_step(tr, tfds, L)
    c_ref, g_ref, V, Y = ostep.stft_dpcl_loss(xm, xn, P, W, hop, NL, E)
    assert Y.shape[-1] == S
    rc.check_step(cost, c_ref, grads, g_ref, P, P_new, ooptim.AMSGrad(1e-3))


def _front_l41(graph=None, B=3, L=1024, normalize=False, **kw):
    from ams_hip import testing
    from models.L41 import L41Model
    from utils.trainer import Front_Separator_Trainer
    tmp = tempfile.mkdtemp(prefix='ams_l41s5_')
    W, N, hop, LS, NL, E = 64, 16, 16, 12, 2, 8
    folder, params = testing.make_pretrained_adapt(os.path.join(tmp, 'pre'), window_size=W, filters=N, hop_size=hop, chunk_size=L,
                                                   batch_size=B, nb_speakers=S)
    a = rc.base_args(**params)
    a.update(layer_size=LS, nb_layers=NL, embedding_size=E, model_folder=folder, model_previous=None, pretraining=False,
             no_normalize=normalize, learning_rate=1e-3, **kw)
    if graph is not None:
        a.update(tot_speakers=251, hip_graph=graph, no_summaries=True)
    a.pop('type')
    tr = Front_Separator_Trainer(L41Model, 'front_L41', **a)
    dist, tfds = tr.prepare()
    return tr, tfds, L, (hop, NL, E)


@pytest.mark.parametrize('normalize', [True, False])
def test_front_l41_step(normalize):
    """experiments.training.front_L41: the L41 loss with five speaker vectors per utterance."""
    tr, tfds, L, (hop, NL, E) = _front_l41(normalize=normalize)
    P, cost, xm, xn, I, grads, P_new = rc.one_train_step(tr, tfds, L)
    assert I.shape[1] == S
    c_ref, g_ref, V, Y = ostep.front_l41_loss(xm, xn, I, P, hop, NL, E, normalize)
    rc.check_step(cost, c_ref, grads, g_ref, P, P_new, ooptim.AMSGrad(1e-3))


def test_front_l41_replay_matches_eager():
    """The same recipe eagerly and under --hip_graph (tests/test_gpu_replay.py, three speakers there): per-step costs and final weights."""
    rp._compare(lambda graph: _front_l41(graph=graph)[:3])


def _checkpoint(prefix, seed, B, L, tries, **kw):
    tmp = tempfile.mkdtemp(prefix=prefix)
    rng = np.random.RandomState(seed)
    W, N, hop, LS, NL, E = 64, 16, 16, 12, 2, 8
    folder, params, P = rc._full_checkpoint(tmp, rng, W, N, hop, L, B, S, LS, NL, E, N, N, **kw)
    T = -(-L // hop)
    idx = np.stack([rng.choice(T * N, S, replace=False) for _ in range(B * tries)]).astype(np.int32)
    return folder, params, P, idx, (hop, NL, E)


def test_front_dpcl_enhance_step():
    """experiments.training.front_DPCL_enhance: hard k-means with five clusters (E = 8) under the enhance stack and its PIT cost over
    120 permutations."""
    from models.dpcl import DPCL
    from utils.trainer import Front_Separator_Enhance_Trainer
    B, L, tries, steps, LSE, NLE = 2, 1024, 2, 3, 8, 2
    folder, params, P, idx, (hop, NL, E) = _checkpoint('ams_enh5_', 31, B, L, tries)
    a = rc.base_args(**params)
    a.update(model_folder=folder, nb_tries=tries, nb_steps=steps, end_assign=True, kmeans_init_indices=idx, layer_size_enhance=LSE,
             nb_layers_enhance=NLE, nonlinearity='softmax', learning_rate=1e-3, pretraining=False)
    a.pop('type')
    tr = Front_Separator_Enhance_Trainer(DPCL, 'front_DPCL_enhance', **a)
    dist, tfds = tr.prepare()
    names = sorted(v.ams_name for v in tr.model.trainable_variables)
    assert names and all(n.startswith('enhance/') for n in names)
    Pg, cost, xm, xn, I, grads, P_new = rc.one_train_step(tr, tfds, L)
    c_ref, g_ref = orec.front_enhance_loss(xm, xn, Pg, hop, NL, E, NLE, idx, tries, steps)
    rc.check_step(cost, c_ref, grads, g_ref, Pg, P_new, ooptim.AMSGrad(1e-3))


def test_front_dpcl_finetuning_step():
    """experiments.training.front_DPCL_finetuning: soft k-means with five clusters (forward, and backward through ams_kmeans_soft_bwd),
    the back end and the Adapt cost's search (mode 2).  The oracle has this objective forward only, so -- as in
    tests/test_gpu_recipes.py::test_front_dpcl_finetuning_step -- the cost is compared with it and the gradients with its central
    differences."""
    from models.dpcl import DPCL
    from utils.trainer import Front_Separator_Finetuning_Trainer
    B, L, tries, steps, beta = 2, 1024, 1, 3, 4.0
    folder, params, P, idx, (hop, NL, E) = _checkpoint('ams_ft5_', 21, B, L, tries)
    a = rc.base_args(**params)
    a.update(model_folder=folder, nb_tries=tries, nb_steps=steps, beta_kmeans=beta, with_silence=True, threshold=2.0, end_assign=True,
             kmeans_init_indices=idx, loss='sdr+l2', optimizer='RMSProp', learning_rate=1e-4, pretraining=False)
    a.pop('type')
    tr = Front_Separator_Finetuning_Trainer(DPCL, 'front_L41_finetuning', **a)
    dist, tfds = tr.prepare()
    assert all(v.ams_name.startswith('prediction/') for v in tr.model.trainable_variables)
    Pg, cost, xm, xn, I, grads, P_new = rc.one_train_step(tr, tfds, L)
    args = (hop, NL, E, idx, tries, steps, beta, True, 2.0, True, 'sdr+l2')
    cost_fn = lambda Pp: orec.front_finetune_cost(xm, xn, Pp, *args)[0]   # noqa: E731
    c_ref = cost_fn(Pg)
    assert abs(cost - c_ref) < 1e-3 * abs(c_ref), (cost, c_ref)
    rc._fd_check(cost_fn, Pg, grads, ('prediction/W', 'prediction/forward_BLSTM_1/rnn/basic_lstm_cell/kernel', 'prediction/b'))


@pytest.fixture(scope='module')
def inference():
    """Front_Separator_Inference at five speakers, hard k-means, injected seeds: (sources, separated, oracle's separated)."""
    from models.dpcl import DPCL
    from utils.trainer import Front_Separator_Inference
    B, L, tries, steps = 2, 2048, 2, 3
    folder, params, P, idx, (hop, NL, E) = _checkpoint('ams_inf5_', 11, B, L, tries)
    a = rc.base_args(**params)
    a.update(model_folder=folder, nb_tries=tries, nb_steps=steps, beta_kmeans=None, with_silence=False, end_assign=True,
             kmeans_init_indices=idx, out=False)
    a.pop('type')
    tr = Front_Separator_Inference(DPCL, 'front_DPCL_inference', **a)
    xm, xn, out = rc._infer(tr, L)
    P64 = {k: v.astype(np.float64) for k, v in P.items()}
    out_ref, lab_ref, V_ref = orec.front_separate_infer(xm, xn, P64, hop, NL, E, idx, tries, steps, beta=None, with_silence=False,
                                                        end_assign=True)
    return xn, out, out_ref, lab_ref


def test_front_separator_inference(inference):
    """front -> DPCL -> hard k-means with five clusters -> back, at INFER_TOL.  The oracle clusters its own float64 embeddings, so the
    case must be one whose labels do not hang on the last bits: checkpoint / seed-index stream RandomState(11) on the first test batch
    of the synthetic set (B = 2, L = 2048) was chosen on the CPU because orec.front_separate_infer returns the same labels with the
    parameters drawn in float64 and with the same parameters rounded to float32 (every cluster holds 313-488 of the 2048 bins of its
    utterance); seeds 11 onwards were tried in order and 11 was the first to pass."""
    xn, out, out_ref, lab_ref = inference
    assert out.shape == xn.shape == (2, S, 2048) and np.isfinite(out_ref).all()
    assert min(np.bincount(np.asarray(lab_ref[b]).ravel().astype(np.int64), minlength=S).min() for b in range(2)) > 0
    err = np.linalg.norm(out - out_ref) / np.linalg.norm(out_ref)
    print('relative L2 error of the separated waveforms: %.3e (tol %.1e)' % (err, rc.INFER_TOL))
    assert err < rc.INFER_TOL, err


def test_scoring_five_sources(inference):
    """The inference output scored by the batched BSS-eval (utils/bss_eval.py) against oracle/bss_eval.py for nsrc = 5, at the smallest
    length and filter order tests/test_gpu_bss_batch.py uses (1500 samples, flen = 37) and its dB rule."""
    from utils import bss_eval as hb
    xn, out, _, _ = inference
    refs = np.ascontiguousarray(xn[:, :, :1500], dtype=np.float64)
    ests = np.ascontiguousarray(out[:, None, :, :1500], dtype=np.float64)
    crit, info = hb.bss_eval_pairs_batch(refs, ests, flen=37)
    assert crit.shape == (2, 1, 3, S, S) and not info.any()
    want, wperm = bb._oracle(refs, ests, 37)
    bb._close_db(crit, want)
    assert np.array_equal(hb.bss_eval_sources_batch(refs, ests, flen=37)[3], wperm)
