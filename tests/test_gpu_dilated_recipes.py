"""GPU: STFT recipes with --add_dilated (reference models/network.py:445-446, 527-551) against a float64 composition: oracle STFT
conditioning -> float64 dilated stack (tests/dilated_ref.py, torch autograd) -> oracle BLSTM / dense / loss and their backward, the
input gradient of BLSTM_0 included.  Replay against eager; an enhance stage and STFT inference on a dilated model."""
import os
import tempfile

import numpy as np
import pytest

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

from oracle import blstm as oblstm, dense as odense, dpcl as odpcl, kmeans as okm, l41 as ol41, optim as ooptim, \
    separate as osep, step as ostep, stft as ostft  # noqa: E402
from tests import dilated_ref as ref  # noqa: E402
from tests.test_gpu_fullstep import _device_mask_spectra, check_step  # noqa: E402
from tests.test_gpu_recipes import INFER_TOL, base_args, one_train_step  # noqa: E402

os.environ.setdefault('AMS_LOG_DIR', tempfile.mkdtemp(prefix='ams_log_'))


def ref_step(kind, xm, xn, P, W, hop, NL, E, I=None, mask_spectra=None, relu_masks=None):
    """(cost, grads) of one STFT_DPCL / STFT_L41 --add_dilated step in float64.  relu_masks: the stack's activation pattern to use
    (the device's; see record_relu_masks) instead of float64's own."""
    B, S, L = xn.shape
    X, X_nm, _ = ostft.stft_preprocessing(xm, xn, W, hop)
    dil = [(P[n + '/weights'], P[n + '/biases']) for n in ref.NAMES]
    Xd = ref.stack_fwd(X, dil) if relu_masks is None else ref.stack_fwd_masked(X, dil, relu_masks)
    spec = X_nm if mask_spectra is None else mask_spectra
    if kind == 'dpcl':
        Y, _ = osep.make_masks(spec, 1.0, 0.0)
        V, cache = ostep.prediction_fwd(Xd, P, NL, E)
        Vf, Yf = V.reshape(B, -1, E), Y.reshape(B, -1, S)
        cost, _ = odpcl.dpcl_cost(Vf, Yf)
        dV = odpcl.dpcl_cost_bwd(Vf, Yf).reshape(V.shape)
    else:
        Y, _ = osep.make_masks(spec, 1.0, -1.0)
        V, cache = ostep.prediction_fwd(Xd, P, NL, E, True)
        cost = ol41.l41_cost(V, Y, P['speaker_centroids'], I, True, None, 0.1)
        dV, dspk = ol41.l41_cost_bwd(V, Y, P['speaker_centroids'], I, True, None, 0.1)
    caches, h, V_, inv = cache
    du = odense.l2norm_bwd(V_, inv, dV) if inv is not None else dV
    du = du.reshape(du.shape[:2] + (-1,))
    dh, dW, db = odense.dense_bwd(h, P['prediction/W'], du)
    dX, lg = oblstm.blstm_stack_bwd(dh, caches, need_dx=True)
    grads = {'prediction/W': dW, 'prediction/b': db}
    for i, g in enumerate(lg):
        for n, v in zip(ostep.lstm_names('prediction', i), g):
            grads[n] = v
    if kind == 'l41':
        grads['speaker_centroids'] = dspk
    _, dg = ref.stack_vjp(X, dil, dX) if relu_masks is None else ref.stack_vjp_masked(X, dil, dX, relu_masks)
    for n, (dw, dbb) in zip(ref.NAMES, dg):
        grads[n + '/weights'], grads[n + '/biases'] = dw, dbb
    return cost, grads


def record_relu_masks(monkeypatch):
    """Collects the post-ReLU output of every dilated layer the device computes (ops.dilated_conv2d_fwd); masks() -> the last 13
    activation patterns (y > 0).  A pre-activation within rounding of zero may fall one way in f32 and the other in float64, and one
    such pixel moves a bias gradient of an untrained stack at the 1e-3 level: the float64 composition takes the device's pattern, as
    the DPCL steps take the device's ideal-mask labels (mask_spectra), and every gradient is then held to check_step's 2e-4."""
    from ams_hip import ops
    seen = []
    fwd = ops.dilated_conv2d_fwd

    def rec(*a, **k):
        y, ay = fwd(*a, **k)
        seen.append(y)
        return y, ay
    monkeypatch.setattr(ops, 'dilated_conv2d_fwd', rec)
    return lambda: [(y > 0).cpu().numpy() for y in seen[-13:]]


def _trainer(kind, B, L, W, hop, LS=12, NL=2, E=8, **kw):
    from utils.trainer import STFT_Separator_Trainer
    if kind == 'dpcl':
        from models.dpcl import DPCL as cls
        name = 'STFT_DPCL'
    else:
        from models.L41 import L41Model as cls
        name = 'STFT_L41'
    a = base_args(batch_size=B, nb_speakers=2, chunk_size=L, window_size=W, hop_size=hop, layer_size=LS, nb_layers=NL,
                  embedding_size=E, model_folder=None, learning_rate=1e-3, add_dilated=True, **kw)
    a.pop('type')
    tr = STFT_Separator_Trainer(cls, name, **a)
    dist, tfds = tr.prepare()
    return tr, tfds


@pytest.mark.parametrize('kind', ['dpcl', 'l41'])
@pytest.mark.parametrize('geo', [(4, 2048, 64, 32), (2, 20480, 512, 256)], ids=['reduced', 'cfg1'])
def test_dilated_step_against_float64(kind, geo, monkeypatch):
    B, L, W, hop = geo
    NL, E = 2, 8
    tr, tfds = _trainer(kind, B, L, W, hop, NL=NL, E=E)
    masks = record_relu_masks(monkeypatch)
    P, cost, xm, xn, I, grads, P_new = one_train_step(tr, tfds, L)
    assert any(n.startswith('dilated/') for n in grads)
    ms = _device_mask_spectra(xn, W, hop, 'dilated ' + kind)
    c_ref, g_ref = ref_step(kind, xm, xn, P, W, hop, NL, E, I=I, mask_spectra=ms, relu_masks=masks())
    # The update is checked on the device's gradients (test_gpu_fullstep.check_step): AMSGrad turns the sign of a gradient entry that
    # is rounding noise into +-lr.
    check_step(cost, c_ref, grads, g_ref, P, P_new, ooptim.AMSGrad(1e-3), what='dilated %s %s' % (kind, geo))


def test_dilated_stft_dpcl_replay_matches_eager():
    from tests.test_gpu_replay import _compare
    B, L, W, hop = 4, 2048, 64, 32

    def make(graph):
        tr, tfds = _trainer('dpcl', B, L, W, hop, hip_graph=graph)
        return tr, tfds, L
    _compare(make)


def test_dilated_enhance_stage_restores_and_freezes_the_stack():
    """STFT_DPCL_enhance on a dilated model folder: Network.load keeps add_dilated, the stack is rebuilt and restored, and
    freeze_all_except('enhance') leaves it untouched by a step."""
    from models.dpcl import DPCL
    from utils.trainer import STFT_Separator_enhance_Trainer
    B, L, W, hop, LS, NL, E = 2, 2048, 64, 32, 12, 2, 8
    tr, tfds = _trainer('dpcl', B, L, W, hop, LS=LS, NL=NL, E=E)
    g0 = tr.graph
    with g0.as_default():
        for n in ref.NAMES:                                  # distinguishable from a fresh initialisation
            g0.variables[n + '/biases'].data.add_(0.01)
        tr.model.save(0)
        saved = {n: v.detach().cpu().numpy().copy() for n, v in g0.variables.items() if n.startswith('dilated/')}
        folder = tr.model._dir()
    Fq = W // 2 + 1
    T = 1 + (L - W) // hop
    rng = np.random.RandomState(3)
    tries, steps = 2, 3
    idx = np.stack([rng.choice(T * Fq, 2, replace=False) for _ in range(B * tries)]).astype(np.int32)
    a = base_args(batch_size=B, nb_speakers=2, chunk_size=L, window_size=W, hop_size=hop, model_folder=folder, nb_tries=tries,
                  nb_steps=steps, end_assign=True, kmeans_init_indices=idx, layer_size_enhance=8, nb_layers_enhance=2,
                  nonlinearity='softmax', learning_rate=1e-3, pretraining=False)
    a.pop('type')
    et = STFT_Separator_enhance_Trainer(DPCL, 'STFT_DPCL_enhance', **a)
    dist, tfds2 = et.prepare()
    g = et.graph
    names = [v.ams_name for v in et.model.trainable_variables]
    assert names and all(n.startswith('enhance/') for n in names)
    for n, v in saved.items():
        assert np.array_equal(g.variables[n].detach().cpu().numpy(), v), n
    Pg, cost, xm, xn, I, grads, P_new = one_train_step(et, tfds2, L)
    assert np.isfinite(cost)
    for n, v in saved.items():
        assert np.array_equal(g.variables[n].detach().cpu().numpy(), v), n


def test_dilated_stft_inference_matches_the_oracle_composition():
    """STFT_Separator_Inference on a dilated model folder: |STFT| -> dilated stack -> DPCL -> hard k-means -> masks on the UNDILATED
    magnitude -> iSTFT (network.py:445-446, 527-551; trainer.py:406-417), against the float64 composition."""
    from ams_hip import testing
    from models.dpcl import DPCL
    from utils.trainer import STFT_Separator_Inference
    tmp = tempfile.mkdtemp(prefix='ams_dinf_')
    rng = np.random.RandomState(12)
    B, S, L, W, hop, LS, NL, E, tries, steps = 2, 2, 2048, 64, 32, 12, 2, 8, 2, 3
    Fq = W // 2 + 1
    P = ostep.init_params(rng, np.float32, N=None, D_in=4 * Fq, layer_size=LS, nb_layers=NL, E=E, F=Fq, conv1d_scale=0.5)
    for n, (w, b) in zip(ref.NAMES, ref.init_params(rng)):
        P[n + '/weights'], P[n + '/biases'] = w, b
    params = dict(testing.ADAPT_DEFAULTS)
    for k in ('filters', 'max_pool'):
        params.pop(k)
    params.update(testing.SEPARATOR_DEFAULTS)
    params.update(window_size=W, hop_size=hop, chunk_size=L, batch_size=B, nb_speakers=S, layer_size=LS, nb_layers=NL,
                  embedding_size=E, type='STFT_DPCL', pretraining=False, add_dilated=True)
    folder = testing.write_checkpoint(os.path.join(tmp, 'ckpt'), P, params)
    T = 1 + (L - W) // hop
    idx = np.stack([rng.choice(T * Fq, S, replace=False) for _ in range(B * tries)]).astype(np.int32)
    a = base_args(**params)
    a.update(model_folder=folder, nb_tries=tries, nb_steps=steps, end_assign=True, kmeans_init_indices=idx, out=False)
    a.pop('type')
    tr = STFT_Separator_Inference(DPCL, 'STFT_DPCL_inference', **a)
    dist, tfds = tr.prepare()
    g, model = tr.graph, tr.model
    assert all(np.array_equal(g.variables[n + '/weights'].detach().cpu().numpy(), P[n + '/weights']) for n in ref.NAMES)
    with g.as_default():
        feed = {tfds.handle: tfds.get_handle(tfds.TEST), tfds.chunk_size: L}
        xm, xn, out = model.infer(feed, 0)
    P64 = {k: v.astype(np.float64) for k, v in P.items()}
    xm64, xn64 = xm.cpu().numpy().astype(np.float64), xn.cpu().numpy().astype(np.float64)
    X, _, ang = ostft.stft_preprocessing(xm64, xn64, W, hop)
    Xd = ref.stack_fwd(X, [(P64[n + '/weights'], P64[n + '/biases']) for n in ref.NAMES])
    assert Xd.shape == (B, T, 4 * Fq) and np.abs(Xd).max() > 0
    V, _ = ostep.prediction_fwd(Xd, P64, NL, E)
    cent, labels, best = okm.kmeans(V.reshape(B, T * Fq, E), idx, S, tries, steps, assign_at_end=True)
    masks = okm.masks_from_labels(labels, S, None).astype(X.dtype)
    sep = osep.apply_masks(X, masks)                         # the masks apply to X_input, the magnitude before the stack
    out_ref = ostft.istft(sep, np.repeat(ang, S, axis=0), W, hop).reshape(B, S, -1)
    assert out.shape == out_ref.shape
    err = np.linalg.norm(out.cpu().numpy() - out_ref) / np.linalg.norm(out_ref)
    assert err < INFER_TOL, err
