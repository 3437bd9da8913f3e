"""GPU: the deep-attractor reconstruction loss of L41ModelV2 (csrc/danet.hip: ams_danet_recon_fwd / _bwd) through
ams_hip.functional against the float64 restatement of reference models/SC_V2.py in tests/danet_ref.py -- with the helpers and the
bounds of the L41 loss's own kernel tests (tests/test_gpu_kernels2.py: TOL on the cost, 5 TOL on gradients relative to the tensor's
largest entry)."""
import numpy as np
import pytest

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

from tests import danet_ref as R
from tests.test_gpu_kernels2 import TOL, dev, host, rel


@pytest.fixture(scope='module')
def F():
    from ams_hip import functional as f
    return f


def _inputs(seed, B, T, Fq, E, S, kind, zmax=None):
    """float32-representable inputs (the device and the float64 restatement read the same numbers)."""
    rng = np.random.RandomState(seed)
    f32 = lambda a: np.asarray(a, np.float32).astype(np.float64)
    V = rng.standard_normal((B, T, Fq, E)) * 0.4 * np.exp(0.5 * rng.standard_normal((B, T, Fq, 1)))
    X = f32(rng.standard_normal((B, T, Fq)))
    X_nm = f32(rng.standard_normal((B, T, Fq, S)))
    lab = rng.randint(0, S, (B, T, Fq))
    y = np.where(lab[..., None] == np.arange(S), 1.0, -1.0)
    if kind == 'fractional':
        y = f32(y * rng.uniform(0.0, 1.0, (B, T, Fq))[..., None])
    elif kind == 'empty_speaker':
        y[0] = -1.0
        y[0, :, :, S - 1] = 1.0                                  # every bin of utterance 0 belongs to the last speaker: den = 1e-12 for the rest
    if zmax is not None:                                         # scale so that the largest |logit| is zmax
        V = f32(V)
        m = R.soft_masks(y)
        A = R.recon_forward(V, m, X, X_nm)[1][0]
        z = np.abs(np.einsum('bes,btfe->btfs', A, V)).max()
        V = V * np.sqrt(zmax / z)                                # A scales with V: z with its square
    return f32(V), y, X, X_nm


def _run(F, V, y, X, X_nm, xs=None, thr=None, rows=False):
    B, T, Fq, E = V.shape
    S = y.shape[-1]
    vt = dev(V).requires_grad_()
    if rows:                                                     # the separator's layout: a permuted view of the [B*S, T, F] rows
        xnm = dev(X_nm.transpose(0, 3, 1, 2)).reshape(B, S, T, Fq).permute(0, 2, 3, 1)
        assert not xnm.is_contiguous()
    else:
        xnm = dev(X_nm)
    c = F.danet_recon_loss(vt, dev(y), dev(X), xnm, dev(xs) if xs is not None else None, thr)
    c.backward()
    return float(c.detach()), host(vt.grad), vt.grad


# T*F: 150 bins (below one block); 2313 = 9 blocks + 9; 10280 (past the 8192-point chunk of the k-means passes, ragged tail)
CASES = [(T, Fq, E, S, kind) for (T, Fq) in ((3, 50), (9, 257)) for (E, S) in ((8, 2), (40, 2), (40, 3), (8, 3))
         for kind in ('binary', 'fractional', 'empty_speaker')] + \
        [(40, 257, 40, 2, 'binary'), (40, 257, 40, 3, 'fractional'), (40, 257, 8, 3, 'empty_speaker'), (40, 257, 8, 2, 'binary')]


@pytest.mark.parametrize('T,Fq,E,S,kind', CASES)
def test_reconstruction_cost_and_gradient(F, T, Fq, E, S, kind):
    reconstruction_case(F, 2, T, Fq, E, S, kind)


def reconstruction_case(F, B, T, Fq, E, S, kind):
    """The body of test_reconstruction_cost_and_gradient (B = 2 there); other batch and embedding sizes: tests/test_gpu_dispatch_arms.py."""
    V, y, X, X_nm = _inputs(100 * E + 10 * S + T, B, T, Fq, E, S, kind)
    m = R.soft_masks(y)
    if kind == 'empty_speaker':
        assert m[0, :, :, 0].sum() == 0.0
    c_ref = R.recon_cost(V, m, X, X_nm)
    d_ref = R.recon_cost_bwd(V, m, X, X_nm)
    c, d, _ = _run(F, V, y, X, X_nm, rows=(S == 2))
    print('cost %.9g ref %.9g; grad rel %.3g (max |d_ref| %.3g)' % (c, c_ref, rel(d, d_ref), np.abs(d_ref).max()))
    assert np.isfinite(c) and np.isfinite(d).all()
    assert abs(c - c_ref) < TOL * max(1.0, abs(c_ref))
    assert rel(d, d_ref) < 5 * TOL


@pytest.mark.parametrize('E,S,T,Fq', [(40, 2, 9, 257), (8, 3, 3, 50)])
def test_saturated_sigmoid(F, E, S, T, Fq):
    """Embeddings scaled so that the logits reach |z| = 30: sigmoid saturates -- finite cost, no NaN, the gradient of the saturated bins
    goes to zero (the float32 a (1 - a) is exactly 0 there, the float64 one ~1e-13)."""
    V, y, X, X_nm = _inputs(77 + E, 2, T, Fq, E, S, 'binary', zmax=30.0)
    m = R.soft_masks(y)
    c_ref, (A, den, a, r) = R.recon_forward(V, m, X, X_nm)
    z = np.einsum('bes,btfe->btfs', A, V)
    assert 29.0 < np.abs(z).max() < 31.0 and (np.abs(z) > 17.0).sum() > 0
    d_ref = R.recon_cost_bwd(V, m, X, X_nm)
    c, d, _ = _run(F, V, y, X, X_nm)
    print('cost %.9g ref %.9g; grad rel %.3g' % (c, c_ref, rel(d, d_ref)))
    assert np.isfinite(c) and np.isfinite(d).all()
    assert abs(c - c_ref) < TOL * max(1.0, abs(c_ref))
    assert rel(d, d_ref) < 5 * TOL


@pytest.mark.parametrize('E,S,T,Fq,kind', [(40, 2, 9, 257, 'binary'), (8, 3, 40, 257, 'fractional'), (8, 2, 3, 50, 'binary')])
def test_silence_mask_folded_into_the_attractor_pass(F, E, S, T, Fq, kind):
    V, y, X, X_nm = _inputs(5 + E + S, 2, T, Fq, E, S, kind)
    xs = np.asarray(np.random.RandomState(9).standard_normal(X.shape), np.float32).astype(np.float64)
    thr = 1.0
    mask = R.silence_mask(xs, thr)
    assert 0.2 < mask.mean() < 0.9
    m = R.soft_masks(y, mask)
    c_ref, d_ref = R.recon_cost(V, m, X, X_nm), R.recon_cost_bwd(V, m, X, X_nm)
    c, d, _ = _run(F, V, y, X, X_nm, xs=xs, thr=thr, rows=True)
    print('cost %.9g ref %.9g; grad rel %.3g' % (c, c_ref, rel(d, d_ref)))
    assert abs(c - c_ref) < TOL * max(1.0, abs(c_ref))
    assert rel(d, d_ref) < 5 * TOL
    assert rel(R.recon_cost_bwd(V, R.soft_masks(y), X, X_nm), d_ref) > 0.1     # the mask is in what is compared


def test_two_calls_give_the_same_bits(F):
    V, y, X, X_nm = _inputs(21, 3, 40, 257, 40, 2, 'fractional')
    xs = X
    c1, _, g1 = _run(F, V, y, X, X_nm, xs=xs, thr=1.0)
    c2, _, g2 = _run(F, V, y, X, X_nm, xs=xs, thr=1.0)
    assert c1 == c2 and torch.equal(g1, g2)


def test_upstream_scalar_scales_the_gradient(F):
    V, y, X, X_nm = _inputs(22, 2, 9, 257, 40, 2, 'binary')
    vt = dev(V).requires_grad_()
    (F.danet_recon_loss(vt, dev(y), dev(X), dev(X_nm)) * 3.0).backward()
    d_ref = 3.0 * R.recon_cost_bwd(V, R.soft_masks(y), X, X_nm)
    assert rel(host(vt.grad), d_ref) < 5 * TOL


@pytest.mark.parametrize('E,S,silence', [(40, 2, False), (8, 3, True)])
def test_whole_cost_adds_into_the_contrastive_gradient(F, E, S, silence):
    """F.danet_sce_loss = L41 loss on l2-normalised embeddings (labels y_ab) + reconstruction (weights m), one node: the reconstruction
    backward ADDS into the tensor the source-contrastive backward wrote, and leaves the bound of the sum with it."""
    from ams_hip import ops as K
    B, T, Fq, NS = 2, 9, 257, 11
    V, y, X, X_nm = _inputs(31 + E, B, T, Fq, E, S, 'binary')
    rng = np.random.RandomState(4)
    spk = np.asarray(rng.standard_normal((NS, E)), np.float32).astype(np.float64)
    I = np.stack([rng.choice(NS, S, replace=False) for _ in range(B)]).astype(np.int32)
    thr = 0.5 if silence else None
    mask = R.silence_mask(X, thr) if silence else None
    tot_ref, (sc_ref, rc_ref), dV_ref, ds_ref = R.sc_v2_cost(V, y, mask, X, X_nm, spk, I)
    ut, st = dev(V.reshape(B, T, Fq * E)).requires_grad_(), dev(spk).requires_grad_()
    yt = dev(y)
    y_ab = K.weight_masks(dev(X).reshape(B, -1), yt.reshape(B, -1, S), None, thr) if silence else yt
    tot, sc, rc = F.danet_sce_loss(ut, y_ab, yt, st, dev(I, np.int32), dev(X), dev(X_nm), dev(X) if silence else None, thr)
    for got, want in ((tot, tot_ref), (sc, sc_ref), (rc, rc_ref)):
        assert abs(float(got.detach()) - want) < TOL * max(1.0, abs(want)), (float(got.detach()), want)
    assert not sc.requires_grad and not rc.requires_grad
    tot.backward()
    print('grad u rel %.3g, spk rel %.3g' % (rel(host(ut.grad).reshape(V.shape), dV_ref), rel(host(st.grad), ds_ref)))
    assert rel(host(ut.grad).reshape(V.shape), dV_ref) < 5 * TOL and rel(host(st.grad), ds_ref) < 5 * TOL
    assert np.abs(dV_ref - R.recon_cost_bwd(V, R.soft_masks(y, mask), X, X_nm)).max() > 1e-3 * np.abs(dV_ref).max()   # both terms are in it


def test_the_accumulating_backward_reports_the_bound_of_the_sum(F):
    from ams_hip import ops as K
    B, T, Fq, E, S = 2, 9, 257, 40, 2
    V, y, X, X_nm = _inputs(41, B, T, Fq, E, S, 'binary')
    v, yt = dev(V).reshape(B, -1, E), dev(y).reshape(B, -1, S)
    cost, attr, g, dattr = K.danet_recon_fwd(v, yt, dev(X).reshape(B, -1), dev(X_nm))
    up = torch.ones(1, device='cuda')
    base = torch.randn_like(v) * 1e-4
    alone = K.danet_recon_bwd(yt, g, attr, dattr, up)
    summed = K.danet_recon_bwd(yt, g, attr, dattr, up, into=base.clone())
    assert rel(host(summed), host(base + alone)) < 1e-6
    if K.F16X3:                                                  # (AMS_GEMM_F16X3=0: nobody computes bounds)
        assert float(K.amax_of(summed)) == float(summed.abs().max()) and float(K.amax_of(alone)) == float(alone.abs().max())
        assert summed._ams_amax[0] is K.amax_of(summed)          # the tag, not a fresh measurement


def test_shapes_outside_the_kernel_domain_are_refused(F):
    from ams_hip import AmsError
    V, y, X, X_nm = _inputs(51, 2, 3, 50, 5, 2, 'binary')        # E = 5: not in the L41 loss's list
    with pytest.raises(AmsError):
        F.danet_recon_loss(dev(V).requires_grad_(), dev(y), dev(X), dev(X_nm))
    V, y, X, X_nm = _inputs(52, 2, 3, 50, 8, 5, 'binary')        # S = 5 > 4
    with pytest.raises(AmsError):
        F.danet_recon_loss(dev(V).requires_grad_(), dev(y), dev(X), dev(X_nm))
    torch.cuda.synchronize()
