"""GPU: the dilated conv2d kernels (csrc/conv2d.hip) of every one of the 13 layer specs against float64 torch conv2d on the CPU
(tests/dilated_ref.py): forward (bias + ReLU), dX (masked by the layer below), dW and db, in the three arithmetic classes; folded
bounds; determinism."""
import numpy as np
import pytest

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

from tests import dilated_ref as ref  # noqa: E402

TOL = 2e-5          # relative to max |reference|: f32-level sums over K <= 3200 terms


def rel(a, b):
    b = np.asarray(b, np.float64)
    return float(np.abs(np.asarray(a, np.float64) - b).max() / max(np.abs(b).max(), 1e-30))


def _arith(mode):
    from ams_hip import _lib
    lib = _lib.load()
    old = lib.ams_gemm_get_arith()
    lib.ams_gemm_set_arith(mode)
    return old


def _run_classes(fn):
    """{'f16x3': fn(bounds=True), 'bf16x6': fn(bounds=False), 'f32': fn(bounds=False) under native f32} (numpy results)."""
    out = {'f16x3': fn(True), 'bf16x6': fn(False)}
    old = _arith(0)
    try:
        out['f32'] = fn(False)
    finally:
        _arith(old)
    torch.cuda.synchronize()
    return out


def _check_classes(res, ref_, what, form='product'):
    """form 'product': the three classes ran (fp16x3 differs from bf16x6 in its bits, bf16x6 from f32) and fp16x3's error is at most
    1.5 x the larger of the other two (tests/test_gpu_gemm_f16.py's rule); 'direct': an f32-FMA kernel that ignores the class (all
    three bit-identical); 'no_bounds': a product the stack runs without bounds (fp16x3 request = bf16x6, bit-identical)."""
    errs = {k: rel(v, ref_) for k, v in res.items()}
    for k, e in errs.items():
        assert e < TOL, (what, k, errs)
    if form == 'direct':
        assert np.array_equal(res['f16x3'], res['bf16x6']) and np.array_equal(res['bf16x6'], res['f32']), what
    elif form == 'no_bounds':
        assert np.array_equal(res['f16x3'], res['bf16x6']) and not np.array_equal(res['bf16x6'], res['f32']), what
    else:
        assert not np.array_equal(res['f16x3'], res['bf16x6']) and not np.array_equal(res['bf16x6'], res['f32']), what
        assert errs['f16x3'] <= 1.5 * max(errs['bf16x6'], errs['f32']), (what, errs)


GEOS = [(2, 79, 257), (3, 37, 65)]


@pytest.mark.parametrize('geo', GEOS, ids=['B2T79F257', 'B3T37F65'])
@pytest.mark.parametrize('layer', range(13))
def test_layer(layer, geo):
    from ams_hip import ops
    B, T, Fq = geo
    (kh, kw), rate, cout = ref.SPECS[layer]
    cin = 1 if layer == 0 else 128
    rng = np.random.RandomState(100 + layer)
    lim = np.sqrt(6.0 / (kh * kw * cin + kh * kw * cout))
    w = rng.uniform(-lim, lim, (kh, kw, cin, cout)).astype(np.float32)
    b = (0.05 * rng.randn(cout)).astype(np.float32)
    x = np.maximum(rng.randn(B, T, Fq, cin), 0).astype(np.float32)          # a post-ReLU input (layer 1: magnitudes)
    if layer == 0:
        x = np.abs(rng.randn(B, T, Fq, 1)).astype(np.float32)
    d = torch.device('cuda')
    xg, wg, bg = (torch.from_numpy(a).to(d) for a in (x, w, b))

    # forward
    y_ref = ref.layer_fwd(x, w, b, rate)

    def fwd(bounds):
        am = (ops.absmax(xg), ops.absmax(wg)) if bounds else None
        y, ay = ops.dilated_conv2d_fwd(xg, wg, bg, rate, amax=am)
        y2, ay2 = ops.dilated_conv2d_fwd(xg, wg, bg, rate, amax=am)
        assert torch.equal(y, y2) and torch.equal(ay, ay2)                       # deterministic
        assert float(ay) == float(y.abs().max())                                 # the folded bound is max |y|, exactly
        return y.cpu().numpy()
    ys = _run_classes(fwd)
    _check_classes(ys, y_ref, 'fwd', 'direct' if (cin == 1 or cout == 4) else 'product')

    # backward: dY' of this layer (gradient of its pre-ReLU sum), the post-ReLU output of the layer below as the mask
    dpre = (rng.randn(B, T, Fq, cout) * (y_ref > 0)).astype(np.float32)
    dx_ref, dw_ref, db_ref = ref.layer_bwd(x, w, b, rate, dpre)
    dg = torch.from_numpy(dpre).to(d)

    def bwd_w(bounds):
        am = (ops.absmax(xg), ops.absmax(dg)) if bounds else None
        dw, db = ops.dilated_conv2d_bwd_filter(xg, dg, wg, rate, amax=am)
        dw2, db2 = ops.dilated_conv2d_bwd_filter(xg, dg, wg, rate, amax=am)
        assert torch.equal(dw, dw2) and torch.equal(db, db2)
        return dw.cpu().numpy(), db.cpu().numpy()
    ws = _run_classes(lambda bounds: bwd_w(bounds)[0])
    form = 'direct' if cout == 4 else 'no_bounds' if cin == 1 else 'product'
    _check_classes(ws, dw_ref, 'dW', form)
    dbs = {k: bwd_w(k == 'f16x3')[1] for k in ('f16x3', 'bf16x6')}
    for k, v in dbs.items():
        assert rel(v, db_ref) < TOL, ('db', k)

    if layer == 0:
        return                                                                   # its input is data: no dX
    mask = x > 0
    dxm_ref = dx_ref * mask

    def bwd_x(bounds):
        am = (ops.absmax(dg), ops.absmax(wg)) if bounds else None
        dx, adx = ops.dilated_conv2d_bwd_data(dg, wg, xg, rate, amax=am)
        dx2, adx2 = ops.dilated_conv2d_bwd_data(dg, wg, xg, rate, amax=am)
        assert torch.equal(dx, dx2) and torch.equal(adx, adx2)
        assert float(adx) == float(dx.abs().max())
        assert not dx[~torch.from_numpy(mask).to(d)].any()                       # the mask of the layer below is applied
        return dx.cpu().numpy()
    xs = _run_classes(bwd_x)
    _check_classes(xs, dxm_ref, 'dX')


def test_relu_bwd_and_the_stack_function_against_float64_autograd():
    """functional.dilated_stack forward + backward (all 13 layers, the top layer's own ReLU included) against float64 autograd.
    The backward is held against float64 on the device's OWN activation pattern (the saved post-ReLU outputs > 0): with float64's
    pattern, the few pre-activations within rounding of zero that fall the other way move the gradients at the 1e-3 level."""
    from ams_hip import functional as F, ops
    B, T, Fq = 2, 37, 65
    rng = np.random.RandomState(7)
    params = ref.init_params(rng)
    x = np.abs(rng.randn(B, T, Fq)).astype(np.float32)
    dout = rng.randn(B, T, 4 * Fq).astype(np.float32)
    d = torch.device('cuda')
    ps = []
    for w, b in params:
        ps += [torch.from_numpy(w).to(d).requires_grad_(True), torch.from_numpy(b).to(d).requires_grad_(True)]
    out = F.dilated_stack(torch.from_numpy(x).to(d), [s[1] for s in ref.SPECS], ps)
    ys = out.grad_fn.saved_tensors[1 + 13:]                                      # (x, 13 weights, 13 post-ReLU outputs)
    masks = [(y > 0).cpu().numpy() for y in ys]
    assert rel(out.detach().cpu().numpy(), ref.stack_fwd(x, params)) < 1e-4
    out.backward(torch.from_numpy(dout).to(d))
    out_ref, g_ref = ref.stack_vjp_masked(x, params, dout, masks)
    assert rel(out.detach().cpu().numpy(), out_ref) < 1e-4
    for i, (dw, db) in enumerate(g_ref):
        assert rel(ps[2 * i].grad.cpu().numpy(), dw) < 1e-4, (i, 'dw')
        assert rel(ps[2 * i + 1].grad.cpu().numpy(), db) < 1e-4, (i, 'db')
    # the top layer's own ReLU backward: dout * (y > 0), and the bound it folds is max |dx| exactly
    yg = out.detach().contiguous()
    dg = torch.from_numpy(dout).to(d)
    dx, adx = ops.dilated_relu_bwd(dg, yg)
    assert torch.equal(dx, dg * (yg > 0)) and float(adx) == float(dx.abs().max())
