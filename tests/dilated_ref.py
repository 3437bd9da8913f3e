"""Float64 reference of the dilated conv2d stack (reference models/network.py:528-551) on the CPU: torch.nn.functional.conv2d with
dilation and SAME padding, independent of the HIP kernels.  Layouts as the kernels': activations NHWC [B,T,F,C], weights HWIO."""
import numpy as np
import torch

# (kernel [kh, kw], rate [rt, rf], cout) of the 13 layers
SPECS = [((1, 7), (1, 1), 128), ((7, 1), (1, 1), 128)] + [((5, 5), (r, 1), 128) for r in (4, 8, 16, 32)] + \
        [((5, 5), (r, r), 128) for r in (1, 2, 4, 8, 16, 32)] + [((5, 5), (1, 1), 4)]
NAMES = ['dilated/Conv'] + ['dilated/Conv_%d' % i for i in range(1, 13)]


def _t(a):
    return torch.as_tensor(np.asarray(a, np.float64))


def conv_pre(x, w, b, rate):
    """pre-ReLU sum: x [B,T,F,cin], w [kh,kw,cin,cout], b [cout] (torch float64) -> [B,T,F,cout]."""
    kh, kw = w.shape[:2]
    y = torch.nn.functional.conv2d(x.permute(0, 3, 1, 2), w.permute(3, 2, 0, 1), b, padding=((kh - 1) // 2 * rate[0], (kw - 1) // 2 * rate[1]),
                                   dilation=tuple(rate))
    return y.permute(0, 2, 3, 1)


def layer_fwd(x, w, b, rate):
    """numpy float64 relu(conv + b)."""
    return torch.relu(conv_pre(_t(x), _t(w), _t(b), rate)).numpy()


def layer_bwd(x, w, b, rate, dpre):
    """(dx, dw, db) of the pre-ReLU sum for the upstream gradient dpre of that sum (numpy float64)."""
    xt, wt, bt = (_t(a).requires_grad_(True) for a in (x, w, b))
    pre = conv_pre(xt, wt, bt, rate)
    pre.backward(_t(dpre))
    return xt.grad.numpy(), wt.grad.numpy(), bt.grad.numpy()


def stack_fwd(x, params, rates=None):
    """x [B,T,F] -> [B,T,4F] (feature f*4 + c); params [(w, b)] * 13 (numpy).  Float64."""
    rates = rates or [s[1] for s in SPECS]
    h = _t(x).unsqueeze(-1)
    for (w, b), r in zip(params, rates):
        h = torch.relu(conv_pre(h, _t(w), _t(b), r))
    B, T, F, C = h.shape
    return h.reshape(B, T, F * C).numpy()


def stack_vjp(x, params, dout, rates=None):
    """(out, [(dw, db)] * 13) of the stack for the upstream gradient dout [B,T,4F], by float64 autograd."""
    rates = rates or [s[1] for s in SPECS]
    ps = [(_t(w).requires_grad_(True), _t(b).requires_grad_(True)) for w, b in params]
    h = _t(x).unsqueeze(-1)
    for (w, b), r in zip(ps, rates):
        h = torch.relu(conv_pre(h, w, b, r))
    B, T, F, C = h.shape
    out = h.reshape(B, T, F * C)
    out.backward(_t(dout))
    return out.detach().numpy(), [(w.grad.numpy(), b.grad.numpy()) for w, b in ps]


def stack_fwd_masked(x, params, masks, rates=None):
    """stack_fwd with each layer's ReLU replaced by a GIVEN mask (see stack_vjp_masked)."""
    rates = rates or [s[1] for s in SPECS]
    h = _t(x).unsqueeze(-1)
    for (w, b), r, m in zip(params, rates, masks):
        h = conv_pre(h, _t(w), _t(b), r) * torch.as_tensor(np.asarray(m, np.float64))
    B, T, F, C = h.shape
    return h.reshape(B, T, F * C).numpy()


def stack_vjp_masked(x, params, dout, masks, rates=None):
    """stack_vjp with each layer's ReLU replaced by a GIVEN mask [B,T,F,C] (bool): the float64 arithmetic of the device's own
    activation pattern, so that a pre-activation within rounding of zero cannot fall the other way than on the device."""
    rates = rates or [s[1] for s in SPECS]
    ps = [(_t(w).requires_grad_(True), _t(b).requires_grad_(True)) for w, b in params]
    h = _t(x).unsqueeze(-1)
    for (w, b), r, m in zip(ps, rates, masks):
        h = conv_pre(h, w, b, r) * torch.as_tensor(np.asarray(m, np.float64))
    B, T, F, C = h.shape
    out = h.reshape(B, T, F * C)
    out.backward(_t(dout))
    return out.detach().numpy(), [(w.grad.numpy(), b.grad.numpy()) for w, b in ps]


def init_params(rng, specs=SPECS, bias_scale=0.05):
    """Xavier-uniform weights (the variables' initialiser) and small non-zero biases, float32."""
    out, cin = [], 1
    for (kh, kw), _, cout in specs:
        lim = np.sqrt(6.0 / (kh * kw * cin + kh * kw * cout))
        out.append((rng.uniform(-lim, lim, (kh, kw, cin, cout)).astype(np.float32), (bias_scale * rng.randn(cout)).astype(np.float32)))
        cin = cout
    return out
