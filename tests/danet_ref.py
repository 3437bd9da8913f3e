"""float64 restatement of the reference's DANet-SCE cost (models/SC_V2.py:44-127) and of whole L41ModelV2 training steps, built from
the oracle's per-op restatements (oracle/ is frozen; this term is new).  Test infrastructure only, numpy only.

  V [B,T,F,E] un-normalised embeddings, y [B,T,F,S] masks (+1 / -1, possibly already weighted by the base class: network.py:381-396),
  mask [B,T,F] the silence mask (SC_V2.py:50-56) or None:   y_ab = y mask,   m = (y + 1) / 2 mask
  A[b,e,s]    = sum_tf V m / (1e-12 + sum_tf m)                                            (:71)
  a           = sigmoid(sum_e A V)                                                         (:82-84)
  cost_recons = mean_b mean_s mean_tf (X_non_mix - X_input a)^2                            (:86-91)
  sc_cost     = L41 cost on l2-normalised embeddings and l2-normalised speaker vectors, labels y_ab   (:97-121)
"""
import numpy as np

from oracle import dense, l41, separate, stft, step as ostep


def _sig(x):
    with np.errstate(over='ignore'):
        return 1.0 / (1.0 + np.exp(-x))


def silence_mask(X, thr):
    """SC_V2.py:51-53: log10(max_{t,f} |X| / |X|) < thr, per utterance.  [B,T,F] of 0/1."""
    ax = np.abs(X)
    with np.errstate(divide='ignore', invalid='ignore'):
        return (separate.log10(ax.max(axis=(1, 2), keepdims=True) / ax) < thr).astype(X.dtype)


def soft_masks(y, mask=None):
    m = (y + 1.0) / 2.0
    return m if mask is None else m * mask[..., None]


def recon_forward(V, m, X_input, X_nm):
    """-> cost, (A [B,E,S], den [B,S], a [B,T,F,S], r [B,T,F,S])."""
    den = 1e-12 + m.sum(axis=(1, 2))                                      # [B,S]
    A = np.einsum('btfe,btfs->bes', V, m) / den[:, None, :]
    a = _sig(np.einsum('bes,btfe->btfs', A, V))
    r = X_input[..., None] * a - X_nm
    return float((r * r).mean(axis=(1, 2)).mean(axis=-1).mean()), (A, den, a, r)


def recon_cost(V, m, X_input, X_nm):
    return recon_forward(V, m, X_input, X_nm)[0]


def recon_cost_bwd(V, m, X_input, X_nm):
    """Closed-form d cost_recons / d V (both paths: through the logits and through the attractors)."""
    B, T, F, S = m.shape
    _, (A, den, a, r) = recon_forward(V, m, X_input, X_nm)
    g = 2.0 * r * X_input[..., None] * a * (1.0 - a) / (B * S * T * F)     # d cost / d logit
    dA = np.einsum('btfs,btfe->bes', g, V)
    return np.einsum('btfs,bes->btfe', g, A) + np.einsum('btfs,bes->btfe', m, dA / den[:, None, :])


def sc_v2_cost(V, y, mask, X_input, X_nm, spk, I, want_grads=True):
    """SC_V2.cost.  -> total, (sc, recons)[, dV, dspk]."""
    y_ab = y if mask is None else y * mask[..., None]
    m = soft_masks(y, mask)
    E = V.shape[-1]
    Vn, inv = dense.l2norm_fwd(V.reshape(V.shape[:2] + (-1,)), E)
    sc = float(l41.l41_cost(Vn, y_ab, spk, I, True))
    rc = recon_cost(V, m, X_input, X_nm)
    if not want_grads:
        return sc + rc, (sc, rc)
    dVn, dspk = l41.l41_cost_bwd(Vn, y_ab, spk, I, True)
    dV = dense.l2norm_bwd(Vn, inv, dVn) + recon_cost_bwd(V, m, X_input, X_nm)
    return sc + rc, (sc, rc), dV, dspk


def _step(X, X_input, X_nm, Y, I, P, nb_layers, E, silence_thr, want_grads):
    V, cache = ostep.prediction_fwd(X, P, nb_layers, E, normalize=False)   # SC_V2.prediction: no Normalize layer
    mask = silence_mask(X, silence_thr) if silence_thr is not None else None
    out = sc_v2_cost(V, Y, mask, X_input, X_nm, P['speaker_centroids'], I, want_grads)
    if not want_grads:
        return out[0], out[1], V, Y
    cost, parts, dV, dspk = out
    grads = ostep.prediction_bwd(dV, cache, P, nb_layers)
    grads['speaker_centroids'] = dspk
    return cost, grads, V, Y, parts


def stft_l41v2_loss(x_mix, x_non_mix, I, P, W, hop, nb_layers, E, silence_thr=None, want_grads=True):
    """experiments.training.STFT_L41V2: |STFT| -> BLSTMs -> Conv1D -> SC_V2.cost (no pre_func / normalisation of the input)."""
    X, X_nm, _ = stft.stft_preprocessing(x_mix, x_non_mix, W, hop)
    Y, _ = separate.make_masks(X_nm, 1.0, -1.0)
    return _step(X, X, X_nm, Y, I, P, nb_layers, E, silence_thr, want_grads)


def front_l41v2_loss(x_mix, x_non_mix, I, P, hop, nb_layers, E, function_mask=None, silence_thr=None, want_grads=True):
    """experiments.training.front_L41V2: signed front representation; the base class weights y first (network.py:381-396), then
    SC_V2.cost applies its own silence mask (to y_ab and to m)."""
    B, S, L = x_non_mix.shape
    yf = ostep.front_rep(x_mix, x_non_mix, P, hop)
    X, X_nm = separate.split_front(yf, B, S)
    Y, _ = separate.make_masks(np.abs(X_nm), 1.0, -1.0)
    if function_mask is not None:
        Y = separate.function_mask(Y, X, function_mask)
    if silence_thr is not None:
        Y = separate.silence_loss_mask(Y, X, silence_thr)
    return _step(X, X, X_nm, Y, I, P, nb_layers, E, silence_thr, want_grads)
