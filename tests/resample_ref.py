"""The resampler's definition (include/ams_resample.h) restated in float64 numpy -- the yardstick of
tests/test_resample_host.py (which holds it to scipy.signal.resample_poly) and of the GPU tests.

    y[n] = sum_k h[n down + half - k up] x[k]     over 0 <= k < N with 0 <= n down + half - k up <= 2 half,   n < M = ceil(N up / down)
"""
import math

import numpy as np

# (up, down), in lowest terms as the library demands; 80 / 883 and 883 / 80 are the large-table pairs (20 * 883 + 1 = 17 661 taps)
PAIRS = [(1, 2), (2, 1), (1, 6), (80, 441), (441, 80), (320, 441), (80, 883), (883, 80)]


def ratio(fs_in, fs_out):
    g = math.gcd(fs_in, fs_out)
    return fs_out // g, fs_in // g


def design(up, down):
    m = max(up, down)
    half = 10 * m
    i = np.arange(2 * half + 1, dtype=np.float64) - half
    h = np.sinc(i / m) / m * np.kaiser(2 * half + 1, 5.0)
    return h / h.sum() * up


def out_len(N, up, down):
    return -((-N * up) // down)


def spans(N, up, down, n=None):
    """(P, lo, hi) per output sample (all of them, or the given ones): the samples lo .. hi reach output n, P = n down + half."""
    half = 10 * max(up, down)
    n = np.arange(out_len(N, up, down), dtype=np.int64) if n is None else np.asarray(n, dtype=np.int64)
    P = n * down + half
    lo = np.maximum(0, -((2 * half - P) // up))
    hi = np.minimum(N - 1, P // up)
    return P, lo, hi


def _apply(h, x, up, down, n=None, N=None, k0=0):
    """x holds the samples k0 .. k0 + x.shape[-1] - 1 of a signal of N samples (default: all of it)."""
    x = np.asarray(x)
    N = x.shape[-1] if N is None else N
    P, lo, hi = spans(N, up, down, n)
    assert lo.min() >= k0 and hi.max() < k0 + x.shape[-1]
    T = int((hi - lo + 1).max())
    k = lo[:, None] + np.arange(T)[None, :]
    ok = k <= hi[:, None]
    t = P[:, None] - k * up
    hh = np.where(ok, h[np.where(ok, t, 0)], 0.0)
    xx = x[..., np.where(ok, k - k0, 0)]
    return (hh * xx).sum(axis=-1)


def window(N, up, down, n):
    """(k0, k1): the samples k0 .. k1 - 1 are all that the outputs n reach."""
    P, lo, hi = spans(N, up, down, n)
    return int(lo.min()), int(hi.max()) + 1


def resample_window(xw, k0, N, up, down, n):
    """(y64, tolerance) for the outputs n of a signal of N samples of which xw holds k0 .. k0 + len(xw) - 1 (see window)."""
    h = design(up, down)
    xw = np.asarray(xw, np.float64)
    y = _apply(h, xw, up, down, n, N, k0)
    A = _apply(np.abs(h), np.abs(xw), up, down, n, N, k0)
    return y, (nb_taps(N, up, down, n) + 2) * 2.0 ** -24 * A


def resample(x, up, down, h=None, n=None):
    """float64 y [..., M] (or the outputs n only) from x [..., N]; h defaults to the float64 design."""
    h = design(up, down) if h is None else np.asarray(h, np.float64)
    return _apply(h, np.asarray(x, np.float64), up, down, n)


def bound(x, up, down, h=None, n=None):
    """A[n] = sum_k |h[.]| |x[k]|."""
    h = design(up, down) if h is None else np.asarray(h, np.float64)
    return _apply(np.abs(h), np.abs(np.asarray(x, np.float64)), up, down, n)


def nb_taps(N, up, down, n=None):
    """T[n]: the number of taps that reach the input for output n."""
    P, lo, hi = spans(N, up, down, n)
    return hi - lo + 1


def downmix32(pcm):
    """int16 [N, CH] -> float32 [N]: the int32 sum of a frame over float32(32768 CH), one float32 division."""
    pcm = np.asarray(pcm, np.int16)
    s = pcm.astype(np.int32).sum(axis=1, dtype=np.int32)
    return s.astype(np.float32) / np.float32(32768 * pcm.shape[1])


def from_pcm16(pcm, up, down, h=None, n=None):
    """float64 outputs of the float32 down-mix (for up = down = 1: the down-mix itself, as float64)."""
    x = downmix32(pcm)
    if up == down:
        return x.astype(np.float64)
    return resample(x, up, down, h, n)


def tolerance(x, up, down, n=None):
    """(T + 2) 2^-24 A per output: one rounding of each tap to float32, one per product, at most T - 1 in the sum."""
    N = np.asarray(x).shape[-1]
    return (nb_taps(N, up, down, n) + 2) * 2.0 ** -24 * bound(x, up, down, n=n)
