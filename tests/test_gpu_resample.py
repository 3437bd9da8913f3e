"""GPU: the resampling kernels (include/ams_resample.h, ams_hip/resample.py) against the float64 restatement tests/resample_ref.py,
inside fenced buffers (tests/fenced.py: NaN-filled outputs, red zones, odd bases).

  * indexing, bit for bit: a unit impulse must come out as the float32 filter itself, for every pair, at both ends of the signal, for
    signals shorter than the filter, through resample() and through from_pcm16();
  * accuracy under the derived bound |y - y64| <= (T + 2) 2^-24 A (one rounding of each tap to float32, one per product, at most
    T - 1 in the sum; T taps reach the input, A = sum |h| |x|), the same bits from a second call, +0.0 from silence;
  * PCM decoding and the down-mix for 1, 2, 3 and 8 channels, full-scale frames, two bases;
  * positions past 2^31: 26.8 M frames at 80 / 441;
  * every limit of the header as AMS_E_INVALID_ARG with the output untouched.

80 / 883 and 883 / 80 stand where the issue that asked for this named 80 / 882 and 882 / 80: those are not in lowest terms, which the
library refuses (gcd(up, down) = 1); 883 is prime, and the filter table is one period longer."""
import ctypes

import numpy as np
import pytest

from tests import resample_ref as ref
from tests.fenced import PATTERN, Fence

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

_H32 = {}


def _h32(up, down):
    if (up, down) not in _H32:
        _H32[(up, down)] = ref.design(up, down).astype(np.float32)
    return _H32[(up, down)]


def _rates(up, down):
    """Two rates whose ratio is up / down (the wrappers take rates)."""
    return down, up


def _bits(a):
    a = a.cpu().numpy() if torch.is_tensor(a) else np.asarray(a, np.float32)
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


@pytest.mark.parametrize('up,down', ref.PAIRS)
def test_impulse_comes_out_as_the_filter(up, down):
    from ams_hip import resample
    fi, fo = _rates(up, down)
    assert resample.ratio(fi, fo) == (up, down)
    h = _h32(up, down)
    half = 10 * max(up, down)
    for N in (1, 2, 37, 1000):
        M = ref.out_len(N, up, down)
        for k0 in sorted({0, 1, N - 1, N // 2} & set(range(N))):
            idx = np.arange(M, dtype=np.int64) * down + half - k0 * up
            ok = (idx >= 0) & (idx <= 2 * half)
            want = np.where(ok, h[np.where(ok, idx, 0)], np.float32(0.0)).astype(np.float32)
            x = np.zeros(N, np.float32)
            x[k0] = 1.0
            with Fence() as fence:
                for base in (0, 4):
                    y = resample.resample(fence.dev(x, base=base), fi, fo)
                    assert y.shape == (M,) and np.array_equal(_bits(y), _bits(want)), (N, k0, base)
                y = resample.resample(fence.dev(np.stack([x, x]), base=4), fi, fo)
                assert y.shape == (2, M) and np.array_equal(_bits(y), _bits(np.stack([want, want]))), (N, k0)
                for ch in (1, 2, 3):
                    pcm = np.zeros((N, ch), np.int16)
                    pcm[k0] = 16384                                # the down-mix is exactly 0.5, and 0.5 h is exact
                    y = resample.from_pcm16(fence.dev(pcm, dtype=np.int16, base=0 if ch != 2 else 4), fi, fo)
                    assert y.shape == (M,) and np.array_equal(_bits(y), _bits(np.float32(0.5) * want)), (N, k0, ch)


@pytest.mark.parametrize('up,down', ref.PAIRS)
def test_accuracy_under_the_derived_bound(up, down):
    from ams_hip import resample
    fi, fo = _rates(up, down)
    rng = np.random.RandomState(100 + up + down)
    worst = 0.0
    cases = [(N, rows, 0) for N in (37, 1000, 4099) for rows in (1, 2, 6)] + [(1000, 3, 77)]      # (.., extra row stride)
    for N, rows, extra in cases:
        wide = (0.1 * rng.randn(rows, N + extra)).astype(np.float32)
        x = wide[:, :N]
        y64 = ref.resample(x, up, down)
        tol = ref.tolerance(x, up, down)
        assert y64.shape == (rows, ref.out_len(N, up, down)) and tol.min() > 0
        with Fence() as fence:
            xd = fence.dev(wide)[:, :N]
            assert xd.stride(0) == N + extra
            y = resample.resample(xd, fi, fo)
            again = resample.resample(xd, fi, fo)
            y1 = resample.resample(fence.dev(x[0], base=4), fi, fo) if rows > 1 else None
            zero = resample.resample(fence.dev(np.zeros((rows, N), np.float32)), fi, fo)
        got = y.cpu().numpy()
        assert got.shape == y64.shape and np.isfinite(got).all()
        r = float((np.abs(got - y64) / tol).max())
        worst = max(worst, r)
        assert r <= 1.0, (N, rows, extra, r)
        assert np.array_equal(_bits(y), _bits(again))
        if y1 is not None:                                          # a row of a batch is that row alone, whatever its base
            assert np.array_equal(_bits(y1), _bits(got[0]))
        assert not _bits(zero).any()
    print('resample %d / %d: worst |y - y64| / bound = %.3f' % (up, down, worst))


@pytest.mark.parametrize('channels', [1, 2, 3, 8])
def test_pcm16_decode_and_downmix(channels):
    from ams_hip import resample
    rng = np.random.RandomState(channels)
    N = 1000
    pcm = rng.randint(-32768, 32768, size=(N, channels)).astype(np.int16)
    pcm[0], pcm[1], pcm[N - 1] = -32768, 32767, -32768
    pcm[2, 0] = 32767
    x32 = ref.downmix32(pcm)
    assert x32[0] == -1.0 and x32.dtype == np.float32
    worst = 0.0
    for base in (0, 4):
        with Fence() as fence:
            d = fence.dev(pcm, dtype=np.int16, base=base)
            y = resample.from_pcm16(d, 8000, 8000)
            assert y.shape == (N,) and np.array_equal(_bits(y), _bits(x32)), base
            if channels == 1:
                assert np.array_equal(_bits(resample.from_pcm16(d.reshape(-1), 8000, 8000)), _bits(x32))
            for up, down in ((1, 2), (80, 441)):
                y = resample.from_pcm16(d, down, up)
                y64 = ref.from_pcm16(pcm, up, down)
                tol = ref.tolerance(x32, up, down)
                r = float((np.abs(y.cpu().numpy() - y64) / tol).max())
                worst = max(worst, r)
                assert y.shape == y64.shape and r <= 1.0, (base, up, down, r)
                assert np.array_equal(_bits(y), _bits(resample.from_pcm16(d, down, up)))
    print('from_pcm16, %d channels: worst |y - y64| / bound = %.3f' % (channels, worst))


def _pattern(k):
    """A fixed pseudo-random int16 for every sample index (int64 arithmetic, the same in torch and numpy)."""
    return ((k * 7919 + (k >> 7) * 104729 + (k >> 15) * 15485863) % 65521) - 32760


@pytest.mark.timeout(300)
def test_positions_past_2_to_the_31():
    from ams_hip import resample
    up, down = 80, 441
    N, M = 441 * 60883, 80 * 60883                                 # the smallest multiple of 441 that satisfies the line below
    assert (M - 1) * down + 10 * down >= 2 ** 31 + 441 * 1000 > (M - 80 - 1) * down + 10 * down and M == ref.out_len(N, up, down)
    with Fence() as fence:
        pcm = torch.empty((N, 1), dtype=torch.int16, device='cuda')
        pcm.copy_(_pattern(torch.arange(N, dtype=torch.int64, device='cuda')).to(torch.int16).reshape(N, 1))
        y = resample.from_pcm16(pcm, 44100, 8000)
        assert y.shape == (M,)
        assert not bool(torch.isnan(y).any())
        head, tail = y[:256].cpu().numpy(), y[M - 1000:].cpu().numpy()
    worst = 0.0
    for n, got in ((np.arange(256), head), (np.arange(M - 1000, M), tail)):
        k0, k1 = ref.window(N, up, down, n)
        xw = ref.downmix32(_pattern(np.arange(k0, k1, dtype=np.int64)).astype(np.int16).reshape(-1, 1))
        y64, tol = ref.resample_window(xw, k0, N, up, down, n)
        r = float((np.abs(got - y64) / tol).max())
        worst = max(worst, r)
        assert r <= 1.0, (int(n[0]), r)
    assert (int(n[-1]) * down + 10 * down) >= 2 ** 31
    print('past 2^31: worst |y - y64| / bound = %.3f' % worst)


def test_limits_are_invalid_arg_and_leave_the_output_alone():
    from ams_hip import _lib, resample
    lib = resample.load()
    INVALID = -1
    assert '#define AMS_E_INVALID_ARG (-1)' in open(_lib.HEADER_PATH).read()
    vp = ctypes.c_void_p
    N, up, down = 1000, 80, 441
    M = ref.out_len(N, up, down)
    nt = 20 * 441 + 1
    with Fence() as fence:
        x = fence.dev(np.zeros((2, N), np.float32))
        pcm = fence.dev(np.zeros((N, 2), np.int16), dtype=np.int16)
        taps = fence.dev(_h32(up, down))
        y = torch.empty((2, M), dtype=torch.float32, device='cuda')
        X, P, T, Y, st = vp(x.data_ptr()), vp(pcm.data_ptr()), vp(taps.data_ptr()), vp(y.data_ptr()), vp(0)

        def f32(x=X, rows=2, n_in=N, xs=N, taps=T, ntaps=nt, up=up, down=down, y=Y, n_out=M, ys=M):
            return lib.ams_resample_f32(x, rows, n_in, xs, taps, ntaps, up, down, y, n_out, ys, st)

        def p16(pcm=P, n_in=N, ch=2, taps=T, ntaps=nt, up=up, down=down, y=Y, n_out=M):
            return lib.ams_resample_pcm16(pcm, n_in, ch, taps, ntaps, up, down, y, n_out, st)

        bad = [f32(x=None), f32(taps=None), f32(y=None), f32(up=0), f32(down=0), f32(up=1025, ntaps=20 * 1025 + 1),
               f32(down=1025, ntaps=20 * 1025 + 1), f32(up=80, down=882, ntaps=20 * 882 + 1, n_out=ref.out_len(N, 40, 441)),
               f32(ntaps=nt - 1), f32(ntaps=nt + 1), f32(rows=0), f32(n_in=0), f32(n_out=M - 1), f32(n_out=M + 1), f32(xs=N - 1),
               f32(ys=M - 1),
               p16(pcm=None), p16(y=None), p16(taps=None), p16(ch=0), p16(ch=9), p16(up=0), p16(down=1025), p16(up=2, down=4),
               p16(ntaps=nt + 2), p16(n_in=0), p16(n_out=M + 1), p16(up=1, down=1, taps=None, n_out=N + 1)]
        assert bad == [INVALID] * len(bad), bad
        torch.cuda.synchronize()
        assert bool((y.view(torch.int32) == PATTERN).all())
        assert f32() == 0 and p16() == 0                             # and the same arguments, valid, go through
        torch.cuda.synchronize()
        assert not bool(torch.isnan(y[0]).any())
