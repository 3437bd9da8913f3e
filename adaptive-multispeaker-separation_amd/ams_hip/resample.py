"""Sample-rate conversion: ctypes binding of libams_resample.so (include/ams_resample.h) and its tensor-level wrappers.

    x8 = from_pcm16(pcm, 44100, 8000)          # [M]: int16 frames [N, CH] decoded, mixed down and resampled in one kernel
    out = model.separate_recording(x8)         # [S, M]
    y = resample(out, 8000, 44100)[:, :N]      # [S, N]: back at the rate of the file

The definition is scipy.signal.resample_poly with its defaults (DESIGN.md 4.8 and the header): a Kaiser-windowed sinc of
20 max(up, down) + 1 taps, zero padding at both ends, zero phase.  Every function enqueues hand-written HIP kernels on torch's current
stream; torch provides device memory and the stream, nothing else.  There is no CPU path and no host synchronisation -- except the
first call for a ratio and device, which designs the filter on the host (numpy, float64) and uploads it (kept from then on).
"""
import ctypes
import math
import os

import numpy as np
import torch

from ._lib import AmsError, check, parse_header

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, 'libams_resample.so')
HEADER_PATH = os.path.normpath(os.path.join(_HERE, '..', '..', 'include', 'ams_resample.h'))
ABI_VERSION = 1            # include/ams_resample.h: ams_resample_abi_version()
MAX_RATIO = 1024
MAX_CHANNELS = 8

_vp = ctypes.c_void_p
_lib = None
_TAPS = {}                 # (up, down, device) -> the float32 filter on the device


def load():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise AmsError('libams_resample.so not found at %s -- the HIP extension is required (no CPU fallback); '
                       'run __graft_entry__.build()' % LIB_PATH)
    lib = ctypes.CDLL(LIB_PATH)             # (torch is imported above: one HIP runtime in the process, see _lib.load)
    for name, (ret, argtypes) in parse_header(HEADER_PATH).items():
        try:
            fn = getattr(lib, name)
        except AttributeError:
            raise AmsError('libams_resample.so does not export %s (declared in include/ams_resample.h)' % name)
        fn.restype = ret
        fn.argtypes = argtypes
    if lib.ams_resample_abi_version() != ABI_VERSION:
        raise AmsError('libams_resample.so ABI version mismatch: the library is %d, this binding is %d -- rebuild (make -C csrc)'
                       % (lib.ams_resample_abi_version(), ABI_VERSION))
    _lib = lib
    return lib


def _p(t):
    return _vp(t.data_ptr())


def _s():
    return _vp(torch.cuda.current_stream().cuda_stream)


def _chk(dtype, *ts):
    for t in ts:
        if not torch.is_tensor(t) or not t.is_cuda:
            raise AmsError('ams_hip.resample needs device tensors (there is no CPU fallback)')
        if t.dtype != dtype or not t.is_contiguous():
            raise AmsError('ams_hip.resample needs contiguous %s tensors, got %s %s' % (dtype, t.dtype, tuple(t.stride())))


def ratio(fs_in, fs_out):
    """(up, down) = (fs_out, fs_in) / gcd: the limits of include/ams_resample.h as a ValueError before anything is built or launched."""
    fs_in, fs_out = int(fs_in), int(fs_out)
    if fs_in < 1 or fs_out < 1:
        raise ValueError('sample rates must be positive, got %d and %d' % (fs_in, fs_out))
    g = math.gcd(fs_in, fs_out)
    up, down = fs_out // g, fs_in // g
    if max(up, down) > MAX_RATIO:
        raise ValueError('%d Hz -> %d Hz is the ratio %d / %d: both terms must be in 1 .. %d (the filter has 20 max(up, down) + 1 taps)'
                         % (fs_in, fs_out, up, down, MAX_RATIO))
    return up, down


def design(up, down):
    """float64 [20 m + 1], m = max(up, down): sinc with cutoff 1 / m of Nyquist, Kaiser window (beta 5.0), unit gain at DC, times up --
    scipy.signal.firwin(20 m + 1, 1 / m, window=('kaiser', 5.0)) * up, with numpy only."""
    m = max(int(up), int(down))
    half = 10 * m
    h = np.sinc((np.arange(2 * half + 1, dtype=np.float64) - half) / m) / m * np.kaiser(2 * half + 1, 5.0)
    return h / h.sum() * up


def out_len(n_in, up, down):
    """M = ceil(n_in up / down)."""
    if n_in < 1:
        raise ValueError('a signal needs at least one sample, got %d' % n_in)
    return -((-int(n_in) * int(up)) // int(down))


def _taps(up, down, device):
    key = (up, down, str(device))
    if key not in _TAPS:
        _TAPS[key] = torch.from_numpy(design(up, down).astype(np.float32)).to(device)
    return _TAPS[key]


def from_pcm16(pcm, fs_in, fs_out):
    """pcm [N, CH] int16 (interleaved frames, CH = 1 .. 8; [N] is one channel) -> float32 [M] at fs_out: the channels' int32 sum over
    32768 CH, filtered -- one kernel, no intermediate signal.  fs_in == fs_out decodes and mixes down only."""
    up, down = ratio(fs_in, fs_out)
    _chk(torch.int16, pcm)
    if pcm.dim() == 1:
        pcm = pcm.reshape(-1, 1)
    if pcm.dim() != 2 or pcm.shape[0] < 1 or not 1 <= pcm.shape[1] <= MAX_CHANNELS:
        raise AmsError('from_pcm16: frames [N, CH] with N >= 1 and CH in 1 .. %d, got %s' % (MAX_CHANNELS, tuple(pcm.shape)))
    N, CH = pcm.shape
    M = out_len(N, up, down)
    y = torch.empty((M,), dtype=torch.float32, device=pcm.device)
    if up == down:
        taps, ntaps = None, 0
    else:
        taps = _taps(up, down, pcm.device)
        ntaps = taps.shape[0]
    check(load().ams_resample_pcm16(_p(pcm), N, CH, _p(taps) if taps is not None else None, ntaps, up, down, _p(y), M, _s()),
          'ams_resample_pcm16')
    return y


def resample(x, fs_in, fs_out):
    """x [R, N] or [N] float32 -> [R, M] or [M] at fs_out; the rows may be further apart than N (a view of a wider tensor), the samples
    of a row may not.  fs_in == fs_out returns x itself."""
    up, down = ratio(fs_in, fs_out)
    if not torch.is_tensor(x) or not x.is_cuda:
        raise AmsError('ams_hip.resample needs device tensors (there is no CPU fallback)')
    if x.dtype != torch.float32 or x.dim() not in (1, 2) or x.shape[-1] < 1 or x.shape[0] < 1:
        raise AmsError('resample: float32 [R, N] or [N] with at least one sample, got %s %s' % (x.dtype, tuple(x.shape)))
    if x.stride(-1) != 1 or (x.dim() == 2 and x.shape[0] > 1 and x.stride(0) < x.shape[1]):
        raise AmsError('resample: the samples of a row must be contiguous and the rows must not overlap, got strides %s'
                       % (tuple(x.stride()),))
    if up == down:
        return x
    rows = 1 if x.dim() == 1 else x.shape[0]
    N = x.shape[-1]
    xs = N if x.dim() == 1 or rows == 1 else x.stride(0)
    M = out_len(N, up, down)
    y = torch.empty((rows, M) if x.dim() == 2 else (M,), dtype=torch.float32, device=x.device)
    taps = _taps(up, down, x.device)
    check(load().ams_resample_f32(_p(x), rows, N, xs, _p(taps), taps.shape[0], up, down, _p(y), M, M, _s()), 'ams_resample_f32')
    return y
