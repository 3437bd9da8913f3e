"""Sample-rate conversion of many recordings of mixed rates in one launch each way: ctypes binding of libams_resample_ragged.so
(include/ams_resample_ragged.h) and its tensor-level wrappers.

    xp, lay = to_model_rate(recs, fs_list, L=L, H=H, S=S)      # int16 frames [N_r, CH_r] or float32 [N_r], each at its own rate
    mix = stitch_batch.chunks_packed(xp, lay)                  # xp is the packed buffer of the layout: no pack, no cat
    ...
    outs = from_model_rate(out_packed, lay, rows, fs_out_list, n_out_list)      # [rows_r, n_out_r] views of one buffer

Every recording's result is bit-equal to ams_hip.resample's on that recording alone (from_pcm16 / resample, and the cut to n_out): both
libraries run the code of csrc/resample/resample_core.h.  One launch per call whatever the number of recordings; the job list is built
here on the host (lengths and rates are known there) and uploaded as ONE buffer per call.  Hand-written HIP kernels on torch's current
stream, torch for device memory and the stream only, no CPU path.  Definitions: DESIGN.md 4.12 and the header.
"""
import ctypes
import os

import numpy as np
import torch

from . import resample as _rs
from . import stitch_batch as _sb
from ._lib import AmsError, check, parse_header

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, 'libams_resample_ragged.so')
HEADER_PATH = os.path.normpath(os.path.join(_HERE, '..', '..', 'include', 'ams_resample_ragged.h'))
ABI_VERSION = 1            # include/ams_resample_ragged.h: ams_rsr_abi_version()
JOB_WORDS = 12             # int64 words per job record; the names of the header, in its order:
SRC, N_IN, ROWS, X_STRIDE, CHANNELS, UP, DOWN, TAP_OFF, DST, Y_STRIDE, N_KEEP, RESERVED = range(JOB_WORDS)
TILE = 256                 # outputs per workgroup
MAX_CHANNELS = _rs.MAX_CHANNELS

_vp = ctypes.c_void_p
_lib = None
_TAPS = {}                 # (the sorted ratios, device) -> (the float32 filters one after the other on the device, {ratio: offset})
_STAGE = {}                # device -> [page-locked host buffer the recordings are packed in, the event of the last upload from it]
STAGING_MAX = 1 << 30      # bytes: the largest packed input kept page-locked
LAUNCHES = 0               # kernel launches made through this module so far (every run entry point of the library is one launch)


def load():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise AmsError('libams_resample_ragged.so not found at %s -- the HIP extension is required (no CPU fallback); '
                       'run __graft_entry__.build()' % LIB_PATH)
    lib = ctypes.CDLL(LIB_PATH)             # (torch is imported above: one HIP runtime in the process, see _lib.load)
    for name, (ret, argtypes) in parse_header(HEADER_PATH).items():
        try:
            fn = getattr(lib, name)
        except AttributeError:
            raise AmsError('libams_resample_ragged.so does not export %s (declared in include/ams_resample_ragged.h)' % name)
        fn.restype = ret
        fn.argtypes = argtypes
    if lib.ams_rsr_abi_version() != ABI_VERSION:
        raise AmsError('libams_resample_ragged.so ABI version mismatch: the library is %d, this binding is %d -- rebuild (make -C csrc)'
                       % (lib.ams_rsr_abi_version(), ABI_VERSION))
    _lib = lib
    return lib


def _p(t):
    return _vp(t.data_ptr())


def _s():
    return _vp(torch.cuda.current_stream().cuda_stream)


def _np(a):
    return a.ctypes.data_as(_vp)


def _staging(nbytes, device):
    """[a page-locked host buffer of at least nbytes, the event of the last upload from it]: one per device, kept and grown, so that
    packing the recordings costs one host copy and the upload none.  The buffer is reused only after the upload that last read it has
    left it (a wait on that copy's event, before anything of this call is enqueued).  Above STAGING_MAX: a pageable buffer per call."""
    if nbytes > STAGING_MAX:
        return [torch.empty(nbytes, dtype=torch.uint8), None]
    key = str(torch.device(device))
    ent = _STAGE.get(key)
    if ent is not None and ent[1] is not None:
        ent[1].synchronize()
        ent[1] = None
    if ent is None or ent[0].numel() < nbytes:
        ent = _STAGE[key] = [torch.empty(max(nbytes, 1 << 20), dtype=torch.uint8, pin_memory=True), None]
    return ent


def _model_rate(fs_model):
    if fs_model is None:
        import config
        return int(config.fs)
    return int(fs_model)


def job(src, n_in, up, down, dst, rows=1, x_stride=None, channels=0, tap_off=0, y_stride=None, n_keep=None):
    """One job record (the header's 12 words) as a list; x_stride defaults to n_in, n_keep to M, y_stride to n_keep."""
    M = _rs.out_len(n_in, up, down)
    n_keep = M if n_keep is None else int(n_keep)
    return [int(src), int(n_in), int(rows), int(n_in if x_stride is None else x_stride), int(channels), int(up), int(down), int(tap_off),
            int(dst), int(n_keep if y_stride is None else y_stride), n_keep, 0]


def tables(jobs, taps_len):
    """jobs [J, 12] (host integers) -> (jobs int64 [J, 12], table int64 [(J + 1) + 12 J]: the prefix of tile counts, then the records) as
    the library builds them; AmsError for a list outside the header's limits."""
    jobs = np.ascontiguousarray(np.asarray(jobs, np.int64).reshape(-1, JOB_WORDS))
    J = jobs.shape[0]
    table = np.zeros((J + 1) + JOB_WORDS * max(J, 1), np.int64)
    check(load().ams_rsr_tables(_np(jobs), J, int(taps_len), _np(table)), 'ams_rsr_tables')
    return jobs, table


def taps_for(ratios, device):
    """The filters of the distinct ratios (up != down) one after the other in ONE device buffer, designed and uploaded once per (set of
    ratios, device) -> (taps float32 [>= 1], {(up, down): offset})."""
    want = tuple(sorted(set((int(u), int(d)) for u, d in ratios if u != d)))
    key = (want, str(torch.device(device)))
    if key not in _TAPS:
        parts, where, at = [], {}, 0
        for u, d in want:
            h = _rs.design(u, d).astype(np.float32)
            where[(u, d)] = at
            parts.append(h)
            at += h.shape[0]
        host = np.concatenate(parts) if parts else np.zeros(1, np.float32)
        _TAPS[key] = (torch.from_numpy(host).to(device), where)
    return _TAPS[key]


def run(x, pcm, taps, jobs, y):
    """ONE launch: the job list `jobs` [J, 12] (host) from the device tensor x (src counts bytes from its first element) into the float32
    device buffer y.  An invalid list is an AmsError before anything is uploaded or launched: y is left as it is."""
    global LAUNCHES
    for t in (x, taps, y):
        if not torch.is_tensor(t) or not t.is_cuda:
            raise AmsError('ams_hip.resample_ragged needs device tensors (there is no CPU fallback)')
    if x.dtype != (torch.int16 if pcm else torch.float32) or taps.dtype != torch.float32 or y.dtype != torch.float32 or not y.is_contiguous():
        raise AmsError('ams_hip.resample_ragged: %s input, float32 taps and a contiguous float32 output, got %s, %s, %s'
                       % ('int16' if pcm else 'float32', x.dtype, taps.dtype, y.dtype))
    lib = load()
    jobs, table = tables(jobs, taps.numel())
    fn, what = (lib.ams_rsr_run_pcm16, 'ams_rsr_run_pcm16') if pcm else (lib.ams_rsr_run_f32, 'ams_rsr_run_f32')
    if not _fits(jobs, pcm, y.numel()):                                    # (the run call says the same, after the table upload)
        raise AmsError('%s failed: AMS_E_INVALID_ARG' % what)
    dev_table = torch.from_numpy(table).to(y.device)
    check(fn(_p(x), _p(taps), taps.numel(), _np(jobs), jobs.shape[0], _p(dev_table), _p(y), y.numel(), _s()), what)
    LAUNCHES += 1
    return y


def _fits(jobs, pcm, y_len):
    """The run calls' own limits (kind of input, rows inside y), restated so that a refusal comes before the table upload."""
    ends = jobs[:, DST] + (jobs[:, ROWS] - 1) * jobs[:, Y_STRIDE] + jobs[:, N_KEEP]
    return bool(((jobs[:, CHANNELS] >= 1) == bool(pcm)).all() and (ends <= y_len).all())


def _ratio_of(r, fs_in, fs_out):
    try:
        return _rs.ratio(fs_in, fs_out)
    except ValueError as e:
        raise ValueError('recording %d: %s' % (r, e))


def model_lengths(lengths, fs_list, fs_model=None):
    """M_r = ceil(N_r up_r / down_r): the lengths at the model's rate, for a stitch_batch.layout made ahead of to_model_rate."""
    fm = _model_rate(fs_model)
    return [_rs.out_len(int(n), *_ratio_of(r, fs, fm)) for r, (n, fs) in enumerate(zip(lengths, fs_list))]


def to_model_rate(recs, fs_list, lay=None, L=None, H=None, S=None, device=None, fs_model=None):
    """recs: R recordings, all int16 frames [N_r] / [N_r, CH_r] (CH_r in 1 .. 8, it may differ from recording to recording) or all float32
    [N_r], host arrays or device tensors; fs_list: their R sample rates -> (x_packed float32 [lay.x_total], lay): recording r decoded,
    mixed down and brought to fs_model (default config.fs) at lay.x_off[r], zeros between the recordings -- the buffer
    stitch_batch.chunks_packed takes.  lay: stitch_batch.layout(model_lengths(...), L, H, S), made here from L, H, S when not given.
    Host inputs are packed into one host buffer and uploaded once; device inputs are read where they lie.  At most one data upload, one
    table upload and ONE launch, whatever R is; no host synchronisation after the uploads."""
    recs, fs_list = list(recs), list(fs_list)
    R = len(recs)
    if R < 1:
        raise ValueError('to_model_rate: at least one recording')
    if len(fs_list) != R:
        raise ValueError('to_model_rate: %d recordings and %d sample rates' % (R, len(fs_list)))
    fm = _model_rate(fs_model)
    ratios = [_ratio_of(r, fs, fm) for r, fs in enumerate(fs_list)]
    recs = [x if torch.is_tensor(x) else np.asarray(x) for x in recs]
    kinds = set(str(x.dtype).replace('torch.', '') for x in recs)
    if len(kinds) > 1 or kinds - {'int16', 'float32'}:
        raise ValueError('to_model_rate: all int16 frames [N, CH] or all float32 [N], got %s' % sorted(kinds))
    pcm = kinds == {'int16'}
    for r, x in enumerate(recs):
        if x.ndim not in ((1, 2) if pcm else (1,)) or x.shape[0] < 1:
            raise ValueError('to_model_rate: recording %d: float32 [N] or int16 frames [N, CH] of at least one sample, got %s %s'
                             % (r, x.dtype, tuple(x.shape)))
        if x.ndim == 2 and not 1 <= x.shape[1] <= MAX_CHANNELS:
            raise ValueError('to_model_rate: recording %d: 1 .. %d channels, got %d' % (r, MAX_CHANNELS, x.shape[1]))
    N = [int(x.shape[0]) for x in recs]
    CH = [(int(x.shape[1]) if x.ndim == 2 else 1) if pcm else 0 for x in recs]
    M = [_rs.out_len(n, u, d) for n, (u, d) in zip(N, ratios)]
    if lay is None:
        if L is None:
            raise ValueError('to_model_rate: a layout, or the chunk size L (and H, S) to make one')
        lay = _sb.layout(M, L, H, S)
    if lay.R != R or lay.n.tolist() != M:
        raise ValueError('to_model_rate: the layout holds recordings of %s samples, these come to %s' % (lay.n.tolist(), M))
    item = 2 if pcm else 4
    on_device = all(torch.is_tensor(x) and x.is_cuda for x in recs)
    if on_device:
        device = recs[0].device
        if any(x.device != device for x in recs):
            raise ValueError('to_model_rate: the recordings lie on different devices')
        keep = [x.contiguous() for x in recs]                              # read where they lie (kept alive until the launch is enqueued)
        base = keep[0]
        src = [x.data_ptr() - base.data_ptr() for x in keep]
    else:
        device = torch.device('cuda', torch.cuda.current_device()) if device is None else torch.device(device)
        words = [n * max(c, 1) for n, c in zip(N, CH)]
        off = np.concatenate([[0], np.cumsum(words)])
        stage = _staging(int(off[-1]) * item, device)
        host = stage[0][:int(off[-1]) * item].view(torch.int16 if pcm else torch.float32)
        flat = host.numpy()
        for x, o, w in zip(recs, off, words):
            flat[o:o + w] = (x.detach().cpu().numpy() if torch.is_tensor(x) else x).reshape(-1)
        base = host.to(device, non_blocking=True)                          # ONE upload, straight from the page-locked buffer
        if stage[0].is_pinned():
            stage[1] = torch.cuda.Event()
            stage[1].record()
        keep = [base]
        src = [int(o) * item for o in off[:-1]]
    taps, where = taps_for(ratios, device)
    jobs = [job(src[r], N[r], ratios[r][0], ratios[r][1], lay.x_off[r], channels=CH[r], tap_off=where.get(ratios[r], 0)) for r in range(R)]
    xp = torch.zeros(lay.x_total, dtype=torch.float32, device=device)
    run(base.reshape(-1), pcm, taps, jobs, xp)
    del keep
    return xp, lay


def from_model_rate(out_packed, lay, rows, fs_out_list, n_out_list, fs_model=None):
    """out_packed: the packed outputs of stitch_batch.overlap_add_many (recording r's [S, n_r] block at lay.out_off[r], row stride n_r);
    rows: rows_r <= S per recording (an int: the same for all) -- the first rows_r tracks; fs_out_list, n_out_list: the rate every
    recording goes to and the samples kept of every row (1 .. ceil(n_r up / down)) -> [float32 [rows_r, n_out_r]]: views of ONE new
    buffer that holds the blocks one after the other.  ONE launch.  A recording with fs_out == fs_model gets a view of out_packed (its
    first rows_r rows, n_out not looked at) and no job."""
    R = lay.R
    rows = [int(rows)] * R if np.ndim(rows) == 0 else [int(v) for v in rows]
    fs_out_list, n_out_list = list(fs_out_list), list(n_out_list)
    if not (len(rows) == len(fs_out_list) == len(n_out_list) == R):
        raise ValueError('from_model_rate: a layout of %d recordings, %d row counts, %d sample rates and %d lengths'
                         % (R, len(rows), len(fs_out_list), len(n_out_list)))
    if lay.S is None:
        raise ValueError('from_model_rate: the layout has no number of sources yet (Layout.set_sources)')
    fm = _model_rate(fs_model)
    ratios = [_ratio_of(r, fm, fs) for r, fs in enumerate(fs_out_list)]
    for r in range(R):
        if not 1 <= rows[r] <= lay.S:
            raise ValueError('from_model_rate: recording %d: 1 .. %d rows, got %d' % (r, lay.S, rows[r]))
        u, d = ratios[r]
        if u != d and not 1 <= int(n_out_list[r]) <= _rs.out_len(int(lay.n[r]), u, d):
            raise ValueError('from_model_rate: recording %d: %d samples at %d Hz give 1 .. %d at %d Hz, asked for %d'
                             % (r, lay.n[r], fm, _rs.out_len(int(lay.n[r]), u, d), fs_out_list[r], n_out_list[r]))
    if not torch.is_tensor(out_packed) or not out_packed.is_cuda:
        raise AmsError('ams_hip.resample_ragged needs device tensors (there is no CPU fallback)')
    if out_packed.dtype != torch.float32 or out_packed.dim() != 1 or not out_packed.is_contiguous() \
            or out_packed.shape[0] < lay.out_off[-1] + lay.S * lay.n[-1]:
        raise AmsError('from_model_rate: a contiguous float32 buffer of at least %d samples, got %s %s'
                       % (lay.out_off[-1] + lay.S * lay.n[-1], out_packed.dtype, tuple(out_packed.shape)))
    taps, where = taps_for(ratios, out_packed.device)
    jobs, at, place = [], 0, []
    for r in range(R):
        u, d = ratios[r]
        if u == d:
            place.append(None)
            continue
        n, k = int(lay.n[r]), int(n_out_list[r])
        jobs.append(job(4 * int(lay.out_off[r]), n, u, d, at, rows=rows[r], tap_off=where[(u, d)], n_keep=k))
        place.append((at, k))
        at += rows[r] * k
    y = None
    if jobs:
        y = torch.empty(at, dtype=torch.float32, device=out_packed.device)
        run(out_packed, False, taps, jobs, y)
    res = []
    for r in range(R):
        if place[r] is None:
            o, n = int(lay.out_off[r]), int(lay.n[r])
            res.append(out_packed[o:o + rows[r] * n].view(rows[r], n))
        else:
            o, k = place[r]
            res.append(y[o:o + rows[r] * k].view(rows[r], k))
    return res
