"""Many recordings in one call: ctypes binding of libams_stitch_batch.so (include/ams_stitch_batch.h) and its tensor-level wrappers.

    lay = layout([len(x) for x in xs], L, H, S)   # host only: where every recording, chunk and block lies
    mix, lay = chunks_many(xs, L, H)              # [Ctot, L]: the chunks of ALL recordings, one after the other
    est = model.infer_chunks(mix)                 # [Ctot, S, L]: full batches, ceil(Ctot / B) model passes
    res = stitch_many(est, lay)                   # per recording (out [S, n_r], trk [C_r, S], Q [C_r - 1, S, S]): views

Every recording's results are bit-equal to ams_hip.stitch's on that recording alone.  The number of kernel launches does not depend on
the number of recordings: the tables that tell a workgroup which recording it works on are built here on the host (the lengths are known
there) and uploaded as ONE buffer per call and device.  Everything else is as in ams_hip/stitch.py: hand-written HIP kernels on torch's
current stream, torch for device memory and the stream only, no CPU path.  Definitions: DESIGN.md 4.9 and the header.
"""
import ctypes
import os

import numpy as np
import torch

from . import stitch as _st
from ._lib import AmsError, check, parse_header

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, 'libams_stitch_batch.so')
HEADER_PATH = os.path.normpath(os.path.join(_HERE, '..', '..', 'include', 'ams_stitch_batch.h'))
ABI_VERSION = 1            # include/ams_stitch_batch.h: ams_stitchb_abi_version()
MAX_SPEAKERS = _st.MAX_SPEAKERS
BLOCK = 1024               # samples per workgroup of the cross-fade

_vp = ctypes.c_void_p
_lib = None


def load():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise AmsError('libams_stitch_batch.so not found at %s -- the HIP extension is required (no CPU fallback); '
                       'run __graft_entry__.build()' % LIB_PATH)
    lib = ctypes.CDLL(LIB_PATH)             # (torch is imported above: one HIP runtime in the process, see _lib.load)
    for name, (ret, argtypes) in parse_header(HEADER_PATH).items():
        try:
            fn = getattr(lib, name)
        except AttributeError:
            raise AmsError('libams_stitch_batch.so does not export %s (declared in include/ams_stitch_batch.h)' % name)
        fn.restype = ret
        fn.argtypes = argtypes
    if lib.ams_stitchb_abi_version() != ABI_VERSION:
        raise AmsError('libams_stitch_batch.so ABI version mismatch: the library is %d, this binding is %d -- rebuild (make -C csrc)'
                       % (lib.ams_stitchb_abi_version(), ABI_VERSION))
    _lib = lib
    return lib


def _p(t):
    return _vp(t.data_ptr())


def _s():
    return _vp(torch.cuda.current_stream().cuda_stream)


def _chk(dtype, *ts):
    for t in ts:
        if not torch.is_tensor(t) or not t.is_cuda:
            raise AmsError('ams_hip.stitch_batch needs device tensors (there is no CPU fallback)')
        if t.dtype != dtype or not t.is_contiguous():
            raise AmsError('ams_hip.stitch_batch needs contiguous %s tensors, got %s %s' % (dtype, t.dtype, tuple(t.stride())))


def _up4(a):
    return (a + 3) // 4 * 4


class Layout(object):
    """Where R recordings lie (all numpy, host only; the names are the header's):
        R, L, H, S, Ctot, nblk, x_total, out_total                     ints
        n, C, x_off, out_off [R]; c_off, blk_off [R + 1]               int64
        chunk_rec [Ctot], blk_rec [nblk]                               int32
    tables(device) uploads them as one buffer (once per layout and device) and returns device views of it."""

    def __init__(self, lengths, L, H, S=None):
        _st.check_geometry(L, H)
        n = np.asarray([int(v) for v in lengths], np.int64).reshape(-1)
        if n.size < 1:
            raise ValueError('layout: at least one recording')
        if n.min() < 1:
            raise ValueError('layout: a recording needs at least one sample, got lengths %s' % (n[n < 1].tolist(),))
        self.R, self.L, self.H, self.S = int(n.size), int(L), int(H), None
        self.n = n
        self.C = 1 + np.maximum(0, -((L - n) // H))
        self.c_off = np.concatenate([[0], np.cumsum(self.C)]).astype(np.int64)
        self.x_off = np.concatenate([[0], np.cumsum(_up4(n))]).astype(np.int64)
        self.blk_off = np.concatenate([[0], np.cumsum((n + BLOCK - 1) // BLOCK)]).astype(np.int64)
        self.x_total, self.x_off = int(self.x_off[-1]), self.x_off[:-1]
        self.Ctot, self.nblk = int(self.c_off[-1]), int(self.blk_off[-1])
        if self.Ctot >= 1 << 31 or self.nblk >= 1 << 31:
            raise ValueError('layout: %d chunks and %d blocks: both must stay below 2^31' % (self.Ctot, self.nblk))
        rec = np.arange(self.R, dtype=np.int32)
        self.chunk_rec = np.repeat(rec, self.C)
        self.blk_rec = np.repeat(rec, np.diff(self.blk_off))
        self._dev = {}
        self.out_off, self.out_total = np.zeros(self.R, np.int64), 0
        if S is not None:
            self.set_sources(S)

    def set_sources(self, S):
        """Fix the number of sources, which sizes the output blocks: out_off[r] = S x_off[r] (a multiple of 4, and S n[r] fit in front
        of the next block).  A layout made without S gets it from the first stitch_many; tables uploaded before that are uploaded again."""
        if not 1 <= S <= MAX_SPEAKERS:
            raise ValueError('layout: 1 .. %d sources, got %d' % (MAX_SPEAKERS, S))
        if self.S == S:
            return self
        if self.S is not None:
            raise ValueError('layout: made for %d sources, asked for %d' % (self.S, S))
        self.S = int(S)
        self.out_off, self.out_total = S * self.x_off, S * self.x_total
        self._dev = {}
        return self

    def tables(self, device):
        """{name: device tensor}: views of ONE uploaded buffer (int64 tables first, the int32 ones behind them on 8-byte boundaries)."""
        key = str(torch.device(device))
        if key not in self._dev:
            wide = [('n', self.n), ('x_off', self.x_off), ('out_off', self.out_off), ('c_off', self.c_off), ('blk_off', self.blk_off)]
            narrow = [('chunk_rec', self.chunk_rec), ('blk_rec', self.blk_rec)]
            words = sum(a.size for _, a in wide) + sum((a.size + 1) // 2 for _, a in narrow)
            host = np.zeros(words, np.int64)
            at, where = 0, {}
            for name, a in wide:
                host[at:at + a.size] = a
                where[name] = (at, a.size, False)
                at += a.size
            for name, a in narrow:
                host[at:at + (a.size + 1) // 2].view(np.int32)[:a.size] = a
                where[name] = (at, a.size, True)
                at += (a.size + 1) // 2
            buf = torch.from_numpy(host).to(device)
            self._dev[key] = {name: (buf[a:a + (m + 1) // 2].view(torch.int32)[:m] if narrow_ else buf[a:a + m])
                              for name, (a, m, narrow_) in where.items()}
        return self._dev[key]

    def rec_chunks(self, r):
        """The global chunks of recording r as a slice."""
        return slice(int(self.c_off[r]), int(self.c_off[r + 1]))


def layout(lengths, L, H=None, S=None):
    """Host only: the tables of include/ams_stitch_batch.h for recordings of `lengths` samples (see Layout).  S may be left open until
    the outputs are laid out (Layout.set_sources)."""
    return Layout(lengths, L, _st.default_hop(L) if H is None else H, S)


def pack(xs, lay):
    """Device float32 [n_r] tensors -> the packed buffer [x_total] (recording r at x_off[r], zeros between): one torch.cat."""
    pad = torch.zeros(3, dtype=torch.float32, device=xs[0].device)
    parts = []
    for x, n in zip(xs, lay.n):
        parts.append(x)
        if n % 4:
            parts.append(pad[:4 - n % 4])
    return torch.cat(parts) if len(parts) > 1 else parts[0]


def chunks_packed(xp, lay):
    """The packed recordings xp [>= x_total] -> mix [Ctot, L]."""
    _chk(torch.float32, xp)
    if xp.dim() != 1 or xp.shape[0] < lay.x_off[-1] + lay.n[-1]:
        raise AmsError('chunks_packed: a 1-D buffer of at least %d samples, got %s' % (lay.x_off[-1] + lay.n[-1], tuple(xp.shape)))
    t = lay.tables(xp.device)
    mix = torch.empty((lay.Ctot, lay.L), dtype=torch.float32, device=xp.device)
    check(load().ams_stitchb_chunks(_p(xp), _p(t['n']), _p(t['x_off']), _p(t['c_off']), _p(t['chunk_rec']), _p(mix), lay.R, lay.Ctot,
                                    lay.L, lay.H, _s()), 'ams_stitchb_chunks')
    return mix


def chunks_many(xs, L, H=None, S=None):
    """xs: device float32 [n_r] tensors -> (mix [Ctot, L], layout): recording r's chunks are mix[c_off[r] : c_off[r + 1]].  S only sizes
    the output blocks of the layout; a caller that knows it passes it and saves stitch_many a second upload of the tables."""
    xs = list(xs)
    if not xs:
        raise ValueError('chunks_many: at least one recording')
    _chk(torch.float32, *xs)
    for x in xs:
        if x.dim() != 1 or x.device != xs[0].device:
            raise AmsError('chunks_many: every recording is a 1-D tensor on one device, got %s on %s' % (tuple(x.shape), x.device))
    lay = layout([x.shape[0] for x in xs], L, H, S)
    return chunks_packed(pack(xs, lay), lay), lay


def _est_ok(est, lay, what):
    _chk(torch.float32, est)
    if est.dim() != 3 or est.shape[0] != lay.Ctot or est.shape[2] != lay.L:
        raise AmsError('%s: est must be [%d, S, %d] for this layout, got %s' % (what, lay.Ctot, lay.L, tuple(est.shape)))
    if not 1 <= est.shape[1] <= MAX_SPEAKERS:
        raise AmsError('%s: 1 .. %d sources, got %d' % (what, MAX_SPEAKERS, est.shape[1]))


def border_stats_many(est, lay):
    """est [Ctot, S, L] -> Q [Ctot, S, S]: row g is the border between chunks g and g + 1 of one recording; zeros on a last chunk."""
    _est_ok(est, lay, 'border_stats_many')
    S = est.shape[1]
    t = lay.tables(est.device)
    lib = load()
    nbytes = lib.ams_stitchb_workspace_bytes(lay.Ctot, S, lay.L, lay.H)
    ws = torch.empty(max(nbytes // 4, 1), dtype=torch.float32, device=est.device)
    Q = torch.empty((lay.Ctot, S, S), dtype=torch.float32, device=est.device)
    check(lib.ams_stitchb_stats(_p(est), _p(t['chunk_rec']), _p(Q), lay.R, lay.Ctot, S, lay.L, lay.H, _p(ws), ws.numel() * 4, _s()),
          'ams_stitchb_stats')
    return Q


def tracks_many(Q, lay):
    """Q [Ctot, S, S] -> (rel [Ctot, S], trk [Ctot, S]) int32: the tracks restart at the identity on every recording's first chunk."""
    from .functional import _perm_table32
    _chk(torch.float32, Q)
    if Q.dim() != 3 or Q.shape[0] != lay.Ctot or Q.shape[1] != Q.shape[2] or not 1 <= Q.shape[1] <= MAX_SPEAKERS:
        raise AmsError('tracks_many: Q must be [%d, S, S] with S in 1 .. %d, got %s' % (lay.Ctot, MAX_SPEAKERS, tuple(Q.shape)))
    S = Q.shape[1]
    t = lay.tables(Q.device)
    perms = _perm_table32(S, Q.device)
    rel = torch.empty((lay.Ctot, S), dtype=torch.int32, device=Q.device)
    trk = torch.empty((lay.Ctot, S), dtype=torch.int32, device=Q.device)
    check(load().ams_stitchb_tracks(_p(Q), _p(perms), _p(t['c_off']), _p(t['chunk_rec']), _p(rel), _p(trk), lay.R, lay.Ctot, S,
                                    perms.shape[0], _s()), 'ams_stitchb_tracks')
    return rel, trk


def overlap_add_many(est, trk, lay, out=None):
    """est [Ctot, S, L], trk [Ctot, S] int32 -> the packed outputs [out_total]: recording r's [S, n_r] block at out_off[r].  out: a
    buffer to write into (what lies between the blocks is left as it is); default a new one."""
    _est_ok(est, lay, 'overlap_add_many')
    _chk(torch.int32, trk)
    S = est.shape[1]
    lay.set_sources(S)
    if tuple(trk.shape) != (lay.Ctot, S):
        raise AmsError('overlap_add_many: est [Ctot, %d, L] and trk [Ctot, %d] for a layout of %d sources, got %s and %s'
                       % (lay.S, lay.S, lay.S, tuple(est.shape), tuple(trk.shape)))
    if out is None:
        out = torch.empty(lay.out_total, dtype=torch.float32, device=est.device)
    _chk(torch.float32, out)
    if out.dim() != 1 or out.shape[0] < lay.out_off[-1] + S * lay.n[-1]:
        raise AmsError('overlap_add_many: out must hold %d samples, got %s' % (lay.out_off[-1] + S * lay.n[-1], tuple(out.shape)))
    t = lay.tables(est.device)
    w = _st._w_head(lay.L - lay.H, est.device)
    check(load().ams_stitchb_ola(_p(est), _p(trk), _p(w), _p(t['n']), _p(t['out_off']), _p(t['c_off']), _p(t['blk_rec']), _p(t['blk_off']),
                                 _p(out), lay.R, lay.Ctot, lay.nblk, S, lay.L, lay.H, _s()), 'ams_stitchb_ola')
    return out


def stitch_many(est, lay, packed=False):
    """est [Ctot, S, L] (the model's output for the chunks of chunks_many) -> [(out [S, n_r], trk [C_r, S], Q [C_r - 1, S, S])] per
    recording: views of three packed buffers.  Five launches in all; nothing synchronises with the host once the cross-fade table of
    this overlap length and the layout's tables are on the device.  packed: return (the packed outputs [out_total], that list)."""
    _est_ok(est, lay, 'stitch_many')
    S = est.shape[1]
    lay.set_sources(S)
    Q = border_stats_many(est, lay)
    trk = tracks_many(Q, lay)[1]
    out = overlap_add_many(est, trk, lay)
    sizes = lay.C.tolist()
    trks, Qs = trk.split(sizes), Q.split(sizes)
    res = []
    for r in range(lay.R):
        o, n = int(lay.out_off[r]), int(lay.n[r])
        res.append((out[o:o + S * n].view(S, n), trks[r], Qs[r][:-1]))
    return (out, res) if packed else res
