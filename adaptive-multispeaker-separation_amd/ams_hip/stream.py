"""Live streams: ctypes binding of libams_stream.so (include/ams_stream.h) and the stateful separator on top of it.

    sep = StreamSeparator(infer, slots, S, L, H)   # infer: mix [rows, L] -> est [rows, S, L], any callable (a model's infer_chunks)
    outs = sep.push([block_0, None, block_2])      # per slot a float32 [k] block (tensor or numpy, k >= 0) or None -> [S, m_s] views
    last = sep.close(0)                            # what is left of stream 0: the stream's outputs, put together, are [S, N]
    sep.reset(0)                                   # slot 0 takes a new stream

A stream is separated as it arrives, one chunk (L samples) behind: chunk c is cut once sample c H + L - 1 is there, separated together
with the ready chunks of ALL streams in one call of `infer`, tracked against the chunk before it and cross-faded, and H more samples
leave.  The output is bit-equal to ams_hip.stitch.stitch on the stream's chunk estimates.  What a stream carries from push to push (the
samples no chunk has taken yet, the last chunk's tail and track permutation) stays on the device; the lengths and counters stay on the
host, so a push never waits for the device: at most two host-to-device copies (the table of the push and, for host blocks, the packed
samples), no copy back, six launches whatever the number of streams, chunks per stream or block sizes.  Everything else is as in
ams_hip/stitch.py: hand-written HIP kernels on torch's current stream, torch for device memory and the stream only, no CPU path.
Definitions: DESIGN.md 4.15 and the header.
"""
import ctypes
import os

import numpy as np
import torch

from . import stitch as _st
from ._lib import AmsError, check, parse_header

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, 'libams_stream.so')
HEADER_PATH = os.path.normpath(os.path.join(_HERE, '..', '..', 'include', 'ams_stream.h'))
ABI_VERSION = 1            # include/ams_stream.h: ams_stream_abi_version()
MAX_SPEAKERS = _st.MAX_SPEAKERS
ENTRY = 12                 # AMS_STREAM_ENTRY: int32 words per table entry
FIRST, CLOSING = 1, 2      # AMS_STREAM_FIRST, AMS_STREAM_CLOSING
FEED_LAUNCHES, ABSORB_LAUNCHES = 2, 4

_vp = ctypes.c_void_p
_lib = None


class StreamError(AmsError):
    """The library is missing or refuses a call, or `infer` returned something else than float32 [rows, S, L] on the device.  After an
    error inside push or close the slots that took part are in no defined state: reset them."""


def load():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise StreamError('libams_stream.so not found at %s -- the HIP extension is required (no CPU fallback); '
                          'run __graft_entry__.build()' % LIB_PATH)
    lib = ctypes.CDLL(LIB_PATH)             # (torch is imported above: one HIP runtime in the process, see _lib.load)
    for name, (ret, argtypes) in parse_header(HEADER_PATH).items():
        try:
            fn = getattr(lib, name)
        except AttributeError:
            raise StreamError('libams_stream.so does not export %s (declared in include/ams_stream.h)' % name)
        fn.restype = ret
        fn.argtypes = argtypes
    if lib.ams_stream_abi_version() != ABI_VERSION:
        raise StreamError('libams_stream.so ABI version mismatch: the library is %d, this binding is %d -- rebuild (make -C csrc)'
                          % (lib.ams_stream_abi_version(), ABI_VERSION))
    _lib = lib
    return lib


def launch_count():
    """Kernel launches libams_stream.so has enqueued in this process so far."""
    return int(load().ams_stream_launch_count())


def _p(t):
    return _vp(t.data_ptr())


def _s():
    return _vp(torch.cuda.current_stream().cuda_stream)


class Plan(object):
    """One push, host only (numpy; the names are the header's):
        slots [n]                      the slots that take part, in table order
        table [n, ENTRY] int32         slot, x_off, k, pend, rows, row0, out_off, m, flags, 0, 0, 0
        rows, max_rows, x_total, out_total, max_m                          ints
        N, D [n]                       samples received and chunks done AFTER the push"""


def plan(slots, N, D, k, closing, L, H):
    """The arithmetic of one push for the streams in `slots` (distinct ints): N, D their samples received and chunks done so far, k
    their new samples (>= 0), closing whether each ends with this push.  A stream cuts chunk D while N >= D H + L; a closing stream with
    N > 0 also cuts a last chunk filled up with zeros if D == 0 or N > (D - 1) H + L, and its output reaches to N.  Raises ValueError
    for a packed size of 2^31 or more."""
    _st.check_geometry(L, H)
    n = len(slots)
    if not (n == len(N) == len(D) == len(k) == len(closing)):
        raise ValueError('plan: one N, D, k and closing flag per slot')
    if len(set(int(s) for s in slots)) != n:
        raise ValueError('plan: a slot takes part once, got %s' % (list(slots),))
    p = Plan()
    p.slots = [int(s) for s in slots]
    p.table = np.zeros((n, ENTRY), np.int32)
    p.N, p.D = np.zeros(n, np.int64), np.zeros(n, np.int64)
    x_off = row0 = out_off = 0
    p.max_rows = p.max_m = 0
    for i in range(n):
        n0, d0, ki = int(N[i]), int(D[i]), int(k[i])
        if ki < 0 or n0 < 0 or d0 < 0 or not 0 <= n0 - d0 * H < L:
            raise ValueError('plan: slot %d: N = %d, D = %d, k = %d is no state of a stream with L = %d, H = %d' % (slots[i], n0, d0, ki, L, H))
        n1 = n0 + ki
        rows = (n1 - d0 * H - L) // H + 1 if n1 >= d0 * H + L else 0
        m = rows * H
        flags = FIRST if d0 == 0 else 0
        if closing[i]:
            flags |= CLOSING
            d1 = d0 + rows
            if n1 > 0 and (d1 == 0 or n1 > (d1 - 1) * H + L):
                rows += 1
            m = n1 - d0 * H
        if x_off + ki >= 1 << 31 or out_off + m >= 1 << 31:
            raise ValueError('plan: a push of more than %d samples in and %d out: the packed sizes of one push must stay below 2^31'
                             % (x_off + ki, out_off + m))
        p.table[i, :9] = (p.slots[i], x_off, ki, n0 - d0 * H, rows, row0, out_off, m, flags)
        p.N[i], p.D[i] = n1, d0 + rows
        x_off, row0, out_off = x_off + ki, row0 + rows, out_off + m
        p.max_rows, p.max_m = max(p.max_rows, rows), max(p.max_m, m)
    p.rows, p.x_total, p.out_total = row0, x_off, out_off
    return p


class StreamSeparator(object):
    """`slots` parallel streams of mono float32 samples at the rate of `infer`'s model, S sources, chunks of L samples H apart (see the
    module docstring).  Attributes: slots, S, L, H, latency_samples (= L: a sample leaves once the chunk behind its own is complete),
    passes (calls of infer so far).  keep_rows=True keeps the rows of the last push for inspection: last = {'plan', 'mix', 'est', 'Q',
    'trk'} (Q [rows, S, S]: a row's border with the chunk before it, zeros for a stream's chunk 0; trk [rows, S])."""

    def __init__(self, infer, slots, S, L, H=None, device=None, keep_rows=False):
        if not callable(infer):
            raise ValueError('StreamSeparator: infer must be callable: mix [rows, L] -> est [rows, S, L]')
        H = _st.default_hop(L) if H is None else int(H)
        _st.check_geometry(L, H)
        if slots < 1 or slots > 65535:
            raise ValueError('StreamSeparator: 1 .. 65535 streams, got %d' % slots)
        if not 1 <= S <= MAX_SPEAKERS:
            raise ValueError('StreamSeparator: 1 .. %d sources, got %d' % (MAX_SPEAKERS, S))
        self.infer, self.slots, self.S, self.L, self.H = infer, int(slots), int(S), int(L), H
        self.latency_samples = self.L
        self.keep_rows, self.last, self.passes = keep_rows, None, 0
        self._N, self._D, self._emitted = [0] * slots, [0] * slots, [0] * slots
        self._closed = [False] * slots
        self._state = None
        self.device = None if device is None else torch.device(device)

    # ---- host side
    def received(self, s):
        return self._N[self._slot(s)]

    def emitted(self, s):
        return self._emitted[self._slot(s)]

    def closed(self, s):
        return self._closed[self._slot(s)]

    def _slot(self, s):
        if not 0 <= int(s) < self.slots:
            raise ValueError('slot %s: this separator has slots 0 .. %d' % (s, self.slots - 1))
        return int(s)

    def arm(self):
        """The state buffer, the cross-fade table and the permutations: made with the first push (the device is known then), or by this
        call ahead of it.  One launch (every slot is reset), once."""
        if self._state is not None:
            return
        from .functional import _perm_table32
        if self.device is None:
            self.device = torch.device('cuda', torch.cuda.current_device())
        lib = load()
        nbytes = lib.ams_stream_state_bytes(self.slots, self.S, self.L, self.H)
        if nbytes == 0:
            raise StreamError('ams_stream_state_bytes refuses slots = %d, S = %d, L = %d, H = %d' % (self.slots, self.S, self.L, self.H))
        self._state = torch.empty(nbytes // 4, dtype=torch.float32, device=self.device)
        self._w = _st._w_head(self.L - self.H, self.device)
        self._perms = _perm_table32(self.S, self.device)
        self._dummy = torch.zeros(4, dtype=torch.float32, device=self.device)
        check(lib.ams_stream_reset(_p(self._state), self.slots, self.S, self.L, self.H, 0, self.slots, _s()), 'ams_stream_reset')

    def _blocks(self, blocks):
        """Validation before anything is uploaded: [(slot, block)] for the slots that take part."""
        if not isinstance(blocks, (list, tuple)) or len(blocks) != self.slots:
            raise ValueError('push: a list of %d blocks (one per slot, None for a slot without samples), got %s'
                             % (self.slots, 'a list of %d' % len(blocks) if isinstance(blocks, (list, tuple)) else type(blocks).__name__))
        taking = []
        for s, b in enumerate(blocks):
            if b is None:
                continue
            if not torch.is_tensor(b):
                if not isinstance(b, np.ndarray):
                    raise ValueError('push: slot %d: a float32 tensor or numpy array [k], got %s' % (s, type(b).__name__))
            kind = str(b.dtype).replace('torch.', '')
            if kind != 'float32':
                raise ValueError('push: slot %d: float32 samples, got %s (int16 input is not built: convert first)' % (s, kind))
            if b.ndim != 1:
                raise ValueError('push: slot %d: one channel [k], got %s' % (s, tuple(b.shape)))
            if self._closed[s]:
                raise ValueError('push: slot %d is closed: reset(%d) before it takes a new stream' % (s, s))
            taking.append((s, b))
        return taking

    def _pack(self, taking, total):
        """The new samples of all streams as one device buffer: host blocks are packed on the host and uploaded once."""
        parts = [b for _, b in taking if b.shape[0] > 0]
        if total == 0:
            return self._dummy
        if all(torch.is_tensor(b) and b.is_cuda for b in parts):
            parts = [b.to(self.device).contiguous() for b in parts]
            return parts[0] if len(parts) == 1 else torch.cat(parts)
        host = np.empty(total, np.float32)
        at = 0
        for b in parts:
            host[at:at + b.shape[0]] = b.detach().cpu().numpy() if torch.is_tensor(b) else b
            at += b.shape[0]
        return torch.from_numpy(host).to(self.device)

    def feed(self, pl, table, x):
        """ams_stream_feed for the plan `pl`, its table on the device and the packed samples x -> mix [rows, L] (two launches)."""
        mix = torch.empty((max(pl.rows, 1), self.L), dtype=torch.float32, device=self.device)
        check(load().ams_stream_feed(_p(self._state), self.slots, self.S, self.L, self.H, _p(table), len(pl.slots), pl.rows, pl.max_rows,
                                     _p(x), pl.x_total, _p(mix), _s()), 'ams_stream_feed')
        return mix[:pl.rows]

    def absorb(self, pl, table, est):
        """ams_stream_absorb for the plan `pl`, its table on the device and est [rows, S, L] (None without rows) -> out [S, out_total]
        (four launches).  With keep_rows also (Q [rows, S, S], trk [rows, S]), else (None, None)."""
        lib, S, L, H, n = load(), self.S, self.L, self.H, len(pl.slots)
        stride = max(pl.out_total, 1)
        out = torch.empty((S, stride), dtype=torch.float32, device=self.device)
        nbytes = lib.ams_stream_workspace_bytes(n, pl.rows, S, L, H)
        ws = torch.empty(max(nbytes // 4, 1), dtype=torch.float32, device=self.device)
        Q = trk = None
        if self.keep_rows:
            Q = torch.zeros((max(pl.rows, 1), S, S), dtype=torch.float32, device=self.device)
            trk = torch.zeros((max(pl.rows, 1), S), dtype=torch.int32, device=self.device)
        check(lib.ams_stream_absorb(_p(self._state), self.slots, S, L, H, _p(table), n, pl.rows, pl.max_rows, pl.max_m,
                                    _p(est) if est is not None else None, _p(self._perms), self._perms.shape[0], _p(self._w), _p(out), stride,
                                    _p(ws), ws.numel() * 4, _p(Q) if Q is not None else None, _p(trk) if trk is not None else None, _s()),
              'ams_stream_absorb')
        return out[:, :pl.out_total], (Q[:pl.rows], trk[:pl.rows]) if self.keep_rows else (None, None)

    def _step(self, taking, closing):
        """One feed, one infer over all ready rows, one absorb -> {slot: [S, m] view}."""
        self.arm()
        slots = [s for s, _ in taking]
        pl = plan(slots, [self._N[s] for s in slots], [self._D[s] for s in slots], [b.shape[0] if b is not None else 0 for _, b in taking],
                  [s in closing for s in slots], self.L, self.H)
        S, L = self.S, self.L
        x = self._pack([(s, b) for s, b in taking if b is not None], pl.x_total)
        table = torch.from_numpy(pl.table.reshape(-1)).to(self.device)
        mix = self.feed(pl, table, x)
        est = None
        if pl.rows:
            est = self.infer(mix)
            self.passes += 1
            if not torch.is_tensor(est) or not est.is_cuda or est.dtype != torch.float32 or tuple(est.shape) != (pl.rows, S, L):
                raise StreamError('infer must return a float32 device tensor [%d, %d, %d] for mix [%d, %d], got %s'
                                  % (pl.rows, S, L, pl.rows, L, (est.dtype, tuple(est.shape)) if torch.is_tensor(est) else type(est).__name__))
            est = est.contiguous()
        out, (Q, trk) = self.absorb(pl, table, est)
        if self.keep_rows:
            self.last = {'plan': pl, 'mix': mix, 'est': est, 'Q': Q, 'trk': trk}
        res = {}
        for i, s in enumerate(slots):
            o, m = int(pl.table[i, 6]), int(pl.table[i, 7])
            self._N[s], self._D[s] = int(pl.N[i]), int(pl.D[i])
            self._emitted[s] += m
            res[s] = out[:, o:o + m]
        return res

    # ---- the public calls
    def push(self, blocks):
        """blocks: a list of `slots` entries, float32 [k_s] each (tensor or numpy, k_s >= 0) or None -> a list of [S, m_s] device
        tensors, views of one buffer; m_s is H times the chunks that became ready, and may be 0.  After every push a stream has emitted
        exactly D H samples, D = the chunks done.  Never synchronises."""
        taking = self._blocks(blocks)
        empty = None
        res = self._step(taking, ()) if taking else {}
        outs = []
        for s in range(self.slots):
            if s in res:
                outs.append(res[s])
            else:
                if empty is None:
                    self.arm()
                    empty = torch.empty((self.S, 0), dtype=torch.float32, device=self.device)
                outs.append(empty)
        return outs

    def close(self, s):
        """Ends stream s -> [S, m]: what push has not emitted yet, so that the stream's outputs add up to its N samples.  A last chunk
        that is short of samples is filled with zeros and goes through `infer` on its own; a stream that received nothing returns
        [S, 0] without a model pass.  The slot refuses further pushes until reset(s)."""
        s = self._slot(s)
        if self._closed[s]:
            raise ValueError('close: slot %d is closed already' % s)
        self._closed[s] = True
        if self._N[s] == 0:
            self.arm()
            return torch.empty((self.S, 0), dtype=torch.float32, device=self.device)
        return self._step([(s, None)], (s,))[s]

    def reset(self, s):
        """Slot s takes a new stream: nothing of the one before it survives (its pending samples, its tail -- NaNs included -- its
        tracks), open or closed."""
        s = self._slot(s)
        self.arm()
        check(load().ams_stream_reset(_p(self._state), self.slots, self.S, self.L, self.H, s, 1, _s()), 'ams_stream_reset')
        self._N[s] = self._D[s] = self._emitted[s] = 0
        self._closed[s] = False
