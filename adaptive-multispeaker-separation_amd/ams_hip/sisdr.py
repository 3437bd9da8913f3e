"""Scale-invariant SDR of recordings of differing lengths and track counts, with the best one-to-one matching of tracks to true sources:
ctypes binding of libams_sisdr.so (include/ams_sisdr.h) and its host side.

    lay = Layout(Sr, Se, lengths)              # where the rows lie, the work table (host, numpy; no library, no device)
    out = si_sdr_ragged(refs, ests, mixtures)  # the public entry: utils.bss_eval.si_sdr_ragged

Recording r has Sr_r references, a mixture and K sets of Se_rk estimated tracks, all float32 of L_r samples; its rows are packed one
after the other (references, mixture, the sets in order) and one library call -- two launches whatever R is -- scores every recording
of a group.  Hand-written HIP kernels on torch's current stream, torch for device memory and the stream only, no CPU path.
Definitions: DESIGN.md 6d and the header; the float64 restatement is tests/sisdr_ref.py.
"""
import ctypes
import os

import numpy as np

from ._lib import AmsError, check, parse_header

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, 'libams_sisdr.so')
HEADER_PATH = os.path.normpath(os.path.join(_HERE, '..', '..', 'include', 'ams_sisdr.h'))
ABI_VERSION = 1            # include/ams_sisdr.h: ams_sisdr_abi_version()
BLOCK = 4096               # AMS_SISDR_BLOCK: samples per row of the work table (load() checks it against the library)
MAX_TRACKS = 6             # references of a recording, tracks of a set
MAX_SETS = 8
MAX_ROWS = 56              # row offsets per recording: 6 + 1 + 8 * 6 = 55 used at most
PART = 8 * 56 + 56         # float64 per block of the workspace
CAP_BYTES = 4 << 30        # packed signals + workspace + tables of one library call; larger sets go in groups of consecutive recordings
KEYS = ('pair', 'match_ref', 'match_est', 'si_sdr', 'si_sdri', 'missed', 'spurious', 'base', 'info')

_vp = ctypes.c_void_p
_lib = None
LAUNCHES = 0               # kernel launches made through this module so far (two per library call)


class SisdrError(ValueError):
    """A refusal of the host side: made before the library or the device is touched."""


def load():
    global _lib
    if _lib is not None:
        return _lib
    import torch  # noqa: F401  (before a library that links libamdhip64: one HIP runtime in the process, see _lib.load)
    if not os.path.exists(LIB_PATH):
        raise AmsError('libams_sisdr.so not found at %s -- the HIP extension is required (no CPU fallback); '
                       'run __graft_entry__.build()' % LIB_PATH)
    lib = ctypes.CDLL(LIB_PATH)
    for name, (ret, argtypes) in parse_header(HEADER_PATH).items():
        try:
            fn = getattr(lib, name)
        except AttributeError:
            raise AmsError('libams_sisdr.so does not export %s (declared in include/ams_sisdr.h)' % name)
        fn.restype = ret
        fn.argtypes = argtypes
    if lib.ams_sisdr_abi_version() != ABI_VERSION:
        raise AmsError('libams_sisdr.so ABI version mismatch: the library is %d, this binding is %d -- rebuild (make -C csrc)'
                       % (lib.ams_sisdr_abi_version(), ABI_VERSION))
    if lib.ams_sisdr_block() != BLOCK:
        raise AmsError('libams_sisdr.so sums in blocks of %d samples, this binding lays out blocks of %d' % (lib.ams_sisdr_block(), BLOCK))
    _lib = lib
    return lib


def block():
    """AMS_SISDR_BLOCK as the library exports it."""
    return int(load().ams_sisdr_block())


class Layout(object):
    """Where R recordings lie (host, numpy; the names are the header's).  Sr [R], Se [R, K], lengths [R] ->
    nrows [R]; row_len: the samples of every packed row in order; rows [R, 56] int64 (unused entries -1); rec [R, 4] int64;
    cnt [R, 16] int32; tab [Btot, 2] int32; floats: the size of the packed buffer."""

    def __init__(self, Sr, Se, lengths):
        self.Sr = np.asarray(Sr, np.int64).reshape(-1)
        self.R = int(self.Sr.size)
        if self.R < 1:
            raise SisdrError('si_sdr layout: R >= 1 recordings')
        self.Se = np.asarray(Se, np.int64).reshape(self.R, -1)
        self.K = int(self.Se.shape[1])
        self.L = np.asarray(lengths, np.int64).reshape(-1)
        if self.R < 1 or self.L.size != self.R or not 1 <= self.K <= MAX_SETS:
            raise SisdrError('si_sdr layout: R >= 1 recordings, 1 .. %d sets, one length per recording' % MAX_SETS)
        if self.Sr.min() < 1 or self.Sr.max() > MAX_TRACKS or self.Se.min() < 1 or self.Se.max() > MAX_TRACKS or self.L.min() < 1:
            raise SisdrError('si_sdr layout: 1 .. %d references and tracks per set, at least one sample' % MAX_TRACKS)
        self.nrows = self.Sr + 1 + self.Se.sum(axis=1)
        self.blocks = (self.L + BLOCK - 1) // BLOCK
        self.b_off = np.concatenate([[0], np.cumsum(self.blocks)]).astype(np.int64)
        self.Btot = int(self.b_off[-1])
        self.x_off = np.concatenate([[0], np.cumsum(self.nrows * self.L)]).astype(np.int64)      # a recording's first float
        self.floats = int(self.x_off[-1])
        self.rows = np.full((self.R, MAX_ROWS), -1, np.int64)
        self.rec = np.zeros((self.R, 4), np.int64)
        self.cnt = np.zeros((self.R, 16), np.int32)
        for r in range(self.R):
            n = int(self.nrows[r])
            self.rows[r, :n] = self.x_off[r] + np.arange(n, dtype=np.int64) * self.L[r]
            self.cnt[r, 2:2 + self.K] = self.Se[r]
        self.rec[:, 0], self.rec[:, 1] = self.L, self.b_off[:-1]
        self.cnt[:, 0], self.cnt[:, 1] = self.Sr, self.nrows
        self.tab = np.empty((self.Btot, 2), np.int32)
        self.tab[:, 0] = np.repeat(np.arange(self.R), self.blocks)
        self.tab[:, 1] = np.arange(self.Btot) - np.repeat(self.b_off[:-1], self.blocks)
        self.row_len = np.repeat(self.L, self.nrows)

    def workspace_bytes(self):
        return 8 * PART * self.Btot

    def table_words(self):
        """int64 words of the one buffer the four tables are uploaded in."""
        return self.R * (MAX_ROWS + 4 + 8) + self.Btot

    def tables(self, device):
        """(rows, rec, cnt, tab) on the device, from ONE upload."""
        import torch
        R = self.R
        host = np.zeros(self.table_words(), np.int64)
        a, b, c = R * MAX_ROWS, R * (MAX_ROWS + 4), R * (MAX_ROWS + 4 + 8)
        host[:a], host[a:b] = self.rows.reshape(-1), self.rec.reshape(-1)
        host[b:c].view(np.int32)[:] = self.cnt.reshape(-1)
        host[c:].view(np.int32)[:] = self.tab.reshape(-1)
        buf = torch.empty(host.size, dtype=torch.int64, device=device)
        buf.copy_(torch.from_numpy(host))
        return buf[:a], buf[a:b], buf[b:c].view(torch.int32), buf[c:].view(torch.int32)


def _is_tensor(x):
    return type(x).__module__.startswith('torch') and hasattr(x, 'data_ptr')


def _shape(x):
    return tuple(x.shape) if hasattr(x, 'shape') else tuple(np.shape(x))


def _is_f32(x):
    if _is_tensor(x):
        return str(x.dtype) == 'torch.float32'
    return getattr(x, 'dtype', None) == np.float32


def check_inputs(refs, ests, mixtures):
    """Every refusal of the shapes and types, before the library or the device is touched -> (Sr [R], Se [R, K], lengths [R], sets):
    sets[r] is the list of the K arrays of recording r."""
    for name, v in (('references', refs), ('estimates', ests), ('mixtures', mixtures)):
        if not isinstance(v, (list, tuple)):
            raise SisdrError('si_sdr: the %s are a list, one entry per recording' % name)
    if len(refs) < 1:
        raise SisdrError('si_sdr: empty list of recordings')
    if not len(refs) == len(ests) == len(mixtures):
        raise SisdrError('si_sdr: %d references, %d estimates and %d mixtures' % (len(refs), len(ests), len(mixtures)))
    Sr, Se, lengths, sets, K = [], [], [], [], None
    for r, (a, e, m) in enumerate(zip(refs, ests, mixtures)):
        es = list(e) if isinstance(e, (list, tuple)) else [e]
        rs, ms = _shape(a), _shape(m)
        if len(rs) != 2 or len(ms) != 1 or any(len(_shape(t)) != 2 for t in es):
            raise SisdrError('si_sdr: recording %d: expected references [Sr, L], a mixture [L] and tracks [Se, L] per set, got %s, %s and %s'
                             % (r, rs, ms, [_shape(t) for t in es]))
        if not 1 <= len(es) <= MAX_SETS:
            raise SisdrError('si_sdr: recording %d has %d sets of estimates, 1 .. %d are taken' % (r, len(es), MAX_SETS))
        if K is None:
            K = len(es)
        if len(es) != K:
            raise SisdrError('si_sdr: recording %d has %d sets of estimates, the first recording has %d' % (r, len(es), K))
        if rs[1] < 1:
            raise SisdrError('si_sdr: recording %d is empty: references %s' % (r, rs))
        if not 1 <= rs[0] <= MAX_TRACKS:
            raise SisdrError('si_sdr: recording %d has %d references, 1 .. %d are taken' % (r, rs[0], MAX_TRACKS))
        if ms[0] != rs[1]:
            raise SisdrError('si_sdr: recording %d: the references have %d samples, the mixture %d' % (r, rs[1], ms[0]))
        for k, t in enumerate(es):
            ts = _shape(t)
            if not 1 <= ts[0] <= MAX_TRACKS:
                raise SisdrError('si_sdr: recording %d, set %d has %d tracks, 1 .. %d are taken' % (r, k, ts[0], MAX_TRACKS))
            if ts[1] != rs[1]:
                raise SisdrError('si_sdr: recording %d, set %d: the references have %d samples, the tracks %d' % (r, k, rs[1], ts[1]))
        for what, t in [('references', a), ('mixture', m)] + [('set %d' % k, t) for k, t in enumerate(es)]:
            if not _is_f32(t):
                raise SisdrError('si_sdr: recording %d: the %s are %s, float32 is taken (float64 inputs are not built)'
                                 % (r, what, getattr(t, 'dtype', type(t).__name__)))
        Sr.append(rs[0])
        Se.append([_shape(t)[0] for t in es])
        lengths.append(rs[1])
        sets.append(es)
    return np.asarray(Sr, np.int64), np.asarray(Se, np.int64), np.asarray(lengths, np.int64), sets


def group_bytes(Sr, Se, lengths):
    """Bytes of one library call on these recordings: the packed float32 rows, the workspace, the tables."""
    Sr, Se, L = np.asarray(Sr, np.int64), np.asarray(Se, np.int64).reshape(len(Sr), -1), np.asarray(lengths, np.int64)
    blocks = int(((L + BLOCK - 1) // BLOCK).sum())
    return int(4 * ((Sr + 1 + Se.sum(axis=1)) * L).sum() + 8 * PART * blocks + 8 * (len(Sr) * (MAX_ROWS + 4 + 8) + blocks))


def groups(Sr, Se, lengths, cap_bytes):
    """Consecutive recordings whose call stays under cap_bytes -> [(first, last + 1)]; a recording above the cap alone is refused."""
    out, r0 = [], 0
    for r in range(len(Sr)):
        alone = group_bytes(Sr[r:r + 1], Se[r:r + 1], lengths[r:r + 1])
        if alone > cap_bytes:
            raise SisdrError('si_sdr: recording %d (%d samples, %d references, tracks per set %s) needs %d bytes, the cap is %d'
                             % (r, lengths[r], Sr[r], np.asarray(Se[r]).reshape(-1).tolist(), alone, cap_bytes))
        if r > r0 and group_bytes(Sr[r0:r + 1], Se[r0:r + 1], lengths[r0:r + 1]) > cap_bytes:
            out.append((r0, r))
            r0 = r
    out.append((r0, len(Sr)))
    return out


def _p(t):
    return _vp(t.data_ptr())


def pack(lay, pieces, device):
    """The rows of a group in the layout's order -> one float32 device buffer.  Host arrays are joined on the host and uploaded once;
    with a device tensor among them everything is joined on the device."""
    import torch
    x = torch.empty(lay.floats, dtype=torch.float32, device=device)
    if not any(_is_tensor(p) for p in pieces):
        x.copy_(torch.from_numpy(np.concatenate([np.ascontiguousarray(p, np.float32).reshape(-1) for p in pieces])))
    else:
        torch.cat([torch.as_tensor(p).to(device).reshape(-1) for p in pieces], out=x)
    return x


def eval_packed(x, lay, zero_mean=True):
    """ONE library call on the packed rows -> the outputs of the header as device tensors with leading axes [R, K]; nothing synchronised."""
    global LAUNCHES
    import torch
    lib = load()
    if not (torch.is_tensor(x) and x.is_cuda and x.dtype == torch.float32 and x.is_contiguous() and x.numel() == lay.floats):
        raise AmsError('si_sdr: a packed float32 device tensor of %d elements is expected' % lay.floats)
    dev, R, K = x.device, lay.R, lay.K
    nb = lib.ams_sisdr_workspace_bytes(R, K, lay.Btot)
    if nb == 0 or nb != lay.workspace_bytes():
        raise AmsError('si_sdr: (R, K, blocks) = (%d, %d, %d): the library asks for %d bytes of workspace, the layout for %d'
                       % (R, K, lay.Btot, nb, lay.workspace_bytes()))
    rows, rec, cnt, tab = lay.tables(dev)
    ws = torch.empty(nb // 8, dtype=torch.float64, device=dev)
    f64 = lambda *s: torch.empty(s, dtype=torch.float64, device=dev)       # noqa: E731
    i32 = lambda *s: torch.empty(s, dtype=torch.int32, device=dev)         # noqa: E731
    out = dict(pair=f64(R, K, 6, 6), match_ref=i32(R, K, 6), match_est=i32(R, K, 6), si_sdr=f64(R, K, 6), si_sdri=f64(R, K, 6),
               missed=i32(R, K), spurious=i32(R, K), base=f64(R, 6), info=i32(R))
    check(lib.ams_sisdr_eval(_p(x), _p(rows), _p(rec), _p(cnt), _p(tab), R, K, lay.Btot, 1 if zero_mean else 0, _p(ws), nb,
                             _p(out['pair']), _p(out['match_ref']), _p(out['match_est']), _p(out['si_sdr']), _p(out['si_sdri']),
                             _p(out['missed']), _p(out['spurious']), _p(out['base']), _p(out['info']),
                             _vp(torch.cuda.current_stream().cuda_stream)), 'ams_sisdr_eval')
    LAUNCHES += 2
    return out


def si_sdr_ragged(refs, ests, mixtures, zero_mean=True, cap_bytes=None):
    """See utils.bss_eval.si_sdr_ragged."""
    Sr, Se, lengths, sets = check_inputs(refs, ests, mixtures)
    cap = CAP_BYTES if cap_bytes is None else int(cap_bytes)
    grp = groups(Sr, Se, lengths, cap)
    import torch
    if not torch.cuda.is_available():
        raise AmsError('si_sdr needs a GPU (there is no CPU fallback)')
    load()
    everything = list(refs) + list(mixtures) + [t for es in sets for t in es]
    dev = next((t.device for t in everything if _is_tensor(t) and t.is_cuda), torch.device('cuda'))
    res = None
    for r0, r1 in grp:
        lay = Layout(Sr[r0:r1], Se[r0:r1], lengths[r0:r1])
        pieces = []
        for r in range(r0, r1):
            pieces += [refs[r], mixtures[r]] + sets[r]
        out = eval_packed(pack(lay, pieces, dev), lay, zero_mean)
        host = {k: v.cpu().numpy() for k, v in out.items()}
        if res is None:
            res = {k: np.empty((len(Sr),) + v.shape[1:], v.dtype) for k, v in host.items()}
        for k, v in host.items():
            res[k][r0:r1] = v
    return res
