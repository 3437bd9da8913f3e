"""Fenced device memory for the kernel tests: red zones around every operand, NaN-filled outputs, odd base addresses.

    with Fence() as fence:
        x = fence.dev(numpy_array)          # an input between two red zones
        y = ops.something(x)                # its torch.empty / torch.zeros outputs and workspaces are fenced too
        fence.check()                       # AssertionError if any zone word changed

While a Fence is active the `torch` module attributes empty / zeros / ones / full and their *_like forms are replaced.  A dense,
contiguous request on the fence's device type becomes a window into one int32 backing tensor (from the ORIGINAL torch.empty):

    [ slack | front zone | payload | back zone ]

  * the payload starts on a 256-byte boundary (plus `base` bytes for Fence.dev(..., base=4 | 8 | 12)), so launch-time choices made on
    the alignment of a pointer go as they do in production -- or, with a base, take the arm production takes for a row of a batch whose
    length is not a multiple of four;
  * the payload ends exactly: the back zone starts at the first 4-byte word after it;
  * both zones, and the payload of every empty / empty_like, hold the word 0x7FF87FF8 -- a NaN as float64 (as a pair of words), float32,
    float16 and bfloat16, and 2146992120 as an int32, outside every label, count, ticket or index the tests use.  An output word a
    kernel does not store is therefore a NaN in the comparison with the oracle; zeros / ones / full keep their values.

REACH (a condition, not a measurement): a zone is `zone_bytes` = 64 KiB.  A stray store or a consumed stray load is seen when it lands
within 64 KiB of the operand it belongs to -- more than a 256-column fp32 tile row and more than any row of the shapes the fenced
tests use.  An access further out is not covered.

Everything else goes to the original function untouched: another device type, out=, pin_memory, names, a sparse layout, a
non-contiguous memory_format (or a *_like of a non-contiguous tensor under preserve_format), a zero-sized tensor.  ams_hip calls none of
Tensor.new_empty / new_zeros / new_full, so those are left alone.  Tensors made inside C++ (x.cuda(), clone, cat, ...) are not fenced.

On entry the persistent scratch caches of ams_hip.ops (CACHES below) are swapped for empty containers of the same type and on exit the
original objects are bound again (whatever was bound in between): scratch created inside a fence is fenced, and no fenced buffer is
handed to a later test.

EXEMPTIONS: none.  The only acceptable one is a padding requirement include/ams.h states for an argument; it would be listed here by
entry point and argument, with the header line that states it.

This is a plain helper module: no pytest hooks, no fixtures, no environment, no allocator settings.
"""
import os
import sys

import numpy as np
import torch

PATTERN = 0x7FF87FF8
ALIGN = 256
CACHES = ('_SK', '_ONE', '_ARENAS', '_RING_ERR', '_STAGE', '_KM_TICKETS', '_DPCL_AHEAD')
PATCHED = ('empty', 'zeros', 'ones', 'full', 'empty_like', 'zeros_like', 'ones_like', 'full_like')

_HERE = os.path.normcase(os.path.abspath(__file__))
_HERE = _HERE[:-1] if _HERE.endswith(('.pyc', '.pyo')) else _HERE
_ACTIVE = [None]


class FenceError(AssertionError):
    """A zone word changed.  zone: 'front' | 'back'; distance: bytes from the payload edge to the start of the changed word nearest to
    it (front: 4 = the word that ends where the payload starts; back: 0 = the word that starts where the payload, rounded up to a whole
    word, ends); word: what was found; site: 'file:line' that asked for the allocation; shape, dtype: of the allocation."""

    def __init__(self, shape, dtype, site, zone, distance, word, nhits):
        self.shape, self.dtype, self.site, self.zone, self.distance, self.word, self.nhits = shape, dtype, site, zone, distance, word, nhits
        where = ('%d bytes before the payload start' if zone == 'front' else '%d bytes past the payload end') % distance
        AssertionError.__init__(self, 'fence: %s zone of %s %s allocated at %s was written: word 0x%08X found %s (%d zone words changed)'
                                % (zone, tuple(shape), dtype, site, word & 0xFFFFFFFF, where, nhits))


class _Pass(Exception):
    """This request is not one the fence takes: hand it to the original function."""


def _site():
    f = sys._getframe(1)
    while f is not None:
        name = os.path.normcase(os.path.abspath(f.f_code.co_filename))
        if name != _HERE:
            return '%s:%d' % (f.f_code.co_filename, f.f_lineno)
        f = f.f_back
    return '?'


def _sizes(args):
    if len(args) == 1 and isinstance(args[0], (tuple, list, torch.Size)):
        args = tuple(args[0])
    out = []
    for a in args:
        if isinstance(a, bool) or not isinstance(a, (int, np.integer)):
            raise _Pass()
        out.append(int(a))
    return tuple(out)


class Fence(object):
    def __init__(self, device_type='cuda', zone_bytes=65536):
        if zone_bytes <= 0 or zone_bytes % 4:
            raise ValueError('zone_bytes must be a positive multiple of 4')
        self.device_type = device_type
        self.zone_bytes = int(zone_bytes)
        self._allocs = []                     # (backing, front word, payload word, payload words, shape, dtype, site)
        self._orig = {}
        self._caches = {}
        self._ops = None

    # ------------------------------------------------------------------ enter / exit
    def __enter__(self):
        if _ACTIVE[0] is not None:
            raise RuntimeError('fence: a Fence is already active (nested fences are refused)')
        ops = None
        try:
            from ams_hip import ops
        except ImportError:
            if self.device_type != 'cpu':     # only the helper's own CPU tests may run without the package
                raise
        _ACTIVE[0] = self
        try:
            self._ops = ops
            if ops is not None:
                for name in CACHES:
                    old = getattr(ops, name)
                    self._caches[name] = old
                    setattr(ops, name, [None] * len(old) if isinstance(old, list) else type(old)())
            for name in PATCHED:
                self._orig[name] = getattr(torch, name)
            for name in PATCHED:
                setattr(torch, name, self._patched(name))
        except BaseException:
            self._restore()
            raise
        return self

    def __exit__(self, exc_type, exc, tb):
        try:
            self.check()
        finally:
            self._restore()
        return False

    def _restore(self):
        for name, fn in self._orig.items():
            setattr(torch, name, fn)
        if self._ops is not None:
            for name, old in self._caches.items():
                setattr(self._ops, name, old)
        self._orig, self._caches, self._allocs = {}, {}, []
        _ACTIVE[0] = None

    # ------------------------------------------------------------------ allocation
    def _takes(self, device):
        if device is None:
            device = torch.get_default_device() if hasattr(torch, 'get_default_device') else torch.device('cpu')
        device = torch.device(device)
        if device.type != self.device_type:
            raise _Pass()
        return device

    def _alloc(self, shape, dtype, device, base=0, fill=None, requires_grad=False):
        """One fenced tensor.  fill None: the payload keeps the pattern; else the value."""
        numel = 1
        for s in shape:
            if s < 0:
                raise _Pass()
            numel *= s
        if numel == 0:
            raise _Pass()
        empty = self._orig['empty']
        item = empty(0, dtype=dtype).element_size()
        words = (numel * item + 3) // 4
        zone = self.zone_bytes
        backing = empty((ALIGN + zone + 16 + words * 4 + zone) // 4 + 1, dtype=torch.int32, device=device)
        backing.fill_(PATTERN)
        p0 = backing.data_ptr()
        start = zone + (-(p0 + zone)) % ALIGN + base            # byte offset of the payload in the backing tensor
        if p0 % 4 or start % item:
            raise ValueError('fence: base %d does not suit %s' % (base, dtype))
        strides, acc = [], 1
        for s in reversed(shape):
            strides.append(acc)
            acc *= max(s, 1)
        t = empty(0, dtype=dtype, device=device).set_(backing.untyped_storage(), start // item, tuple(shape), tuple(reversed(strides)))
        assert t.data_ptr() == p0 + start and t.data_ptr() % ALIGN == base
        if fill is not None:
            t.fill_(fill)
        self._allocs.append((backing, (start - zone) // 4, start // 4, words, tuple(shape), dtype, _site()))
        if requires_grad:
            t.requires_grad_(True)
        return t

    def _patched(self, name):
        orig = self._orig[name]
        like = name.endswith('_like')
        kind = name.split('_')[0]

        def fn(*args, **kwargs):
            try:
                kw = dict(kwargs)
                if kw.pop('out', None) is not None or kw.pop('pin_memory', False) or kw.pop('names', None) is not None:
                    raise _Pass()
                if kw.pop('layout', torch.strided) not in (torch.strided, None):
                    raise _Pass()
                mf = kw.pop('memory_format', None)
                dtype, device, rg = kw.pop('dtype', None), kw.pop('device', None), kw.pop('requires_grad', False)
                a = list(args)
                if like:
                    x = a.pop(0) if a else kw.pop('input')
                    if not isinstance(x, torch.Tensor) or x.layout != torch.strided:
                        raise _Pass()
                    if mf in (None, torch.preserve_format):
                        if not x.is_contiguous():
                            raise _Pass()
                    elif mf != torch.contiguous_format:
                        raise _Pass()
                    shape = tuple(x.shape)
                    dtype = x.dtype if dtype is None else dtype
                    device = x.device if device is None else device
                    if kind == 'full':
                        value = a.pop(0) if a else kw.pop('fill_value')
                else:
                    if mf not in (None, torch.contiguous_format):
                        raise _Pass()
                    if kind == 'full':
                        size = a.pop(0) if a else kw.pop('size')
                        value = a.pop(0) if a else kw.pop('fill_value')
                        shape = _sizes((size,))
                        if dtype is None:
                            dtype = orig((), value).dtype
                    else:
                        shape = _sizes(tuple(a)) if a else _sizes((kw.pop('size'),))
                        a = []
                    if dtype is None:
                        dtype = torch.get_default_dtype()
                if a or kw:
                    raise _Pass()
                device = self._takes(device)
                fill = {'empty': None, 'zeros': 0, 'ones': 1}.get(kind)
                if kind == 'full':
                    fill = value
                    if isinstance(value, torch.Tensor):
                        raise _Pass()
                return self._alloc(shape, dtype, device, 0, fill, rg)
            except (_Pass, KeyError):
                return orig(*args, **kwargs)
        fn.__name__ = name
        fn._fence_original = orig
        return fn

    def dev(self, x, dtype=np.float32, base=0):
        """Upload a numpy array into a fenced payload that begins `base` (0, 4, 8 or 12) bytes past a 256-byte boundary.  A dtype wider
        than four bytes gets the largest multiple of its width that is not above `base`."""
        if base not in (0, 4, 8, 12):
            raise ValueError('fence: base must be 0, 4, 8 or 12')
        if _ACTIVE[0] is not self:
            raise RuntimeError('fence: dev() outside the with block')
        arr = np.ascontiguousarray(x, dtype=dtype)
        src = torch.from_numpy(arr)
        device = torch.device(self.device_type)
        if device.type == 'cuda':
            device = torch.device('cuda', torch.cuda.current_device())
        if arr.size == 0:
            return src.to(device)
        base -= base % src.element_size()
        t = self._alloc(tuple(arr.shape), src.dtype, device, base, None)
        t.copy_(src)
        return t

    # ------------------------------------------------------------------ the check
    def check(self):
        """Every zone of every allocation made so far still holds the pattern (compared on the device, as int32)."""
        if self.device_type == 'cuda' and torch.cuda.is_initialized():
            torch.cuda.synchronize()
        zw = self.zone_bytes // 4
        total = {}
        for backing, f0, p0, words, shape, dtype, site in self._allocs:
            n = (backing[f0:f0 + zw] != PATTERN).sum() + (backing[p0 + words:p0 + words + zw] != PATTERN).sum()
            total[backing.device] = n if backing.device not in total else total[backing.device] + n
        if all(int(n) == 0 for n in total.values()):
            return
        for backing, f0, p0, words, shape, dtype, site in self._allocs:
            for zone, z0 in (('front', f0), ('back', p0 + words)):
                z = backing[z0:z0 + zw].cpu().numpy()
                hit = np.nonzero(z != np.int32(PATTERN))[0]
                if hit.size:
                    i = int(hit[-1] if zone == 'front' else hit[0])
                    dist = (zw - i) * 4 if zone == 'front' else i * 4
                    raise FenceError(shape, dtype, site, zone, dist, int(z[i]), int(hit.size))
        raise AssertionError('fence: a zone changed between two reads of it')
