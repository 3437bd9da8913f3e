"""tests/fenced.py checked on the CPU: the fence sees a store next to a payload and says where, its fills are what it says they are, and
it puts everything back."""
import numpy as np
import pytest

torch = pytest.importorskip('torch')

from tests import fenced
from tests.fenced import Fence, FenceError, PATTERN

ZONE = 4096                                   # a smaller zone keeps these quick; the default is checked once below


def _poke(t, element, value):
    """Store `value` at `element` of t's flat payload, where element may lie outside it (-1: just before, numel: just after)."""
    w = torch.empty(0, dtype=t.dtype).set_(t.untyped_storage(), t.storage_offset() + element, (1,), (1,))
    w.fill_(value)


def _here():
    import sys
    f = sys._getframe(1)
    return f.f_code.co_filename, f.f_lineno


def test_a_store_one_element_before_the_payload_is_reported():
    with pytest.raises(FenceError) as e:
        with Fence('cpu', ZONE) as fence:
            name, line = _here(); t = torch.empty(5, 7, dtype=torch.float32, device='cpu')  # noqa: E702
            _poke(t, -1, 3.0)
            fence.check()
    err = e.value
    assert isinstance(err, AssertionError)
    assert (err.zone, err.distance, err.nhits) == ('front', 4, 1)
    assert err.site == '%s:%d' % (name, line)
    assert err.shape == (5, 7) and err.dtype == torch.float32
    assert err.word == int(np.float32(3.0).view(np.int32))
    for part in ('front', '(5, 7)', 'torch.float32', '%s:%d' % (name, line), '4 bytes before', '0x40400000'):
        assert part in str(err), (part, str(err))


def test_a_store_one_element_after_the_payload_is_reported():
    with pytest.raises(FenceError) as e:
        with Fence('cpu', ZONE) as fence:
            torch.zeros(3, device='cpu')                               # a clean neighbour allocated first
            name, line = _here(); t = torch.zeros((2, 3), dtype=torch.float32, device='cpu')  # noqa: E702
            _poke(t, t.numel(), -1.0)
            fence.check()
    err = e.value
    assert (err.zone, err.distance, err.nhits) == ('back', 0, 1)
    assert err.site == '%s:%d' % (name, line) and err.shape == (2, 3)
    assert '0 bytes past the payload end' in str(err)


def test_the_back_zone_starts_at_the_first_word_after_a_payload_of_odd_bytes():
    with pytest.raises(FenceError) as e:
        with Fence('cpu', ZONE):
            t = torch.empty(7, dtype=torch.uint8, device='cpu')       # 7 bytes: the eighth shares the payload's last word
            _poke(t, 7, 1)                                            # not zone
            _poke(t, 8, 1)                                            # zone
    assert (e.value.zone, e.value.distance) == ('back', 0)
    with Fence('cpu', ZONE):
        t = torch.empty(7, dtype=torch.uint8, device='cpu')
        _poke(t, 7, 1)


@pytest.mark.parametrize('zone', [ZONE, 65536])
def test_the_last_word_of_either_zone_is_covered_and_a_clean_run_reports_nothing(zone):
    with Fence('cpu', zone) as fence:
        a = torch.empty(100, device='cpu')
        b = torch.full((3, 3), 2.5, device='cpu')
        a.fill_(1.0)
        b.mul_(2.0)
        fence.check()
        fence.check()
    for element, want in ((-(zone // 4), ('front', zone)), (100 + zone // 4 - 1, ('back', zone - 4))):
        with pytest.raises(FenceError) as e:
            with Fence('cpu', zone):
                t = torch.empty(100, dtype=torch.float32, device='cpu')
                _poke(t, element, 0.0)
        assert (e.value.zone, e.value.distance) == want
    assert Fence().zone_bytes == 65536


def test_empty_is_nan_in_the_four_float_widths_and_the_pattern_in_the_integers():
    assert PATTERN == 0x7FF87FF8 == 2146992120
    with Fence('cpu', ZONE):
        for dt in (torch.float64, torch.float32, torch.float16, torch.bfloat16):
            for n in (1, 2, 5):
                t = torch.empty(n, dtype=dt, device='cpu')
                assert t.dtype == dt and bool(torch.isnan(t).all()), dt
            assert bool(torch.isnan(torch.empty_like(torch.empty((2, 3), dtype=dt, device='cpu'))).all())
        assert torch.empty(3, dtype=torch.int32, device='cpu').tolist() == [PATTERN] * 3
        assert torch.empty(2, dtype=torch.int64, device='cpu').tolist() == [PATTERN << 32 | PATTERN] * 2
        assert torch.empty(5, dtype=torch.uint8, device='cpu').tolist() == [0xF8, 0x7F, 0xF8, 0x7F, 0xF8]


def test_zeros_ones_full_keep_their_values_and_like_keeps_shape_and_dtype():
    with Fence('cpu', ZONE) as fence:
        z = torch.zeros(3, 4, device='cpu')
        assert len(fence._allocs) == 1
        assert z.shape == (3, 4) and z.dtype == torch.float32 and z.is_contiguous() and float(z.abs().sum()) == 0.0
        assert torch.ones((2, 2), dtype=torch.int32, device='cpu').tolist() == [[1, 1], [1, 1]]
        f = torch.full((5,), 7, device='cpu')
        assert f.dtype == torch.int64 and f.tolist() == [7] * 5
        assert torch.full((2,), 0.5, dtype=torch.float16, device='cpu').tolist() == [0.5, 0.5]
        src = torch.empty((2, 3, 5), dtype=torch.float64, device='cpu')
        for fn, val in ((torch.zeros_like, 0.0), (torch.ones_like, 1.0), (lambda x, **k: torch.full_like(x, 3.0, **k), 3.0)):
            y = fn(src)
            assert y.shape == src.shape and y.dtype == torch.float64 and y.is_contiguous() and bool((y == val).all())
            y = fn(src, dtype=torch.int32)
            assert y.shape == src.shape and y.dtype == torch.int32 and bool((y == int(val)).all())
        e = torch.empty_like(src, dtype=torch.float32)
        assert e.shape == src.shape and e.dtype == torch.float32
        g = torch.zeros(4, device='cpu', requires_grad=True)
        assert g.requires_grad and g.is_leaf
        n = len(fence._allocs)
        # what the fence does not take goes to the original function
        assert torch.empty(0, device='cpu').numel() == 0
        out = torch.empty(3)
        assert torch.zeros(3, out=out) is out
        assert not torch.empty_like(torch.empty((4, 6), device='cpu').t()).is_contiguous()
        assert torch.empty((2, 3, 4, 5), device='cpu', memory_format=torch.channels_last).stride() == (60, 1, 15, 3)
        assert len(fence._allocs) == n + 2                           # `out` and the contiguous source of the transpose


@pytest.mark.parametrize('base', [0, 4, 8, 12])
def test_base_sets_the_address_and_the_payload_ends_exactly(base):
    x = np.arange(21, dtype=np.float64).reshape(3, 7)
    with pytest.raises(FenceError) as e:
        with Fence('cpu', ZONE) as fence:
            t = fence.dev(x, base=base)
            assert t.dtype == torch.float32 and t.shape == (3, 7) and t.is_contiguous()
            assert t.data_ptr() % 256 == base
            assert np.array_equal(t.numpy(), x.astype(np.float32))
            i = fence.dev(np.arange(5), np.int32, base=base)
            assert i.dtype == torch.int32 and i.tolist() == [0, 1, 2, 3, 4] and i.data_ptr() % 256 == base
            assert fence.dev(np.arange(3), np.int64, base=base).data_ptr() % 256 == base - base % 8
            assert fence.dev(x).data_ptr() % 256 == 0
            fence.check()
            _poke(t, t.numel(), 0.0)                                 # the element after the last one is zone
    assert (e.value.zone, e.value.distance, e.value.shape) == ('back', 0, (3, 7))
    with pytest.raises(FenceError) as e:
        with Fence('cpu', ZONE) as fence:
            _poke(fence.dev(x, base=base), -1, 0.0)
    assert (e.value.zone, e.value.distance) == ('front', 4)


def test_another_device_type_gets_an_ordinary_tensor():
    with Fence('cuda', ZONE) as fence:
        a = torch.empty(5, device='cpu')
        b = torch.zeros(5)
        c = torch.ones_like(b)
        assert not fence._allocs
        assert a.untyped_storage().nbytes() == 20 and b.tolist() == [0.0] * 5 and c.tolist() == [1.0] * 5
        m = torch.empty(3, device='meta')
        assert m.device.type == 'meta'


def _state():
    from ams_hip import ops
    return [getattr(torch, n) for n in fenced.PATCHED], [getattr(ops, n) for n in fenced.CACHES]


def test_everything_is_restored_after_a_normal_exit_and_after_an_exception():
    from ams_hip import ops
    ops._ONE['fence-test'] = 1
    try:
        before = _state()
        with Fence('cpu', ZONE):
            inside = _state()
            assert all(a is not b for a, b in zip(before[0], inside[0]))
            assert all(a is not b and type(a) is type(b) for a, b in zip(before[1], inside[1]))
            assert ops._ONE == {} and ops._SK == {} and ops._DPCL_AHEAD == [None]
            ops._SK['x'] = 2
        after = _state()
        assert all(a is b for a, b in zip(before[0] + before[1], after[0] + after[1]))
        assert ops._ONE == {'fence-test': 1} and 'x' not in ops._SK
        with pytest.raises(KeyError):
            with Fence('cpu', ZONE):
                ops._STAGE = {'rebound': 1}                          # rebound, not mutated: the original object still comes back
                raise KeyError('body')
        after = _state()
        assert all(a is b for a, b in zip(before[0] + before[1], after[0] + after[1]))
        assert fenced._ACTIVE[0] is None
        with pytest.raises(FenceError):                             # ... and after a failed check
            with Fence('cpu', ZONE):
                _poke(torch.empty(3, device='cpu'), 3, 0.0)
        after = _state()
        assert all(a is b for a, b in zip(before[0] + before[1], after[0] + after[1]))
    finally:
        del ops._ONE['fence-test']


def test_a_failed_entry_leaves_no_fence_active(monkeypatch):
    from ams_hip import ops
    before = _state()
    monkeypatch.delattr(ops, '_KM_TICKETS')                        # a cache the fence expects has gone: entering fails half way
    with pytest.raises(AttributeError):
        with Fence('cpu', ZONE):
            pass
    monkeypatch.undo()
    assert fenced._ACTIVE[0] is None
    after = _state()
    assert all(a is b for a, b in zip(before[0] + before[1], after[0] + after[1]))
    with Fence('cpu', ZONE):
        pass


def test_nested_fences_are_refused():
    with Fence('cpu', ZONE):
        with pytest.raises(RuntimeError):
            with Fence('cpu', ZONE):
                pass
        assert fenced._ACTIVE[0] is not None
    assert fenced._ACTIVE[0] is None
    with Fence('cpu', ZONE):
        pass


def test_backing_tensors_are_held_until_exit():
    with Fence('cpu', ZONE) as fence:
        for _ in range(3):
            torch.empty(1000, device='cpu')                          # dropped at once by the caller
        assert len(fence._allocs) == 3 and len(set(a[0].data_ptr() for a in fence._allocs)) == 3
    assert not fence._allocs
