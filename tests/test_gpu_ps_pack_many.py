"""GPU: ams_ps_pack_many (csrc/gemm_ps.hip) -- several PS32 operand images from ONE flat launch -- against the separate launches
ams_ps_pack_rows / ams_ps_pack_cols, which run the same two device functions: every image byte for byte, nothing outside an image
touched (tests/fenced.py: red zones, NaN-filled outputs).

Shapes: K = 40 and 88 (the last k-tile partly past K), K = 256, K = 8 (one partial tile), R / N = 72 (not a multiple of 64) and 1, a row
pitch larger than the row (a column slice of a wider matrix), a bound per region.  Tables of 1 region, of 8, of rows and cols mixed, and
of more than 8 (the wrapper's second launch)."""
import numpy as np
import pytest

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

# (kind, rows of the source, columns of the source, row pitch of the source or 0 = dense, bound)
ROWS = [('rows', 72, 40, 0, 1.0), ('rows', 130, 88, 0, 0.37), ('rows', 64, 256, 0, 3.0), ('rows', 72, 40, 56, 0.02),
        ('rows', 1, 8, 0, 1.0), ('rows', 300, 264, 272, 5.0)]
COLS = [('cols', 40, 72, 0, 1.0), ('cols', 88, 130, 0, 0.37), ('cols', 256, 64, 0, 3.0), ('cols', 40, 72, 100, 0.02),
        ('cols', 8, 1, 0, 1.0), ('cols', 600, 200, 208, 5.0)]
TABLES = {
    'one_rows': ROWS[:1],
    'one_cols': COLS[1:2],
    'eight_mixed': [ROWS[0], COLS[0], ROWS[1], COLS[1], COLS[3], ROWS[3], ROWS[2], COLS[2]],
    'eight_rows_then_cols': ROWS[:4] + COLS[:4],
    'cols_first_big': [COLS[5], ROWS[5], COLS[4], ROWS[4]],
    'twelve': ROWS + COLS,
}


def _operands(table, fence, seed):
    rng = np.random.RandomState(seed)
    items = []
    for kind, r, c, ld, bound in table:
        wide = rng.uniform(-bound, bound, (r, ld if ld else c)).astype(np.float32)
        wide[rng.randint(r), rng.randint(c)] = bound            # the bound is met
        src = fence.dev(wide)[:, :c]                            # (a view: row pitch ld, dense rows)
        items.append((src, fence.dev(np.array([bound], np.float32)), kind))
    return items


@pytest.mark.parametrize('name', sorted(TABLES))
def test_one_launch_equals_the_separate_launches(name):
    from ams_hip import ops as K
    from tests.fenced import Fence
    with Fence() as fence:
        items = _operands(TABLES[name], fence, seed=len(name))
        many = K.ps_pack_many(items)
        fence.check()
        single = [(K.ps_pack_rows if kind == 'rows' else K.ps_pack_cols)(src, amax) for src, amax, kind in items]
        fence.check()
        assert len(many) == len(single) == len(items)
        for (src, amax, kind), a, b in zip(items, many, single):
            K_len = src.shape[1] if kind == 'rows' else src.shape[0]
            R = src.shape[0] if kind == 'rows' else src.shape[1]
            assert tuple(a.shape) == tuple(b.shape) == (R, (K_len + 31) // 32 * 128) and a.dtype == torch.uint8
            assert torch.equal(a, b), (name, kind, tuple(src.shape))
            # every byte of the image was written (no NaN pattern left) and k >= K is zero in both planes
            planes = a.cpu().numpy().view(np.float16).reshape(R, -1, 2, 32)
            assert not np.isnan(planes.astype(np.float32)).any()
            tail = planes.transpose(0, 2, 1, 3).reshape(R, 2, -1)[:, :, K_len:]
            assert not tail.any()


@pytest.mark.parametrize('workgroups,lds_pad', [(1, 0), (3, 0), (7, 128 * 1024), (10 ** 6, 4096)])
def test_fewer_workgroups_than_blocks_and_a_padded_launch(workgroups, lds_pad):
    """The launch form of the forward side branch (few workgroups walking the blocks with the grid's stride, a dynamic-LDS pad that
    keeps them off the CUs of a recurrence ring): rows bodies and cols bodies, whose LDS tile is reused from block to block, alternate
    in one workgroup.  Same bytes, nothing outside."""
    from ams_hip import ops as K
    from tests.fenced import Fence
    with Fence() as fence:
        items = _operands(TABLES['eight_mixed'], fence, seed=11)
        many = K.ps_pack_many(items, workgroups=workgroups, lds_pad=lds_pad)
        fence.check()
        for (src, amax, kind), a in zip(items, many):
            assert torch.equal(a, (K.ps_pack_rows if kind == 'rows' else K.ps_pack_cols)(src, amax)), (kind, tuple(src.shape))


def test_regions_take_their_own_bounds():
    """The same matrix under two bounds in one table: two different images, each the one its own launch writes."""
    from ams_hip import ops as K
    from tests.fenced import Fence
    with Fence() as fence:
        x = fence.dev(np.random.RandomState(3).uniform(-1, 1, (72, 88)).astype(np.float32))
        b1, b2 = fence.dev(np.array([1.0], np.float32)), fence.dev(np.array([64.0], np.float32))
        a1, a2, c2 = K.ps_pack_many([(x, b1, 'rows'), (x, b2, 'rows'), (x, b2, 'cols')])
        assert torch.equal(a1, K.ps_pack_rows(x, b1)) and torch.equal(a2, K.ps_pack_rows(x, b2)) and torch.equal(c2, K.ps_pack_cols(x, b2))
        assert not torch.equal(a1, a2)


def test_refused_tables():
    from ams_hip import ops as K
    from ams_hip._lib import AmsError
    import ctypes
    x = torch.ones(8, 8, device='cuda')
    b = torch.ones(1, device='cuda')
    with pytest.raises(AmsError):
        K.ps_pack_many([(x, b, 'diag')])
    with pytest.raises(AmsError):
        K.ps_pack_many([(x.t(), b, 'rows')])
    lib = K.load()
    tab = (K._PackRegion * 9)()
    assert lib.ams_ps_pack_many(ctypes.cast(tab, ctypes.c_void_p), 9, 0, 0, None) == -1       # more than AMS_PS_PACK_MAX regions
    assert lib.ams_ps_pack_many(ctypes.cast(tab, ctypes.c_void_p), 0, 0, 0, None) == -1
    assert lib.ams_ps_pack_many(ctypes.cast(tab, ctypes.c_void_p), 1, 0, 0, None) == -1       # a region without pointers
    assert lib.ams_ps_pack_many(ctypes.cast(tab, ctypes.c_void_p), 1, -1, 0, None) == -1
    assert lib.ams_ps_pack_many(ctypes.cast(tab, ctypes.c_void_p), 1, 0, 200 * 1024, None) == -1
