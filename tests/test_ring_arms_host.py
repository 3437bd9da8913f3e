"""CPU: the arm table of the BLSTM ring kernels (tests/ring_arms.py) against its own statement and against the library.

tests/test_gpu_ring_arms.py takes its hidden sizes from ring_arms.H_CASES and its expectation of which kernel a size reaches from
ring_arms.fwd_arm / bwd_arm; what is held here needs no device."""
from tests import ring_arms as RA


def test_h_cases_cover_every_arm_at_both_ends():
    """Recomputed from fwd_arm / bwd_arm, not from a literal: every forward and every backward arm is in H_CASES with its first and
    its last hidden size, the arms 2..7 of the forward kernel with an interior size whose last workgroup, last granule and last group
    of four workgroups are partial."""
    first_f, last_f, first_b, last_b = {}, {}, {}, {}
    for H in range(1, RA.RING_MAX_H + 1):
        assert RA.takes_ring(H)
        first_f.setdefault(RA.fwd_arm(H), H)
        last_f[RA.fwd_arm(H)] = H
        first_b.setdefault(RA.bwd_arm(H), H)
        last_b[RA.bwd_arm(H)] = H
    assert not RA.takes_ring(RA.RING_MAX_H + 1)
    assert tuple(sorted(first_f)) == RA.FWD_ARMS and tuple(sorted(first_b)) == RA.BWD_ARMS
    cases = set(RA.H_CASES)
    assert len(cases) == len(RA.H_CASES) and max(cases) == RA.RING_MAX_H
    for arm in RA.FWD_ARMS:
        assert {first_f[arm], last_f[arm]} - {1} <= cases, ('forward', arm)
    for arm in RA.BWD_ARMS:
        assert {first_b[arm], last_b[arm]} - {1} <= cases, ('backward', arm)
    assert {RA.fwd_arm(H) for H in cases} == set(RA.FWD_ARMS)
    assert {RA.bwd_arm(H) for H in cases} == set(RA.BWD_ARMS)
    # the stated boundaries are where the arm changes, and nowhere else
    assert RA.FWD_BOUNDARIES == tuple((last_f[a], first_f[a + 1]) for a in RA.FWD_ARMS[:-1])
    assert RA.BWD_BOUNDARIES == tuple((last_b[a], first_b[a + 1]) for a in RA.BWD_ARMS[:-1])
    assert last_f[RA.FWD_ARMS[-1]] == last_b[RA.BWD_ARMS[-1]] == RA.RING_MAX_H
    for arm in RA.FWD_ARMS[1:]:
        inner = [H for H in RA.INTERIOR if RA.fwd_arm(H) == arm]
        assert len(inner) == 1, arm
        H = inner[0]
        assert first_f[arm] < H < last_f[arm] and H % 12 and H % 3 and RA.nw(H) % 4, H
    for a, b in RA.FWD_BOUNDARIES + RA.BWD_BOUNDARIES:
        assert a % 12 == 0 and b % 12 == 1                       # (why the interior sizes are needed)


def test_back_to_back_allocations_are_not_twins():
    """What the sweep found at H = 96, 192 and 288 (the only swept sizes whose 4H-float biases are a multiple of the caching
    allocator's 512 bytes): two SEPARATE bias tensors lay back to back, ops._twin took them for the halves of one interleaved block
    on their addresses alone, and blstm_fwd asked for a view of 8H elements of a 4H-element storage (RuntimeError).  Two storages at
    adjacent addresses are not twins; two halves of one storage are."""
    import numpy as np
    import torch
    from ams_hip import ops
    C = 128
    buf = np.zeros(4 * C, dtype=np.float32)
    a, b = torch.from_numpy(buf[:C]), torch.from_numpy(buf[C:2 * C])
    assert b.data_ptr() == a.data_ptr() + 4 * C and a.untyped_storage().data_ptr() != b.untyped_storage().data_ptr()
    assert not ops._twin(a, b)
    flat = torch.from_numpy(buf)
    assert ops._twin(flat[:C], flat[C:2 * C]) and not ops._twin(flat[C:2 * C], flat[:C])
    blk = flat.view(2, 2, C)                                      # [rows, direction, C]: the kernels' interleaved layout
    assert ops._twin(blk[:, 0], blk[:, 1]) and not ops._twin(blk[:, 1], blk[:, 0])
    assert torch.as_strided(flat[:C], (2 * C,), (1,)).numel() == 2 * C


def test_restated_nw_is_the_librarys():
    """NW, the one input of both dispatches, pinned without pinning the buffer layout: for B = 16 the bytes of a ring's sync buffer are
    constant over H = 12 k - 11 .. 12 k, strictly larger at 12 k + 1, and 0 (no ring) at 337.  These grids are 8 NW <= 224 workgroups:
    under the 512 the library assumes without a device, and under what an MI355X holds."""
    from ams_hip import _lib
    lib = _lib.load()
    for backward in (0, 1):
        prev = 0
        for k in range(1, 29):
            sizes = {int(lib.ams_blstm_ring_sync_bytes(16, H, backward)) for H in range(12 * k - 11, 12 * k + 1)}
            assert len(sizes) == 1, (backward, k, sorted(sizes))
            assert all(RA.nw(H) == k for H in range(12 * k - 11, 12 * k + 1))
            now = sizes.pop()
            assert now > prev, (backward, k, now, prev)          # k = 1: non-zero; k > 1: strictly larger at 12 (k - 1) + 1
            prev = now
        assert lib.ams_blstm_ring_sync_bytes(16, 337, backward) == 0
        assert lib.ams_blstm_ring_sync_head_bytes(16, 337, backward) == 0
    assert RA.nw(336) == 28 and RA.nw(337) == 29
