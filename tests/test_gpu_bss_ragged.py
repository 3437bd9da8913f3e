"""GPU: ragged BSS-eval (include/ams_bss_ragged.h through utils/bss_eval.py) against the numpy oracle on each recording alone, the pinned
reference vectors and the batched path, plus the properties a ragged call must keep: a result is a function of its recording's data only
(bit-equal to the call on the recording alone, at any position, under any grouping), a silent reference poisons its own recording only,
nothing outside the operands is touched, and a short workspace launches nothing.

dB rule (tests/test_bss_golden.py, unchanged): 1e-6 dB where the expected value is below 100 dB, "stays above 100 dB" above."""
import functools

import numpy as np
import pytest

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

from oracle import bss_eval as obss
from tests.bss_common import G, close_db as _close_db, cupy_db as _cupy_db, mix as _mix, oracle as _oracle


def _ragged(seed, lengths, K, nsrc):
    """The _batch construction of tests/test_gpu_bss_batch.py, one length per recording."""
    rng = np.random.RandomState(seed)
    refs, ests = [], []
    for L in lengths:
        r, e = _mix(rng, nsrc, L)
        refs.append(r)
        ests.append(np.stack([e[::-1]] + [e + 0.2 * k * rng.randn(nsrc, L) for k in range(1, K)]))
    return refs, ests


def _lengths():
    from utils import bss_eval as hb
    B, F = hb.ragged_block(), 32
    return [100, 255, 256, 257, B - F, B - F + 1, B - F + 2, B, B + 1, 2 * B + 3]


@functools.lru_cache(maxsize=None)
def _ten():
    """The 10-recording case (F = 32, S = 2, K = 2): data, the oracle, one ragged call.  Computed once, never modified."""
    from utils import bss_eval as hb
    refs, ests = _ragged(10, _lengths(), 2, 2)
    want, _ = _oracle(refs, ests, 32)
    crit, info = hb.bss_eval_pairs_ragged(refs, ests, flen=32)
    return refs, ests, want, crit, info


def test_ten_recordings_against_the_oracle_and_alone():
    from utils import bss_eval as hb
    refs, ests, want, crit, info = _ten()
    assert crit.shape == (10, 2, 3, 2, 2) and not info.any()
    for r in range(10):
        _close_db(crit[r], want[r])
    back, binfo = hb.bss_eval_pairs_ragged(refs[::-1], ests[::-1], flen=32)            # the same list reversed, a second call
    assert not binfo.any()
    for r in range(10):
        _close_db(back[9 - r], want[r])
        alone, ainfo = hb.bss_eval_pairs_ragged(refs[r:r + 1], ests[r:r + 1], flen=32)
        assert not ainfo.any()
        assert np.array_equal(crit[r], alone[0]), r              # bit-equal: a function of the recording's data only
        assert np.array_equal(back[9 - r], alone[0]), r


def test_device_tensors_and_a_single_set():
    from utils import bss_eval as hb
    refs, ests, want, crit, _ = _ten()
    t = lambda a: torch.tensor(a, dtype=torch.float64, device='cuda')                  # noqa: E731
    got, info = hb.bss_eval_pairs_ragged([t(r) for r in refs[:4]], [t(e) for e in ests[:4]], flen=32)
    assert not info.any() and np.array_equal(got, crit[:4])
    one, info = hb.bss_eval_pairs_ragged(refs[:4], [e[1] for e in ests[:4]], flen=32)  # [S, L_r]: K = 1
    assert one.shape == (4, 1, 3, 2, 2)
    assert np.array_equal(one[:, 0], crit[:4, 1])               # a set's result does not depend on the other sets


@pytest.mark.parametrize('names', [('n2_L20480', 'n2_L3000', 'n2_mixture_as_estimate', 'n2_near_silent_estimate'), ('n3_L3000', 'n3_L20480')])
def test_pinned_vectors_flen_512(names):
    """The golden shapes (S = 2 and 3, L = 3000 and 20480) in ONE ragged call per S, against tests/golden/bss_eval.npz."""
    from utils import bss_eval as hb
    refs = [G[n + '/ref'] for n in names]
    ests = [G[n + '/est'] for n in names]
    assert len({r.shape[1] for r in refs}) == 2
    crit, info = hb.bss_eval_pairs_ragged(refs, ests)
    assert not info.any()
    for r, n in enumerate(names):
        ref_c = _cupy_db(n)
        for c in range(3):
            _close_db(crit[r, 0, c], ref_c[c])
    perm = hb.bss_eval_sources_ragged(refs, ests)[3]
    for r, n in enumerate(names):
        assert np.array_equal(perm[r, 0], G[n + '/perm'])


def test_long_recording_flen_512():
    from utils import bss_eval as hb
    refs, ests = _ragged(70001, [70001], 1, 2)
    crit, info = hb.bss_eval_pairs_ragged(refs, ests)
    assert not info.any()
    _close_db(crit, _oracle(refs, ests, obss.FLEN)[0])


def test_equal_lengths_against_the_batched_path_and_the_oracle():
    from utils import bss_eval as hb
    U, K, S, L = 3, 2, 2, 3000
    refs, ests = _ragged(33, [L] * U, K, S)
    crit, info = hb.bss_eval_pairs_ragged(refs, ests)
    assert not info.any()
    batch, binfo = hb.bss_eval_pairs_batch(np.stack(refs), np.stack(ests))
    assert not binfo.any()
    _close_db(crit, batch)
    want, wperm = _oracle(refs, ests, obss.FLEN)
    _close_db(crit, want)
    got = hb.bss_eval_sources_ragged(refs, ests)
    ref = hb.bss_eval_sources_batch(np.stack(refs), np.stack(ests))
    assert np.array_equal(got[3], ref[3]) and np.array_equal(got[3], wperm)
    for c in range(3):
        _close_db(got[c], ref[c])


@pytest.mark.parametrize('S', [1, 6])
def test_one_and_six_sources(S):
    """F = 16: the Gram order 96 of S = 6 is not a multiple of the 64-row tiles."""
    from utils import bss_eval as hb
    refs, ests = _ragged(S, [500, 431], 1, S)
    crit, info = hb.bss_eval_pairs_ragged(refs, ests, flen=16)
    assert crit.shape == (2, 1, 3, S, S) and not info.any()
    _close_db(crit, _oracle(refs, ests, 16)[0])


@pytest.mark.parametrize('flen', [20, 1, 300])
def test_lag_tiles_that_are_not_full(flen):
    """F = 20 and F = 1: one tile of 256 lags, mostly empty; F = 300: a full tile and a partial one."""
    from utils import bss_eval as hb
    refs, ests = _ragged(flen, [1500, 777], 2, 2)
    crit, info = hb.bss_eval_pairs_ragged(refs, ests, flen=flen)
    assert not info.any()
    _close_db(crit, _oracle(refs, ests, flen)[0])


def test_silent_reference_poisons_its_own_recording_only():
    from utils import bss_eval as hb
    refs, ests = _ragged(5, [3000, 1200, 5000, 800], 2, 2)
    refs[2] = refs[2].copy()
    refs[2][1] = 0.0                                           # a Gram matrix of recording 2 is singular (a numerical condition)
    crit, info = hb.bss_eval_pairs_ragged(refs, ests, flen=64)
    assert info[2] != 0 and not info[[0, 1, 3]].any()
    assert np.isnan(crit[2]).all()
    rest, rinfo = hb.bss_eval_pairs_ragged(refs[:2] + refs[3:], ests[:2] + ests[3:], flen=64)
    assert not rinfo.any() and np.isfinite(rest).all()
    assert np.array_equal(crit[[0, 1, 3]], rest)               # bit-equal to the same call without it


def test_forty_short_recordings():
    from utils import bss_eval as hb
    rng = np.random.RandomState(40)
    lengths = rng.randint(60, 400, size=40).tolist()
    refs, ests = _ragged(41, lengths, 1, 2)
    crit, info = hb.bss_eval_pairs_ragged(refs, ests, flen=8)
    assert crit.shape == (40, 1, 3, 2, 2) and not info.any()
    _close_db(crit, _oracle(refs, ests, 8)[0])


def test_grouping_under_the_cap_changes_nothing():
    from utils import bss_eval as hb
    refs, ests, _, crit, _ = _ten()
    lengths = _lengths()
    lib = hb._load_ragged()
    B = hb.ragged_block()
    cap = max(lib.ams_bssr_workspace_bytes(1, 2, 2, 32, -(-(L + 31) // B)) for L in lengths) * 3
    assert hb._ragged_groups(lengths, 2, 2, 32, 1 << 40) == [(0, 10)] and len(hb._ragged_groups(lengths, 2, 2, 32, cap)) >= 3
    whole, wi = hb.bss_eval_pairs_ragged(refs, ests, flen=32, cap_bytes=1 << 40)
    split, si = hb.bss_eval_pairs_ragged(refs, ests, flen=32, cap_bytes=cap)
    assert not wi.any() and not si.any()
    assert np.array_equal(whole, split) and np.array_equal(whole, crit)
    with pytest.raises(hb.BssError, match='cap'):
        hb.bss_eval_pairs_ragged(refs, ests, flen=32, cap_bytes=1000)


def _packed(refs, ests):
    return np.concatenate([r.reshape(-1) for r in refs]), np.concatenate([e.reshape(-1) for e in ests])


def test_inside_fenced_buffers():
    """Red zones around the operands, NaN-filled outputs and workspace, the operands at a base of 8 bytes past a 256-byte boundary (the
    alignment float64 needs and no more): the results are the unfenced ones and no zone word changes."""
    from tests.fenced import Fence
    from utils import bss_eval as hb
    refs, ests, _, crit, _ = _ten()
    pr, pe = _packed(refs, ests)
    lengths = _lengths()
    hb._ragged_layout(lengths, 32).tables('cuda')              # the tables are uploaded (and kept) outside the fence
    with Fence() as fence:
        for base in (0, 8):
            r = fence.dev(pr, dtype=np.float64, base=base)
            e = fence.dev(pe, dtype=np.float64, base=base)
            assert r.data_ptr() % 256 == base
            c, info = hb.bss_eval_pairs_ragged_packed(r, e, lengths, 2, 2, 32)
            fence.check()
            assert not info.cpu().numpy().any()
            assert np.array_equal(c.cpu().numpy(), crit), base
            assert torch.equal(r.cpu(), torch.from_numpy(pr)) and torch.equal(e.cpu(), torch.from_numpy(pe))


def test_short_workspace_launches_nothing():
    from utils import bss_eval as hb
    refs, ests, _, _, _ = _ten()
    pr, pe = _packed(refs[:3], ests[:3])
    lengths = _lengths()[:3]
    lay = hb._ragged_layout(lengths, 32)
    lib = hb._load_ragged()
    nb = lib.ams_bssr_workspace_bytes(lay.R, 2, 2, 32, lay.Btot)
    r, e = torch.from_numpy(pr).cuda(), torch.from_numpy(pe).cuda()
    ws = torch.zeros(nb, dtype=torch.uint8, device='cuda')
    with pytest.raises(hb.BssError, match='-2'):
        hb.bss_eval_pairs_ragged_packed(r, e, lengths, 2, 2, 32, ws=ws[:nb - 1])
    l_off, b_off, tab = lay.tables('cuda')
    crit = torch.full((3, 2, 3, 2, 2), 7.0, dtype=torch.float64, device='cuda')
    info = torch.full((3,), 9, dtype=torch.int32, device='cuda')
    args = [r.data_ptr(), e.data_ptr(), l_off.data_ptr(), b_off.data_ptr(), tab.data_ptr(), 3, 2, 2, 32, lay.Btot, crit.data_ptr(),
            info.data_ptr(), ws.data_ptr()]
    assert lib.ams_bssr_eval(*args, nb - 1, torch.cuda.current_stream().cuda_stream) == -2
    torch.cuda.synchronize()
    assert (crit == 7.0).all() and (info == 9).all() and not ws.any()          # nothing was launched
    assert lib.ams_bssr_eval(*args, nb, torch.cuda.current_stream().cuda_stream) == 0
    torch.cuda.synchronize()
    got, _ = hb.bss_eval_pairs_ragged(refs[:3], ests[:3], flen=32)
    assert np.array_equal(crit.cpu().numpy(), got) and not info.cpu().numpy().any()
