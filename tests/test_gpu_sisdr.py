"""GPU: utils.bss_eval.si_sdr_ragged (include/ams_sisdr.h) against the numpy float64 restatement tests/sisdr_ref.py -- the
reference project has no counterpart.  ONE call over 36 recordings covers every (Sr, Se) in 1..6 x 1..6, with a second set whose track
count differs, lengths cycled through {64, B - 1, B, B + 1, 3 B + 7} (B the exported block size: the smallest set that crosses a block
border and leaves a ragged tail), signals from tests/bss_common.mix rounded to float32 plus a DC offset.

Values by the project's dB rule (tests/bss_common.close_db: 1e-6 dB below 100 dB) where the restatement is finite, and the same NaN /
+inf / -inf where it is not; matchings exactly, under the asserted condition that the restatement's best and second-best assignment
differ by more than 1e-3 dB in mean; every recording bit-equal alone, under any grouping and from call to call."""
import numpy as np
import pytest

from tests import sisdr_ref as ref
from tests.bss_common import close_db, mix

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

FLOATS = ('pair', 'base', 'si_sdr', 'si_sdri')
EXACT = ('match_ref', 'match_est', 'missed', 'spurious', 'info')
MIN_GAP_DB = 1e-3
_CASE = {}


def _recording(rng, Sr, counts, L):
    """refs [Sr, L], one [Se, L] per count, mixture [L]: float32 with a DC offset on every row."""
    n = max([Sr] + list(counts))
    s, est = mix(rng, n, L)
    dc = lambda rows: 0.5 * rng.randn(rows, 1)                    # noqa: E731
    sets = [np.asarray((est if k == 0 else (est + 0.2 * rng.randn(n, L))[::-1])[:c] + dc(c), np.float32) for k, c in enumerate(counts)]
    x = s[:Sr].sum(axis=0) + 0.05 * rng.randn(L) + 0.5 * rng.randn()
    return np.asarray(s[:Sr] + dc(Sr), np.float32), sets, np.asarray(x, np.float32)


def _case():
    """The 36 recordings, the restatement on them (computed once, never changed) and the one call."""
    if not _CASE:
        from ams_hip import sisdr
        from utils.bss_eval import si_sdr_ragged
        B = sisdr.block()
        lengths = [64, B - 1, B, B + 1, 3 * B + 7]
        rng = np.random.RandomState(20)
        refs, ests, mixes = [], [], []
        for i, (Sr, Se) in enumerate((a, b) for a in range(1, 7) for b in range(1, 7)):
            r, e, x = _recording(rng, Sr, (Se, Se % 6 + 1), lengths[i % 5])
            refs.append(r)
            ests.append(e)
            mixes.append(x)
        want = ref.score_many(refs, ests, mixes)
        for v in want.values():
            v.setflags(write=False)
        _CASE.update(refs=refs, ests=ests, mixes=mixes, want=want, B=B, got=si_sdr_ragged(refs, ests, mixes))
    return _CASE


def _same_bits(a, b):
    return all(a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes() for k in FLOATS + EXACT)


def _rows(out, idx):
    return {k: out[k][idx] for k in FLOATS + EXACT}


def _close(got, want):
    """The dB rule where the restatement is finite; the same NaN, +inf and -inf elsewhere."""
    for key in FLOATS:
        g, w = got[key], want[key]
        assert g.shape == w.shape and g.dtype == np.float64, key
        for test in (np.isnan, np.isposinf, np.isneginf):
            assert np.array_equal(test(g), test(w)), (key, test.__name__)
        fin = np.isfinite(w)
        print(key, end=': ')
        close_db(g[fin], w[fin])


def test_one_call_over_every_pair_of_counts():
    c = _case()
    got, want = c['got'], c['want']
    assert sorted((r.shape[0], e[0].shape[0]) for r, e in zip(c['refs'], c['ests'])) == [(a, b) for a in range(1, 7) for b in range(1, 7)]
    assert all(e[0].shape[0] != e[1].shape[0] for e in c['ests'])
    assert sorted(set(r.shape[1] for r in c['refs'])) == [64, c['B'] - 1, c['B'], c['B'] + 1, 3 * c['B'] + 7]
    assert got['pair'].shape == (36, 2, 6, 6) and got['base'].shape == (36, 6) and got['missed'].shape == (36, 2)
    assert not want['info'].any() and np.isfinite(want['pair']).sum() == sum(r.shape[0] * (e[0].shape[0] + e[1].shape[0])
                                                                             for r, e in zip(c['refs'], c['ests']))
    print('range of the pair table: %.1f .. %.1f dB' % (np.nanmin(want['pair']), np.nanmax(want['pair'])))
    _close(got, want)
    # the condition for equal matchings, on the restatement and these inputs: no case left out
    gaps = [ref.gap(want['pair'][r, k], c['ests'][r][k].shape[0], c['refs'][r].shape[0]) for r in range(36) for k in range(2)]
    print('smallest gap between the best and the second-best assignment: %.4g dB in mean' % min(gaps))
    assert min(gaps) > MIN_GAP_DB
    for key in EXACT:
        assert got[key].dtype == np.int32 and np.array_equal(got[key], want[key]), key
    for r in range(36):
        Sr = c['refs'][r].shape[0]
        for k in range(2):
            n = min(Sr, c['ests'][r][k].shape[0])
            assert got['missed'][r, k] == Sr - n and got['spurious'][r, k] == c['ests'][r][k].shape[0] - n


def test_zero_mean_off_is_the_restatement_too():
    from utils.bss_eval import si_sdr_ragged
    c = _case()
    idx = [0, 7, 21, 35]
    args = [[c[k][r] for r in idx] for k in ('refs', 'ests', 'mixes')]
    want = ref.score_many(*args, zero_mean=False)
    got = si_sdr_ragged(*args, zero_mean=False)
    _close(got, want)
    assert min(ref.gap(want['pair'][i, k], c['ests'][r][k].shape[0], c['refs'][r].shape[0]) for i, r in enumerate(idx) for k in range(2)) > MIN_GAP_DB
    for key in EXACT:
        assert np.array_equal(got[key], want[key]), key
    assert not np.array_equal(got['pair'], _rows(c['got'], idx)['pair'])


def test_a_recording_does_not_depend_on_its_companions_or_the_grouping():
    from ams_hip import sisdr
    from utils.bss_eval import si_sdr_ragged
    c = _case()
    got = c['got']
    assert _same_bits(si_sdr_ragged(c['refs'], c['ests'], c['mixes']), got)                    # two identical calls
    for r in range(36):                                                                          # every recording alone
        alone = si_sdr_ragged(c['refs'][r:r + 1], c['ests'][r:r + 1], c['mixes'][r:r + 1])
        assert _same_bits(alone, _rows(got, slice(r, r + 1))), r
    # a cap that forces several groups
    Sr = [r.shape[0] for r in c['refs']]
    Se = [[e[0].shape[0], e[1].shape[0]] for e in c['ests']]
    L = [r.shape[1] for r in c['refs']]
    cap = max(sisdr.group_bytes(Sr[r:r + 1], Se[r:r + 1], L[r:r + 1]) for r in range(36))
    groups = sisdr.groups(Sr, Se, L, cap)
    assert 3 < len(groups) < 36
    before = sisdr.LAUNCHES
    assert _same_bits(si_sdr_ragged(c['refs'], c['ests'], c['mixes'], cap_bytes=cap), got)
    assert sisdr.LAUNCHES - before == 2 * len(groups)
    # reversed order: another position in the call, another grouping of the blocks
    back = si_sdr_ragged(c['refs'][::-1], c['ests'][::-1], c['mixes'][::-1])
    assert _same_bits(_rows(back, slice(None, None, -1)), got)
    before = sisdr.LAUNCHES
    si_sdr_ragged(c['refs'][:1], c['ests'][:1], c['mixes'][:1])
    assert sisdr.LAUNCHES - before == 2                                                          # as for 36 recordings


def test_flagged_recordings_follow_the_rules_and_leave_the_others_alone():
    from utils.bss_eval import si_sdr_ragged
    c = _case()
    keep = [7, 14, 33]                                            # (2, 2), (3, 3), (6, 4): recordings of the one call
    refs, ests, mixes = ([c[k][r] for r in keep] for k in ('refs', 'ests', 'mixes'))
    silent_ref = c['refs'][7].copy()
    silent_ref[1] = 0
    silent_est = [e.copy() for e in c['ests'][14]]
    silent_est[0][2] = 0
    equal = [e.copy() for e in c['ests'][7]]
    equal[0][1] = c['refs'][7][0]
    refs = [refs[0], silent_ref, refs[1], c['refs'][14], c['refs'][7], refs[2]]
    ests = [ests[0], c['ests'][7], ests[1], silent_est, equal, ests[2]]
    mixes = [mixes[0], c['mixes'][7], mixes[1], c['mixes'][14], c['mixes'][7], mixes[2]]
    got = si_sdr_ragged(refs, ests, mixes)
    want = ref.score_many(refs, ests, mixes)
    _close(got, want)
    for key in EXACT:
        assert np.array_equal(got[key], want[key]), key
    assert got['info'].tolist() == [0, 1, 0, 0, 0, 0]
    # the silent reference: its column NaN, the other column scored, no matching, nothing counted
    assert np.isnan(got['pair'][1, :, :, 1]).all() and np.isfinite(got['pair'][1, 0, :2, 0]).all() and np.isnan(got['base'][1, 1])
    assert (got['match_ref'][1] == -1).all() and (got['match_est'][1] == -1).all() and np.isnan(got['si_sdr'][1]).all()
    assert got['missed'][1].tolist() == [0, 0] and got['spurious'][1].tolist() == [0, 0]
    # the silent estimate: -inf in its row, still matched (three tracks for three references)
    assert np.isneginf(got['pair'][3, 0, 2, :3]).all() and sorted(got['match_ref'][3, 0, :3].tolist()) == [0, 1, 2]
    assert np.isneginf(got['si_sdr'][3, 0]).sum() == 1
    # the estimate equal to its reference: +inf, and matched to it
    assert np.isposinf(got['pair'][4, 0, 1, 0]) and got['match_ref'][4, 0, 0] == 1 and np.isposinf(got['si_sdri'][4, 0, 0])
    # the other recordings keep their bits
    assert _same_bits(_rows(got, [0, 2, 5]), _rows(c['got'], keep))


def test_inside_fenced_memory_from_device_tensors():
    from tests.fenced import Fence
    from utils.bss_eval import si_sdr_ragged
    c = _case()
    with Fence() as fence:
        refs = [fence.dev(r, base=4 * (i % 4)) for i, r in enumerate(c['refs'])]
        ests = [[fence.dev(t) for t in e] for e in c['ests']]
        mixes = [fence.dev(x) for x in c['mixes']]
        got = si_sdr_ragged(refs, ests, mixes)
        fence.check()                                             # no zone word changed
    # every output word was stored: nothing of the fill pattern (a NaN, 2146992120 as an integer) where the restatement has a value
    assert _same_bits(got, c['got'])
    for key in FLOATS:
        assert np.array_equal(np.isnan(got[key]), np.isnan(c['want'][key])), key
    for key in EXACT:
        assert np.array_equal(got[key], c['want'][key]), key
