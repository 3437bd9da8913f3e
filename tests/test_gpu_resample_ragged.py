"""GPU: the ragged resampler (include/ams_resample_ragged.h, ams_hip/resample_ragged.py) against the single-signal library
(ams_hip/resample.py), bit for bit per job, and against the float64 restatement tests/resample_ref.py -- inside fenced buffers
(tests/fenced.py: NaN-filled outputs, red zones, bases 0 and 4).

  * one launch of 43 jobs of mixed ratios, lengths and channel counts, destinations adjacent: every job equals the single call on it;
    (1, 20) is the smallest pair whose 256-output window passes the 4096 staged inputs (two rounds of the decimating arm);
  * the way back: blocks of 1, 2 and 6 rows with row stride n, n_keep < M in every arm, the next block at the very next word and the
    last one ending at the red zone;
  * to_model_rate writes the packed buffer of stitch_batch.pack, gap words included; from_model_rate returns views;
  * exactly one launch per call; an invalid job list leaves the output as it was."""
import numpy as np
import pytest

from tests import resample_ref as ref
from tests.fenced import PATTERN, Fence

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

PAIRS = list(ref.PAIRS) + [(1, 1), (1, 20)]
CASES = [(u, d, N) for (u, d) in PAIRS for N in (1, 7, 1000, 5003)] + [(1, 2, 512), (1, 2, 514), (1, 20, 12000)]
CHANNELS = (1, 2, 3, 8)


def _bits(a):
    a = a.cpu().numpy() if torch.is_tensor(a) else np.asarray(a, np.float32)
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def _signals():
    rng = np.random.RandomState(412)
    return [(0.1 * rng.randn(N)).astype(np.float32) for _, _, N in CASES]


def _frames():
    rng = np.random.RandomState(413)
    out = []
    for j, (_, _, N) in enumerate(CASES):
        f = rng.randint(-32768, 32768, size=(N, CHANNELS[j % 4])).astype(np.int16)
        f[0], f[N // 2], f[N - 1] = -32768, 32767, 32767 if j % 2 else -32768
        out.append(f)
    return out


def test_the_cases_reach_two_rounds_and_the_tile_edge():
    """What the list above is chosen for, restated: a 256-output tile of (1, 20) needs more than 4096 inputs, no pair of
    resample_ref.PAIRS does; (1, 2) at 512 and 514 samples gives 256 and 257 outputs."""
    for up, down in ref.PAIRS + [(1, 20)]:
        if down > up:
            k0, k1 = ref.window(10 ** 6, up, down, np.arange(1024, 1280))
            assert (k1 - k0 > 4096) == ((up, down) == (1, 20)), (up, down, k1 - k0)
    assert [ref.out_len(N, 1, 2) for N in (512, 514)] == [256, 257]
    assert len(CASES) == 43


@pytest.mark.parametrize('base', [0, 4])
def test_one_mixed_float32_launch_is_every_single_call(base):
    from ams_hip import resample, resample_ragged as rr
    xs = _signals()
    M = [ref.out_len(N, u, d) for u, d, N in CASES]
    dst = np.concatenate([[0], np.cumsum(M)])
    with Fence() as fence:
        if base == 0:                                               # one packed input: offsets
            x = fence.dev(np.concatenate(xs))
            off = np.concatenate([[0], np.cumsum([a.shape[0] for a in xs])])
            parts = [x[off[j]:off[j + 1]] for j in range(len(xs))]
            src = [4 * int(o) for o in off[:-1]]
        else:                                                       # every signal where it lies, 4 bytes past a 256-byte boundary: addresses
            parts = [fence.dev(a, base=4) for a in xs]
            x = parts[0]
            src = [p.data_ptr() - x.data_ptr() for p in parts]
        taps, where = rr.taps_for([(u, d) for u, d, _ in CASES], x.device)
        jobs = [rr.job(src[j], N, u, d, dst[j], tap_off=where.get((u, d), 0)) for j, (u, d, N) in enumerate(CASES)]
        y = torch.empty(int(dst[-1]), dtype=torch.float32, device=x.device)
        before = rr.LAUNCHES
        rr.run(x, False, taps, jobs, y)
        assert rr.LAUNCHES == before + 1
        singles = [resample.resample(parts[j], d, u) for j, (u, d, N) in enumerate(CASES)]
        fence.check()
        got = y.cpu().numpy()
        assert np.isfinite(got).all()
        for j, (u, d, N) in enumerate(CASES):
            assert singles[j].shape == (M[j],)
            assert np.array_equal(_bits(got[dst[j]:dst[j + 1]]), _bits(singles[j])), (u, d, N)
    # and the float64 restatement under its derived bound
    for j, (u, d, N) in enumerate(CASES):
        mine = got[dst[j]:dst[j + 1]].astype(np.float64)
        if u == d:
            assert np.array_equal(mine, xs[j].astype(np.float64))
        else:
            assert (np.abs(mine - ref.resample(xs[j], u, d)) <= ref.tolerance(xs[j], u, d)).all(), (u, d, N)


def test_one_mixed_int16_launch_is_every_single_call():
    from ams_hip import resample, resample_ragged as rr
    fs = _frames()
    M = [ref.out_len(N, u, d) for u, d, N in CASES]
    dst = np.concatenate([[0], np.cumsum(M)])
    words = [f.size for f in fs]
    off = np.concatenate([[0], np.cumsum(words)])
    with Fence() as fence:
        x = fence.dev(np.concatenate([f.reshape(-1) for f in fs]), dtype=np.int16)
        taps, where = rr.taps_for([(u, d) for u, d, _ in CASES], x.device)
        jobs = [rr.job(2 * int(off[j]), N, u, d, dst[j], channels=fs[j].shape[1], tap_off=where.get((u, d), 0))
                for j, (u, d, N) in enumerate(CASES)]
        y = torch.empty(int(dst[-1]), dtype=torch.float32, device=x.device)
        before = rr.LAUNCHES
        rr.run(x, True, taps, jobs, y)
        assert rr.LAUNCHES == before + 1
        singles = [resample.from_pcm16(fence.dev(fs[j], dtype=np.int16), d, u) for j, (u, d, N) in enumerate(CASES)]
        fence.check()
        got = y.cpu().numpy()
        assert np.isfinite(got).all()
        for j, (u, d, N) in enumerate(CASES):
            assert np.array_equal(_bits(got[dst[j]:dst[j + 1]]), _bits(singles[j])), (u, d, N, fs[j].shape[1])
    for j, (u, d, N) in enumerate(CASES):                           # the decode itself, where nothing is filtered
        if u == d:
            assert np.array_equal(_bits(got[dst[j]:dst[j + 1]]), _bits(ref.downmix32(fs[j])))


# (up, down, n, n_keep): the way back of 7001 samples at 44.1 kHz (1271 at 8 kHz, 7007 back, 7001 kept); cuts inside a tile, at a tile
# edge and one short of M in the interpolating, the decimating (one and two rounds) and the copying arm
BACK = [(441, 80, 1271, 7001), (2, 1, 1271, 2541), (6, 1, 500, 2816), (1, 2, 1271, 300), (80, 441, 5003, 907), (1, 20, 12000, 300),
        (1, 20, 12000, 599), (1, 1, 777, 300)]


@pytest.mark.parametrize('rows', [1, 2, 6])
def test_the_way_back_cuts_every_block_to_n_keep(rows):
    from ams_hip import resample, resample_ragged as rr
    rng = np.random.RandomState(500 + rows)
    blocks = [(0.1 * rng.randn(rows, n)).astype(np.float32) for _, _, n, _ in BACK]
    off = np.concatenate([[0], np.cumsum([b.size for b in blocks])])
    dst = np.concatenate([[0], np.cumsum([rows * k for _, _, _, k in BACK])])
    for (u, d, n, k) in BACK:
        assert 1 <= k < ref.out_len(n, u, d)
    with Fence() as fence:
        x = fence.dev(np.concatenate([b.reshape(-1) for b in blocks]), base=4 if rows == 2 else 0)
        taps, where = rr.taps_for([(u, d) for u, d, _, _ in BACK], x.device)
        jobs = [rr.job(4 * int(off[j]), n, u, d, dst[j], rows=rows, tap_off=where.get((u, d), 0), n_keep=k)
                for j, (u, d, n, k) in enumerate(BACK)]
        assert all(q[3] == q[1] and q[9] == q[10] for q in jobs)    # row stride n in, n_keep out: nothing between the rows
        y = torch.empty(int(dst[-1]), dtype=torch.float32, device=x.device)     # the last block ends at the red zone
        rr.run(x, False, taps, jobs, y)
        for j, (u, d, n, k) in enumerate(BACK):
            block = x[off[j]:off[j + 1]].view(rows, n)
            want = (block if u == d else resample.resample(block, d, u))[:, :k]
            got = y[dst[j]:dst[j + 1]].view(rows, k)
            assert np.array_equal(_bits(got), _bits(want.contiguous())), (u, d, n, k)
        fence.check()


def test_to_model_rate_writes_the_packed_buffer_of_the_layout():
    from ams_hip import resample, resample_ragged as rr
    from ams_hip import stitch_batch as sb
    rng = np.random.RandomState(61)
    lengths, chans, rates = (7001, 9000, 2100, 333), (2, 1, 3, 8), [16000, 44100, 8000, 48000]
    frames = [rng.randint(-32768, 32768, size=(N, c)).astype(np.int16) for N, c in zip(lengths, chans)]
    frames[1] = frames[1][:, 0]                                     # [N]: one channel
    floats = [(0.1 * rng.randn(N)).astype(np.float32) for N in lengths]
    with Fence() as fence:
        for recs, pcm in ((frames, True), (floats, False)):
            dev = [fence.dev(a, dtype=a.dtype, base=0) for a in recs]
            singles = [resample.from_pcm16(t, fs, 8000) if pcm else resample.resample(t, fs, 8000) for t, fs in zip(dev, rates)]
            before = rr.LAUNCHES
            xp, lay = rr.to_model_rate(recs, rates, L=2048, H=1024, S=2, fs_model=8000)          # host arrays: one upload
            xd, lay_d = rr.to_model_rate(dev, rates, lay=lay, fs_model=8000)                      # device tensors: read where they lie
            assert rr.LAUNCHES == before + 2 and lay_d is lay
            assert lay.n.tolist() == [3501, 1633, 2100, 56] == [int(s.shape[0]) for s in singles] and lay.x_total == 3504 + 1636 + 2100 + 56
            want = sb.pack(singles, lay)
            assert xp.shape == want.shape == (lay.x_total,)
            assert np.array_equal(_bits(xp), _bits(want)) and np.array_equal(_bits(xd), _bits(want))     # gap words included: zeros
            fence.check()


def test_from_model_rate_returns_views_of_one_buffer():
    from ams_hip import resample, resample_ragged as rr
    from ams_hip import stitch_batch as sb
    S = 6
    lay = sb.layout([1271, 500, 3000], 2048, 1024, S)
    rng = np.random.RandomState(62)
    rows, fs_out, keep = [1, 2, 6], [44100, 8000, 16000], [7001, 123, 5999]
    with Fence() as fence:
        out = fence.dev((0.1 * rng.randn(lay.out_total)).astype(np.float32))
        before = rr.LAUNCHES
        res = rr.from_model_rate(out, lay, rows, fs_out, keep, fs_model=8000)
        assert rr.LAUNCHES == before + 1
        for r in range(3):
            o, n = int(lay.out_off[r]), int(lay.n[r])
            block = out[o:o + rows[r] * n].view(rows[r], n)
            if fs_out[r] == 8000:
                assert res[r].data_ptr() == block.data_ptr() and res[r].shape == block.shape       # a view of the input, no job
            else:
                want = resample.resample(block, 8000, fs_out[r])[:, :keep[r]]
                assert res[r].shape == (rows[r], keep[r]) and np.array_equal(_bits(res[r]), _bits(want.contiguous()))
        assert res[2].data_ptr() == res[0].data_ptr() + 4 * 1 * 7001                              # one buffer, the blocks adjacent
        same = rr.from_model_rate(out, lay, 2, [8000] * 3, [1, 1, 1], fs_model=8000)              # nothing to convert: no launch
        assert rr.LAUNCHES == before + 1 and [tuple(t.shape) for t in same] == [(2, 1271), (2, 500), (2, 3000)]
        fence.check()


@pytest.mark.parametrize('R', [1, 23])
def test_one_launch_whatever_the_number_of_recordings(R):
    from ams_hip import resample, resample_ragged as rr
    rng = np.random.RandomState(R)
    rates = [(16000, 44100, 48000, 8000)[r % 4] for r in range(R)]
    recs = [(0.1 * rng.randn(300 + 37 * r)).astype(np.float32) for r in range(R)]
    with Fence():
        before = rr.LAUNCHES
        xp, lay = rr.to_model_rate(recs, rates, L=2048, H=1024, S=2, fs_model=8000)
        assert rr.LAUNCHES == before + 1
        outs = rr.from_model_rate(torch.zeros(lay.out_total, dtype=torch.float32, device=xp.device), lay, 2, rates,
                                  [r.shape[0] for r in recs], fs_model=8000)
        assert rr.LAUNCHES == before + 2 and len(outs) == R
        for r in range(R):
            want = resample.resample(torch.from_numpy(recs[r]).cuda(), rates[r], 8000)
            assert np.array_equal(_bits(xp[int(lay.x_off[r]):int(lay.x_off[r]) + int(lay.n[r])]), _bits(want)), r
            assert outs[r].shape == (2, recs[r].shape[0]) and not _bits(outs[r]).any()            # +0.0 from silence


def test_an_invalid_job_list_leaves_the_output_untouched():
    from ams_hip import resample_ragged as rr
    from ams_hip._lib import AmsError
    with Fence() as fence:
        x = fence.dev(np.ones(4000, np.float32))
        pcm = fence.dev(np.ones(4000, np.int16), dtype=np.int16)
        taps, where = rr.taps_for([(1, 2), (2, 1)], x.device)
        y = torch.empty(3000, dtype=torch.float32, device=x.device)
        good = rr.job(0, 1000, 1, 2, 0, tap_off=where[(1, 2)])
        before = rr.LAUNCHES
        for bad in ([good, rr.job(0, 1000, 1, 2, 500, tap_off=where[(1, 2)], n_keep=501)],           # n_keep = M + 1
                    [good, rr.job(0, 1000, 2, 1, 1001, tap_off=where[(2, 1)])],                      # 2000 outputs from 1001: past the end of y
                    [good, rr.job(0, 500, 2, 1, 500, rows=3, tap_off=where[(2, 1)])],                # the third row leaves y
                    [good, rr.job(0, 1000, 2, 4, 500)], [good, rr.job(0, 1000, 1, 2, 500, tap_off=where[(1, 2)] + 42)],
                    [good, rr.job(2, 1000, 1, 2, 500, tap_off=where[(1, 2)])], [good, rr.job(0, 1000, 1, 2, 500, channels=2)], []):
            with pytest.raises(AmsError, match='INVALID_ARG'):
                rr.run(x, False, taps, bad, y)
        with pytest.raises(AmsError, match='INVALID_ARG'):
            rr.run(pcm, True, taps, [good], y)                      # float32 rows to the int16 call
        with pytest.raises(AmsError):
            rr.run(pcm, False, taps, [good], y)                     # int16 data to the float32 call
        assert rr.LAUNCHES == before
        torch.cuda.synchronize()
        assert (y.view(torch.int32) == PATTERN).all()               # the NaN fill, every word
        rr.run(x, False, taps, [good], y)                           # and the good job alone goes through
        assert rr.LAUNCHES == before + 1 and bool(torch.isfinite(y[:500]).all()) and (y[500:].view(torch.int32) == PATTERN).all()
