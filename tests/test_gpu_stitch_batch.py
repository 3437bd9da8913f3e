"""GPU: libams_stitch_batch.so (include/ams_stitch_batch.h) against libams_stitch.so run on every recording alone -- bit for bit -- and
against the numpy restatement tests/stitch_ref.py, inside fenced buffers.  Material: stitch_ref.material(1000 + r, S, L, H, N_r); with
these seeds every border's margin in the restatement is >= 0.13 (asserted below on the host before anything is compared), so no border
is excused by the margin rule of DESIGN.md 4.7.  Not tested: offsets past 2^31 (the buffers would be over 8 GB)."""
import ctypes
import functools

import numpy as np
import pytest

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

from tests import stitch_ref as ref
from tests.fenced import Fence

GEOMETRIES = [(256, 128), (250, 125), (256, 255), (2052, 1028)]      # the 16-byte arm; the dword arm; V = 1; two slabs
SOURCES = [1, 2, 3, 6]
TOL_F64 = 2e-5                  # the project's kernel tolerance against float64
MARGIN = 0.13


def _lengths(kind, L, H):
    if kind == 'eight':         # single-chunk recordings between multi-chunk ones
        return [1, L - 1, L, L + 1, L + H, L + H + 1, 5 * L + 3, 2 * L]
    return [5 * L + 3] if kind == 'one' else [L - 1]


@functools.lru_cache(maxsize=None)
def _material(kind, S, L, H):
    """Per recording (x [N], est [C, S, L], truth [C, S], Q64 [C - 1, S, S]); computed once, shared and left unchanged."""
    recs = []
    for r, N in enumerate(_lengths(kind, L, H)):
        src, est, perm, truth = ref.material(1000 + r, S, L, H, N)
        Q64 = ref.border_stats(est, H)
        if Q64.shape[0]:
            rel, margin = ref.search(Q64)
            assert margin.min() >= MARGIN, (r, margin.min())       # a condition on the inputs, not a tolerance
            assert np.array_equal(ref.tracks(rel), truth)
        x = src.sum(axis=0).astype(np.float32)
        for a in (x, est, truth, Q64):
            a.setflags(write=False)
        recs.append((x, est, truth, Q64))
    return recs


def _np(t):
    return t.detach().cpu().numpy()


def _bits(t):
    return t.contiguous().view(torch.int32)


def _single(est_r, N, H, S):
    """libams_stitch.so on one recording's slice: (Q, rel, trk, out); a one-chunk recording has no border."""
    from ams_hip import stitch
    if est_r.shape[0] == 1:
        out, trk, Q = stitch.stitch(est_r, N, H)
        return Q, torch.empty((0, S), dtype=torch.int32, device=est_r.device), trk, out
    Q = stitch.border_stats(est_r, H)
    rel, trk = stitch.tracks(Q, S)
    return Q, rel, trk, stitch.overlap_add(est_r, trk, N, H)


def _compare(kind, S, L, H, base=0):
    from ams_hip import stitch
    from ams_hip import stitch_batch as sb
    recs = _material(kind, S, L, H)
    R = len(recs)
    ident = torch.arange(S, dtype=torch.int32, device='cuda')
    nan = float('nan')
    with Fence() as fence:
        xs = [fence.dev(x.copy()) for x, _, _, _ in recs]              # (the shared material is read-only)
        mix, lay = sb.chunks_many(xs, L, H)
        assert lay.S is None and mix.shape == (lay.Ctot, L) and lay.R == R
        # the same recordings in a packed buffer whose padding is NaN: none of it reaches mix
        xp = torch.full((lay.x_total + 4,), nan, device='cuda')
        for x, o in zip(xs, lay.x_off):
            xp[o:o + x.shape[0]] = x
        assert int(torch.isnan(xp).sum()) == lay.x_total + 4 - int(lay.n.sum())
        mix2 = sb.chunks_packed(xp, lay)
        fence.check()
        assert torch.equal(_bits(mix), _bits(mix2)) and not bool(torch.isnan(mix2).any())
        for r in range(R):
            assert torch.equal(mix[lay.rec_chunks(r)], stitch.chunks(xs[r], L, H)), r

        est = fence.dev(np.concatenate([e for _, e, _, _ in recs]), base=base)
        Q = sb.border_stats_many(est, lay)
        rel, trk = sb.tracks_many(Q, lay)
        assert Q.shape == (lay.Ctot, S, S) and rel.shape == trk.shape == (lay.Ctot, S) and rel.dtype == trk.dtype == torch.int32
        lay.set_sources(S)
        packed = torch.full((lay.out_total + 8,), nan, device='cuda')      # NaN between the blocks and behind the last one
        assert sb.overlap_add_many(est, trk, lay, out=packed) is packed
        fence.check()
        inside = torch.zeros(lay.out_total + 8, dtype=torch.bool, device='cuda')
        crossed = 0
        for r, (x, est_r, truth, Q64) in enumerate(recs):
            sl, N, o = lay.rec_chunks(r), x.shape[0], int(lay.out_off[r])
            last = sl.stop - 1
            Q1, rel1, trk1, out1 = _single(est[sl], N, H, S)
            # bit-equal to the library for one recording, row for row
            assert torch.equal(_bits(Q[sl.start:last]), _bits(Q1)), r
            assert torch.equal(rel[sl.start:last], rel1) and torch.equal(trk[sl], trk1), r
            block = packed[o:o + S * N].view(S, N)
            assert torch.equal(_bits(block), _bits(out1)), r
            inside[o:o + S * N] = True
            # the rows of a recording's last chunk: zeros, the identity
            assert bool((_bits(Q[last]) == 0).all()) and torch.equal(rel[last], ident), r
            # the float64 restatement, the truth of the material, a fresh start in every recording
            if Q64.shape[0]:
                err = np.abs(_np(Q[sl.start:last]) - Q64).max() / np.abs(Q64).max()
                print('batch stats S=%d L=%d H=%d recording %d: max|Q - Q64| / max|Q64| = %.3g' % (S, L, H, r, err))
                assert err <= TOL_F64, (r, err)
            assert np.array_equal(_np(trk[sl]), truth) and torch.equal(trk[sl.start], ident), r
            if r and not torch.equal(trk[sl.start - 1], ident):
                crossed += 1                                       # the recording before ended on another permutation
            assert np.array_equal(_np(block), ref.overlap_add(est_r, truth, N, H)), r
        if kind == 'eight' and S > 1:
            assert crossed >= 1                                    # ... so the identity above shows that no chain crosses a recording
        # nothing outside the blocks was written, every sample inside was
        assert torch.equal(torch.isnan(packed), ~inside)

        # stitch_many: the same again as views, and the same bits from call to call
        for _ in range(2):
            res = sb.stitch_many(est, lay)
            fence.check()
            assert len(res) == R
            for r, (out_r, trk_r, Q_r) in enumerate(res):
                sl, N, o = lay.rec_chunks(r), recs[r][0].shape[0], int(lay.out_off[r])
                assert out_r.shape == (S, N) and trk_r.shape == (sl.stop - sl.start, S) and Q_r.shape == (sl.stop - sl.start - 1, S, S)
                assert torch.equal(_bits(out_r), _bits(packed[o:o + S * N].view(S, N))), r
                assert torch.equal(trk_r, trk[sl]) and torch.equal(_bits(Q_r), _bits(Q[sl.start:sl.stop - 1])), r


@pytest.mark.parametrize('kind', ['eight', 'one', 'short'])
@pytest.mark.parametrize('S', SOURCES)
@pytest.mark.parametrize('L,H', GEOMETRIES)
def test_batch_is_bit_equal_to_every_recording_alone(L, H, S, kind):
    _compare(kind, S, L, H)


@pytest.mark.parametrize('S', [4, 5])
@pytest.mark.parametrize('L,H', [(16, 8), (9, 5)])                 # one slab on the 16-byte arm; one on the dword arm
def test_four_and_five_sources_on_both_arms(L, H, S):
    """The source counts that SOURCES leaves out, at the smallest geometry of either arm (with seeds 1000 + r the margin is >= 0.99)."""
    _compare('eight', S, L, H)


def test_a_misaligned_est_takes_the_dword_arm_in_both():
    _compare('eight', 2, 256, 128, base=4)


@pytest.mark.parametrize('S,L,H', [(2, 256, 128), (3, 250, 125), (6, 256, 128)])
def test_a_nan_chunk_stays_in_its_own_recording(S, L, H):
    from ams_hip import stitch
    from ams_hip import stitch_batch as sb
    recs = _material('eight', S, L, H)
    lay = sb.layout([x.shape[0] for x, _, _, _ in recs], L, H, S)
    hit, bad = 6, 2                                                # chunk 2 of the ten-chunk recording
    clean = np.concatenate([e for _, e, _, _ in recs])
    dirty = clean.copy()
    dirty[lay.c_off[hit] + bad] = np.nan
    with Fence() as fence:
        want = sb.stitch_many(fence.dev(clean), lay)
        d = fence.dev(dirty)
        got = sb.stitch_many(d, lay)
        fence.check()
        for r in range(lay.R):
            if r != hit:
                for a, b in zip(got[r], want[r]):
                    assert torch.equal(_bits(a) if a.dtype == torch.float32 else a, _bits(b) if b.dtype == torch.float32 else b), r
        N = int(lay.n[hit])
        out1, trk1, Q1 = stitch.stitch(d[lay.rec_chunks(hit)], N, H)
        fence.check()
        out, trk, Q = got[hit]
        assert torch.equal(_bits(out), _bits(out1)) and torch.equal(trk, trk1) and torch.equal(_bits(Q), _bits(Q1))
        ident = torch.arange(S, dtype=torch.int32, device='cuda')
        rel = sb.tracks_many(sb.border_stats_many(d, lay), lay)[0]
        g = int(lay.c_off[hit]) + bad                              # both borders of the NaN chunk: every cost NaN, the identity
        assert torch.equal(rel[g - 1], ident) and torch.equal(rel[g], ident)
        nan = np.zeros(N, bool)
        nan[bad * H:bad * H + L] = True
        assert np.array_equal(np.isnan(_np(out)), np.tile(nan, (S, 1)))


def test_invalid_arguments_launch_nothing():
    from ams_hip import stitch_batch as sb
    lib = sb.load()
    S, L, H = 2, 256, 128
    lay = sb.layout([700, 100, 300], L, H, S)
    R, Ctot, nblk = lay.R, lay.Ctot, lay.nblk
    dev = torch.device('cuda')
    t = lay.tables(dev)
    nan = float('nan')
    x = torch.zeros(lay.x_total, device=dev)
    est = torch.zeros(Ctot, S, L, device=dev)
    perms = torch.tensor([[0, 1], [1, 0]], dtype=torch.int32, device=dev)
    w = torch.from_numpy(ref.w_head(L - H)).to(dev)
    ws = torch.full((1024,), nan, device=dev)
    mix, Q, out = torch.full((Ctot, L), nan, device=dev), torch.full((Ctot, S, S), nan, device=dev), torch.full((lay.out_total,), nan, device=dev)
    rel, trk = torch.full((Ctot, S), 7, dtype=torch.int32, device=dev), torch.full((Ctot, S), 7, dtype=torch.int32, device=dev)
    p = lambda a: ctypes.c_void_p(a.data_ptr())
    null, st = ctypes.c_void_p(0), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    need = lib.ams_stitchb_workspace_bytes(Ctot, S, L, H)
    assert need == Ctot * 1 * S * S * 4 <= 4096

    def chunks(x=p(x), n=p(t['n']), xo=p(t['x_off']), co=p(t['c_off']), cr=p(t['chunk_rec']), mix=p(mix), R=R, Ctot=Ctot, L=L, H=H):
        return lib.ams_stitchb_chunks(x, n, xo, co, cr, mix, R, Ctot, L, H, st)

    def stats(est=p(est), cr=p(t['chunk_rec']), Q=p(Q), R=R, Ctot=Ctot, S=S, L=L, H=H, ws=p(ws), nbytes=4096):
        return lib.ams_stitchb_stats(est, cr, Q, R, Ctot, S, L, H, ws, nbytes, st)

    def tracks(Q=p(Q), perms=p(perms), co=p(t['c_off']), cr=p(t['chunk_rec']), rel=p(rel), trk=p(trk), R=R, Ctot=Ctot, S=S, P=2):
        return lib.ams_stitchb_tracks(Q, perms, co, cr, rel, trk, R, Ctot, S, P, st)

    def ola(est=p(est), trk=p(trk), w=p(w), n=p(t['n']), oo=p(t['out_off']), co=p(t['c_off']), br=p(t['blk_rec']), bo=p(t['blk_off']),
            out=p(out), R=R, Ctot=Ctot, nblk=nblk, S=S, L=L, H=H):
        return lib.ams_stitchb_ola(est, trk, w, n, oo, co, br, bo, out, R, Ctot, nblk, S, L, H, st)

    calls = []
    for s in (7, 0):                                               # S = 7
        calls += [stats(S=s), tracks(S=s), ola(S=s)]
    for l, h in [(L, H - 1), (L, L), (251, 125), (1, 1), (2 ** 30 + 2, 2 ** 29 + 1)]:      # a bad H (and a bad L)
        calls += [chunks(L=l, H=h), stats(L=l, H=h), ola(L=l, H=h)]
    for r, c in [(0, Ctot), (-1, Ctot), (R, R - 1), (Ctot + 1, Ctot)]:                     # R = 0; Ctot < R
        calls += [chunks(R=r, Ctot=c), stats(R=r, Ctot=c), tracks(R=r, Ctot=c), ola(R=r, Ctot=c)]
    calls += [ola(nblk=R - 1), tracks(P=1), tracks(P=6)]
    calls += [stats(nbytes=need - 4), stats(nbytes=0)]                                     # a short workspace
    for f, names in ((chunks, ('x', 'n', 'xo', 'co', 'cr', 'mix')), (stats, ('est', 'cr', 'Q', 'ws')),
                     (tracks, ('Q', 'perms', 'co', 'cr', 'rel', 'trk')), (ola, ('est', 'trk', 'w', 'n', 'oo', 'co', 'br', 'bo', 'out'))):
        calls += [f(**{name: null}) for name in names]                                     # a NULL pointer
    assert calls == [-1] * len(calls), calls
    torch.cuda.synchronize()
    for a in (mix, Q, out, ws):
        assert bool(torch.isnan(a).all())
    for a in (rel, trk):
        assert bool((a == 7).all())
    # and the same arguments made valid run: the outputs above were reachable
    assert chunks() == 0 and stats(nbytes=need) == 0 and tracks() == 0 and ola() == 0
    torch.cuda.synchronize()
    ident = torch.arange(S, dtype=torch.int32, device=dev).expand(Ctot, S)
    assert bool((mix == 0).all()) and bool((Q == 0).all()) and torch.equal(rel, ident) and torch.equal(trk, ident)
    for r in range(R):
        o, n = int(lay.out_off[r]), int(lay.n[r])
        assert bool((out[o:o + S * n] == 0).all())
