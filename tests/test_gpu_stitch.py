"""GPU: libams_stitch.so (include/ams_stitch.h) against the numpy restatement tests/stitch_ref.py, inside fenced buffers: every output
is NaN-filled before the kernel runs and sits between two red zones, inputs are placed at base 0 (the 16-byte arms) and base 4 (the
dword arms).  The reference project has no counterpart of this feature; tests/stitch_ref.py is what the kernels are held to."""
import ctypes

import numpy as np
import pytest

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

from tests import stitch_ref as ref
from tests.fenced import Fence

NLH = [(700, 256, 128), (251, 250, 125), (100, 256, 128), (256, 256, 128), (257, 256, 128), (5000, 2052, 1028)]
TOL_F64 = 2e-5                  # the project's kernel tolerance against float64


def _np(t):
    return t.detach().cpu().numpy()


@pytest.mark.parametrize('N,L,H', NLH)
@pytest.mark.parametrize('base', [0, 4])
def test_chunks_bit_equal(N, L, H, base):
    from ams_hip import stitch
    x = np.random.RandomState(N + L).randn(N).astype(np.float32)
    want = ref.chunks(x, L, H)
    with Fence() as fence:
        got = stitch.chunks(fence.dev(x, base=base), L, H)
        fence.check()
        assert got.shape == want.shape == (stitch.nb_chunks(N, L, H), L)
        assert np.array_equal(_np(got), want)


@pytest.mark.parametrize('L,H', [(256, 128), (250, 125), (256, 255), (2052, 1028), (4100, 2050),
                                 (4104, 2052)])      # the last: several slabs on the 16-byte arm too, ragged last one
def test_border_stats_against_float64(L, H):
    from ams_hip import stitch
    C = 3
    for S in (1, 2, 3, 6):
        est = np.random.RandomState(100 * S + L).randn(C, S, L).astype(np.float32)
        Q64 = ref.border_stats(est, H)
        for base in (0, 4):
            with Fence() as fence:
                d = fence.dev(est, base=base)
                Q = stitch.border_stats(d, H)
                Q2 = stitch.border_stats(d, H)
                fence.check()
                q, q2 = _np(Q), _np(Q2)
            err = np.abs(q - Q64).max() / np.abs(Q64).max()
            print('stats S=%d L=%d H=%d base=%d: max|Q - Q64| / max|Q64| = %.3g' % (S, L, H, base, err))
            assert q.shape == (C - 1, S, S)
            assert err <= TOL_F64, (S, base, err)
            assert np.array_equal(q.view(np.int32), q2.view(np.int32)), (S, base)      # the same bits from run to run


@pytest.mark.parametrize('S', [1, 2, 3, 4, 5, 6])
@pytest.mark.parametrize('L,H,base', [(16, 8, 0), (9, 5, 0), (16, 8, 4)])      # the 16-byte arm; the dword arm; the dword arm by misalignment
def test_border_stats_every_source_count_on_every_arm(L, H, base, S):
    """One slab, three chunks: every instantiated (S, arm) of the border sums (the slabs do not depend on S, the test above has them)."""
    from ams_hip import stitch
    C = 3
    est = np.random.RandomState(100 * S + L).randn(C, S, L).astype(np.float32)
    Q64 = ref.border_stats(est, H)
    with Fence() as fence:
        d = fence.dev(est, base=base)
        Q = stitch.border_stats(d, H)
        Q2 = stitch.border_stats(d, H)
        fence.check()
        q, q2 = _np(Q), _np(Q2)
    err = np.abs(q - Q64).max() / np.abs(Q64).max()
    print('stats S=%d L=%d H=%d base=%d: max|Q - Q64| / max|Q64| = %.3g' % (S, L, H, base, err))
    assert q.shape == (C - 1, S, S)
    assert err <= TOL_F64, (S, base, err)
    assert np.array_equal(q.view(np.int32), q2.view(np.int32)), (S, base)          # the same bits from run to run


@pytest.mark.parametrize('S', [1, 2, 3, 4, 5, 6])
def test_tracks_match_the_restatement(S):
    from ams_hip import stitch
    L, H, C = 64, 32, 10
    N = L + (C - 1) * H - 5
    src, est, perm, truth = ref.material(40 + S, S, L, H, N)
    assert est.shape[0] == C
    rel_ref, margin = ref.search(ref.border_stats(est, H))
    assert margin.min() >= 1e-3, margin.min()                     # a condition on the inputs, not a tolerance
    trk_ref = ref.tracks(rel_ref)
    assert np.array_equal(trk_ref, truth)
    with Fence() as fence:
        Q = stitch.border_stats(fence.dev(est), H)
        rel, trk = stitch.tracks(Q, S)
        fence.check()
        assert rel.dtype == trk.dtype == torch.int32
        assert np.array_equal(_np(rel), rel_ref) and np.array_equal(_np(trk), trk_ref)
        # all-zero estimates: every cost ties at zero, the lowest index -- the identity -- wins
        rel0, trk0 = stitch.tracks(stitch.border_stats(fence.dev(np.zeros_like(est)), H), S)
        fence.check()
        ident = np.tile(np.arange(S, dtype=np.int32), (C, 1))
        assert np.array_equal(_np(rel0), ident[1:]) and np.array_equal(_np(trk0), ident)


@pytest.mark.parametrize('S', [2, 6])
def test_a_nan_chunk_stays_in_its_own_samples(S):
    from ams_hip import stitch
    L, H, C, bad = 64, 32, 10, 4
    N = L + (C - 1) * H - 5
    src, est, perm, truth = ref.material(50 + S, S, L, H, N)
    est[bad] = np.nan
    rel_ref = ref.search(ref.border_stats(est, H))[0]
    ident = np.arange(S, dtype=np.int32)
    assert np.array_equal(rel_ref[bad - 1], ident) and np.array_equal(rel_ref[bad], ident)
    with Fence() as fence:
        d = fence.dev(est)
        Q = stitch.border_stats(d, H)
        rel, trk = stitch.tracks(Q, S)
        out, trk2, Q2 = stitch.stitch(d, N, H)
        fence.check()
        rel, trk, out = _np(rel), _np(trk), _np(out)
        assert np.array_equal(_np(trk2), trk)
    assert np.array_equal(rel, rel_ref) and np.array_equal(trk, ref.tracks(rel_ref))
    assert np.array_equal(rel[bad - 1], ident) and np.array_equal(rel[bad], ident)
    nan = np.zeros(N, bool)
    nan[bad * H:bad * H + L] = True
    assert np.array_equal(np.isnan(out), np.tile(nan, (S, 1)))
    want = ref.overlap_add(est, trk, N, H)
    assert np.array_equal(out[:, ~nan], want[:, ~nan])


@pytest.mark.parametrize('N,L,H', NLH)
@pytest.mark.parametrize('base', [0, 4])
def test_overlap_add_bit_equal(N, L, H, base):
    from ams_hip import stitch
    C = ref.nb_chunks(N, L, H)
    for S in (1, 3):
        rng = np.random.RandomState(N + 7 * S + base)
        est = rng.randn(C, S, L).astype(np.float32)
        trk = np.stack([rng.permutation(S) for _ in range(C)]).astype(np.int32)
        want = ref.overlap_add(est, trk, N, H)
        with Fence() as fence:
            out = stitch.overlap_add(fence.dev(est, base=base), fence.dev(trk, dtype=np.int32), N, H)
            fence.check()                                          # nothing beyond the S N samples ...
            got = _np(out)
        assert got.shape == (S, N)
        assert np.array_equal(got.view(np.int32), want.view(np.int32)), (S, int(np.isnan(got).sum()))      # ... and every one of them


@pytest.mark.parametrize('S,L,H,N', [(2, 256, 128, 700), (3, 256, 192, 1000), (6, 64, 32, 333), (2, 250, 125, 251), (5, 2052, 1028, 5000),
                                     (2, 256, 128, 200)])
def test_stitch_recovers_permuted_sources(S, L, H, N):
    """Exactly permuted true sources, no noise: outside the overlaps the stitched tracks are the sources bit for bit; inside,
    |out - src| <= 4 * 2^-24 |src|: w_tail = fl(1 - w_head) is off by at most 2^-25 in absolute terms, each of the two products by
    2^-24 relative, the add by 2^-24 relative, on two terms of the same sign that sum to src."""
    from ams_hip import stitch
    src, est, perm, truth = ref.material(60 + S, S, L, H, N, noise=0)
    want = src[np.argsort(perm[0])]
    C = ref.nb_chunks(N, L, H)
    with Fence() as fence:
        out, trk, Q = stitch.stitch(fence.dev(est), N, H)
        fence.check()
        out, trk, Q = _np(out), _np(trk), _np(Q)
    assert out.shape == (S, N) and trk.shape == (C, S) and Q.shape == (C - 1, S, S)
    assert np.array_equal(trk, truth)
    n = np.arange(N)
    c1 = np.minimum(n // H, C - 1)
    fade = (c1 > 0) & (n - c1 * H < L - H)
    assert np.array_equal(out[:, ~fade], want[:, ~fade])
    assert np.all(np.abs(out[:, fade] - want[:, fade]) <= 4 * 2.0 ** -24 * np.abs(want[:, fade]))
    assert np.array_equal(out, ref.overlap_add(est, truth, N, H))


def test_invalid_arguments_launch_nothing():
    from ams_hip import stitch
    lib = stitch.load()
    S, L, H, N = 2, 256, 128, 700
    C = ref.nb_chunks(N, L, H)
    dev = torch.device('cuda')
    x = torch.zeros(N, device=dev)
    est = torch.zeros(C, S, L, device=dev)
    perms = torch.tensor([[0, 1], [1, 0]], dtype=torch.int32, device=dev)
    w = torch.from_numpy(ref.w_head(L - H)).to(dev)
    ws = torch.full((1024,), 7.0, device=dev)
    mix, Q, out = torch.full((C, L), 7.0, device=dev), torch.full((C - 1, S, S), 7.0, device=dev), torch.full((S, N), 7.0, device=dev)
    rel, trk = torch.full((C - 1, S), 7, dtype=torch.int32, device=dev), torch.full((C, S), 7, dtype=torch.int32, device=dev)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    null, st = ctypes.c_void_p(0), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    geometry = [(1, 1), (2 ** 30 + 2, 2 ** 29 + 1), (L, H - 1), (L, L), (251, 125)]       # L < 2, L > 2^30, H below, H = L, H < ceil(L / 2)
    calls = []
    for l, h in geometry:
        calls += [lib.ams_stitch_chunks(p(x), N, p(mix), C, l, h, st),
                  lib.ams_stitch_stats(p(est), p(Q), C, S, l, h, p(ws), 4096, st),
                  lib.ams_stitch_ola(p(est), p(trk), p(w), p(out), N, C, S, l, h, st)]
    for s in (0, 7):
        calls += [lib.ams_stitch_stats(p(est), p(Q), C, s, L, H, p(ws), 4096, st),
                  lib.ams_stitch_tracks(p(Q), p(perms), p(rel), p(trk), C, s, 2, st),
                  lib.ams_stitch_ola(p(est), p(trk), p(w), p(out), N, C, s, L, H, st)]
    for c in (C - 1, C + 1, 0):                                    # C inconsistent with (N, L, H)
        calls += [lib.ams_stitch_chunks(p(x), N, p(mix), c, L, H, st), lib.ams_stitch_ola(p(est), p(trk), p(w), p(out), N, c, S, L, H, st)]
    calls += [lib.ams_stitch_stats(p(est), p(Q), 1, S, L, H, p(ws), 4096, st),             # no border
              lib.ams_stitch_tracks(p(Q), p(perms), p(rel), p(trk), 1, S, 2, st)]
    for n in (0, -5):                                              # N < 1
        calls += [lib.ams_stitch_chunks(p(x), n, p(mix), 1, L, H, st), lib.ams_stitch_ola(p(est), p(trk), p(w), p(out), n, 1, S, L, H, st)]
    for P in (1, 3, 6):                                            # P != S!
        calls.append(lib.ams_stitch_tracks(p(Q), p(perms), p(rel), p(trk), C, S, P, st))
    calls += [lib.ams_stitch_chunks(null, N, p(mix), C, L, H, st), lib.ams_stitch_chunks(p(x), N, null, C, L, H, st),
              lib.ams_stitch_stats(null, p(Q), C, S, L, H, p(ws), 4096, st), lib.ams_stitch_stats(p(est), null, C, S, L, H, p(ws), 4096, st),
              lib.ams_stitch_stats(p(est), p(Q), C, S, L, H, null, 4096, st),
              lib.ams_stitch_tracks(null, p(perms), p(rel), p(trk), C, S, 2, st), lib.ams_stitch_tracks(p(Q), null, p(rel), p(trk), C, S, 2, st),
              lib.ams_stitch_tracks(p(Q), p(perms), null, p(trk), C, S, 2, st), lib.ams_stitch_tracks(p(Q), p(perms), p(rel), null, C, S, 2, st),
              lib.ams_stitch_ola(null, p(trk), p(w), p(out), N, C, S, L, H, st), lib.ams_stitch_ola(p(est), null, p(w), p(out), N, C, S, L, H, st),
              lib.ams_stitch_ola(p(est), p(trk), null, p(out), N, C, S, L, H, st), lib.ams_stitch_ola(p(est), p(trk), p(w), null, N, C, S, L, H, st)]
    assert calls == [-1] * len(calls), calls
    assert lib.ams_stitch_stats(p(est), p(Q), C, S, L, H, p(ws), 8, st) == -2              # workspace too small: nothing launched either
    torch.cuda.synchronize()
    for t in (mix, Q, out, ws):
        assert bool((t == 7.0).all())
    for t in (rel, trk):
        assert bool((t == 7).all())
    # and the same arguments made valid run: the outputs above were reachable
    trk.copy_(torch.arange(S, dtype=torch.int32, device=dev).expand(C, S))
    assert lib.ams_stitch_chunks(p(x), N, p(mix), C, L, H, st) == 0 and lib.ams_stitch_ola(p(est), p(trk), p(w), p(out), N, C, S, L, H, st) == 0
    torch.cuda.synchronize()
    assert bool((mix == 0).all()) and bool((out == 0).all())
