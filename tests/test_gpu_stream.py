"""GPU: libams_stream.so alone (ams_hip/stream.py: StreamSeparator with a stub in place of the model) against the offline stitcher
libams_stitch.so on the same chunk estimates -- bit for bit -- and against the numpy restatement tests/stream_ref.py.

The stub returns rows of stitch_ref.material estimates (noise 1e-3): the test mirrors which chunks of which stream a push makes ready
(the definition of DESIGN.md 4.15, stepped chunk by chunk here, not ams_hip.stream.plan) and the stub hands out exactly those.

Geometries.  The dword arms: (16, 8), (9, 5), (8, 7); the 16-byte arm: (2048, 1024) with one slab of border positions and (4104, 2052)
with three.  The feature request named (4096, 1536) for the three-slab case; that hop is below ceil(L / 2), which check_geometry and
every stitcher library refuse (no sample may lie in more than two chunks) -- test_the_refused_geometry asserts the refusal, and
(4104, 2052), V = 2052 = 2 * 1024 + 4, takes its place: three slabs, the last one of a single 16-byte group."""
import numpy as np
import pytest

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

from tests import stitch_ref as ref
from tests import stream_ref as sref

GEOMETRIES = [(16, 8), (9, 5), (8, 7), (2048, 1024), (4104, 2052)]
PER_PUSH = 6                                                       # 2 launches of feed + 4 of absorb, whatever is pushed


def _bits(t):
    return t.contiguous().view(torch.int32)


class Stub(object):
    """infer: hands out the rows of `ests` {slot: [C, S, L] numpy} that `next` [(slot, first chunk, rows)] names; keeps the mix rows."""

    def __init__(self, ests, up=None):
        self.ests, self.next, self.mix, self.calls = ests, None, {s: [] for s in ests}, 0
        self.up = up or (lambda a: torch.from_numpy(a).cuda())

    def __call__(self, mix):
        self.calls += 1
        want = [self.ests[s][c0:c0 + r] for s, c0, r in self.next if r]
        est = np.ascontiguousarray(np.concatenate(want))
        assert mix.shape[0] == est.shape[0]
        at = 0
        for s, c0, r in self.next:
            if r:
                self.mix[s].append(mix[at:at + r].clone())
            at += r
        return self.up(est)


def _ready(N, D, k, closing, L, H):
    """rows a push of k samples makes ready for a stream at (N, D) -- stepped chunk by chunk -- and (N, D) after it"""
    n1, d = N + k, D
    while n1 >= d * H + L:
        d += 1
    if closing and n1 > 0 and (d == 0 or n1 > (d - 1) * H + L):
        d += 1
    return d - D, n1, d


def _drive(sep, stub, xs, sizes, up=None):
    """xs {slot: x}, sizes {slot: [block sizes]} (adding up to len(x)): round r pushes block r of every slot that still has one (None
    for the others) and then closes the slots whose blocks are used up.  -> {slot: (out [S, N], Q rows, trk rows)}, launches per call"""
    from ams_hip import stream
    up = up or (lambda a: torch.from_numpy(a).cuda())
    L, H = sep.L, sep.H
    sep.arm()                                                      # (the one launch that resets every slot: not part of a push)
    state = {s: (0, 0) for s in xs}
    outs, Qs, trks, launches = {s: [] for s in xs}, {s: [] for s in xs}, {s: [] for s in xs}, []

    def step(blocks, closing):
        slots = [s for s in sorted(xs) if blocks.get(s) is not None or s in closing]
        stub.next = []
        for s in slots:
            k = 0 if s in closing else blocks[s].shape[0]
            rows, n1, d1 = _ready(state[s][0], state[s][1], k, s in closing, L, H)
            stub.next.append((s, state[s][1], rows))
            state[s] = (n1, d1)
        before = stream.launch_count()
        if closing:
            (s,) = closing
            res = {s: sep.close(s)}
        else:
            got = sep.push([blocks.get(s) for s in range(sep.slots)])
            res = {s: got[s] for s in slots}
            assert all(got[s].shape == (sep.S, 0) for s in range(sep.slots) if s not in slots)
        launches.append(stream.launch_count() - before)
        at = 0
        for s, c0, rows in stub.next:
            outs[s].append(res[s].clone())
            if rows:
                Qs[s].append(sep.last['Q'][at:at + rows].clone())
                trks[s].append(sep.last['trk'][at:at + rows].clone())
            at += rows
            assert sep.received(s) == state[s][0]
            assert sep.emitted(s) == (state[s][0] if s in closing else state[s][1] * H) == sum(o.shape[1] for o in outs[s])

    at = {s: 0 for s in xs}
    done = set()
    r = 0
    while len(done) < len(xs):
        blocks = {}
        for s in xs:
            if s not in done and r < len(sizes[s]):
                k = sizes[s][r]
                blocks[s] = up(xs[s][at[s]:at[s] + k])
                at[s] += k
        if blocks:
            step(blocks, ())
        for s in sorted(xs):
            if s not in done and r + 1 >= len(sizes[s]):
                assert at[s] == xs[s].shape[0]
                step({}, (s,))
                done.add(s)
        r += 1
    S = sep.S
    res = {}
    for s in xs:
        Q = torch.cat(Qs[s]) if Qs[s] else torch.zeros((0, S, S), device='cuda')
        trk = torch.cat(trks[s]) if trks[s] else torch.zeros((0, S), dtype=torch.int32, device='cuda')
        res[s] = (torch.cat(outs[s], dim=1), Q, trk)
    return res, launches


def _material(seed, S, L, H, N, nan_chunk=None):
    src, est, _, truth = ref.material(seed, S, L, H, N, noise=1e-3)
    if nan_chunk is not None:
        est[nan_chunk] = np.nan
    return src.sum(axis=0).astype(np.float32), est, truth


def _check_stream(x, est, got, mixes, S, L, H, truth=None):
    """One stream's pushes against the offline stitcher on the same estimates (bits) and against the restatement."""
    from ams_hip import stitch
    out, Q, trk = got
    N = x.shape[0]
    if N == 0:
        assert out.shape == (S, 0) and not mixes
        return
    C = ref.nb_chunks(N, L, H)
    dev = torch.from_numpy(est).cuda()
    assert torch.equal(torch.cat(mixes), stitch.chunks(torch.from_numpy(x).cuda(), L, H))
    assert np.array_equal(torch.cat(mixes).cpu().numpy(), ref.chunks(x, L, H))
    want, wtrk, wQ = stitch.stitch(dev, N, H)
    assert Q.shape == (C, S, S) and trk.shape == (C, S)
    assert not Q[0].any() and torch.equal(_bits(Q[1:]), _bits(wQ))          # chunk 0 has no border in front of it
    assert torch.equal(trk, wtrk)
    if truth is not None:
        assert np.array_equal(trk.cpu().numpy(), truth)
    assert out.shape == (S, N) and torch.equal(_bits(out), _bits(want))
    calls = []

    def infer(row):
        calls.append(0)
        return est[len(calls) - 1]

    st = sref.Stream(S, L, H, infer)
    mine = np.concatenate([st.push(x), st.close()], axis=1)
    assert np.array_equal(np.stack(st.trks), trk.cpu().numpy())
    assert np.array_equal(mine, out.cpu().numpy(), equal_nan=True)
    if not np.isnan(est).any():
        assert np.array_equal(mine.view(np.int32), out.cpu().numpy().view(np.int32))


def _cut(N, pattern):
    """block sizes from `pattern`, cut to N samples; what is left goes last"""
    sizes, left = [], N
    for k in pattern:
        k = min(k, left)
        sizes.append(k)
        left -= k
    if left:
        sizes.append(left)
    return sizes


def _five_streams(S, L, H, nan=False):
    """The block patterns and stream ends of the feature request, one stream each: 0 samples, 1 sample, exactly H and more than 2 L in one
    push (several chained chunks); N <= L, N = 1, N = 0, and a close exactly at (C - 1) H + L."""
    lengths = [3 * L + H + 2, L - 1, 1, 0, 2 * H + L]
    patterns = [[0, 1, H, 2 * L + 3, 5], [H], [1], [0], [L, H, H]]
    xs, ests, truths, sizes = {}, {}, {}, {}
    for s, (N, pat) in enumerate(zip(lengths, patterns)):
        if N:
            xs[s], ests[s], truths[s] = _material(10 * S + s, S, L, H, N, nan_chunk=1 if nan and s in (0, 4) else None)
        else:
            xs[s], ests[s], truths[s] = np.zeros(0, np.float32), np.zeros((0, S, L), np.float32), None
        sizes[s] = _cut(N, pat)
    return xs, ests, truths, sizes


# S = 4, 5 at the smallest geometry of either arm: stream 0 carries a tail (row stride Vp) over several pushes there too
@pytest.mark.parametrize('L,H,S', [(L, H, S) for L, H in GEOMETRIES for S in (1, 2, 3, 6)] +
                         [(L, H, S) for L, H in [(16, 8), (9, 5)] for S in (4, 5)])
def test_streams_equal_the_offline_stitcher(L, H, S):
    from ams_hip import stream
    xs, ests, truths, sizes = _five_streams(S, L, H)
    stub = Stub(ests)
    sep = stream.StreamSeparator(stub, 5, S, L, H, keep_rows=True)
    assert sep.latency_samples == L
    res, launches = _drive(sep, stub, xs, sizes)
    assert set(launches) == {PER_PUSH, 0}
    for s in xs:
        _check_stream(xs[s], ests[s], res[s], stub.mix[s], S, L, H, truths[s])
    assert all(sep.closed(s) for s in xs) and launches.count(0) == 1        # only the close of the empty stream launches nothing
    with pytest.raises(ValueError, match='closed'):
        sep.push([np.zeros(1, np.float32)] + [None] * 4)
    with pytest.raises(ValueError, match='closed'):
        sep.close(0)
    # every stream alone in a one-slot separator: the same bits
    for s in xs:
        one_stub = Stub({0: ests[s]})
        alone = stream.StreamSeparator(one_stub, 1, S, L, H, keep_rows=True)
        got, _ = _drive(alone, one_stub, {0: xs[s]}, {0: sizes[s]})
        for a, b in zip(got[0], res[s]):
            assert a.shape == b.shape and torch.equal(_bits(a), _bits(b))


@pytest.mark.parametrize('L,H,S', [(16, 8, 2), (9, 5, 3), (8, 7, 6), (2048, 1024, 2), (4104, 2052, 3)])
def test_a_chunk_of_nans(L, H, S):
    """Chunk 1 of two streams is all NaN: both borders around it have NaN costs only and take the identity; the NaNs leave with the
    samples of that chunk and nothing else.  Bits against the offline stitcher; the restatement up to the NaNs' payload."""
    from ams_hip import stream
    xs, ests, truths, sizes = _five_streams(S, L, H, nan=True)
    stub = Stub(ests)
    sep = stream.StreamSeparator(stub, 5, S, L, H, keep_rows=True)
    res, _ = _drive(sep, stub, xs, sizes)
    for s in xs:
        _check_stream(xs[s], ests[s], res[s], stub.mix[s], S, L, H)
    for s in (0, 4):
        out, Q, trk = res[s]
        assert bool(torch.isnan(Q[1:3]).all()) and torch.equal(trk[0], trk[1]) and torch.equal(trk[1], trk[2])
        bad = torch.isnan(out).any(dim=0).cpu().numpy()
        assert bad[H:2 * H].all() and not bad[:H].any() and not bad[H + L:].any()


@pytest.mark.parametrize('L,H,S', [(9, 5, 3), (2048, 1024, 2)])
def test_launches_do_not_depend_on_the_number_of_streams(L, H, S):
    """1, 5 and 40 streams of unequal lengths in random blocks of 0 .. 2 L + 1 samples: every push and every close is six launches."""
    from ams_hip import stream
    rng = np.random.RandomState(L)
    per_n = {}
    for n in (1, 5, 40):
        lengths = [int(v) for v in rng.randint(1, 4 * L, size=n)]
        xs, ests, sizes = {}, {}, {}
        for s, N in enumerate(lengths):
            xs[s], ests[s], _ = _material(1000 * n + s, S, L, H, N)
            sizes[s] = sref.split(rng, N, 2 * L + 1)
        stub = Stub(ests)
        sep = stream.StreamSeparator(stub, n, S, L, H, keep_rows=True)
        res, launches = _drive(sep, stub, xs, sizes)
        per_n[n] = set(launches)
        for s in (0, n // 2, n - 1):
            _check_stream(xs[s], ests[s], res[s], stub.mix[s], S, L, H)
        for s in {0, n - 1}:                                       # ... and the same bits as the stream alone
            one_stub = Stub({0: ests[s]})
            alone = stream.StreamSeparator(one_stub, 1, S, L, H, keep_rows=True)
            got, _ = _drive(alone, one_stub, {0: xs[s]}, {0: sizes[s]})
            assert torch.equal(_bits(got[0][0]), _bits(res[s][0]))
    assert per_n[1] == per_n[5] == per_n[40] == {PER_PUSH}
    assert PER_PUSH == stream.FEED_LAUNCHES + stream.ABSORB_LAUNCHES


@pytest.mark.parametrize('L,H,S', [(16, 8, 2), (2048, 1024, 3)])
def test_reset_leaves_nothing_of_the_stream_before(L, H, S):
    """A slot that closed on a NaN tail, and one that is reset in mid-stream, separate their next stream as a fresh separator does."""
    from ams_hip import stream
    N = 2 * H + L
    xa, ea, _ = _material(1, S, L, H, N, nan_chunk=2)              # the last chunk: the carried tail is NaN
    xb, eb, _ = _material(2, S, L, H, N + 3)
    sizes_a, sizes_b = _cut(N, [L, H, H]), _cut(N + 3, [3, 2 * L])
    stub = Stub({0: ea, 1: ea})
    sep = stream.StreamSeparator(stub, 2, S, L, H, keep_rows=True)
    first, _ = _drive(sep, stub, {0: xa}, {0: sizes_a})
    assert bool(torch.isnan(first[0][0][:, -(L - H):]).all()) and sep.closed(0)
    stub.next = [(1, 0, 1)]
    sep.push([None, xa[:L + 1]])                                   # slot 1: one chunk done, one sample pending, a tail carried
    assert (sep.received(1), sep.emitted(1)) == (L + 1, H)
    sep.reset(0)
    sep.reset(1)
    assert [(sep.received(s), sep.emitted(s), sep.closed(s)) for s in (0, 1)] == [(0, 0, False)] * 2
    stub.ests, stub.mix = {0: eb, 1: eb}, {0: [], 1: []}
    again, _ = _drive(sep, stub, {0: xb, 1: xb}, {0: sizes_b, 1: sizes_b})
    fresh_stub = Stub({0: eb})
    fresh, _ = _drive(stream.StreamSeparator(fresh_stub, 1, S, L, H, keep_rows=True), fresh_stub, {0: xb}, {0: sizes_b})
    for s in (0, 1):
        _check_stream(xb, eb, again[s], stub.mix[s], S, L, H)
        assert not bool(torch.isnan(again[s][0]).any())
        for a, b in zip(again[s], fresh[0]):
            assert torch.equal(_bits(a), _bits(b))


@pytest.mark.parametrize('base', [4, 8, 12])
def test_fenced_buffers_at_odd_bases(base):
    """A dword geometry inside tests/fenced.py: the state, the rows, the workspace and the outputs between red zones, the pushed
    blocks and the estimates `base` bytes past a 256-byte boundary."""
    from ams_hip import functional, stitch, stream
    from tests.fenced import Fence
    L, H, S = 9, 5, 3
    xs, ests, truths, sizes = _five_streams(S, L, H)
    want = {}
    for s in xs:
        if xs[s].shape[0]:
            want[s] = stitch.stitch(torch.from_numpy(ests[s]).cuda(), xs[s].shape[0], H)[0]
    stitch._w_head(L - H, torch.device('cuda', torch.cuda.current_device()))             # the cached tables: made outside the fence
    functional._perm_table32(S, torch.device('cuda', torch.cuda.current_device()))
    with Fence() as fence:
        up = lambda a: fence.dev(a, base=base) if a.size else torch.from_numpy(a).cuda()          # noqa: E731
        stub = Stub(ests, up)
        sep = stream.StreamSeparator(stub, 5, S, L, H, keep_rows=True)
        res, _ = _drive(sep, stub, xs, sizes, up)
        fence.check()
        for s in want:
            assert res[s][0].data_ptr() % 4 == 0 and torch.equal(_bits(res[s][0]), _bits(want[s]))
            assert np.array_equal(res[s][2].cpu().numpy(), truths[s])


def test_the_refused_geometry():
    """(4096, 1536): a hop below half a chunk -- a sample would lie in three chunks -- is refused here as by the offline stitcher."""
    from ams_hip import stitch, stream
    with pytest.raises(ValueError, match='hop'):
        stitch.check_geometry(4096, 1536)
    with pytest.raises(ValueError, match='hop'):
        stream.StreamSeparator(lambda mix: mix, 1, 2, 4096, 1536)
    assert stream.load().ams_stream_state_bytes(1, 2, 4096, 1536) == 0


def test_device_blocks_and_wrong_estimates():
    """Blocks that are device tensors already (no upload of samples), mixed with host blocks; an `infer` that returns the wrong shape."""
    from ams_hip import stream
    L, H, S = 16, 8, 2
    x, est, truth = _material(3, S, L, H, 3 * L)
    stub = Stub({0: est, 1: est})
    sep = stream.StreamSeparator(stub, 2, S, L, H, keep_rows=True)
    stub.next = [(0, 0, 5), (1, 0, 5)]
    a, b = sep.push([torch.from_numpy(x).cuda(), x])
    assert a.shape == (S, 5 * H) and torch.equal(_bits(a), _bits(b))
    bad = stream.StreamSeparator(lambda mix: torch.zeros((mix.shape[0], S + 1, L), device='cuda'), 1, S, L, H)
    with pytest.raises(stream.StreamError, match='infer must return'):
        bad.push([x])
