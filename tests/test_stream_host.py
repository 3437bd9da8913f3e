"""CPU: the boundary of the stream separator -- include/ams_stream.h against the exports of libams_stream.so, every invalid-argument
status with pointers that are never dereferenced, ams_hip.stream.plan against the definition, tests/stream_ref.py against
tests/stitch_ref.py on whole streams (the sweep of DESIGN.md 4.15), the refusals of StreamSeparator, Network.open_streams and
experiments/evaluation/separate_stream.py, its block readers and incremental .wav writer, and the kernels' resource usage."""
import ctypes
import io
import os
import re
import subprocess
import sys
import wave

import numpy as np
import pytest

from tests import stitch_ref as ref
from tests import stream_ref as sref

torch = pytest.importorskip('torch')

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, 'adaptive-multispeaker-separation_amd')
NAMES = {'ams_stream_abi_version', 'ams_stream_launch_count', 'ams_stream_state_bytes', 'ams_stream_reset', 'ams_stream_feed',
         'ams_stream_workspace_bytes', 'ams_stream_absorb'}
AMS_OK, AMS_E_INVALID_ARG = 0, -1                               # include/ams.h


def _built(path):
    if not os.path.exists(path):
        import __graft_entry__
        __graft_entry__.build()
    return path


def _lib():
    from ams_hip import stream
    _built(stream.LIB_PATH)
    return stream.load()


def test_header_and_exports():
    src = open(os.path.join(ROOT, 'include', 'ams_stream.h')).read()
    src = re.sub(r'/\*.*?\*/', ' ', src, flags=re.S)
    assert set(re.findall(r'\b(ams_\w+)\s*\(', src)) == NAMES
    from ams_hip import _lib as base, stitch, stitch_batch, stream
    assert set(base.parse_header(stream.HEADER_PATH)) == NAMES
    path = _built(stream.LIB_PATH)
    out = subprocess.run(['nm', '-D', '--defined-only', path], capture_output=True, text=True, check=True).stdout
    exported = set(ln.split()[-1] for ln in out.splitlines() if ln.split() and ln.split()[-1].startswith('ams_'))
    assert exported == NAMES
    lib = _lib()
    assert lib.ams_stream_abi_version() == 1 == stream.ABI_VERSION
    assert (stream.ENTRY, stream.FIRST, stream.CLOSING) == tuple(
        int(re.search(r'#define %s (\d+)' % n, src).group(1)) for n in ('AMS_STREAM_ENTRY', 'AMS_STREAM_FIRST', 'AMS_STREAM_CLOSING'))
    # the state: per slot ceil4(L) + S ceil4(V) floats and 8 words; the workspace: slab sums and tracks
    assert lib.ams_stream_state_bytes(3, 2, 20480, 10240) == 3 * (20480 + 2 * 10240 + 8) * 4
    assert lib.ams_stream_state_bytes(1, 3, 9, 5) == (12 + 3 * 4 + 8) * 4
    assert lib.ams_stream_state_bytes(0, 2, 256, 128) == 0 and lib.ams_stream_state_bytes(65536, 2, 256, 128) == 0
    assert lib.ams_stream_state_bytes(1, 7, 256, 128) == 0 and lib.ams_stream_state_bytes(1, 2, 256, 127) == 0
    assert lib.ams_stream_workspace_bytes(5, 7, 2, 4104, 2052) == (7 * 3 * 4 + 12 * 2) * 4
    assert lib.ams_stream_workspace_bytes(1, 0, 6, 16, 8) == 6 * 4
    assert lib.ams_stream_workspace_bytes(0, 1, 2, 16, 8) == 0 and lib.ams_stream_workspace_bytes(1, -1, 2, 16, 8) == 0
    for other in (stitch.LIB_PATH, stitch_batch.LIB_PATH, base.LIB_PATH):             # the other libraries gained nothing
        syms = subprocess.run(['nm', '-D', '--defined-only', _built(other)], capture_output=True, text=True, check=True).stdout
        assert 'ams_stream_' not in syms, other
    for other in (stitch.HEADER_PATH, stitch_batch.HEADER_PATH, base.HEADER_PATH):
        assert 'ams_stream' not in open(other).read()


def test_every_invalid_argument_is_refused_before_a_launch():
    """Host addresses stand in for the device pointers: a call that got past its checks would launch on them; none does, and the
    launch counter stays where it was."""
    lib = _lib()
    before = lib.ams_stream_launch_count()
    buf = (ctypes.c_char * 4096)()
    a = (ctypes.addressof(buf) + 15) & ~15                         # 16-byte aligned
    good_reset = dict(state=a, slots=4, S=2, L=16, H=8, first=0, count=4)
    good_feed = dict(state=a, slots=4, S=2, L=16, H=8, table=a, n=2, rows=3, max_rows=2, x=a, x_total=10, mix=a)
    good_absorb = dict(state=a, slots=4, S=2, L=16, H=8, table=a, n=2, rows=3, max_rows=2, max_m=16, est=a, perms=a, P=2, w_head=a, out=a,
                       out_stride=40, ws=a, ws_bytes=1 << 20, Q_rows=None, trk_rows=None)
    shape = [dict(slots=0), dict(slots=65536), dict(S=0), dict(S=7), dict(L=1), dict(L=(1 << 30) + 1, H=1 << 29), dict(H=7), dict(H=16),
             dict(state=None), dict(state=a + 4)]
    push = [dict(table=None), dict(n=0), dict(n=5), dict(rows=-1), dict(max_rows=-1), dict(max_rows=4), dict(rows=70000, max_rows=65536)]
    cases = [(lib.ams_stream_reset, good_reset, shape + [dict(first=-1), dict(count=0), dict(first=2, count=3)]),
             (lib.ams_stream_feed, good_feed, shape + push + [dict(x=None), dict(mix=None), dict(x_total=-1), dict(x_total=1 << 31)]),
             (lib.ams_stream_absorb, good_absorb, shape + push + [
                 dict(est=None), dict(perms=None), dict(w_head=None), dict(out=None), dict(ws=None), dict(P=1), dict(P=6), dict(max_m=-1),
                 dict(out_stride=0), dict(max_m=41), dict(out_stride=1 << 30), dict(ws_bytes=(3 * 4 + 5 * 2) * 4 - 1)])]
    count = 0
    for fn, good, bads in cases:
        for bad in bads:
            kw = dict(good, **bad)
            rc = fn(*(list(kw.values()) + [None]))
            assert rc == AMS_E_INVALID_ARG, (fn.__name__, bad, rc)
            count += 1
    assert count == 13 + 21 + 29
    assert lib.ams_stream_launch_count() == before


def _by_definition(N, D, k, closing, L, H):
    """rows, m, D after: the definition of DESIGN.md 4.15, stepped chunk by chunk"""
    n1, d, rows = N + k, D, 0
    while n1 >= d * H + L:
        d, rows = d + 1, rows + 1
    m = rows * H
    if closing:
        if n1 > 0 and (d == 0 or n1 > (d - 1) * H + L):
            d, rows = d + 1, rows + 1
        m = n1 - D * H
    return rows, m, d


@pytest.mark.parametrize('L,H', [(8, 4), (9, 5), (8, 7), (16, 11), (2, 1), (20480, 10240)])
def test_plan_arithmetic(L, H):
    from ams_hip import stream
    rng = np.random.RandomState(L + H)
    N, D = [0] * 7, [0] * 7
    slots = [4, 0, 6, 2, 1, 5, 3]
    # stream 1 ends exactly at (C - 1) H + L, stream 2 gets nothing at all, stream 3 one sample
    ends = {1: 2 * H + L, 2: 0, 3: 1}
    for step in range(12):
        k = [int(rng.randint(0, 2 * L + 2)) for _ in slots]
        closing = [step == 11] * 7
        for i, s in enumerate(slots):
            if s in ends:                                          # all of it by step 10, nothing with the close
                k[i] = ends[s] - N[i] if step == 10 else 0 if step == 11 else min(k[i], ends[s] - N[i])
        p = stream.plan(slots, N, D, k, closing, L, H)
        assert p.table.dtype == np.int32 and p.table.shape == (7, stream.ENTRY) and not p.table[:, 9:].any()
        x_off = row0 = out_off = 0
        for i, s in enumerate(slots):
            rows, m, d1 = _by_definition(N[i], D[i], k[i], closing[i], L, H)
            flags = (stream.FIRST if D[i] == 0 else 0) | (stream.CLOSING if closing[i] else 0)
            assert p.table[i, :9].tolist() == [s, x_off, k[i], N[i] - D[i] * H, rows, row0, out_off, m, flags], (step, i)
            assert (p.N[i], p.D[i]) == (N[i] + k[i], d1)
            if not closing[i]:
                assert m == rows * H and 0 <= p.N[i] - p.D[i] * H < L            # exactly D H emitted; fewer than L pending
            else:
                assert D[i] * H + m == N[i] + k[i]                             # the total emitted is exactly N
                if s == 1:
                    assert (rows, m) == (0, L - H) and N[i] == ends[1]         # N at (C - 1) H + L: no padded chunk, the carried tail
                if s == 2:
                    assert (rows, m) == (0, 0)                                 # N = 0: no row, no model pass
                if s == 3:
                    assert (rows, m) == (1, 1)
            x_off, row0, out_off = x_off + k[i], row0 + rows, out_off + m
        assert (p.rows, p.x_total, p.out_total) == (row0, x_off, out_off)
        assert p.max_rows == p.table[:, 4].max() and p.max_m == p.table[:, 7].max()
        N, D = p.N.tolist(), p.D.tolist()


def test_plan_refusals():
    from ams_hip import stream
    with pytest.raises(ValueError, match='hop'):
        stream.plan([0], [0], [0], [1], [False], 16, 7)
    with pytest.raises(ValueError, match='once'):
        stream.plan([1, 1], [0, 0], [0, 0], [1, 1], [False, False], 16, 8)
    with pytest.raises(ValueError):
        stream.plan([0], [0], [0], [-1], [False], 16, 8)
    with pytest.raises(ValueError):
        stream.plan([0], [16], [0], [1], [False], 16, 8)           # 16 samples pending: chunk 0 would have been cut
    with pytest.raises(ValueError, match='2\\^31'):
        stream.plan([0, 1], [0, 0], [0, 0], [1 << 30, 1 << 30], [False, False], 20480, 10240)
    p = stream.plan([0], [0], [0], [(1 << 31) - 1], [False], 1 << 30, 1 << 29)       # just below: one chunk of 2^30 leaves 2^29 samples
    assert (p.rows, p.out_total) == (2, 1 << 30)


@pytest.mark.parametrize('S', [1, 2, 3])
@pytest.mark.parametrize('L,H', [(8, 4), (9, 5), (8, 7), (16, 11), (2, 1)])
def test_restatement_equals_the_offline_stitcher(S, L, H):
    """Every N = 1 .. 3 L + 2, three random splits each into blocks of 0 .. 2 L + 1 samples: the chunks are stitch_ref.chunks' and the
    concatenated output is bit-equal to search / tracks / overlap_add on the same estimates."""
    rng = np.random.RandomState(100 * S + L + H)
    cases = 0
    for N in range(1, 3 * L + 3):
        src, est, _, truth = ref.material(N, S, L, H, N)
        x = src.sum(axis=0).astype(np.float32)
        C = ref.nb_chunks(N, L, H)
        if C > 1:
            trk = ref.tracks(ref.search(ref.border_stats(est, H))[0])
        else:
            trk = np.arange(S, dtype=np.int32)[None]
        want = ref.overlap_add(est, trk, N, H)
        for _ in range(3):
            calls = []

            def infer(row):
                calls.append(row)
                return est[len(calls) - 1]

            st = sref.Stream(S, L, H, infer)
            outs = []
            for k in sref.split(rng, N, 2 * L + 1):
                at = st.N
                outs.append(st.push(x[at:at + k]))
                assert sum(o.shape[1] for o in outs) == st.D * H and st.N - st.D * H < L
            outs.append(st.close())
            got = np.concatenate(outs, axis=1)
            assert len(calls) == C and np.array_equal(np.stack(st.rows), ref.chunks(x, L, H))
            assert np.array_equal(np.stack(st.trks), trk)
            assert got.shape == (S, N) and np.array_equal(got.view(np.int32), want.view(np.int32)), (N,)
            cases += 1
    assert cases == 3 * (3 * L + 2)
    empty = sref.Stream(S, L, H, None)
    empty.push(np.zeros(0, np.float32))
    assert empty.close().shape == (S, 0)                           # N = 0: [S, 0], no model pass


def test_separator_refusals_need_no_device():
    from ams_hip import stream

    def infer(mix):
        raise AssertionError('nothing may reach the model')

    for bad in (dict(slots=0), dict(S=0), dict(S=7), dict(H=127), dict(H=256), dict(infer=None)):
        kw = dict(dict(infer=infer, slots=2, S=2, L=256, H=128), **bad)
        with pytest.raises(ValueError):
            stream.StreamSeparator(**kw)
    sep = stream.StreamSeparator(infer, 2, 2, 256)
    assert (sep.H, sep.latency_samples, sep.received(1), sep.emitted(1), sep.closed(1)) == (128, 256, 0, 0, False)
    x = np.zeros(10, np.float32)
    for blocks in ([x], [x, x, x], x, None, 'ab',                                          # the list
                   [x, x.astype(np.float64)], [x.astype(np.int16), None], [torch.zeros(4, dtype=torch.float16), x],      # dtype
                   [x.reshape(2, 5), None], [None, torch.zeros(2, 2)], [x, [0.0, 1.0]]):   # rank, kind
        with pytest.raises(ValueError):
            sep.push(blocks)
    for s in (-1, 2):
        with pytest.raises(ValueError):
            sep.close(s)
    assert sep._state is None                                      # nothing was allocated or uploaded
    assert issubclass(stream.StreamError, RuntimeError)


def test_open_streams_refusals_on_a_model_stub():
    from models.network import Network

    class Stub(object):
        S = 2
        pretraining = False
        output = object()
        args = {'chunk_size': 256, 'batch_size': 2}
        _refuse_unless_separating = Network._refuse_unless_separating
        open_streams = Network.open_streams

        def infer_chunks(self, mix, batch_size=None):
            raise AssertionError('nothing may reach the model')

    for n in (0, -3):
        with pytest.raises(ValueError, match='at least one stream'):
            Stub().open_streams(n)
    for hop in (127, 256):
        with pytest.raises(ValueError, match='hop'):
            Stub().open_streams(2, hop=hop)
    with pytest.raises(ValueError, match='batch size'):
        Stub().open_streams(2, batch_size=0)
    pre = Stub()
    pre.pretraining = True
    with pytest.raises(ValueError, match='clean sources'):
        pre.open_streams(2)
    bare = Stub()
    bare.output = None
    with pytest.raises(ValueError, match='no `output`'):
        bare.open_streams(2)
    assert 'seeds depend on the pass and the row' in Network.open_streams.__doc__


def _write_wav(path, pcm, fs, channels=1):
    with wave.open(path, 'wb') as w:
        w.setnchannels(channels)
        w.setsampwidth(2)
        w.setframerate(fs)
        w.writeframes(np.asarray(pcm, '<i2').tobytes())


def test_cli_refusals(tmp_path):
    import config
    from experiments.evaluation import separate_stream as cli
    pcm = np.random.RandomState(5).randint(-32768, 32768, size=1234).astype(np.int16)
    good, other, slow, stereo = (str(tmp_path / n) for n in ('good.wav', 'other.wav', 'slow.wav', 'stereo.wav'))
    _write_wav(good, pcm, config.fs)
    _write_wav(other, pcm[:1000], config.fs)
    _write_wav(slow, pcm, 2 * config.fs)
    _write_wav(stereo, pcm, config.fs, channels=2)
    base = ['--model_folder', 'm', '--sortofmodel', 'front_DPCL']
    files = ['--inputs', good, other, '--output_dir', str(tmp_path / 'o')]
    a = cli.build_parser().get_args(base + files + ['--block', '777', '--hop', '12000'])
    assert (a.inputs, a.input, a.format, a.block, a.hop, a.clustering, a.resample, a.speakers) == \
        ([good, other], None, None, 777, 12000, 'chunk', False, None)
    assert cli.check_args(a) == ('files', [good, other])
    a = cli.build_parser().get_args(base + ['--input', '-', '--format', 's16le', '--output_prefix', 'p'])
    assert cli.check_args(a) == ('stdin', None)

    def refused(extra, *words, sort='front_DPCL'):
        with pytest.raises(SystemExit) as e:                       # each before a model is built: 'm' is no model folder
            cli.main(['--model_folder', 'm', '--sortofmodel', sort] + extra)
        for w in words:
            assert w in str(e.value), (w, str(e.value))

    refused(files + ['--resample'], '--resample', 'not built')
    for mode in ('recording', 'recording_soft'):
        refused(files + ['--clustering', mode], '--clustering', 'not built')
    refused(files + ['--speakers', 'auto'], '--speakers', 'not built')
    refused(files, 'pretraining', 'clean sources', sort='pretraining')
    refused([], '--inputs')                                        # neither
    refused(files + ['--input', '-'], '--inputs')                  # both
    refused(['--inputs', good, '--output_prefix', 'p'], '--output_dir')
    refused(['--inputs', good, slow, '--output_dir', 'o'], 'sample rate', 'nothing here resamples')      # read_wav's words
    refused(['--inputs', stereo, '--output_dir', 'o'], '2 channels', 'one channel only')
    refused(['--inputs', good, str(tmp_path / 'x.npy'), '--output_dir', 'o'], '.npy')
    os.makedirs(str(tmp_path / 'sub'))
    twin = str(tmp_path / 'sub' / 'good.wav')
    _write_wav(twin, pcm, config.fs)
    refused(['--inputs', good, twin, '--output_dir', 'o'], 'file name of its own')
    refused(files + ['--block', '0'], '--block')
    refused(['--input', 'a.raw', '--format', 's16le', '--output_prefix', 'p'], "'-'")
    refused(['--input', '-', '--output_prefix', 'p'], '--format')
    refused(['--input', '-', '--format', 'f32le'], '--output_prefix')
    refused(files + ['--hop', '3'], '--hop')
    assert not os.path.exists(str(tmp_path / 'o'))


def test_cli_block_readers_and_incremental_writer_round_trip(tmp_path):
    import config
    from experiments.evaluation import separate as one
    from experiments.evaluation import separate_stream as cli
    rng = np.random.RandomState(8)
    pcm = rng.randint(-32767, 32768, size=5000).astype(np.int16)   # (-32768 is not written back: write_wav clips symmetrically)
    src = str(tmp_path / 'src.wav')
    _write_wav(src, pcm, config.fs)
    whole = one.read_wav(src)
    r = cli.WavBlocks(src)
    parts = [r.read(n) for n in (1, 0, 999, 4000, 10, 10)]
    r.close()
    assert [p.shape[0] for p in parts] == [1, 0, 999, 4000, 0, 0] and all(p.dtype == np.float32 for p in parts)
    assert np.array_equal(np.concatenate(parts), whole)
    # raw input: both formats, a reader that hands out fewer bytes than asked for, an input that ends inside a sample
    class Dribble(io.BytesIO):
        def read(self, n=-1):
            return io.BytesIO.read(self, min(n, 7))
    for fmt, raw, want in (('s16le', pcm.astype('<i2').tobytes(), whole), ('f32le', whole.astype('<f4').tobytes(), whole)):
        r = cli.RawBlocks(Dribble(raw), fmt)
        parts = [r.read(n) for n in (3, 1000, 5000, 5)]
        assert [p.shape[0] for p in parts] == [3, 1000, 3997, 0] and np.array_equal(np.concatenate(parts), want)
    with pytest.raises(SystemExit, match='inside a sample'):
        cli.RawBlocks(io.BytesIO(b'\x00' * 7), 'f32le').read(10)
    # the writer: pieces of any size give the file write_wav gives for the whole, header included
    x = (1.2 * rng.randn(5000)).astype(np.float32)                 # some samples clip
    x[:4] = [1.0, -1.0, 0.99998474, 0.5 / 32768]
    a, b = str(tmp_path / 'a.wav'), str(tmp_path / 'b.wav')
    one.write_wav(a, x)
    t = cli.WavTrack(b)
    at = 0
    for n in (0, 1, 1023, 3000, 976):
        t.write(x[at:at + n])
        at += n
    t.close()
    assert at == 5000 and t.frames == 5000 and open(a, 'rb').read() == open(b, 'rb').read()
    with wave.open(b, 'rb') as w:
        assert (w.getnchannels(), w.getsampwidth(), w.getframerate(), w.getnframes()) == (1, 2, config.fs, 5000)
    t = cli.WavTrack(str(tmp_path / 'c.wav'))
    with pytest.raises(SystemExit, match='not finite'):
        t.write(np.array([0.0, np.nan], np.float32))
    t.close()

    # run(): blocks in, pieces out, every stream closed once -- with a separator that delays by one block
    class Echo(object):
        S = 2

        def __init__(self, n):
            self.held, self.pushes, self.closes = [np.zeros(0, np.float32)] * n, [], []

        def push(self, blocks):
            self.pushes.append([None if b is None else b.shape[0] for b in blocks])
            outs = []
            for s, b in enumerate(blocks):
                old, self.held[s] = (self.held[s], b) if b is not None else (np.zeros(0, np.float32), self.held[s])
                outs.append(torch.from_numpy(np.stack([old, -old])))
            return outs

        def close(self, s):
            self.closes.append(s)
            return torch.from_numpy(np.stack([self.held[s], -self.held[s]]))

    short = str(tmp_path / 'short.wav')
    _write_wav(short, pcm[:700], config.fs)
    sep = Echo(2)
    names = [[str(tmp_path / ('t%d_%d.wav' % (s, k))) for k in range(2)] for s in range(2)]
    written = cli.run(sep, [cli.WavBlocks(src), cli.WavBlocks(short)], [[cli.WavTrack(p) for p in row] for row in names], 300)
    assert written == [5000, 700] and sep.closes == [1, 0]
    assert sep.pushes[:3] == [[300, 300], [300, 300], [300, 100]] and sep.pushes[3] == [300, None] and sep.pushes[-1] == [200, None]
    for s, n in ((0, 5000), (1, 700)):
        assert np.array_equal(one.read_wav(names[s][0]), whole[:n])
        assert np.array_equal(one.read_wav(names[s][1]), -whole[:n])


def test_stream_kernels_compile_for_gfx950_without_scratch():
    """tools/kernel_resources.py on csrc/stream/stream.hip with the library's flags: twelve border kernels and six others, no
    scratch, no spill, no warning; only the border sums and the tracker use LDS."""
    run = subprocess.run([sys.executable, os.path.join(ROOT, 'tools', 'kernel_resources.py'),
                          os.path.join(PKG, 'csrc', 'stream', 'stream.hip'), '-ffp-contract=off'],
                         capture_output=True, text=True, check=True)
    assert 'warning' not in run.stderr
    out = run.stdout.splitlines()[1:]
    names = ' '.join(out)
    for S in range(1, 7):
        for vec in ('true', 'false'):
            assert 'stats_kernel<%d, %s>' % (S, vec) in names, (S, vec)
    others = ('reset_kernel', 'cut_kernel', 'keep_kernel', 'track_kernel', 'ola_kernel', 'tail_kernel')
    for k in others:
        assert k in names, k
    rows = [ln.split() for ln in out if ln.strip()]
    assert len(rows) == 12 + len(others)
    for r in rows:
        vgpr, agpr, spill, scratch, occ, lds = r[-6:]
        assert spill == '0' and scratch == '0', r
        if not ('stats_kernel' in ' '.join(r) or 'track_kernel' in ' '.join(r)):
            assert lds == '0', r
