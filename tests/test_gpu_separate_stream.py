"""GPU: live streams through a model -- Network.open_streams (models/network.py, ams_hip/stream.py) on the tiny
Front_Separator_Inference set-up of tests/test_gpu_separate_recording.py: three streams pushed in uneven blocks, the rows every model
pass saw and returned recorded, and the outputs compared bit for bit with ams_hip.stitch.stitch of the recorded estimates; the
refusals; and the command line (experiments/evaluation/separate_stream.py)."""
import os
import tempfile
import wave

import numpy as np
import pytest

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

from tests.test_gpu_separate_recording import B, L, S, STEPS, TRIES, _front, _recording

H = L // 2
LENGTHS = [4396, 1000, 3300]
BLOCKS = [[700, 2500, 1, 1195], [1000], [1500, 0, 1800]]          # uneven; stream 0's second block completes two chunks at once


def _ready(N, D, k, closing):
    n1, d = N + k, D
    while n1 >= d * H + L:
        d += 1
    if closing and n1 > 0 and (d == 0 or n1 > (d - 1) * H + L):
        d += 1
    return d - D, n1, d


class Recorder(object):
    """Wraps model.infer_chunks (every call: the rows in and out) and model._eval_guarded (the model passes); undone by close()."""

    def __init__(self, model):
        self.model, self.calls, self.passes = model, [], 0
        inner, run = model.infer_chunks, model._eval_guarded

        def infer_chunks(mix, batch_size=None):
            est = inner(mix, batch_size)
            self.calls.append((mix.clone(), est.clone()))
            return est

        def eval_guarded(*a, **kw):
            self.passes += 1
            return run(*a, **kw)

        model.infer_chunks, model._eval_guarded = infer_chunks, eval_guarded

    def close(self):
        del self.model.infer_chunks, self.model._eval_guarded      # the instance attributes: the class's methods show again


def _push_all(sep, xs, blocks, rec=None, batch=B):
    """Round r pushes block r of every stream that has one, then closes the streams whose blocks are used up.
    -> outputs [S, N] per stream, and per stream the list of (call, row) of its chunks in rec.calls"""
    n = len(xs)
    state, at, outs, rows_of = [(0, 0)] * n, [0] * n, [[] for _ in xs], [[] for _ in xs]

    def account(slots, ks, closing):
        before = (len(rec.calls), rec.passes) if rec else None
        ready = []
        for s, k in zip(slots, ks):
            r, n1, d1 = _ready(state[s][0], state[s][1], k, closing)
            state[s] = (n1, d1)
            ready.append(r)
        return before, ready

    def settle(before, slots, ready):
        if rec is None:
            return
        total = sum(ready)
        assert len(rec.calls) - before[0] == (1 if total else 0)
        assert rec.passes - before[1] == -(-total // batch)                    # ceil(ready rows / B) model passes per push
        row = 0
        for s, r in zip(slots, ready):
            rows_of[s] += [(len(rec.calls) - 1, row + i) for i in range(r)]
            row += r

    for r in range(max(len(b) for b in blocks)):
        slots = [s for s in range(n) if r < len(blocks[s])]
        ks = [blocks[s][r] for s in slots]
        before, ready = account(slots, ks, False)
        got = sep.push([xs[s][at[s]:at[s] + blocks[s][r]] if s in slots else None for s in range(n)])
        settle(before, slots, ready)
        for s in slots:
            at[s] += blocks[s][r]
            outs[s].append(got[s].clone())
            assert got[s].shape == (S, ready[slots.index(s)] * H)
        for s in slots:
            if r + 1 == len(blocks[s]):
                before, ready = account([s], [0], True)
                outs[s].append(sep.close(s).clone())
                settle(before, [s], ready)
                assert (sep.received(s), sep.emitted(s)) == (xs[s].shape[0], xs[s].shape[0])
    return [torch.cat(o, dim=1) for o in outs], rows_of


@pytest.mark.parametrize('beta', [None, 5.0])
def test_streams_are_chunks_infer_stitch(beta):
    from ams_hip import stitch
    tr, _, _ = _front(beta)
    model = tr.model
    xs = [_recording(N, 20 + i) for i, N in enumerate(LENGTHS)]
    assert [sum(b) for b in BLOCKS] == LENGTHS
    rec = Recorder(model)
    try:
        with tr.graph.as_default():
            sep = model.open_streams(3)
            assert (sep.slots, sep.S, sep.L, sep.H, sep.latency_samples) == (3, S, L, H, L)
            outs, rows_of = _push_all(sep, xs, BLOCKS, rec)
    finally:
        rec.close()
    assert 'infer_chunks' not in vars(model) and '_eval_guarded' not in vars(model)
    for s, (x, N) in enumerate(zip(xs, LENGTHS)):
        mix = torch.stack([rec.calls[c][0][i] for c, i in rows_of[s]])
        est = torch.stack([rec.calls[c][1][i] for c, i in rows_of[s]])
        assert torch.equal(mix, stitch.chunks(torch.from_numpy(x).cuda(), L, H))
        want = stitch.stitch(est, N, H)[0]
        assert outs[s].shape == (S, N) and bool(torch.isfinite(outs[s]).all())
        assert torch.equal(outs[s].contiguous().view(torch.int32), want.view(torch.int32))


def test_another_hop():
    """Another hop, a block on the device, three chunks ready at once: two passes of B = 2 rows, the second filled up."""
    from ams_hip import stitch
    tr, _, _ = _front(None)
    model = tr.model
    hop = 1280
    x = _recording(5000, 31)
    rec = Recorder(model)
    try:
        with tr.graph.as_default():
            sep = model.open_streams(1, hop=hop)
            a = sep.push([torch.from_numpy(x[:4700]).cuda()])[0].clone()       # chunks 0, 1, 2 at once
            assert rec.passes == 2 and len(rec.calls) == 1 and a.shape == (S, 3 * hop)
            b = sep.push([x[4700:]])[0].clone()
            c = sep.close(0).clone()
    finally:
        rec.close()
    assert b.shape == (S, 0) and rec.passes == 3 and len(rec.calls) == 2
    est = torch.cat([e for _, e in rec.calls])
    assert est.shape[0] == stitch.nb_chunks(5000, L, hop) == 4
    want = stitch.stitch(est, 5000, hop)[0]
    assert torch.equal(torch.cat([a, b, c], dim=1).contiguous().view(torch.int32), want.view(torch.int32))


def test_refusals():
    from ams_hip import testing
    from utils.trainer import Pretrained_Inference
    from tests.test_gpu_recipes import base_args
    from tests.test_gpu_separate_recording import HOP, NF, W
    tmp = tempfile.mkdtemp(prefix='ams_pstr_')
    folder, params = testing.make_pretrained_adapt(os.path.join(tmp, 'pre'), window_size=W, filters=NF, hop_size=HOP, chunk_size=L,
                                                   batch_size=B, nb_speakers=S)
    a = base_args(**params)
    a.update(model_folder=folder, out=False)
    a.pop('type')
    pre = Pretrained_Inference(None, 'pretrained_inference', **a)
    model = pre.prepare_inference()
    with pre.graph.as_default():
        with pytest.raises(ValueError, match='clean sources'):
            model.open_streams(2)
    tr, _, _ = _front(None)
    model = tr.model
    rec = Recorder(model)
    try:
        with tr.graph.as_default():
            for n in (0, -1):
                with pytest.raises(ValueError, match='at least one stream'):
                    model.open_streams(n)
            for hop in (L // 2 - 1, L):
                with pytest.raises(ValueError, match='hop'):
                    model.open_streams(2, hop=hop)
            sep = model.open_streams(2)
            x = _recording(100)
            for blocks in ([x], [x, x, x], x, [x.astype(np.float64), None], [torch.zeros(4, dtype=torch.int16), None],
                           [x.reshape(1, -1), None], [None, torch.zeros(2, 3, device='cuda')]):
                with pytest.raises(ValueError):
                    sep.push(blocks)
            assert sep._state is None and sep.received(0) == 0                 # nothing was uploaded
            sep.push([x, None])
            assert sep.close(0).shape == (S, 100) and sep.close(1).shape == (S, 0)
            for blocks in ([x, None], [None, x]):
                with pytest.raises(ValueError, match='closed'):
                    sep.push(blocks)
            sep.reset(1)
            assert sep.push([None, x])[1].shape == (S, 0) and sep.received(1) == 100
    finally:
        rec.close()
    assert rec.passes == 1                                          # the one closing chunk of slot 0; the empty stream cost nothing
    from experiments.evaluation import separate_stream as cli
    with pytest.raises(SystemExit) as e:
        cli.main(['--model_folder', folder, '--sortofmodel', 'pretraining', '--inputs', 'x.wav', '--output_dir', 'o'])
    assert 'pretraining' in str(e.value)


def test_command_line_equals_the_api_on_the_same_blocks():
    import config
    from experiments.evaluation import separate as one
    from experiments.evaluation import separate_stream as cli
    tr, _, folder = _front(None)
    tmp = tempfile.mkdtemp(prefix='ams_scli_')
    lengths, block = [3300, 2500], 900
    srcs = [os.path.join(tmp, 'a.wav'), os.path.join(tmp, 'b.wav')]
    for p, N, seed in zip(srcs, lengths, (41, 42)):
        one.write_wav(p, _recording(N, seed))
    xs = [one.read_wav(p) for p in srcs]
    # the reading loop of the command line on the shared model ...
    names = [[os.path.join(tmp, 'run%d_%d.wav' % (s, k)) for k in range(S)] for s in range(2)]
    with tr.graph.as_default():
        sep = tr.model.open_streams(2)
        written = cli.run(sep, [cli.WavBlocks(p) for p in srcs], [[cli.WavTrack(p) for p in row] for row in names], block)
        # ... and the API with the same blocks
        blocks = [[min(block, N - at) for at in range(0, N, block)] for N in lengths]
        outs, _ = _push_all(tr.model.open_streams(2), xs, blocks)
    assert written == lengths
    for s in range(2):
        for k in range(S):
            ref_path = os.path.join(tmp, 'api%d_%d.wav' % (s, k))
            one.write_wav(ref_path, outs[s][k].cpu().numpy())
            assert open(names[s][k], 'rb').read() == open(ref_path, 'rb').read()
    # the command line itself: a model of its own from the checkpoint, a .wav per stream and track, each of its input's length
    out_dir = os.path.join(tmp, 'out')
    paths = cli.main(['--model_folder', folder, '--sortofmodel', 'front_DPCL', '--inputs'] + srcs + [
        '--output_dir', out_dir, '--block', str(block), '--chunk_size', str(L), '--batch_size', str(B), '--nb_speakers', str(S),
        '--nb_tries', str(TRIES), '--nb_steps', str(STEPS), '--no_summaries'])
    assert paths == [os.path.join(out_dir, '%s_%d.wav' % (st, k)) for st in ('a', 'b') for k in range(S)]
    for p, N in zip(paths, [lengths[0]] * S + [lengths[1]] * S):
        with wave.open(p, 'rb') as w:
            assert (w.getnchannels(), w.getsampwidth(), w.getframerate(), w.getnframes()) == (1, 2, config.fs, N)
        assert np.abs(one.read_wav(p)).max() > 0
