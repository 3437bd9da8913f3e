"""GPU: recordings of different sample rates through one chunk stream -- Network.separate_recordings(xs, fs=[...], output_fs=...)
(models/network.py, ams_hip/resample_ragged.py) on the tiny Front_Separator_Inference of
tests/test_gpu_separate_recording.py (B = 2, L = 2048), against the composition written out with the single-recording calls of
ams_hip.resample, and the command line's --one_stream.  Every comparison is exact."""
import os
import tempfile
import wave

import numpy as np
import pytest

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

from tests.test_gpu_separate_clustered import _seeds
from tests.test_gpu_separate_recording import B, L, S, STEPS, TRIES, _front
from tests.test_gpu_separate_recordings import _counting

LENGTHS, CH, FS = (7001, 9000, 2100), (2, 1, 3), [16000, 44100, 8000]
H = L // 2
_CACHE = {}


def _frames():
    rng = np.random.RandomState(71)
    return [rng.randint(-9000, 9000, size=(N, c)).astype(np.int16) for N, c in zip(LENGTHS, CH)]


def _n_out(N, fs_in, fs_out):
    return -((-N * fs_out) // fs_in)


def _composition(model, frames, fs, pcm=True):
    """The definition, with the single-recording calls: from_pcm16 (resample) per recording -> chunks_many -> infer_chunks -> stitch_many.
    -> (the tracks at the model's rate per recording, the layout).  Computed once per input set and left unchanged."""
    import config
    from ams_hip import resample as Rs
    from ams_hip import stitch_batch as sb
    key = (pcm, tuple(fs))
    if key not in _CACHE:
        dev = [torch.from_numpy(f).cuda() for f in frames]
        ys = [Rs.from_pcm16(d, f, config.fs) if pcm else Rs.resample(d, f, config.fs) for d, f in zip(dev, fs)]
        mix, lay = sb.chunks_many([y.contiguous() for y in ys], L, H, S)
        _CACHE[key] = ([p[0] for p in sb.stitch_many(model.infer_chunks(mix), lay)], lay)
    return _CACHE[key]


def _back(part, N, fs_in, fs_out):
    """The way back of one recording with the single call: resample, then the cut to ceil(N fs_out / fs_in)."""
    import config
    from ams_hip import resample as Rs
    if fs_out == config.fs:
        return part
    return Rs.resample(part.contiguous(), config.fs, fs_out)[:, :_n_out(N, fs_in, fs_out)]


class _NoSingleCalls(object):
    """While active, ams_hip.resample.resample and from_pcm16 raise: the call under test may not go through them."""

    def __enter__(self):
        from ams_hip import resample as Rs
        self.Rs, self.saved = Rs, (Rs.resample, Rs.from_pcm16)

        def refuse(*a, **k):
            raise AssertionError('separate_recordings went through a single-recording resampler call')
        Rs.resample = Rs.from_pcm16 = refuse
        return self

    def __exit__(self, *exc):
        self.Rs.resample, self.Rs.from_pcm16 = self.saved
        return False


def test_int16_frames_of_mixed_rates_share_one_stream():
    from ams_hip import resample_ragged as rr
    tr, _, _ = _front(None)
    model = tr.model
    frames = _frames()
    with tr.graph.as_default():
        parts, lay = _composition(model, frames, FS)
        Ctot = lay.Ctot
        assert lay.n.tolist() == [3501, 1633, 2100] and lay.C.tolist() == [3, 1, 2]
        calls, undo = _counting(model)
        n0 = rr.LAUNCHES
        try:
            with _NoSingleCalls():
                outs = model.separate_recordings(frames, fs=FS)
        finally:
            undo()
        assert len(calls) == -(-Ctot // B) == 3                    # one chunk stream: ceil(Ctot / B) model passes
        assert rr.LAUNCHES - n0 == 2                               # one launch each way, whatever the number of recordings
        for out, part, N, f in zip(outs, parts, LENGTHS, FS):
            assert out.shape == (S, N) and out.is_cuda and bool(torch.isfinite(out).all()) and float(out.abs().max()) > 0
            assert torch.equal(out, _back(part, N, f, f))
        # device tensors in: read where they lie
        with _NoSingleCalls():
            again = model.separate_recordings([torch.from_numpy(f).cuda() for f in frames], fs=FS)
        for out, a in zip(outs, again):
            assert torch.equal(out, a)


def test_other_forms_of_the_arguments():
    import config
    tr, _, _ = _front(None)
    model = tr.model
    frames = _frames()
    with tr.graph.as_default():
        parts, lay = _composition(model, frames, FS)
        with _NoSingleCalls():
            low = model.separate_recordings(frames, fs=FS, output_fs=config.fs)
            mixed = model.separate_recordings(frames, fs=FS, output_fs=[8000, 16000, 44100])
            one = model.separate_recordings(frames, fs=FS, output_fs=16000)
        for r, (part, N) in enumerate(zip(parts, LENGTHS)):
            assert low[r].shape == (S, int(lay.n[r])) and torch.equal(low[r], part)                     # the 8 kHz tracks
            fo = [8000, 16000, 44100][r]
            assert mixed[r].shape == (S, _n_out(N, FS[r], fo)) and torch.equal(mixed[r], _back(part, N, FS[r], fo))
            assert one[r].shape == (S, _n_out(N, FS[r], 16000)) and torch.equal(one[r], _back(part, N, FS[r], 16000))
        # float32 recordings, one of them at the model's rate
        rng = np.random.RandomState(72)
        floats, fs = [(0.3 * rng.randn(N)).astype(np.float32) for N in (3300, 7001)], [8000, 16000]
        fparts, flay = _composition(model, floats, fs, pcm=False)
        with _NoSingleCalls():
            fouts = model.separate_recordings(floats, fs=fs)
            fdev = model.separate_recordings([torch.from_numpy(x).cuda() for x in floats], fs=fs, output_fs=[16000, 8000])
        for r, (part, N) in enumerate(zip(fparts, (3300, 7001))):
            assert fouts[r].shape == (S, N) and torch.equal(fouts[r], _back(part, N, fs[r], fs[r]))
            fo = [16000, 8000][r]
            assert fdev[r].shape == (S, _n_out(N, fs[r], fo)) and torch.equal(fdev[r], _back(part, N, fs[r], fo))


def test_recording_level_clustering_with_mixed_rates():
    import config
    from ams_hip import resample as Rs
    from ams_hip import stitch_batch as sb
    tr, _, _ = _front(None)
    model = tr.model
    frames = _frames()
    counts = [3, 1, 2]
    seeds = [_seeds(C, 80 + r) for r, C in enumerate(counts)]
    with tr.graph.as_default():
        with _NoSingleCalls():
            outs = model.separate_recordings(frames, fs=FS, clustering='recording', kmeans_init_indices=seeds)
        ys = [Rs.from_pcm16(torch.from_numpy(f).cuda(), fs, config.fs) for f, fs in zip(frames, FS)]
        mix, lay = sb.chunks_many(ys, L, H, S)
        assert lay.C.tolist() == counts
        checked = model._check_clustering('recording', seeds, len(frames))
        est = model._infer_chunks_clustered(mix, lay.C.tolist(), checked, None, None, None)
        trk = torch.arange(S, dtype=torch.int32, device=est.device).repeat(lay.Ctot, 1)
        packed = sb.overlap_add_many(est, trk, lay)
        for r, (out, N) in enumerate(zip(outs, LENGTHS)):
            o, n = int(lay.out_off[r]), int(lay.n[r])
            assert out.shape == (S, N) and torch.equal(out, _back(packed[o:o + S * n].view(S, n), N, FS[r], FS[r]))


def _write(path, pcm, fs):
    with wave.open(path, 'wb') as w:
        w.setnchannels(pcm.shape[1])
        w.setsampwidth(2)
        w.setframerate(fs)
        w.writeframes(np.ascontiguousarray(pcm, '<i2').tobytes())


def test_command_line_one_stream(monkeypatch):
    from ams_hip import stitch_batch as sb
    from experiments.evaluation import separate_many as cli
    from models.network import Network
    _, _, folder = _front(None)
    tmp = tempfile.mkdtemp(prefix='ams_cli_mixed_')
    rng = np.random.RandomState(73)
    files = [('a', 8000, 3300, 1), ('b', 16000, 7001, 2), ('c', 44100, 9000, 1)]
    for stem, fs, N, ch in files:
        _write(os.path.join(tmp, stem + '.wav'), np.clip(np.rint(0.3 * rng.randn(N, ch) * 32768), -32767, 32767).astype('<i2'), fs)
    calls, orig = [], Network._eval_guarded

    def counted(self, *a, **k):
        calls.append(1)
        return orig(self, *a, **k)
    monkeypatch.setattr(Network, '_eval_guarded', counted)
    out_dir = os.path.join(tmp, 'out')
    paths = cli.main(['--model_folder', folder, '--sortofmodel', 'front_DPCL', '--inputs'] + [os.path.join(tmp, f[0] + '.wav') for f in files]
                     + ['--output_dir', out_dir, '--chunk_size', str(L), '--batch_size', str(B), '--nb_speakers', str(S), '--nb_tries',
                        str(TRIES), '--nb_steps', str(STEPS), '--no_summaries', '--resample', '--one_stream'])
    assert paths == [os.path.join(out_dir, '%s_%d.wav' % (f[0], k)) for f in files for k in range(S)]
    for p in paths:
        stem, fs, N, _ = [f for f in files if os.path.basename(p).startswith(f[0] + '_')][0]
        with wave.open(p, 'rb') as w:
            assert (w.getnchannels(), w.getsampwidth(), w.getframerate(), w.getnframes()) == (1, 2, fs, N)
            assert np.abs(np.frombuffer(w.readframes(N), '<i2')).max() > 0
    lay = sb.layout([3300, 3501, 1633], L, H, S)
    assert len(calls) == -(-lay.Ctot // B)                         # ONE stream for the three rates
    with pytest.raises(SystemExit, match='--resample'):
        cli.main(['--model_folder', folder, '--sortofmodel', 'front_DPCL', '--inputs', os.path.join(tmp, 'a.wav'), '--output_dir', out_dir,
                  '--one_stream'])
