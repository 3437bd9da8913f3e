"""GPU: recording-level clustering of a SOFT k-means model -- Network.separate_recording / separate_recordings with
clustering='recording_soft' (models/network.py) on the tiny Front_Separator_Inference of
tests/test_gpu_separate_recording.py built with beta_kmeans = 5 and --with_silence (B = 2, L = 2048, E = 8, S = 2; 2048 points per
chunk, so the four chunks of the longest recording are one summation chunk of 8192 points to the point), and both command lines.
Comparisons are exact where the same kernels see the same points in the same order; against chunk mode, whose summation order differs,
the masks are held within the soft forward's 1e-3."""
import os
import tempfile

import numpy as np
import pytest

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

from tests.test_gpu_separate_clustered import H, TF, _fresh_model, _identity, _seeds
from tests.test_gpu_separate_recording import B, E, L, S, STEPS, TRIES, _front, _recording
from tests.test_gpu_separate_recordings import LENGTHS, _counting

BETA = 5.0


def _pooled_soft_masks(model, mix, counts, seeds, batch_size=None):
    """The definition: embed_chunks, then ONE ragged soft run over every recording's pooled points with its seeds -> masks [Ctot, TF, S]."""
    from ams_hip import kmeans_ragged_soft as krs
    pts, wts = model.embed_chunks(mix, batch_size)
    assert wts is not None and pts.shape == (mix.shape[0], TF, E) and wts.shape == (mix.shape[0], TF)
    cent, masks, best = krs.kmeans_ragged_soft(pts.view(-1, E), [C * TF for C in counts], np.concatenate(seeds), S, TRIES, STEPS, BETA,
                                               w=wts.view(-1), assign_at_end=True, normalize_input=False)
    return masks.view(-1, TF, S), cent, best


@pytest.mark.parametrize('N,C', [(4396, 4), (3300, 3)])          # two full batches; a last batch padded by repetition
def test_recording_soft_is_embed_pool_soft_masks_overlap_add(N, C):
    from ams_hip import stitch
    tr, _, _ = _front(BETA)
    model = tr.model
    x = torch.from_numpy(_recording(N)).cuda()
    seeds = [_seeds(C, N)]
    with tr.graph.as_default():
        calls, undo = _counting(model)
        try:
            out = model.separate_recording(x, clustering='recording_soft', kmeans_init_indices=seeds)
        finally:
            undo()
        assert len(calls) == 2 * -(-C // B)
        got = model.last_clustering
        mix = stitch.chunks(x, L, H)
        assert mix.shape == (C, L)
        masks, cent, best = _pooled_soft_masks(model, mix, [C], seeds)
        want = stitch.overlap_add(model.infer_chunks_masked(mix, masks, B), _identity(C), N, H)
        again = model.separate_recording(x.cpu().numpy(), clustering='recording_soft', kmeans_init_indices=seeds)
        tracked = model.separate_recording(x)
    assert out.shape == (S, N) and bool(torch.isfinite(out).all()) and float(out.abs().max()) > 0
    assert torch.equal(out, want) and torch.equal(out, again)
    assert sorted(got) == ['best', 'centroids', 'first_chunk', 'groups', 'masks'] and 'labels' not in got
    assert got['masks'].shape == (C, TF, S) and got['masks'].dtype == torch.float32 and torch.equal(got['masks'], masks)
    assert torch.equal(got['centroids'], cent) and got['centroids'].shape == (1, S, E) and torch.equal(got['best'], best)
    rows = got['masks'].sum(dim=2)
    print('mask rows sum to 1 within %.2g; soft entries (0.01 .. 0.99): %d of %d'
          % (float((rows - 1).abs().max()), int(((got['masks'] > 0.01) & (got['masks'] < 0.99)).sum()), got['masks'].numel()))
    assert float((rows - 1).abs().max()) <= 1e-6
    assert tracked.shape == out.shape                              # (the default path still runs on the same model)


def test_many_recordings_one_ragged_soft_call_two_sweeps():
    from ams_hip import kmeans_ragged_soft as krs
    tr, _, _ = _front(BETA)
    model = tr.model
    xs = [torch.from_numpy(_recording(N, 20 + r)).cuda() for r, N in enumerate(LENGTHS)]
    counts = [4, 1, 3]
    assert LENGTHS == [4396, 1000, 3300]
    seeds = [_seeds(C, 50 + r) for r, C in enumerate(counts)]
    with tr.graph.as_default():
        calls, undo = _counting(model)
        n0 = krs.LAUNCHES
        try:
            outs = model.separate_recordings(xs, clustering='recording_soft', kmeans_init_indices=seeds)
        finally:
            undo()
        assert len(calls) == 2 * -(-sum(counts) // B) == 8         # two sweeps of the chunk stream, whatever the number of recordings
        assert krs.LAUNCHES - n0 == STEPS + 4                       # ... and ONE soft k-means run for all of them
        got = model.last_clustering
        # a cap of five chunks' embeddings: recordings 0 and 1 together, recording 2 behind them; a cap of four: recording 0 alone
        two = model.separate_recordings(xs, clustering='recording_soft', kmeans_init_indices=seeds, cluster_cap_bytes=5 * TF * E * 4)
        groups2, masks2 = model.last_clustering['groups'], model.last_clustering['masks']
        three = model.separate_recordings([x.cpu().numpy() for x in xs], clustering='recording_soft', kmeans_init_indices=seeds,
                                          cluster_cap_bytes=4 * TF * E * 4)
        groups3, masks3 = model.last_clustering['groups'], model.last_clustering['masks']
        with pytest.raises(ValueError, match='above the cap'):
            model.separate_recordings(xs, clustering='recording_soft', kmeans_init_indices=seeds, cluster_cap_bytes=4 * TF * E * 4 - 1)
        singles = [model.separate_recording(x, clustering='recording_soft', kmeans_init_indices=seeds[r:r + 1]) for r, x in enumerate(xs)]
    assert got['groups'] == [(0, 3)] and groups2 == [(0, 2), (2, 3)] and groups3 == [(0, 1), (1, 3)]
    assert got['masks'].shape == (8, TF, S) and got['centroids'].shape == (3, S, E) and got['best'].shape == (3,)
    assert torch.equal(got['masks'], masks2) and torch.equal(got['masks'], masks3)
    for r, (out, N) in enumerate(zip(outs, LENGTHS)):
        assert out.shape == (S, N) and bool(torch.isfinite(out).all())
        assert torch.equal(out, two[r]) and torch.equal(out, three[r])
        assert torch.equal(out, singles[r]), r                      # per recording, the single call with the same seeds


def test_one_chunk_against_chunk_mode_with_the_same_seeds():
    """N <= L: both modes cluster the same TF points with the same seeds (chunk mode takes rows 0 .. TRIES - 1 of the model's seeds for
    the chunk in batch row 0; its second batch row is a copy of the chunk, so the tiled weights are the chunk's).  The summation orders
    differ (chunk mode: the batch kernel's 512 / rows chunks per row), so the masks are compared within the soft forward's 1e-3."""
    tr, _, _ = _front(BETA)
    model = tr.model
    sep = getattr(model, 'sepNet', None) or model
    idx = np.asarray(sep.kmeans.init_indices)[:TRIES]
    assert idx.shape == (TRIES, S)
    for N in (1500, L):
        x = torch.from_numpy(_recording(N, 8)).cuda()
        pad = torch.zeros(1, L, device='cuda')
        pad[0, :N] = x
        with tr.graph.as_default():
            chunk = model.separate_recording(x)
            rec = model.separate_recording(x, clustering='recording_soft', kmeans_init_indices=[idx])
            mine = model.last_clustering['masks']
            (_, _, ins), = list(model._chunk_batches(pad, None, 'test'))
            theirs = model._eval_guarded({}, lambda run: sep.masks.value(run), inputs=ins)[:1]
        assert mine.shape == theirs.shape == (1, TF, S) and rec.shape == chunk.shape == (S, N)
        err = float((mine - theirs).abs().max())
        print('N = %d: masks against chunk mode: max difference %.2g' % (N, err))
        assert err <= 1e-3


def test_refusals_on_real_models():
    tr, _, _ = _front(BETA)
    x = _recording(3000)
    with tr.graph.as_default():
        for call in (lambda **k: tr.model.separate_recording(x, **k), lambda **k: tr.model.separate_recordings([x], **k)):
            with pytest.raises(ValueError, match='hard assignment only'):
                call(clustering='recording')
            with pytest.raises(ValueError, match="needs clustering='recording'"):
                call(clustering='recording_soft', speakers='auto')
        with pytest.raises(ValueError, match='recording 0.*outside'):      # an index past the recording's 2 TF points: the wrapper's check
            tr.model.separate_recording(x, clustering='recording_soft', kmeans_init_indices=[np.array([[0, 2 * TF], [1, 2]])])
    tr, _, _ = _front(None)
    with tr.graph.as_default():
        with pytest.raises(ValueError, match='beta_kmeans'):
            tr.model.separate_recording(x, clustering='recording_soft')
        with pytest.raises(ValueError, match='beta_kmeans'):
            tr.model.separate_recordings([x], clustering='recording_soft')


def test_command_lines_write_what_the_methods_return():
    from experiments.evaluation import separate as one
    from experiments.evaluation import separate_many as many
    _, _, folder = _front(BETA)
    tmp = tempfile.mkdtemp(prefix='ams_cli_soft_')
    lengths = {'first': 3300, 'second': 1500}
    for r, (stem, N) in enumerate(lengths.items()):
        one.write_wav(os.path.join(tmp, stem + '.wav'), _recording(N, 40 + r))
    common = ['--model_folder', folder, '--sortofmodel', 'front_DPCL', '--chunk_size', str(L), '--batch_size', str(B), '--nb_speakers', str(S),
              '--nb_tries', str(TRIES), '--nb_steps', str(STEPS), '--hop', '1280', '--no_summaries', '--beta_kmeans', str(BETA),
              '--with_silence', '--end_assign', '--clustering', 'recording_soft']
    # one recording
    argv = common + ['--input', os.path.join(tmp, 'first.wav'), '--output_prefix', os.path.join(tmp, 'cli')]
    paths = one.main(argv)
    tr, model, args = _fresh_model(one, argv)
    with tr.graph.as_default():
        out = model.separate_recording(one.read_input(args.input), hop=args.hop, clustering='recording_soft').cpu().numpy()
        assert 'masks' in model.last_clustering
    want = one.write_outputs(os.path.join(tmp, 'method'), out, False, None)
    assert paths == [os.path.join(tmp, 'cli_%d.wav' % k) for k in range(S)] and len(want) == S
    for p, q in zip(paths, want):
        assert open(p, 'rb').read() == open(q, 'rb').read() and np.abs(one.read_wav(p)).max() > 0
    # two recordings
    argv = common + ['--inputs', os.path.join(tmp, 'first.wav'), os.path.join(tmp, 'second.wav'), '--output_dir', os.path.join(tmp, 'out')]
    paths = many.main(argv)
    tr, model, args = _fresh_model(many, argv)
    with tr.graph.as_default():
        outs = model.separate_recordings([one.read_input(p) for p in args.inputs], hop=args.hop, clustering='recording_soft')
    assert paths == [os.path.join(tmp, 'out', '%s_%d.wav' % (stem, k)) for stem in lengths for k in range(S)]
    for r, stem in enumerate(lengths):
        assert outs[r].shape == (S, lengths[stem])
        want = one.write_outputs(os.path.join(tmp, 'm_' + stem), outs[r].cpu().numpy(), False, None)
        for k in range(S):
            assert open(paths[r * S + k], 'rb').read() == open(want[k], 'rb').read()
