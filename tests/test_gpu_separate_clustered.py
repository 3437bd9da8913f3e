"""GPU: recording-level clustering -- Network.separate_recording / separate_recordings with clustering='recording' (models/network.py,
DESIGN.md 4.10) on the tiny Front_Separator_Inference of tests/test_gpu_separate_recording.py (B = 2, L = 2048, E = 8, S = 2), one STFT
recipe and both command lines.  Every comparison is exact: the same points, the same seeds, the same kernels in the same order."""
import os
import tempfile

import numpy as np
import pytest

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

from tests.test_gpu_recipes import _full_checkpoint, base_args
from tests.test_gpu_separate_recording import B, E, HOP, L, LS, NF, NL, S, STEPS, TRIES, _front, _recording
from tests.test_gpu_separate_recordings import LENGTHS, _counting

TF = -(-L // HOP) * NF
H = L // 2


def _seeds(C, seed, tf=TF):
    """[TRIES, S] distinct point indices over the C tf points of a recording."""
    rng = np.random.RandomState(seed)
    return np.stack([rng.choice(C * tf, S, replace=False) for _ in range(TRIES)]).astype(np.int32)


def _pooled_masks(model, mix, counts, seeds, batch_size=None):
    """The definition: embed_chunks, every recording's points pooled as ONE utterance for ops.kmeans_run with its seeds -> (masks, labels)."""
    from ams_hip import functional as F
    from ams_hip import ops
    pts, wts = model.embed_chunks(mix, batch_size)
    assert wts is None and pts.shape[0] == mix.shape[0] and pts.shape[2] == E
    tf = pts.shape[1]
    labels, c0 = [], 0
    for C, idx in zip(counts, seeds):
        xn = pts[c0:c0 + C].reshape(1, C * tf, E).contiguous()
        _, lab, _, _ = ops.kmeans_run(xn, torch.from_numpy(idx).cuda(), S, TRIES, STEPS, assign_at_end=True)
        labels.append(lab.view(C, tf))
        c0 += C
    labels = torch.cat(labels)
    return F.one_hot_masks(labels, S), labels


def _identity(C):
    return torch.arange(S, dtype=torch.int32, device='cuda').repeat(C, 1)


def test_one_chunk_is_chunk_mode_with_the_same_seeds():
    """N <= L: both modes cluster the same TF points; chunk mode takes rows 0 .. TRIES - 1 of the model's seeds for the chunk in batch row 0."""
    tr, _, _ = _front(None)
    idx = np.asarray(getattr(tr.model, 'sepNet', tr.model).kmeans.init_indices)[:TRIES]
    assert idx.shape == (TRIES, S)
    for N in (1500, L):
        x = torch.from_numpy(_recording(N, 8)).cuda()
        with tr.graph.as_default():
            chunk = tr.model.separate_recording(x)
            also = tr.model.separate_recording(x, clustering='chunk')
            rec = tr.model.separate_recording(x, clustering='recording', kmeans_init_indices=[idx])
            many = tr.model.separate_recordings([x], clustering='recording', kmeans_init_indices=[idx])
        assert rec.shape == (S, N) and torch.equal(rec, chunk) and torch.equal(also, chunk) and torch.equal(many[0], chunk)


@pytest.mark.parametrize('N,C', [(4396, 4), (3300, 3)])          # two full batches; a last batch padded by repetition
def test_recording_mode_is_embed_pool_mask_overlap_add(N, C):
    from ams_hip import stitch
    tr, _, _ = _front(None)
    model = tr.model
    x = torch.from_numpy(_recording(N)).cuda()
    seeds = [_seeds(C, N)]
    with tr.graph.as_default():
        calls, undo = _counting(model)
        try:
            out = model.separate_recording(x, clustering='recording', kmeans_init_indices=seeds)
        finally:
            undo()
        assert len(calls) == 2 * -(-C // B)
        got = model.last_clustering
        mix = stitch.chunks(x, L, H)
        assert mix.shape == (C, L)
        masks, labels = _pooled_masks(model, mix, [C], seeds)
        want = stitch.overlap_add(model.infer_chunks_masked(mix, masks, B), _identity(C), N, H)
        again = model.separate_recording(x.cpu().numpy(), clustering='recording', kmeans_init_indices=seeds)
        tracked = model.separate_recording(x)
    assert out.shape == (S, N) and bool(torch.isfinite(out).all())
    assert torch.equal(out, want) and torch.equal(out, again)
    assert got['labels'].shape == (C, TF) and torch.equal(got['labels'], labels)
    assert got['centroids'].shape == (1, S, E) and got['best'].shape == (1,)
    assert 0 < int(labels.sum()) < labels.numel()                  # both clusters are used
    assert tracked.shape == out.shape                              # (the default path still runs on the same model)


def test_many_recordings_one_ragged_call_two_sweeps():
    from ams_hip import kmeans_ragged as kr
    from ams_hip import stitch_batch as sb
    tr, _, _ = _front(None)
    model = tr.model
    xs = [torch.from_numpy(_recording(N, 20 + r)).cuda() for r, N in enumerate(LENGTHS)]
    counts = [4, 1, 3]
    seeds = [_seeds(C, 50 + r) for r, C in enumerate(counts)]
    with tr.graph.as_default():
        calls, undo = _counting(model)
        n0 = kr.LAUNCHES
        try:
            outs = model.separate_recordings(xs, clustering='recording', kmeans_init_indices=seeds)
        finally:
            undo()
        assert len(calls) == 2 * -(-sum(counts) // B) == 8         # two sweeps of the chunk stream, whatever the number of recordings
        assert kr.LAUNCHES - n0 == STEPS + 4                        # ... and ONE k-means run for all of them
        got = model.last_clustering
        mix, lay = sb.chunks_many(xs, L, H, S)
        assert lay.C.tolist() == counts
        masks, labels = _pooled_masks(model, mix, counts, seeds)
        packed = sb.overlap_add_many(model.infer_chunks_masked(mix, masks, B), _identity(lay.Ctot), lay)
        # a cap of five chunks' embeddings: recordings 0 and 1 (4 + 1 chunks) together, recording 2 behind them; a cap of four: recording 0
        # alone, recordings 1 and 2 (1 + 3 chunks) together.  A batch then straddles two groups; the model passes stay the same eight
        two = model.separate_recordings(xs, clustering='recording', kmeans_init_indices=seeds, cluster_cap_bytes=5 * TF * E * 4)
        groups2 = model.last_clustering['groups']
        three = model.separate_recordings([x.cpu().numpy() for x in xs], clustering='recording', kmeans_init_indices=seeds,
                                          cluster_cap_bytes=4 * TF * E * 4)
        groups3 = model.last_clustering['groups']
        assert torch.equal(model.last_clustering['labels'], labels)
        with pytest.raises(ValueError, match='above the cap'):
            model.separate_recordings(xs, clustering='recording', kmeans_init_indices=seeds, cluster_cap_bytes=4 * TF * E * 4 - 1)
        one = model.separate_recording(xs[2], clustering='recording', kmeans_init_indices=seeds[2:])
    assert got['groups'] == [(0, 3)] and groups2 == [(0, 2), (2, 3)] and groups3 == [(0, 1), (1, 3)]
    assert torch.equal(got['labels'], labels) and got['centroids'].shape == (3, S, E) and got['best'].shape == (3,)
    for r, (out, N) in enumerate(zip(outs, LENGTHS)):
        o = int(lay.out_off[r])
        assert out.shape == (S, N) and bool(torch.isfinite(out).all())
        assert torch.equal(out, packed[o:o + S * N].view(S, N))
        assert torch.equal(out, two[r]) and torch.equal(out, three[r])
    assert one.shape == (S, LENGTHS[2])


def test_default_seeds_are_drawn_per_recording_in_list_order():
    """Without kmeans_init_indices the model draws: with 'reference' seeding one np.random.choice(P_r, S, replace=False) per try from the
    global generator, recording after recording."""
    tr, _, _ = _front(None)
    model = tr.model
    xs = [torch.from_numpy(_recording(N, 30 + r)).cuda() for r, N in enumerate((3300, 1000))]
    with tr.graph.as_default():
        state = np.random.get_state()
        drawn = model.separate_recordings(xs, clustering='recording')
        np.random.set_state(state)
        seeds = [np.stack([np.random.choice(C * TF, S, replace=False) for _ in range(TRIES)]).astype(np.int32) for C in (3, 1)]
        given = model.separate_recordings(xs, clustering='recording', kmeans_init_indices=seeds)
    for a, b in zip(drawn, given):
        assert torch.equal(a, b)


def test_stft_recipe_with_silence_weights():
    """An STFT model built --with_silence: embed_chunks returns the per-chunk silence weights and the ragged k-means takes them."""
    from ams_hip import functional as F
    from ams_hip import ops, stitch
    from models.dpcl import DPCL
    from utils.trainer import STFT_Separator_Inference
    tmp = tempfile.mkdtemp(prefix='ams_crec_')
    rng = np.random.RandomState(12)
    Bs, W2, hop2 = 2, 64, 32
    Fq = W2 // 2 + 1
    folder, params, P = _full_checkpoint(tmp, rng, W2, None, hop2, L, Bs, S, LS, NL, E, Fq, Fq, front=False)
    a = base_args(**params)
    a.update(model_folder=folder, nb_tries=TRIES, nb_steps=STEPS, end_assign=False, with_silence=True, out=False)
    a.pop('type')
    tr = STFT_Separator_Inference(DPCL, 'STFT_DPCL_inference', **a)
    model = tr.prepare_inference()
    N, C = 3300, 3
    tf = (1 + (L - W2) // hop2) * Fq
    seeds = [_seeds(C, 9, tf)]
    x = torch.from_numpy(_recording(N, 5)).cuda()
    with tr.graph.as_default():
        out = model.separate_recording(x, clustering='recording', kmeans_init_indices=seeds)
        mix = stitch.chunks(x, L, H)
        pts, wts = model.embed_chunks(mix)
        assert pts.shape == (C, tf, E) and wts.shape == (C, tf) and bool(((wts == 0) | (wts == 1)).all())
        print('silent points: %d of %d' % (int((wts == 0).sum()), wts.numel()))
        _, lab, _, _ = ops.kmeans_run(pts.reshape(1, C * tf, E), torch.from_numpy(seeds[0]).cuda(), S, TRIES, STEPS,
                                      w=wts.reshape(1, C * tf), assign_at_end=False)
        assert torch.equal(model.last_clustering['labels'], lab.view(C, tf))
        want = stitch.overlap_add(model.infer_chunks_masked(mix, F.one_hot_masks(lab.view(C, tf), S)), _identity(C), N, H)
    assert out.shape == (S, N) and bool(torch.isfinite(out).all()) and float(out.abs().max()) > 0 and torch.equal(out, want)


def test_refusals_on_a_real_model():
    tr, _, _ = _front(5.0)                                         # a soft k-means
    x = _recording(3000)
    with tr.graph.as_default():
        with pytest.raises(ValueError, match='hard assignment only'):
            tr.model.separate_recording(x, clustering='recording')
        with pytest.raises(ValueError, match='hard assignment only'):
            tr.model.separate_recordings([x], clustering='recording')
    tr, _, _ = _front(None)
    with tr.graph.as_default():
        with pytest.raises(ValueError, match="'chunk' or 'recording'"):
            tr.model.separate_recording(x, clustering='both')
        with pytest.raises(ValueError, match='per recording'):
            tr.model.separate_recordings([x, x], clustering='recording', kmeans_init_indices=[_seeds(2, 1)])
        with pytest.raises(ValueError, match='recording 0.*outside'):      # an index past the recording's 2 TF points: the wrapper's check
            tr.model.separate_recording(x, clustering='recording', kmeans_init_indices=[np.array([[0, 2 * TF], [1, 2]])])
        with pytest.raises(ValueError, match='masks'):
            tr.model.infer_chunks_masked(torch.zeros(2, L, device='cuda'), torch.zeros(3, TF, S, device='cuda'))


def _fresh_model(cli, argv):
    """The model the command line builds for argv (a fresh one: the reference seed stream starts where the command line's started)."""
    from experiments.evaluation.eval import pick
    args = cli.build_parser().get_args(argv)
    inferencer, sep = pick(args.sortofmodel)
    tr = inferencer(sep, 'inference', **vars(args))
    return tr, tr.prepare_inference(), args


def test_command_lines_write_what_the_methods_return():
    from experiments.evaluation import separate as one
    from experiments.evaluation import separate_many as many
    _, _, folder = _front(None)
    tmp = tempfile.mkdtemp(prefix='ams_cli_clu_')
    lengths = {'first': 3300, 'second': 1500}
    for r, (stem, N) in enumerate(lengths.items()):
        one.write_wav(os.path.join(tmp, stem + '.wav'), _recording(N, 40 + r))
    common = ['--model_folder', folder, '--sortofmodel', 'front_DPCL', '--chunk_size', str(L), '--batch_size', str(B), '--nb_speakers', str(S),
              '--nb_tries', str(TRIES), '--nb_steps', str(STEPS), '--hop', '1280', '--no_summaries', '--clustering', 'recording']
    # one recording
    argv = common + ['--input', os.path.join(tmp, 'first.wav'), '--output_prefix', os.path.join(tmp, 'cli')]
    paths = one.main(argv)
    tr, model, args = _fresh_model(one, argv)
    with tr.graph.as_default():
        out = model.separate_recording(one.read_input(args.input), hop=args.hop, clustering='recording').cpu().numpy()
    want = one.write_outputs(os.path.join(tmp, 'method'), out, False, None)
    assert paths == [os.path.join(tmp, 'cli_%d.wav' % k) for k in range(S)] and len(want) == S
    for p, q in zip(paths, want):
        assert open(p, 'rb').read() == open(q, 'rb').read() and np.abs(one.read_wav(p)).max() > 0
    # two recordings
    argv = common + ['--inputs', os.path.join(tmp, 'first.wav'), os.path.join(tmp, 'second.wav'), '--output_dir', os.path.join(tmp, 'out')]
    paths = many.main(argv)
    tr, model, args = _fresh_model(many, argv)
    with tr.graph.as_default():
        outs = model.separate_recordings([one.read_input(p) for p in args.inputs], hop=args.hop, clustering='recording')
    assert paths == [os.path.join(tmp, 'out', '%s_%d.wav' % (stem, k)) for stem in lengths for k in range(S)]
    for r, stem in enumerate(lengths):
        assert outs[r].shape == (S, lengths[stem])
        want = one.write_outputs(os.path.join(tmp, 'm_' + stem), outs[r].cpu().numpy(), False, None)
        for k in range(S):
            assert open(paths[r * S + k], 'rb').read() == open(want[k], 'rb').read()
