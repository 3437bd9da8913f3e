"""GPU: k-means++ seeds for the recording-level modes -- Network.separate_recording / separate_recordings with
recording_seeding='plusplus' (models/network.py) on the tiny models of tests/test_gpu_separate_recording.py (hard, and soft
--with_silence), tests/test_gpu_separate_counted.py (three speakers) and a hard --with_silence one of the same recipe.  Every comparison
is exact: the seeds are those of the numpy restatement (tests/kmeans_seed_ref.py) on the embed_chunks points, and from equal seeds the
same kernels see the same points in the same order."""
import os
import tempfile

import numpy as np
import pytest

from tests import kmeans_seed_ref as ref

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

from tests.test_gpu_recipes import _full_checkpoint, base_args
from tests.test_gpu_separate_clustered import H, TF, _fresh_model, _seeds
from tests.test_gpu_separate_recording import B, E, HOP, L, LS, NF, NL, S, STEPS, TRIES, W, _front, _recording
from tests.test_gpu_separate_recordings import LENGTHS

COUNTS = [4, 1, 3]              # chunks of LENGTHS
_SILENT = []


def _front_silent():
    """The hard Front_Separator_Inference of tests/test_gpu_separate_recording.py::_front built --with_silence; built once."""
    if not _SILENT:
        from models.dpcl import DPCL
        from utils.trainer import Front_Separator_Inference
        tmp = tempfile.mkdtemp(prefix='ams_seed_')
        rng = np.random.RandomState(11)
        folder, params, P = _full_checkpoint(tmp, rng, W, NF, HOP, L, B, S, LS, NL, E, NF, NF)
        idx = np.stack([rng.choice(TF, S, replace=False) for _ in range(B * TRIES)]).astype(np.int32)
        a = base_args(**params)
        a.update(model_folder=folder, nb_tries=TRIES, nb_steps=STEPS, beta_kmeans=None, with_silence=True, end_assign=True,
                 kmeans_init_indices=idx, out=False)
        a.pop('type')
        tr = Front_Separator_Inference(DPCL, 'front_DPCL_inference', **a)
        tr.prepare()
        _SILENT.append(tr)
    return _SILENT[0]


def _draws(seed, clusters=S):
    rng = np.random.RandomState(seed)
    return (rng.randint(0, 1 << 32, size=(TRIES, clusters)).astype(np.uint64) << np.uint64(32)) | \
        rng.randint(0, 1 << 32, size=(TRIES, clusters)).astype(np.uint64)


def _inputs(clusters=S, seed=20):
    xs = [torch.from_numpy(_recording(N, seed + r)).cuda() for r, N in enumerate(LENGTHS)]
    return xs, [_draws(70 + r, clusters) for r in range(len(LENGTHS))]


def _restated(model, xs, draws, silence):
    """The restatement's seeds, one [TRIES, clusters] array per recording, from the points and weights embed_chunks gives."""
    from ams_hip import stitch_batch as sb
    mix, lay = sb.chunks_many(xs, L, H, model.S)
    pts, wts = model.embed_chunks(mix)
    assert (wts is not None) == silence and pts.shape[1:] == (TF, E)
    first = np.concatenate([[0], np.cumsum(lay.C)])
    ph, wh = pts.cpu().numpy(), None if wts is None else wts.cpu().numpy()
    return [ref.seed_segment(ph[first[r]:first[r + 1]].reshape(-1, E), draws[r],
                             None if wh is None else wh[first[r]:first[r + 1]].reshape(-1)) for r in range(len(xs))]


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a,
                                                                     b.view(torch.int32) if b.dtype == torch.float32 else b)


def _check_mode(tr, clustering, silence, clusters=S, **more):
    model = tr.model
    xs, draws = _inputs(clusters)
    with tr.graph.as_default():
        want_seeds = _restated(model, xs, draws, silence)
        got = model.separate_recordings(xs, clustering=clustering, recording_seeding='plusplus', kmeans_seed_draws=draws, **more)
        lg = model.last_clustering
        want = model.separate_recordings(xs, clustering=clustering, kmeans_init_indices=want_seeds, **more)
        lw = model.last_clustering
        # the grouping of the embedding buffer changes nothing: recordings 0 and 1 together and 2 behind them
        two = model.separate_recordings(xs, clustering=clustering, recording_seeding='plusplus', kmeans_seed_draws=draws,
                                        cluster_cap_bytes=5 * TF * E * 4, **more)
        l2 = model.last_clustering
        ones = [model.separate_recording(x, clustering=clustering, recording_seeding='plusplus', kmeans_seed_draws=draws[r:r + 1], **more)
                for r, x in enumerate(xs)]
        l1 = model.last_clustering
        alone = model.separate_recordings(xs[2:], clustering=clustering, recording_seeding='plusplus', kmeans_seed_draws=draws[2:], **more)
    assert lg['seeds'].dtype == torch.int32 and lg['seeds'].shape == (3, TRIES, clusters) and lg['seeds'].is_cuda
    assert np.array_equal(lg['seeds'].cpu().numpy(), np.stack(want_seeds))
    assert 'seeds' not in lw and sorted(set(lg) - {'seeds'}) == sorted(lw)
    assert l2['groups'] == [(0, 2), (2, 3)] and torch.equal(l2['seeds'], lg['seeds'])
    assert l1['seeds'].shape == (1, TRIES, clusters) and torch.equal(l1['seeds'][0], lg['seeds'][2])
    for key in lw:
        if torch.is_tensor(lw[key]):
            assert _same(lg[key], lw[key]), key
    for r, N in enumerate(LENGTHS):
        assert got[r].shape[1] == N and bool(torch.isfinite(got[r]).all())
        assert _same(got[r], want[r]) and _same(got[r], two[r]) and _same(got[r], ones[r]), r
    assert _same(alone[0], ones[2])                                # separate_recording is separate_recordings of the one recording
    return lg


def test_recording_mode_from_plusplus_seeds_is_recording_mode_from_the_restated_seeds():
    tr, _, _ = _front(None)
    lg = _check_mode(tr, 'recording', False)
    assert lg['labels'].shape == (sum(COUNTS), TF)


def test_recording_soft_on_a_soft_model_with_silence_weights():
    tr, _, _ = _front(5.0)
    lg = _check_mode(tr, 'recording_soft', True)
    assert lg['masks'].shape == (sum(COUNTS), TF, S)


def test_a_hard_model_with_silence_weights():
    _check_mode(_front_silent(), 'recording', True)


def test_counted_recordings_take_the_first_columns_of_one_seeding():
    from tests.test_gpu_separate_counted import S as S3, _front3
    tr, _ = _front3()
    lg = _check_mode(tr, 'recording', False, clusters=S3, speakers='auto')
    assert lg['counts'].shape == (3,) and lg['scores'].shape == (3, S3 - 1)


def test_the_default_is_the_models_seeding_unchanged():
    tr, _, _ = _front(None)
    model = tr.model
    xs, _ = _inputs()
    seeds = [_seeds(C, 50 + r) for r, C in enumerate(COUNTS)]
    with tr.graph.as_default():
        plain = model.separate_recordings(xs, clustering='recording', kmeans_init_indices=seeds)
        lp = model.last_clustering
        named = model.separate_recordings(xs, clustering='recording', kmeans_init_indices=seeds, recording_seeding='model')
        ln = model.last_clustering
        one_p = model.separate_recording(xs[0], clustering='recording', kmeans_init_indices=seeds[:1])
        one_n = model.separate_recording(xs[0], clustering='recording', kmeans_init_indices=seeds[:1], recording_seeding='model',
                                         kmeans_seed_draws=None)
        chunk_p = model.separate_recording(xs[1])
        chunk_n = model.separate_recording(xs[1], recording_seeding='model')
    assert sorted(lp) == sorted(ln) == ['best', 'centroids', 'first_chunk', 'groups', 'labels']
    for a, b in zip(plain, named):
        assert _same(a, b)
    assert _same(lp['labels'], ln['labels']) and _same(one_p, one_n) and _same(one_p, plain[0]) and _same(chunk_p, chunk_n)


def test_models_built_alike_draw_the_same_default_seeds():
    """Two models from one command line: the default draws come from the KMeans object's own stream (KMeans.seed_draws), recording after
    recording in list order -- and the command line passes --recording_seeding straight through."""
    from experiments.evaluation import separate as one
    from experiments.evaluation import separate_many as many
    _, _, folder = _front(None)
    tmp = tempfile.mkdtemp(prefix='ams_cli_seed_')
    lengths = {'first': 3300, 'second': 1500}
    for r, (stem, N) in enumerate(lengths.items()):
        one.write_wav(os.path.join(tmp, stem + '.wav'), _recording(N, 40 + r))
    argv = ['--model_folder', folder, '--sortofmodel', 'front_DPCL', '--chunk_size', str(L), '--batch_size', str(B), '--nb_speakers', str(S),
            '--nb_tries', str(TRIES), '--nb_steps', str(STEPS), '--hop', '1280', '--no_summaries', '--clustering', 'recording',
            '--recording_seeding', 'plusplus', '--inputs', os.path.join(tmp, 'first.wav'), os.path.join(tmp, 'second.wav'),
            '--output_dir', os.path.join(tmp, 'out')]
    paths = many.main(argv)
    res = []
    for _ in range(2):
        tr, model, args = _fresh_model(many, argv)
        assert args.recording_seeding == 'plusplus'
        xs = [one.read_input(p) for p in args.inputs]
        with tr.graph.as_default():
            outs = model.separate_recordings(xs, hop=args.hop, clustering='recording', recording_seeding='plusplus')
            seeds = model.last_clustering['seeds']
            sep = getattr(model, 'sepNet', None) or model
            assert sep.kmeans._pp_draws == 2                       # one draw per recording
            # ... which are the stream's first two draws, handed in by hand
            km = type(sep.kmeans).__new__(type(sep.kmeans))
            byhand = model.separate_recordings(xs, hop=args.hop, clustering='recording', recording_seeding='plusplus',
                                               kmeans_seed_draws=[km.seed_draws(TRIES, S), km.seed_draws(TRIES, S)])
            assert torch.equal(model.last_clustering['seeds'], seeds) and all(_same(a, b) for a, b in zip(outs, byhand))
        res.append((outs, seeds))
    assert torch.equal(res[0][1], res[1][1]) and res[0][1].shape == (2, TRIES, S)
    for r, stem in enumerate(lengths):
        assert _same(res[0][0][r], res[1][0][r]) and res[0][0][r].shape == (S, lengths[stem])
        want = one.write_outputs(os.path.join(tmp, 'm_' + stem), res[0][0][r].cpu().numpy(), False, None)
        for k in range(S):
            assert open(paths[r * S + k], 'rb').read() == open(want[k], 'rb').read()
