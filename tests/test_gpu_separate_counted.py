"""GPU: a number of speakers per recording -- Network.separate_recording / separate_recordings with speakers=(lo, hi)
(models/network.py) on the tiny Front_Separator_Inference of tests/test_gpu_separate_clustered.py built with THREE
speakers (B = 2, L = 2048, E = 8, S = 3), and both command lines.  Every comparison of separated samples is exact: the same points, the
same seeds, the same kernels in the same order.

The embeddings of a model with random weights have no planted structure, so the restatement's margins between the candidate counts
are asserted (>= 1e-6) for the fixed recording seeds below; SEED was picked on one MI355X among 20 .. 79 for counts that differ
between the recordings and the widest margins (the figures: test_counted_recordings_are_the_composition)."""
import json
import os
import tempfile

import numpy as np
import pytest

from tests import speaker_count_ref as ref

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

from tests.test_gpu_recipes import _full_checkpoint, base_args
from tests.test_gpu_separate_recording import B, E, HOP, L, LS, NF, NL, STEPS, TRIES, W, _recording
from tests.test_gpu_separate_recordings import LENGTHS, _counting

S = 3
TF = -(-L // HOP) * NF
H = L // 2
COUNTS = [4, 1, 3]              # chunks of LENGTHS
SEED = 45
MARGIN = 1e-6
_MODEL = []


def _front3():
    """The Front_Separator_Inference of tests/test_gpu_separate_recording.py::_front with three speakers and a hard k-means; built once."""
    if not _MODEL:
        from models.dpcl import DPCL
        from utils.trainer import Front_Separator_Inference
        tmp = tempfile.mkdtemp(prefix='ams_cnt_')
        rng = np.random.RandomState(11)
        folder, params, P = _full_checkpoint(tmp, rng, W, NF, HOP, L, B, S, LS, NL, E, NF, NF)
        idx = np.stack([rng.choice(TF, S, replace=False) for _ in range(B * TRIES)]).astype(np.int32)
        a = base_args(**params)
        a.update(model_folder=folder, nb_tries=TRIES, nb_steps=STEPS, beta_kmeans=None, with_silence=False, end_assign=True,
                 kmeans_init_indices=idx, out=False)
        a.pop('type')
        tr = Front_Separator_Inference(DPCL, 'front_DPCL_inference', **a)
        tr.prepare()
        _MODEL.append((tr, folder))
    return _MODEL[0]


def _seeds(C, seed):
    """[TRIES, S] distinct point indices over the C TF points of a recording."""
    rng = np.random.RandomState(seed)
    return np.stack([rng.choice(C * TF, S, replace=False) for _ in range(TRIES)]).astype(np.int32)


def _inputs():
    xs = [torch.from_numpy(_recording(N, SEED + r)).cuda() for r, N in enumerate(LENGTHS)]
    return xs, [_seeds(C, 50 + r) for r, C in enumerate(COUNTS)]


def _identity(C):
    return torch.arange(S, dtype=torch.int32, device='cuda').repeat(C, 1)


def test_the_models_own_count_is_recording_mode():
    """speakers=(S, S): one candidate, the model's S; with no non-finite try everything is bit-equal to clustering='recording'."""
    tr, _ = _front3()
    model = tr.model
    xs, seeds = _inputs()
    with tr.graph.as_default():
        want = model.separate_recordings(xs, clustering='recording', kmeans_init_indices=seeds)
        lw = model.last_clustering
        got = model.separate_recordings(xs, clustering='recording', kmeans_init_indices=seeds, speakers=(S, S))
        lg = model.last_clustering
        one_w = model.separate_recording(xs[2], clustering='recording', kmeans_init_indices=seeds[2:])
        one_g = model.separate_recording(xs[2], clustering='recording', kmeans_init_indices=seeds[2:], speakers=(S, S))
    assert bool((lg['tries'] >= 0).all())                         # the premise: every try's inertia is finite
    assert lg['counts'].tolist() == [S] * 3 and lg['scores'].shape == (3, 1) and lg['tries'].shape == (3, 1)
    for a, b, N in zip(got, want, LENGTHS):
        assert a.shape == (S, N) and torch.equal(a, b)
    assert torch.equal(lg['labels'], lw['labels']) and torch.equal(lg['centroids'], lw['centroids']) and torch.equal(lg['best'], lw['best'])
    assert torch.equal(one_g, one_w) and torch.equal(one_g, got[2])


def test_counted_recordings_are_the_composition():
    """[4396, 1000, 3300] with speakers=(2, 3) against embed_chunks -> kmeans_ragged per candidate -> the restatement's choice on those
    points and centroids -> infer_chunks_masked -> the identity cross-fade -> the first S_r rows; bit-equal, the dropped rows exactly
    zero, 2 ceil(Ctot / B) model passes, two caps of the embedding buffer with equal results.

    Measured on one MI355X (one run, SEED = 45): counts [2, 3, 2], margins between the two candidates' scores 0.0192, 0.0487 and
    0.0226, chosen tries [0, 1], [0, 0] and [0, 1].  The assertion is margin >= 1e-6 for every recording."""
    from ams_hip import functional as F
    from ams_hip import kmeans_ragged as kr
    from ams_hip import stitch_batch as sb
    tr, _ = _front3()
    model = tr.model
    xs, seeds = _inputs()
    with tr.graph.as_default():
        calls, undo = _counting(model)
        try:
            outs = model.separate_recordings(xs, clustering='recording', kmeans_init_indices=seeds, speakers=(2, S))
        finally:
            undo()
        assert len(calls) == 2 * -(-sum(COUNTS) // B) == 8
        got = model.last_clustering
        auto = model.separate_recordings(xs, clustering='recording', kmeans_init_indices=seeds, speakers='auto')
        # the composition
        mix, lay = sb.chunks_many(xs, L, H, S)
        assert lay.C.tolist() == COUNTS
        pts, wts = model.embed_chunks(mix)
        assert wts is None and pts.shape == (sum(COUNTS), TF, E)
        seg = kr.segments([c * TF for c in COUNTS])
        idx = np.concatenate(seeds)
        x2 = pts.view(-1, E)
        runs, tries = [], []
        for C in (2, 3):
            sd = np.ascontiguousarray(idx[:, :C])
            tries.append([t.cpu().numpy() for t in kr.kmeans_ragged_tries(x2, seg, sd, C, TRIES, STEPS, normalize_input=False)])
            runs.append(kr.kmeans_ragged(x2, seg, sd, C, TRIES, STEPS, assign_at_end=True, normalize_input=False))
        xh = x2.cpu().numpy()
        labels = torch.empty(seg.Ptot, dtype=torch.int32, device='cuda')
        counts = []
        for r in range(3):
            rows = seg.rows(r)
            want = ref.count(xh[rows], None, None, 2, S, STEPS, cents=[t[0][r * TRIES:(r + 1) * TRIES] for t in tries],
                             inertias=[t[1][r * TRIES:(r + 1) * TRIES] for t in tries])
            m = ref.margin(want['scores'])
            print('recording %d: count %d, scores %s, tries %s, margin %.6g' % (r, want['count'], want['scores'].tolist(),
                                                                              want['tries'].tolist(), m))
            assert m >= MARGIN and (want['tries'] >= 0).all()
            assert np.all(np.abs(got['scores'][r].cpu().numpy() - want['scores']) <= 1e-9)
            assert np.array_equal(got['tries'][r].cpu().numpy(), want['tries'])
            # every try is finite, so kmeans_ragged's own selection is the restatement's try
            assert int(runs[want['cand']][2][r]) == want['tries'][want['cand']]
            labels[rows] = runs[want['cand']][1][rows]
            counts.append(want['count'])
        assert got['counts'].tolist() == counts
        assert torch.equal(got['labels'].view(-1), labels)
        packed = sb.overlap_add_many(model.infer_chunks_masked(mix, F.one_hot_masks(labels.view(-1, TF), S), B), _identity(lay.Ctot), lay)
        # two caps: recordings 0 and 1 together and 2 behind them; recording 0 alone, then 1 and 2
        two = model.separate_recordings(xs, clustering='recording', kmeans_init_indices=seeds, speakers=(2, S), cluster_cap_bytes=5 * TF * E * 4)
        groups2, counts2 = model.last_clustering['groups'], model.last_clustering['counts'].tolist()
        three = model.separate_recordings([x.cpu().numpy() for x in xs], clustering='recording', kmeans_init_indices=seeds, speakers=(2, S),
                                          cluster_cap_bytes=4 * TF * E * 4)
        groups3, scores3 = model.last_clustering['groups'], model.last_clustering['scores']
        one = model.separate_recording(xs[2], clustering='recording', kmeans_init_indices=seeds[2:], speakers=(2, S))
    assert got['groups'] == [(0, 3)] and groups2 == [(0, 2), (2, 3)] and groups3 == [(0, 1), (1, 3)]
    assert counts2 == counts and torch.equal(scores3, got['scores'])
    for r, (out, N) in enumerate(zip(outs, LENGTHS)):
        o = int(lay.out_off[r])
        full = packed[o:o + S * N].view(S, N)
        assert out.shape == (counts[r], N) and bool(torch.isfinite(out).all())
        assert torch.equal(out, full[:counts[r]])
        assert not bool(full[counts[r]:].any())                   # the dropped rows are exactly zero
        assert torch.equal(out, two[r]) and torch.equal(out, three[r]) and torch.equal(out, auto[r])
    assert torch.equal(one, outs[2])


def _fresh_model(cli, argv):
    from experiments.evaluation.eval import pick
    args = cli.build_parser().get_args(argv)
    inferencer, sep = pick(args.sortofmodel)
    tr = inferencer(sep, 'inference', **vars(args))
    return tr, tr.prepare_inference(), args


def test_command_lines_write_one_file_per_counted_speaker():
    from experiments.evaluation import separate as one
    from experiments.evaluation import separate_many as many
    _, folder = _front3()
    tmp = tempfile.mkdtemp(prefix='ams_cli_cnt_')
    lengths = {'first': 3300, 'second': 1500}
    for r, (stem, N) in enumerate(lengths.items()):
        one.write_wav(os.path.join(tmp, stem + '.wav'), _recording(N, 40 + r))
    common = ['--model_folder', folder, '--sortofmodel', 'front_DPCL', '--chunk_size', str(L), '--batch_size', str(B), '--nb_speakers', str(S),
              '--nb_tries', str(TRIES), '--nb_steps', str(STEPS), '--hop', '1280', '--no_summaries', '--clustering', 'recording',
              '--speakers', 'auto']
    # one recording
    argv = common + ['--input', os.path.join(tmp, 'first.wav'), '--output_prefix', os.path.join(tmp, 'cli')]
    paths = one.main(argv)
    tr, model, args = _fresh_model(one, argv)
    with tr.graph.as_default():
        out = model.separate_recording(one.read_input(args.input), hop=args.hop, clustering='recording', speakers='auto').cpu().numpy()
    n = int(model.last_clustering['counts'][0])
    assert 2 <= n <= S and out.shape == (n, 3300)
    want = one.write_outputs(os.path.join(tmp, 'method'), out, False, None)
    assert paths == [os.path.join(tmp, 'cli_%d.wav' % k) for k in range(n)] and len(want) == n
    assert not os.path.exists(os.path.join(tmp, 'cli_%d.wav' % n))
    for p, q in zip(paths, want):
        assert open(p, 'rb').read() == open(q, 'rb').read() and np.abs(one.read_wav(p)).max() > 0
    # two recordings
    argv = common + ['--inputs', os.path.join(tmp, 'first.wav'), os.path.join(tmp, 'second.wav'), '--output_dir', os.path.join(tmp, 'out')]
    paths = many.main(argv)
    tr, model, args = _fresh_model(many, argv)
    with tr.graph.as_default():
        outs = model.separate_recordings([one.read_input(p) for p in args.inputs], hop=args.hop, clustering='recording', speakers='auto')
    counts = model.last_clustering['counts'].tolist()
    scores = model.last_clustering['scores'].tolist()
    assert paths == [os.path.join(tmp, 'out', '%s_%d.wav' % (stem, k)) for stem, c in zip(lengths, counts) for k in range(c)] + \
        [os.path.join(tmp, 'out', 'counts.json')]
    assert sorted(os.listdir(os.path.join(tmp, 'out'))) == sorted(os.path.basename(p) for p in paths)
    cj = json.load(open(paths[-1]))
    assert cj['speakers'] == [2, S] and cj['candidates'] == [2, 3] and cj['min_score'] is None
    at = 0
    for r, stem in enumerate(lengths):
        assert outs[r].shape == (counts[r], lengths[stem])
        assert cj['recordings'][stem] == {'count': counts[r], 'scores': scores[r]}
        want = one.write_outputs(os.path.join(tmp, 'm_' + stem), outs[r].cpu().numpy(), False, None)
        for k in range(counts[r]):
            assert open(paths[at + k], 'rb').read() == open(want[k], 'rb').read()
        at += counts[r]
