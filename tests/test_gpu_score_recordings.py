"""GPU: experiments/evaluation/separate_many.py --reference_dir -- three synthetic recordings (the lengths of
tests/test_gpu_separate_recordings.py) through the tiny random-weight front_DPCL model of tests/test_gpu_separate_recording.py, scored by
ONE ragged BSS-eval call.  scores.json is held to utils.bss_eval.bss_eval_sources_ragged on the written tracks and to the numpy oracle
on them (the project's dB rule; the permutations exactly), and scoring changes no written track."""
import json
import os
import tempfile

import numpy as np
import pytest

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

from oracle import bss_eval as obss
from tests.bss_common import TOL_DB, close_db as _close_db
from tests.test_gpu_separate_recording import B, L, S, STEPS, TRIES, _front, _recording
from tests.test_gpu_separate_recordings import LENGTHS

_RUNS = {}


def _runs():
    """The command line three times on the same inputs (built once): without scoring, with --reference_dir, with both clusterings."""
    if not _RUNS:
        from experiments.evaluation import separate as one
        from experiments.evaluation import separate_many as many
        _, _, folder = _front(None)
        tmp = tempfile.mkdtemp(prefix='ams_score_')
        refd = os.path.join(tmp, 'refs')
        os.makedirs(refd)
        stems = ['rec%d' % r for r in range(len(LENGTHS))]
        for r, (stem, N) in enumerate(zip(stems, LENGTHS)):
            srcs = [0.5 * _recording(N, 70 + 10 * r + k) for k in range(S)]
            paths = one.write_outputs(os.path.join(refd, stem), np.stack(srcs), False, None)
            one.write_wav(os.path.join(tmp, stem + '.wav'), sum(one.read_input(p) for p in paths))      # the mixture of the WRITTEN sources
        common = ['--model_folder', folder, '--sortofmodel', 'front_DPCL', '--chunk_size', str(L), '--batch_size', str(B), '--nb_speakers', str(S),
                  '--nb_tries', str(TRIES), '--nb_steps', str(STEPS), '--no_summaries', '--inputs'] + [os.path.join(tmp, s + '.wav') for s in stems]
        _RUNS['stems'], _RUNS['tmp'], _RUNS['refd'] = stems, tmp, refd
        for name, extra in (('plain', []), ('scored', ['--reference_dir', refd]),
                            ('both', ['--reference_dir', refd, '--score_both_clusterings'])):
            _RUNS[name] = many.main(common + ['--output_dir', os.path.join(tmp, name)] + extra)
    return _RUNS


def _data(run):
    from experiments.evaluation import separate as one
    r = _runs()
    refs = [np.stack([one.read_input(os.path.join(r['refd'], '%s_%d.wav' % (s, k))) for k in range(S)]) for s in r['stems']]
    mixes = [one.read_input(os.path.join(r['tmp'], s + '.wav')) for s in r['stems']]
    tracks = [np.stack([one.read_input(os.path.join(r['tmp'], run, '%s_%d.wav' % (s, k))) for k in range(S)]) for s in r['stems']]
    return refs, mixes, tracks


def _check_set(entry, name, sdr, sir, sar, perm):
    got = entry['sets'][name]
    assert got['perm'] == [int(v) for v in perm]
    for key, want in (('sdr', sdr), ('sir', sir), ('sar', sar)):
        _close_db(np.array(got[key], np.float64), want)


def test_scoring_changes_no_written_track():
    r = _runs()
    n = len(r['stems']) * S
    assert len(r['plain']) == n and [os.path.basename(p) for p in r['scored'][:n]] == [os.path.basename(p) for p in r['plain']]
    assert r['scored'][n:] == [os.path.join(r['tmp'], 'scored', 'scores.json')] and r['both'][n:] == [os.path.join(r['tmp'], 'both', 'scores.json')]
    for p, q, b in zip(r['plain'], r['scored'], r['both']):
        raw = open(p, 'rb').read()
        assert raw == open(q, 'rb').read() and raw == open(b, 'rb').read() and len(raw) > 44
    assert not os.path.exists(os.path.join(r['tmp'], 'plain', 'scores.json'))


def test_scores_equal_the_ragged_call_and_the_oracle():
    from utils import bss_eval as hb
    r = _runs()
    refs, mixes, tracks = _data('scored')
    sc = json.load(open(os.path.join(r['tmp'], 'scored', 'scores.json')))
    assert sc['sets'] == ['mixture', 'separated'] and sc['scored'] == len(LENGTHS)
    assert [e['samples'] for e in sc['recordings']] == LENGTHS and [e['info'] for e in sc['recordings']] == [0] * len(LENGTHS)
    ests = [np.stack([np.stack([m] * S), t]) for m, t in zip(mixes, tracks)]
    sdr, sir, sar, perm = hb.bss_eval_sources_ragged(refs, ests)
    vals = np.empty((len(LENGTHS), 2, 3, S))
    for i, e in enumerate(sc['recordings']):
        for k, name in enumerate(sc['sets']):
            _check_set(e, name, sdr[i, k], sir[i, k], sar[i, k], perm[i, k])
            o = obss.bss_eval_sources(refs[i].astype(np.float64), ests[i][k].astype(np.float64))
            _check_set(e, name, *o[:4])
            vals[i, k] = o[:3]
    m = vals.mean(axis=(0, 3))
    for k, name in enumerate(sc['sets']):
        for j, c in enumerate(('sdr', 'sir', 'sar')):
            assert abs(sc['means'][name][c] - m[k, j]) < 2 * TOL_DB
    assert abs(sc['improvement']['separated']['sdr'] - (m[1, 0] - m[0, 0])) < 4 * TOL_DB


def test_both_clusterings_are_three_sets_of_one_call():
    from experiments.evaluation import separate_many as many
    from tests.test_gpu_separate_clustered import _fresh_model
    from utils import bss_eval as hb
    r = _runs()
    refs, mixes, tracks = _data('both')
    sc = json.load(open(os.path.join(r['tmp'], 'both', 'scores.json')))
    assert sc['sets'] == ['mixture', 'chunk', 'recording'] and sc['scored'] == len(LENGTHS)
    one_set = json.load(open(os.path.join(r['tmp'], 'scored', 'scores.json')))
    for a, b in zip(sc['recordings'], one_set['recordings']):                 # the written clustering ('chunk'): the sets share the Gram matrices
        assert a['sets']['mixture'] == b['sets']['mixture'] and a['sets']['chunk'] == b['sets']['separated']
    # the third set: the tracks clustering='recording' gives AFTER the chunk pass (the order in which the command line draws its seeds)
    argv = ['--model_folder', _front(None)[2], '--sortofmodel', 'front_DPCL', '--chunk_size', str(L), '--batch_size', str(B), '--nb_speakers', str(S),
            '--nb_tries', str(TRIES), '--nb_steps', str(STEPS), '--no_summaries', '--output_dir', 'unused', '--inputs', 'unused.wav']
    tr, model, _ = _fresh_model(many, argv)
    with tr.graph.as_default():
        model.separate_recordings(mixes, clustering='chunk')
        rec = [many.as_written(o.cpu().numpy(), False) for o in model.separate_recordings(mixes, clustering='recording')]
    ests = [np.stack([np.stack([m] * S), t, q]) for m, t, q in zip(mixes, tracks, rec)]
    sdr, sir, sar, perm = hb.bss_eval_sources_ragged(refs, ests)
    for i, e in enumerate(sc['recordings']):
        for k, name in enumerate(sc['sets']):
            _check_set(e, name, sdr[i, k], sir[i, k], sar[i, k], perm[i, k])
