"""GPU: experiments/evaluation/separate_many.py --speakers auto --reference_dir R --metric si_sdr on the tiny random-weight
three-speaker model of tests/test_gpu_separate_counted.py: three short recordings, two with 2 true sources and one with 3, counted,
written and scored by ONE ragged SI-SDR call.  scores.json is held to utils.bss_eval.si_sdr_ragged on the tracks as written and read
back (exactly) and to the restatement tests/sisdr_ref.py (the project's dB rule; the matchings exactly, under the asserted gap
condition); count_accuracy and the confusion table to counts.json; scoring changes no written byte; the default metric writes the
keys it wrote before."""
import json
import os
import tempfile

import numpy as np
import pytest

from tests import sisdr_ref as ref

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

from tests.bss_common import close_db
from tests.test_gpu_separate_counted import B, L, S, STEPS, TRIES, _front3
from tests.test_gpu_separate_recording import _recording
from tests.test_gpu_separate_recordings import LENGTHS

TRUE = [2, 3, 2]                 # true sources per recording
MIN_GAP_DB = 1e-3
_RUNS = {}


def _runs():
    """The command line on the same inputs (built once): counted without scoring, counted and scored by si_sdr, and the recording with
    S true sources at fixed S under the default metric."""
    if not _RUNS:
        from experiments.evaluation import separate as one
        from experiments.evaluation import separate_many as many
        _, folder = _front3()
        tmp = tempfile.mkdtemp(prefix='ams_score_cnt_')
        refd = os.path.join(tmp, 'refs')
        os.makedirs(refd)
        stems = ['rec%d' % r for r in range(len(LENGTHS))]
        for r, (stem, N) in enumerate(zip(stems, LENGTHS)):
            srcs = [0.4 * _recording(N, 90 + 10 * r + k) for k in range(TRUE[r])]
            paths = one.write_outputs(os.path.join(refd, stem), np.stack(srcs), False, None)
            one.write_wav(os.path.join(tmp, stem + '.wav'), sum(one.read_input(p) for p in paths))      # the mixture of the WRITTEN sources
        model = ['--model_folder', folder, '--sortofmodel', 'front_DPCL', '--chunk_size', str(L), '--batch_size', str(B), '--nb_speakers', str(S),
                 '--nb_tries', str(TRIES), '--nb_steps', str(STEPS), '--hop', '1280', '--no_summaries']
        inputs = ['--inputs'] + [os.path.join(tmp, s + '.wav') for s in stems]
        counted = ['--clustering', 'recording', '--speakers', 'auto']
        _RUNS.update(stems=stems, tmp=tmp, refd=refd)
        _RUNS['plain'] = many.main(model + inputs + counted + ['--output_dir', os.path.join(tmp, 'plain')])
        _RUNS['scored'] = many.main(model + inputs + counted + ['--output_dir', os.path.join(tmp, 'scored'), '--reference_dir', refd,
                                                                 '--metric', 'si_sdr'])
        _RUNS['fixed'] = many.main(model + ['--inputs', os.path.join(tmp, 'rec1.wav'), '--output_dir', os.path.join(tmp, 'fixed'),
                                            '--reference_dir', refd])
    return _RUNS


def _null(v):
    """numbers as scores.json holds them: non-finite -> None."""
    return [None if not np.isfinite(a) else float(a) for a in v]


def _arr(v):
    return np.array([np.nan if a is None else a for a in v], np.float64)


def test_scoring_changes_no_written_byte():
    r = _runs()
    assert [os.path.basename(p) for p in r['scored'][:-1]] == [os.path.basename(p) for p in r['plain']]
    assert os.path.basename(r['plain'][-1]) == 'counts.json' and r['scored'][-1] == os.path.join(r['tmp'], 'scored', 'scores.json')
    for p, q in zip(r['plain'], r['scored']):
        raw = open(p, 'rb').read()
        assert raw == open(q, 'rb').read() and len(raw) > 44
    assert not os.path.exists(os.path.join(r['tmp'], 'plain', 'scores.json'))


def test_scores_are_the_ragged_call_and_the_restatement():
    from experiments.evaluation import separate as one
    from utils.bss_eval import si_sdr_ragged
    r = _runs()
    sc = json.load(open(os.path.join(r['tmp'], 'scored', 'scores.json')))
    cj = json.load(open(os.path.join(r['tmp'], 'scored', 'counts.json')))
    counts = [cj['recordings'][s]['count'] for s in r['stems']]
    assert all(2 <= c <= S for c in counts)
    refs = [np.stack([one.read_input(os.path.join(r['refd'], '%s_%d.wav' % (s, k))) for k in range(t)]) for s, t in zip(r['stems'], TRUE)]
    mixes = [one.read_input(os.path.join(r['tmp'], s + '.wav')) for s in r['stems']]
    tracks = [np.stack([one.read_input(os.path.join(r['tmp'], 'scored', '%s_%d.wav' % (s, k))) for k in range(c)])
              for s, c in zip(r['stems'], counts)]
    assert sc['metric'] == 'si_sdr' and sc['sets'] == ['separated'] and sc['scored'] == 3
    assert [e['samples'] for e in sc['recordings']] == LENGTHS and [e['references'] for e in sc['recordings']] == TRUE
    assert [e['info'] for e in sc['recordings']] == [0, 0, 0]
    got = si_sdr_ragged(refs, tracks, mixes)
    want = ref.score_many(refs, tracks, mixes)
    gaps = [ref.gap(want['pair'][i, 0], counts[i], TRUE[i]) for i in range(3)]
    print('counts %s, gaps between the best and the second-best assignment: %s dB in mean' % (counts, gaps))
    assert min(gaps) > MIN_GAP_DB
    pooled, pooled_i = [], []
    for i, e in enumerate(sc['recordings']):
        Sr, Se, s = TRUE[i], counts[i], e['sets']['separated']
        n = min(Sr, Se)
        # exactly what the call returns, cut to [Se, Sr]
        assert s['tracks'] == Se and e['base'] == _null(got['base'][i, :Sr])
        assert s['pair'] == [_null(row[:Sr]) for row in got['pair'][i, 0, :Se]]
        assert s['si_sdr'] == _null(got['si_sdr'][i, 0, :Sr]) and s['si_sdri'] == _null(got['si_sdri'][i, 0, :Sr])
        assert s['match_ref'] == got['match_ref'][i, 0, :Sr].tolist() and s['match_est'] == got['match_est'][i, 0, :Se].tolist()
        assert s['missed'] == int(got['missed'][i, 0]) == Sr - n and s['spurious'] == int(got['spurious'][i, 0]) == Se - n
        assert (got['match_ref'][i, 0, Sr:] == -1).all() and (got['match_est'][i, 0, Se:] == -1).all()
        # the restatement: the dB rule, the matchings exactly
        assert s['match_ref'] == want['match_ref'][i, 0, :Sr].tolist() and s['match_est'] == want['match_est'][i, 0, :Se].tolist()
        assert np.isfinite(want['pair'][i, 0, :Se, :Sr]).all() and np.isfinite(want['base'][i, :Sr]).all()
        close_db(np.array(s['pair'], np.float64), want['pair'][i, 0, :Se, :Sr])
        close_db(np.array(e['base'], np.float64), want['base'][i, :Sr])
        m = want['match_ref'][i, 0, :Sr] >= 0
        assert np.array_equal(np.isnan(_arr(s['si_sdr'])), ~m)
        close_db(_arr(s['si_sdr'])[m], want['si_sdr'][i, 0, :Sr][m])
        close_db(_arr(s['si_sdri'])[m], want['si_sdri'][i, 0, :Sr][m])
        pooled += want['si_sdr'][i, 0, :Sr][m].tolist()
        pooled_i += want['si_sdri'][i, 0, :Sr][m].tolist()
    assert abs(sc['means']['separated']['si_sdr'] - np.mean(pooled)) < 2e-6 and abs(sc['means']['separated']['si_sdri'] - np.mean(pooled_i)) < 4e-6
    assert sc['missed'] == {'separated': sum(max(t - c, 0) for t, c in zip(TRUE, counts))}
    assert sc['spurious'] == {'separated': sum(max(c - t, 0) for t, c in zip(TRUE, counts))}
    # the counts against the true counts
    assert sc['count_accuracy'] == float(np.mean([c == t for c, t in zip(counts, TRUE)]))
    table = {}
    for c, t in zip(counts, TRUE):
        table.setdefault(str(t), {}).setdefault(str(c), 0)
        table[str(t)][str(c)] += 1
    assert sc['confusion'] == table and sum(n for row in sc['confusion'].values() for n in row.values()) == 3


def test_the_default_metric_writes_the_keys_it_wrote_before():
    r = _runs()
    assert r['fixed'][-1] == os.path.join(r['tmp'], 'fixed', 'scores.json') and len(r['fixed']) == S + 1
    sc = json.load(open(r['fixed'][-1]))
    assert list(sc) == ['flen', 'sets', 'recordings', 'scored', 'means', 'improvement'] and 'metric' not in sc
    assert sc['sets'] == ['mixture', 'separated'] and sc['flen'] == 512
    assert list(sc['recordings'][0]) == ['input', 'samples', 'info', 'sets']
    assert list(sc['recordings'][0]['sets']['separated']) == ['sdr', 'sir', 'sar', 'perm']
