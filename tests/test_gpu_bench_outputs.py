"""GPU: a plain `bench.py` run (no --full) times exactly --steps steps, reports the headline and nothing measured around it, and
with --dump-outputs leaves what its last timed step returned: the cost and the updated trainable variables.  A reduced geometry of
the bench step (batch 4, 4096-sample chunks): this checks the command line, not a number."""
import glob
import json
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_bench_reports_the_headline_and_dumps_the_last_step():
    out = tempfile.mkdtemp(prefix='ams_bench_out_')
    env = dict(os.environ)
    for k in ('RANK', 'LOCAL_RANK', 'WORLD_SIZE', 'MASTER_ADDR', 'MASTER_PORT'):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '1', '--steps', '3', '--warmup', '1', '--batch', '4',
                        '--chunk', '4096', '--dump-outputs', out], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith('{')]
    assert len(lines) == 1, r.stdout[-2000:]
    j = json.loads(lines[0])
    assert j['steps'] == 3 and j['warmup'] == 1 and j['n_gpus'] == 1
    assert j['unit'] == 'mixtures/s' and j['higher_is_better'] is True and j['dtype']
    assert j['ms_per_step'] > 0 and abs(j['value'] - 4 / (j['ms_per_step'] * 1e-3)) <= 1e-2 * j['value']
    for k in ('roofline', 'roofline_hbm', 'north_star_targets', 'secondary', 'value_native_f32', 'cpu_baseline'):
        assert k not in j, k
    cost = np.load(os.path.join(out, 'cost.npy'))
    assert cost.dtype == np.float64 and cost.shape == (1,) and abs(float(cost[0]) - j['final_cost']) <= 1e-6 * abs(j['final_cost'])
    files = [f for f in glob.glob(os.path.join(out, '*.npy')) if not f.endswith('cost.npy')]
    names = set(os.path.basename(f)[:-4] for f in files)
    assert 'prediction.W' in names and 'prediction.b' in names and any('BLSTM' in n for n in names), names
    for f in files:
        a = np.load(f)
        assert a.dtype == np.float32 and a.size and np.isfinite(a).all(), f
    assert sum(os.path.getsize(f) for f in glob.glob(os.path.join(out, '*'))) <= 64 * 10 ** 6
