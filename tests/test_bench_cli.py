"""bench.py launcher contract (CPU): `--gpus N` without a launcher re-executes the command under torch.distributed.run with N ranks
on 127.0.0.1; with a launcher present it never re-spawns."""
import importlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_gpus_flag_spawns_that_many_ranks(monkeypatch):
    sys.path.insert(0, ROOT)
    bench = importlib.import_module('bench')
    seen = {}

    def fake_call(cmd, env=None):
        seen['cmd'], seen['env'] = cmd, env
        return 0
    import subprocess
    monkeypatch.setattr(subprocess, 'call', fake_call)
    monkeypatch.setattr(sys, 'argv', ['bench.py', '--gpus', '4', '--steps', '7', '--warmup', '2'])
    for k in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK'):
        monkeypatch.delenv(k, raising=False)
    try:
        bench.main()
    except SystemExit as e:
        assert e.code == 0
    cmd = seen['cmd']
    assert cmd[1:3] == ['-m', 'torch.distributed.run']
    assert cmd[cmd.index('--nproc-per-node') + 1] == '4' and cmd[cmd.index('--master-addr') + 1] == '127.0.0.1'
    assert cmd[-6:] == ['--gpus', '4', '--steps', '7', '--warmup', '2'] and cmd[-7].endswith('bench.py')
    assert seen['env']['HSA_ENABLE_IPC_MODE_LEGACY'] == '0'


def test_dump_outputs_keeps_to_its_budget_and_samples_the_same_entries(tmp_path, monkeypatch):
    """--dump-outputs: the cost as float64, every variable as float32 under its name; past the budget, the large variables become
    a fixed sample (same entries on every call) and the files together stay within it."""
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    bench = importlib.import_module('bench')

    class Var(object):
        def __init__(self, name, t):
            self.ams_name, self.t = name, t

        def detach(self):
            return self.t
    gen = torch.Generator().manual_seed(0)
    vs = [Var('prediction/W', torch.rand(600, 1000, generator=gen)), Var('prediction/b', torch.rand(1000, generator=gen)),
          Var('prediction/forward_BLSTM_0/rnn/basic_lstm_cell/kernel', torch.rand(556, 1200, generator=gen))]
    whole = tmp_path / 'whole'
    bench.dump_outputs(str(whole), 1.25, vs)
    assert np.load(str(whole / 'cost.npy')).dtype == np.float64 and float(np.load(str(whole / 'cost.npy'))[0]) == 1.25
    for v in vs:
        a = np.load(str(whole / (v.ams_name.replace('/', '.') + '.npy')))
        assert a.dtype == np.float32 and np.array_equal(a, v.t.numpy())
    monkeypatch.setattr(bench, 'DUMP_BUDGET_BYTES', 2 * 10 ** 6)
    runs = []
    for k in range(2):
        d = tmp_path / ('cut%d' % k)
        bench.dump_outputs(str(d), 1.25, vs)
        runs.append({p.name: np.load(str(p)) for p in d.iterdir()})
        assert sum(p.stat().st_size for p in d.iterdir()) <= 2 * 10 ** 6
    assert sorted(runs[0]) == sorted(runs[1]) and all(np.array_equal(runs[0][n], runs[1][n]) for n in runs[0])
    assert np.array_equal(runs[0]['prediction.b.npy'], vs[1].t.numpy())           # small enough to stay whole
    W = runs[0]['prediction.W.npy']
    assert W.ndim == 1 and W.size < 600 * 1000 and np.isin(W, vs[0].t.numpy()).all()
