"""CPU: the index planner of data/resident.py against the host record pipeline (data/dataset.py), the pool layout, and the header."""
import os

import numpy as np
import pytest

from ams_hip import _lib
from data import tfrecord


def write_split(folder, split, L, seed=0, per_file=10):
    """{split}_{M,F}.tfrecords with ~10 utterances each.  Lengths: shorter than L, exactly L (the strict filter drops it), L + 1,
    exactly 3 L, odd ones.  Keys repeat inside a file and ACROSS the files, so the distinct-speaker filter has tuples to drop."""
    rng = np.random.RandomState(seed)
    lens = [L - 7, L, L + 1, 3 * L, 2 * L + 3, 5 * L + 1, 4 * L - 1, 3 * L + 5, 6 * L + 7, 2 * L + 1][:per_file]
    for g, keys in (('M', [0, 1, 2, 0, 3, 1, 4, 5, 2, 0]), ('F', [100, 1, 101, 0, 102, 100, 2, 103, 104, 101])):
        items = [((0.05 * rng.randn(n) + 0.01).astype(np.float32), keys[i]) for i, n in enumerate(lens)]
        tfrecord.write_audio_records(os.path.join(str(folder), '%s_%s.tfrecords' % (split, g)), items)


def host_batches(folder, split, sex, S, L, B, normalize, nrp, epoch, drop):
    from data.dataset import record_mixture_stream
    return list(record_mixture_stream(str(folder), split, sex, S, L, B, normalize, nrp, epoch, drop))


def materialize(rec, plan, L):
    """non_mix [n, S, L] of a plan [n, S, 2] from the host copy of the pool (ResidentRecords(device=None))."""
    out = np.empty(plan.shape[:2] + (L,), dtype=np.float32)
    for j in range(plan.shape[0]):
        for s in range(plan.shape[1]):
            o = int(rec.utt_off[plan[j, s, 0]]) + int(plan[j, s, 1]) * L
            out[j, s] = rec.host_pool[o:o + L]
    return out


BRANCHES = {'alternate': (['M', 'F'], True), 'combos': (['M', 'F'], False), 'single': (['F'], True)}


@pytest.mark.parametrize('L', [256, 250])
@pytest.mark.parametrize('normalize', [False, True])
@pytest.mark.parametrize('S', [1, 2, 3, 6])
def test_plan_is_the_pipeline(tmp_path, S, normalize, L):
    from data import resident
    write_split(tmp_path, 'train', L)
    rec = resident.ResidentRecords(str(tmp_path), 'train', normalize, None)
    B = 4
    dropped = 0
    for branch, (sex, nrp) in BRANCHES.items():
        for epoch in (0, 1):
            for drop in (False, True):
                ref = host_batches(tmp_path, 'train', sex, S, L, B, normalize, nrp, epoch, drop)
                plan = resident.plan_pass(rec, sex, S, L, B, nrp, epoch, drop)
                dropped += plan.dropped
                assert plan.nb_batches == len(ref), (branch, epoch, drop)
                assert plan.table.dtype == np.int32 and plan.keys.dtype == np.int32
                nm = materialize(rec, plan.table, L)
                for k, (mix, non_mix, ind) in enumerate(ref):
                    first, size = plan.batch(k)
                    assert size == mix.shape[0], (branch, epoch, drop, k)
                    got = nm[first:first + size]
                    assert np.array_equal(got, non_mix), (branch, epoch, drop, k)
                    assert np.array_equal(np.stack([g.sum(axis=0) for g in got]), mix)
                    assert np.array_equal(plan.keys[first:first + size], ind) and ind.dtype == plan.keys.dtype
                if ref and not drop:
                    assert plan.n == sum(b[0].shape[0] for b in ref)
                if drop:
                    assert plan.n % B == 0
    if S > 1:
        assert dropped >= 1                                              # the distinct-speaker filter had work to do


def test_short_last_batch_and_strict_length_filter(tmp_path):
    from data import resident
    L = 256
    write_split(tmp_path, 'train', L)
    rec = resident.ResidentRecords(str(tmp_path), 'train', False, None)
    plan = resident.plan_pass(rec, ['M'], 1, L, 4, True, 0, False)
    # per file: lengths L-7 and L give nothing; L+1 -> 1, 3L -> 3, 2L+3 -> 2, 5L+1 -> 5, 4L-1 -> 3, 3L+5 -> 3, 6L+7 -> 6, 2L+1 -> 2
    assert plan.n == 25 and plan.nb_batches == 7 and plan.batch(6) == (24, 1)
    used = set(int(u) for u in plan.table[:, 0, 0])
    assert 0 not in used and 1 not in used                              # shorter than L; exactly L
    assert resident.plan_pass(rec, ['M'], 1, L, 4, True, 0, True).n == 24


def test_pool_layout_and_plan_validation(tmp_path):
    from data import resident
    L = 250
    write_split(tmp_path, 'valid', L)
    rec = resident.ResidentRecords(str(tmp_path), 'valid', False, None)
    assert rec.lengths.shape == (20,) and rec.ids['M'] == list(range(10)) and rec.ids['F'] == list(range(10, 20))
    assert np.all(rec.utt_off % 4 == 0) and rec.utt_off.dtype == np.int64
    assert np.all(rec.utt_off[1:] >= rec.utt_off[:-1] + rec.lengths[:-1])           # no overlap
    assert rec.pool_floats >= int(rec.utt_off[-1] + rec.lengths[-1]) and rec.pool_bytes == 4 * rec.pool_floats
    audio = [a for g in 'MF' for a, _ in tfrecord.read_audio_records(os.path.join(str(tmp_path), 'valid_%s.tfrecords' % g))]
    for u, a in enumerate(audio):
        assert np.array_equal(rec.host_pool[rec.utt_off[u]:rec.utt_off[u] + a.shape[0]], a)
    # utterance 3 has exactly 3 L samples: chunks 0..2 exist, chunk 3 does not; utterance 2 (L + 1) has chunk 0 only
    rec.validate(np.array([[[3, 2], [2, 0]]], np.int32), L)
    for bad in ([[3, 3]], [[2, 1]], [[0, 0]], [[20, 0]], [[-1, 0]], [[3, -1]]):
        with pytest.raises(ValueError):
            rec.validate(np.array([bad], np.int32), L)
    os.remove(os.path.join(str(tmp_path), 'valid_F.tfrecords'))
    with pytest.raises(IOError):                                                      # a gender without a file is an error, not silence
        resident.plan_pass(resident.ResidentRecords(str(tmp_path), 'valid', False, None), ['M', 'F'], 2, L, 4)


def test_normalised_pool_holds_the_pipeline_values(tmp_path):
    from data import resident
    write_split(tmp_path, 'test', 256)
    rec = resident.ResidentRecords(str(tmp_path), 'test', True, None)
    for u, (a, _) in enumerate(tfrecord.read_audio_records(os.path.join(str(tmp_path), 'test_M.tfrecords'))):
        want = (a - a.mean()) / np.sqrt(a.var())
        assert want.dtype == np.float32 and np.array_equal(rec.host_pool[rec.utt_off[u]:rec.utt_off[u] + a.shape[0]], want)


def test_header_and_abi():
    protos = _lib.parse_header()
    assert 'ams_mix_gather' in protos
    ret, args = protos['ams_mix_gather']
    import ctypes
    assert ret is ctypes.c_int32 and len(args) == 12 and args[4] is ctypes.c_long and args[8:11] == [ctypes.c_int] * 3
    assert _lib.ABI_VERSION == 10
    assert '#define AMS_ABI_VERSION 10' in open(_lib.HEADER_PATH).read()


def test_mix_gather_refuses_cpu_tensors():
    torch = pytest.importorskip('torch')
    from ams_hip import ops, AmsError
    with pytest.raises(AmsError):
        ops.mix_gather(torch.zeros(16), torch.zeros(1, dtype=torch.int64), torch.zeros((1, 1, 2), dtype=torch.int32),
                       torch.zeros((1, 1), dtype=torch.int32), 0, 1, 4)


def test_mix_kernels_compile_for_gfx950_without_scratch():
    """tools/kernel_resources.py on csrc/mix.hip: twelve variants (S = 1 .. 6, vector and scalar arm), no scratch, no LDS, no warning."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    run = subprocess.run([sys.executable, os.path.join(root, 'tools', 'kernel_resources.py'),
                          os.path.join(root, 'adaptive-multispeaker-separation_amd', 'csrc', 'mix.hip')],
                         capture_output=True, text=True, check=True)
    assert 'warning' not in run.stderr
    out = run.stdout.splitlines()
    rows = [ln.split() for ln in out[1:] if 'mix_gather_kernel' in ln]
    names = ' '.join(out[1:])
    for S in range(1, 7):
        for vec in ('true', 'false'):
            assert 'mix_gather_kernel<%d, %s>' % (S, vec) in names, (S, vec)
    assert len(rows) == 12
    for r in rows:
        vgpr, agpr, spill, scratch, occ, lds = r[-6:]
        assert spill == '0' and scratch == '0' and lds == '0', r


def test_no_getenv_in_mix_source():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    assert 'getenv' not in open(os.path.join(root, 'adaptive-multispeaker-separation_amd', 'csrc', 'mix.hip')).read()
