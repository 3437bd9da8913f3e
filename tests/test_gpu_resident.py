"""GPU: the device-resident record path (csrc/mix.hip, data/resident.py, TFDataset(resident=True)) against the host pipeline.
Everything is compared bit for bit: the kernel copies chunks and adds them in numpy's order."""
import ctypes
import os
import tempfile

import numpy as np
import pytest

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

from tests.test_resident_host import BRANCHES, host_batches, write_split

os.environ.setdefault('AMS_LOG_DIR', tempfile.mkdtemp(prefix='ams_log_'))
B = 4


def _equal(got, ref):
    """device (mix, non_mix, ind) == host (mix, non_mix, ind), values, shapes and dtypes."""
    return all(g.dtype == torch.from_numpy(r).dtype and torch.equal(g.cpu(), torch.from_numpy(r)) for g, r in zip(got, ref))


@pytest.mark.parametrize('L', [256, 250])
@pytest.mark.parametrize('S', [1, 2, 3, 6])
def test_kernel_matches_host_pipeline(tmp_path, S, L):
    from data import resident
    from models.network import Network
    write_split(tmp_path, 'train', L)
    dropped = 0
    for normalize in (False, True):
        rec = resident.ResidentRecords(str(tmp_path), 'train', normalize, 'cuda')
        assert rec.pool.data_ptr() % 16 == 0 and rec.host_pool is None
        for branch, (sex, nrp) in BRANCHES.items():
            for epoch in (0, 1):
                for drop in (False, True):
                    ref = host_batches(tmp_path, 'train', sex, S, L, B, normalize, nrp, epoch, drop)
                    plan = resident.plan_pass(rec, sex, S, L, B, nrp, epoch, drop)
                    dropped += plan.dropped
                    assert plan.nb_batches == len(ref)
                    for k, r in enumerate(ref):
                        got = resident.gather(rec, plan, k)
                        assert _equal(got, r), (normalize, branch, epoch, drop, k)
                        assert Network._back_to_back(got[0], got[1])
                        if L == 256:
                            assert got[0].data_ptr() % 16 == 0
                    if ref and not drop:
                        assert ref[-1][0].shape[0] == plan.n - (len(ref) - 1) * B       # the short final batch came through
    assert S == 1 or dropped >= 1


@pytest.mark.parametrize('L', [256, 250])
def test_fenced_batch(tmp_path, L):
    """One pass inside red zones with NaN-filled outputs: L = 256 the vector arm, L = 250 the scalar arm."""
    from ams_hip import ops
    from data import resident
    from tests.fenced import Fence
    S = 3
    write_split(tmp_path, 'train', L)
    host = resident.ResidentRecords(str(tmp_path), 'train', False, None)
    # the alternating branch: 18 examples here, so the pass ends on a short batch (the 2^S round robin always yields a multiple of 8)
    ref = host_batches(tmp_path, 'train', ['M', 'F'], S, L, B, False, True, 0, False)
    plan = resident.plan_pass(host, ['M', 'F'], S, L, B, True, 0, False)
    assert len(ref) >= 2 and ref[-1][0].shape[0] < B
    with Fence() as fence:
        pool = fence.dev(host.host_pool)
        off = fence.dev(host.utt_off, dtype=np.int64)
        table = fence.dev(plan.table, dtype=np.int32)
        keys = fence.dev(plan.keys, dtype=np.int32)
        for k, r in enumerate(ref):
            first, size = plan.batch(k)
            got = ops.mix_gather(pool, off, table, keys, first, size, L)
            assert not any(bool(torch.isnan(t).any()) for t in got[:2])
            assert _equal(got, r), k
        fence.check()


def _direct(L, S, nb, pool_base=0, odd_rows=False, fence=None, seed=0):
    """The kernel on a hand-made pool: (got, want) for a batch of nb examples taken from the middle of a longer plan."""
    from ams_hip import ops
    rng = np.random.RandomState(seed)
    U, n, first = 5, nb + 5, 3
    lengths = rng.randint(L, 4 * L, U)
    step = (lengths + 3) // 4 * 4 + (np.arange(U) % 4 if odd_rows else 0)         # odd_rows: utterances at any 4-byte boundary
    off = np.concatenate([[2 if odd_rows else 0], np.cumsum(step)[:-1]]).astype(np.int64)
    pool = rng.randn(int(off[-1] + lengths[-1])).astype(np.float32)
    table = np.zeros((n, S, 2), np.int32)
    table[:, :, 0] = rng.randint(0, U, (n, S))
    table[:, :, 1] = rng.randint(0, 1 << 20, (n, S)) % (lengths[table[:, :, 0]] // L)
    keys = rng.randint(0, 1000, (n, S)).astype(np.int32)
    rows = np.stack([[pool[off[u] + c * L: off[u] + (c + 1) * L] for u, c in ex] for ex in table[first:first + nb]])
    want = (np.stack([np.stack(list(r)).sum(axis=0) for r in rows]), rows, keys[first:first + nb])
    if fence is not None:
        dev = (fence.dev(pool, base=pool_base), fence.dev(off, dtype=np.int64), fence.dev(table, dtype=np.int32), fence.dev(keys, dtype=np.int32))
    else:
        assert pool_base == 0
        dev = tuple(torch.from_numpy(a).cuda() for a in (pool, off, table, keys))
    return ops.mix_gather(dev[0], dev[1], dev[2], dev[3], first, nb, L), want


@pytest.mark.parametrize('L,S,pool_base,odd_rows', [(2052, 2, 0, False),      # vector arm, 3 blocks along L, one live thread in the last
                                                    (2052, 6, 0, True),       # vector stores, chunks off the 16-byte grid: dword loads
                                                    (2052, 3, 4, False),      # pool base off the 16-byte grid: scalar arm
                                                    (2050, 6, 0, False),      # scalar arm, 3 blocks, ragged tail
                                                    (1024, 1, 0, False), (1, 2, 0, False)])
def test_kernel_blocks_and_alignments_fenced(L, S, pool_base, odd_rows):
    from tests.fenced import Fence
    with Fence() as fence:
        got, want = _direct(L, S, 5, pool_base, odd_rows, fence)
        assert _equal(got, want)
        fence.check()


def test_pool_offsets_past_2_31_floats():
    """Offsets are 64-bit end to end: an utterance that starts past 2^31 floats (8.6 GB into the pool; only its samples are written)."""
    from ams_hip import ops
    L, S = 256, 2
    base = (1 << 31) + 8
    pool = torch.empty(base + 4 * L, dtype=torch.float32, device='cuda')
    audio = np.random.RandomState(1).randn(4 * L).astype(np.float32)
    pool[base:] = torch.from_numpy(audio).cuda()
    pool[:4 * L] = 0.0                                                      # what a 32-bit offset would reach
    off = torch.tensor([base], dtype=torch.int64, device='cuda')
    table = torch.tensor([[[0, 3], [0, 1]], [[0, 2], [0, 0]]], dtype=torch.int32, device='cuda')
    keys = torch.tensor([[7, 8], [9, 10]], dtype=torch.int32, device='cuda')
    mix, non_mix, ind = ops.mix_gather(pool, off, table, keys, 0, 2, L)
    rows = np.stack([[audio[c * L:(c + 1) * L] for c in cs] for cs in ((3, 1), (2, 0))])
    assert _equal((mix, non_mix, ind), (rows.sum(axis=1), rows, np.array([[7, 8], [9, 10]], np.int32)))


def test_bad_arguments_are_refused_before_any_launch():
    from ams_hip import ops, AmsError, load
    lib = load()
    L = 16
    pool = torch.arange(64, dtype=torch.float32, device='cuda')
    off = torch.zeros(1, dtype=torch.int64, device='cuda')
    table = torch.zeros((2, 7, 2), dtype=torch.int32, device='cuda')
    keys = torch.zeros((2, 7), dtype=torch.int32, device='cuda')
    mix = torch.full((2 * L,), -1.0, device='cuda')
    non_mix = torch.full((2 * 7 * L,), -1.0, device='cuda')
    ind = torch.full((2 * 7,), -1, dtype=torch.int32, device='cuda')
    p = [t.data_ptr() for t in (pool, off, table, keys)]
    o = [t.data_ptr() for t in (mix, non_mix, ind)]
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call(ptrs_in, outs, Bn, S, Ln, first=0):
        return lib.ams_mix_gather(*[ctypes.c_void_p(x) for x in ptrs_in], first, *[ctypes.c_void_p(x) for x in outs], Bn, S, Ln, st)
    assert call(p, o, 2, 0, L) == -1 and call(p, o, 2, 7, L) == -1            # AMS_E_INVALID_ARG
    assert call(p, o, 0, 2, L) == -1 and call(p, o, 2, 2, 0) == -1 and call(p, o, 2, 2, L, first=-1) == -1
    for i in range(4):
        assert call(p[:i] + [0] + p[i + 1:], o, 2, 2, L) == -1
    for i in range(3):
        assert call(p, o[:i] + [0] + o[i + 1:], 2, 2, L) == -1
    torch.cuda.synchronize()
    assert bool((mix == -1).all()) and bool((non_mix == -1).all()) and bool((ind == -1).all())       # nothing ran
    assert call(p, o, 2, 2, L) == 0                                          # the same buffers, valid sizes: it does run
    torch.cuda.synchronize()
    assert bool((mix[:L] == 2 * pool[:L]).all())
    with pytest.raises(AmsError):                                            # a window past the plan's end
        ops.mix_gather(pool, off, table[:, :2].contiguous(), keys[:, :2].contiguous(), 1, 2, L)
    with pytest.raises(AmsError):
        ops.mix_gather(pool, off, table, keys, 0, 2, L)                      # S = 7 through the wrapper


# ---------------------------------------------------------------------------------------------------------------- TFDataset
class _Dist(object):
    def __init__(self, world_size, rank):
        self.world_size, self.rank = world_size, rank


def _pair(monkeypatch, folder, S=2, L=256, **kw):
    """Two TFDataset objects over the same files: (host path, resident path)."""
    from ams_hip.graph import Graph
    from data.dataset import TFDataset
    monkeypatch.setenv('AMS_DATA_DIR', str(folder))
    monkeypatch.delenv('AMS_DATA_RESIDENT', raising=False)
    out = []
    for resident in (False, True):
        with Graph().as_default():
            out.append(TFDataset(batch_size=B, nb_speakers=S, chunk_size=L, dataset='records', resident=resident, **kw))
    assert out[1].resident and not out[0].resident
    return out


def _next(ds, split, L):
    """One _next call: the batch, or None at StopIteration."""
    from ams_hip.graph import Run
    try:
        return ds._next(Run({ds.handle: split, ds.chunk_size: L}, new_pass=False))
    except StopIteration:
        return None


def _same_call(host, res, split, L):
    a, b = _next(host, split, L), _next(res, split, L)
    assert (a is None) == (b is None)
    if a is not None:
        assert all(x.dtype == y.dtype and x.device == y.device and torch.equal(x, y) for x, y in zip(a, b))
    return a is not None


def _files(folder, L):
    for split in ('train', 'valid', 'test', 'test_other'):
        write_split(folder, split, L, seed=len(split))


@pytest.mark.parametrize('nrp', [False, True])
def test_tfdataset_sequence(tmp_path, monkeypatch, nrp):
    L = 256
    _files(tmp_path, L)
    host, res = _pair(monkeypatch, tmp_path, no_random_picking=nrp, dataset_normalize=nrp)
    assert host.length(host.TRAIN) == res.length(res.TRAIN) >= 2
    assert host.length(host.VALID) == res.length(res.VALID) >= 1
    for init in range(2):                                     # two initialisations of TRAIN: the second pass is reshuffled
        host.initialize(host.TRAIN)
        res.initialize(res.TRAIN)
        calls = 0
        while _same_call(host, res, 'train', L):             # past length(): up to StopIteration, which falls at the same call
            calls += 1
        assert calls >= host.length(host.TRAIN) - 1
        assert not _same_call(host, res, 'train', L)
    host.initialize(host.VALID)
    res.initialize(res.VALID)
    while _same_call(host, res, 'valid', L):
        pass
    # another chunk size fed mid-way: the running pass keeps its own, the roll-over and the next initialisation take the fed one
    host.initialize(host.TRAIN)
    res.initialize(res.TRAIN)
    assert _same_call(host, res, 'train', L) and _same_call(host, res, 'train', 250) and _same_call(host, res, 'train', 250)
    host.initialize(host.TRAIN)
    res.initialize(res.TRAIN)
    n = 0
    while _same_call(host, res, 'train', 250):
        n += 1
    assert n >= 2
    assert host.cursor == res.cursor and host._epochs == res._epochs


def test_tfdataset_environment_switch_and_synthetic(tmp_path, monkeypatch):
    from ams_hip.graph import Graph
    from data.dataset import TFDataset
    _files(tmp_path, 256)
    monkeypatch.setenv('AMS_DATA_DIR', str(tmp_path))
    monkeypatch.setenv('AMS_DATA_RESIDENT', '1')
    with Graph().as_default():
        assert TFDataset(batch_size=B, nb_speakers=2, chunk_size=256, dataset='records').resident
        assert not TFDataset(batch_size=B, nb_speakers=2, chunk_size=256, dataset='records', resident=False).resident
        assert not TFDataset(batch_size=B, nb_speakers=2, chunk_size=256, dataset='synthetic').resident
        assert not TFDataset(batch_size=B, nb_speakers=2, chunk_size=256, dataset='synthetic', resident=True).resident


@pytest.mark.parametrize('rank', [0, 1])
def test_data_parallel_indexing(tmp_path, monkeypatch, rank):
    """world_size = 2 through a stub: rank r keeps batch 2 k + r of the pass, short batches are dropped, length() is halved."""
    L = 256
    _files(tmp_path, L)
    host, res = _pair(monkeypatch, tmp_path, dist=_Dist(2, rank))
    single = _pair(monkeypatch, tmp_path)[1]
    assert host.length(host.TRAIN) == res.length(res.TRAIN) >= 1
    host.initialize(host.TRAIN)
    res.initialize(res.TRAIN)
    single.initialize(single.TRAIN)
    first, first_host = _next(res, 'train', L), _next(host, 'train', L)
    alone = [_next(single, 'train', L) for _ in range(2)]
    assert all(torch.equal(x, y) and torch.equal(x, z) for x, y, z in zip(first, alone[rank], first_host))
    while _same_call(host, res, 'train', L):
        pass
    host.initialize(host.TRAIN)
    res.initialize(res.TRAIN)
    while _same_call(host, res, 'train', L):
        pass


# ---------------------------------------------------------------------------------------------------------------- training
def _trainer(tmp_path, tag, resident, graph):
    import utils.ops
    from ams_hip import testing
    from models.dpcl import DPCL
    from utils.trainer import Front_Separator_Trainer
    L, Bt, S = 1024, 3, 2
    utils.ops.rng.seed(42)
    torch.manual_seed(0)
    folder, params = testing.make_pretrained_adapt(os.path.join(str(tmp_path), 'pre_' + tag), window_size=64, filters=16, hop_size=16,
                                                   chunk_size=L, batch_size=Bt, nb_speakers=S)
    a = dict(params)
    a.update(testing.SEPARATOR_DEFAULTS)
    a.update(layer_size=12, nb_layers=2, embedding_size=8, model_folder=folder, model_previous=None, pretraining=False,
             learning_rate=1e-3, dataset='h5py_files/train-clean-100-8-s.h5', no_summaries=True, resident=resident, hip_graph=graph)
    a.pop('type')
    tr = Front_Separator_Trainer(DPCL, 'front_DPCL', **a)
    dist, tfds = tr.prepare()
    assert tfds.resident == resident
    return tr, tfds, L


def _train(tr, tfds, L, steps):
    tfds.initialize(tfds.TRAIN)
    with tr.graph.as_default():
        feed = {tfds.handle: tfds.get_handle(tfds.TRAIN), tfds.chunk_size: L}
        costs = [float(tr.model.train(feed, i)) for i in range(steps)]
    torch.cuda.synchronize()
    return costs


def test_training_step_resident_equals_host(tmp_path, monkeypatch):
    """The tiny front_DPCL setup of test_gpu_step.py::test_training_from_tfrecord_files.  Eager: same inputs, same kernels -- the
    costs of three steps are bit-equal.  --hip_graph: the resident batch is back to back, so the captured step stages it with the one
    fused launch (which leaves the waveforms' bound on the static buffer), and agrees with the eager run as replay does elsewhere
    (tests/test_gpu_replay.py: rtol 1e-5)."""
    from ams_hip import ops
    L = 1024
    rng = np.random.RandomState(3)
    for split in ('train', 'valid', 'test', 'test_other'):
        for g_, base in (('M', 0), ('F', 100)):
            from data import tfrecord
            tfrecord.write_audio_records(str(tmp_path / ('%s_%s.tfrecords' % (split, g_))),
                                         [((0.05 * rng.randn(rng.randint(L + 1, 4 * L))).astype(np.float32), base + i) for i in range(10)])
    monkeypatch.setenv('AMS_DATA_DIR', str(tmp_path))
    monkeypatch.delenv('AMS_DATA_RESIDENT', raising=False)
    steps = 4
    tr, tfds, _ = _trainer(tmp_path, 'host', False, False)
    assert tfds.length(tfds.TRAIN) >= steps + 1                  # so that dropping the remainder under --hip_graph leaves `steps` batches
    c_host = _train(tr, tfds, L, steps)
    tr, tfds, _ = _trainer(tmp_path, 'res', True, False)
    c_res = _train(tr, tfds, L, steps)
    print('eager costs host', c_host, 'resident', c_res)
    assert np.all(np.isfinite(c_host)) and c_res == c_host
    tr, tfds, _ = _trainer(tmp_path, 'graph', True, True)
    c_graph = _train(tr, tfds, L, steps)
    print('graph costs', c_graph)
    assert np.all(np.isfinite(c_graph))
    static = tr.model._cg_state['static']
    assert hasattr(static[0], '_ams_x_amax')                     # only the fused staging launch sets it
    if ops.F16X3:
        am = static[0]._ams_x_amax
        assert am is not None and float(am) == float(max(static[0].abs().max(), static[1].abs().max()))
    assert np.allclose(c_res, c_graph, rtol=1e-5, atol=0), (c_res, c_graph)
