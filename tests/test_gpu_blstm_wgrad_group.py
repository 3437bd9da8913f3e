"""GPU: the three weight-gradient products of one BLSTM layer as ONE grouped launch (include/ams.h: ams_blstm_bwd_weights_f32).

The reference is float64 numpy written out per utterance (utils/ops.py:358-383 under tf.gradients):
    dWx = sum x^T dz,   dU_f = sum_b sum_{t>=1} h_f[b,t-1]^T dz_f[b,t],   dU_b = sum_b sum_{t<=T-2} h_b[b,t+1]^T dz_b[b,t],   db = colsum(dz)
Shapes (B, T, D, H), the smallest at which each thing can break:
    (3, 7, 36, 20)      everything below one tile, K = 21, one slab: direct stores, column sums finished inside the launch, the
                        utterance-boundary mask at T = 7
    (5, 40, 256, 300)   50 items, K = 200, still one slab
    (13, 80, 256, 300)  K = 1040: several slabs (5 by the split model: 250 items), finishing launch; in a child under AMS_GEMM_SPLITS=8:
                        7 slabs, 350 items, more than resident workgroups -- the persistent walk wraps across regions
    (4, 80, 600, 300)   5 row tiles in the wx region: the shape of layers 2-3
    (64, 80, 256, 300)  the benchmark step's first layer (fp16x3, accumulate; uncapped and capped)
Every shape with accumulate 0 / 1, uncapped / under ops.lds_pad(50000), fp16x3 (bounds from ops.absmax) / bf16x6 (no bounds).
Bounds (tests/test_gpu_gemm_f16.py, its error metric per region): uncapped < 1e-7; capped < max(2 x today's capped launches on the
same data, 2e-7); db relative to the column norms of dz < 1e-6."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

from tests.fenced import Fence
from tests.test_gpu_gemm_f16 import _err

SHAPES = [(3, 7, 36, 20), (5, 40, 256, 300), (13, 80, 256, 300), (4, 80, 600, 300)]
AMS_E_INVALID_ARG = -1


@pytest.fixture(scope='module')
def ops():
    from ams_hip import ops as o
    return o


@functools.lru_cache(maxsize=None)
def _case(B, T, D, H):
    """Seeded inputs and the float64 operands / results of the three regions (computed once per shape, never written)."""
    rng = np.random.RandomState(B * 1000 + T * 10 + D + H)
    x = rng.uniform(-1, 1, (B, T, D)).astype(np.float32)
    h = rng.uniform(-1, 1, (B, T, 2 * H)).astype(np.float32)
    dz = rng.randn(B, T, 8 * H).astype(np.float32)
    dK0 = rng.uniform(-1, 1, (D + H, 8 * H)).astype(np.float32)
    db0 = rng.uniform(-1, 1, (8 * H,)).astype(np.float32)
    x64, h64, z64 = x.astype(np.float64), h.astype(np.float64), dz.astype(np.float64)
    regs = {
        'wx': (x64.reshape(-1, D).T, z64.reshape(-1, 8 * H)),
        'u_f': (h64[:, :-1, :H].reshape(-1, H).T, z64[:, 1:, :4 * H].reshape(-1, 4 * H)),
        'u_b': (h64[:, 1:, H:].reshape(-1, H).T, z64[:, :-1, 4 * H:].reshape(-1, 4 * H)),
    }
    # the same sums, written out per utterance
    dWx = sum(x64[b].T @ z64[b] for b in range(B))
    dUf = sum(h64[b, :T - 1, :H].T @ z64[b, 1:, :4 * H] for b in range(B))            # h_f[b, t-1] with dz_f[b, t], t >= 1
    dUb = sum(h64[b, 1:, H:].T @ z64[b, :T - 1, 4 * H:] for b in range(B))            # h_b[b, t+1] with dz_b[b, t], t <= T-2
    for k, r in (('wx', dWx), ('u_f', dUf), ('u_b', dUb)):
        assert np.allclose(regs[k][0] @ regs[k][1], r, rtol=1e-12, atol=1e-9)
    for v in regs.values():
        v[0].setflags(write=False)
        v[1].setflags(write=False)
    return x, h, dz, dK0, db0, regs, z64.reshape(-1, 8 * H).sum(0), np.linalg.norm(z64.reshape(-1, 8 * H), axis=0)


def _views(dK, db, D, H):
    """The twin-interleaved views optim.FlatOptimizer hands out: dKf / dKb the two column halves of one [(D + H), 8H] block."""
    blk = dK.view(D + H, 2, 4 * H)
    return blk[:, 0, :], db.view(2, 4 * H)[0], blk[:, 1, :], db.view(2, 4 * H)[1]


def _run(ops, shape, acc, capped, f16, group, dev=None):
    B, T, D, H = shape
    x, h, dz, dK0, db0 = _case(*shape)[:5]
    up = dev if dev is not None else (lambda a: torch.from_numpy(a).cuda())
    xd, hd, zd, dK, db = up(x), up(h), up(dz), up(dK0), up(db0)
    if dev is not None and not acc:             # inside a fence torch.empty is NaN-filled: a word the launches do not store stays one
        dK, db = torch.empty(dK0.shape, dtype=torch.float32, device='cuda'), torch.empty(db0.shape, dtype=torch.float32, device='cuda')
    amax = (ops.absmax(xd), ops.absmax(hd), ops.absmax(zd)) if f16 else None
    dKf, dbf, dKb, dbb = _views(dK, db, D, H)
    old = ops.WGRAD_GROUP
    ops.WGRAD_GROUP = group
    try:
        with ops.lds_pad(50000 if capped else 0):
            ops.blstm_bwd_weights(xd, hd, zd, dKf, dbf, dKb, dbb, acc, part='all', amax=amax)
    finally:
        ops.WGRAD_GROUP = old
    return dK, db, (xd, hd, zd)


def _errors(shape, acc, dK, db):
    B, T, D, H = shape
    dK0, db0, regs, dbref, znorm = _case(*shape)[3:]
    out = dK.double().cpu() - (torch.from_numpy(dK0).double() if acc else 0.0)
    e = {'wx': _err(out[:D], *regs['wx']), 'u_f': _err(out[D:, :4 * H], *regs['u_f']), 'u_b': _err(out[D:, 4 * H:], *regs['u_b'])}
    dbo = db.double().cpu().numpy() - (db0.astype(np.float64) if acc else 0.0)
    e['db'] = (np.abs(dbo - dbref) / znorm).max()
    return e


def _grouped_launches(ops, monkeypatch):
    """Counts the calls that really went through the grouped entry (a refusal that fell back to the separate launches would pass the
    numeric checks unseen)."""
    calls = []
    real = ops.blstm_bwd_weights_grouped

    def counted(*a, **k):
        r = real(*a, **k)
        calls.append(r)
        return r
    monkeypatch.setattr(ops, 'blstm_bwd_weights_grouped', counted)
    return calls


@pytest.mark.parametrize('f16', [True, False], ids=['fp16x3', 'bf16x6'])
@pytest.mark.parametrize('capped', [False, True], ids=['uncapped', 'capped'])
@pytest.mark.parametrize('acc', [0, 1], ids=['store', 'accumulate'])
@pytest.mark.parametrize('shape', SHAPES, ids=['x'.join(map(str, s)) for s in SHAPES])
def test_grouped_launch_against_float64(ops, monkeypatch, shape, acc, capped, f16):
    calls = _grouped_launches(ops, monkeypatch)
    dK, db, _ = _run(ops, shape, acc, capped, f16, 1)
    assert calls == [True]
    e = _errors(shape, acc, dK, db)
    if capped:
        dK_t, db_t, _ = _run(ops, shape, acc, True, f16, 0)
        assert calls == [True]                                         # (the comparison ran today's separate launches)
        e_t = _errors(shape, acc, dK_t, db_t)
        print('grouped capped', shape, acc, f16, e, 'separate capped', e_t)
        for k in ('wx', 'u_f', 'u_b'):
            assert e[k] < max(2.0 * e_t[k], 2e-7), (k, e, e_t)
    else:
        print('grouped uncapped', shape, acc, f16, e)
        for k in ('wx', 'u_f', 'u_b'):
            assert e[k] < 1e-7, (k, e)
    assert e['db'] < 1e-6, e


@pytest.mark.parametrize('capped', [False, True], ids=['uncapped', 'capped'])
def test_two_calls_give_the_same_bits(ops, capped):
    a = _run(ops, SHAPES[2], 0, capped, True, 1)
    b = _run(ops, SHAPES[2], 0, capped, True, 1)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


@pytest.mark.parametrize('shape', [SHAPES[0], SHAPES[2]], ids=['direct', 'slabs'])
def test_nothing_outside_the_outputs_and_the_workspace_changes(ops, monkeypatch, shape):
    """Operands, outputs and the workspace between NaN-filled red zones (tests/fenced.py): no zone word changes, the inputs keep their
    bits, and every word of dK and db is a number."""
    calls = _grouped_launches(ops, monkeypatch)
    with Fence() as fence:
        dK, db, ins = _run(ops, shape, 0, False, True, 1, dev=fence.dev)
        fence.check()
        assert calls == [True]
        for t, ref in zip(ins, _case(*shape)[:3]):
            assert np.array_equal(t.cpu().numpy(), ref)
        assert torch.isfinite(dK).all() and torch.isfinite(db).all()
        e = _errors(shape, 0, dK, db)
        assert max(e['wx'], e['u_f'], e['u_b']) < 1e-7 and e['db'] < 1e-6, e


def test_refusals(ops):
    from ams_hip._lib import load
    from ams_hip.ops import _p, _s, _vp
    lib = load()
    B, T, D, H = 3, 7, 36, 20

    def call(D=D, xoff=0, bounds=(1, 1, 1), ldk=8 * H):
        x = torch.zeros(B * T * D + 4, device='cuda')[xoff:]
        h = torch.zeros(B * T * 2 * H, device='cuda')
        dz = torch.zeros(B * T * 8 * H, device='cuda')
        dK = torch.zeros((D + H) * 8 * H, device='cuda')
        db = torch.zeros(8 * H, device='cuda')
        one = torch.ones(1, device='cuda')
        nb = max(int(lib.ams_blstm_bwd_weights_workspace_bytes(B, T, 36, H, 0)), 16)
        ws = torch.zeros(nb // 4 + 4, device='cuda')
        pb = [_p(one) if b else _vp(0) for b in bounds]
        st = lib.ams_blstm_bwd_weights_f32(B, T, D, H, _p(x), D, _p(h), _p(dz), _p(dK), ldk, _p(db), 0, pb[0], pb[1], pb[2], 0,
                                           _p(ws), ws.numel() * 4, _s())
        torch.cuda.synchronize()
        return st
    assert call() == 0
    assert call(bounds=(0, 0, 0)) == 0
    assert call(D=258) == AMS_E_INVALID_ARG
    assert lib.ams_blstm_bwd_weights_workspace_bytes(B, T, 258, H, 0) == 0
    assert call(xoff=1) == AMS_E_INVALID_ARG
    assert call(bounds=(1, 0, 1)) == AMS_E_INVALID_ARG
    assert call(bounds=(0, 0, 1)) == AMS_E_INVALID_ARG
    assert call(ldk=8 * H + 4) == AMS_E_INVALID_ARG


def test_an_input_width_that_is_no_multiple_of_four_takes_the_separate_launches(ops, monkeypatch):
    calls = _grouped_launches(ops, monkeypatch)
    shape = (3, 7, 258, 20)
    dK, db, _ = _run(ops, shape, 0, False, True, 1)
    assert calls == [False]
    e = _errors(shape, 0, dK, db)
    assert max(e['wx'], e['u_f'], e['u_b']) < 1e-7 and e['db'] < 1e-6, e


def _items(shape, s):
    """Work items of the grouped launch of `shape` asked for s slabs: per region, tiles of 128 x 256 times the slabs that launch()'s
    rounding of k_per_split to the 32-deep k-tile leaves (csrc/gemm.hip: bw_group_plan)."""
    B, T, D, H = shape
    n = 0
    for M, N, K in ((D, 8 * H, B * T), (H, 4 * H, B * T - 1), (H, 4 * H, B * T - 1)):
        kps = -(-(-(-K // s)) // 32) * 32
        n += -(-M // 128) * -(-N // 256) * -(-K // kps)
    return n


def _resident_workgroups():
    """Grid of the uncapped (persistent) grouped launch when there are more items: the CUs rounded up to whole XCDs, one workgroup each."""
    return (torch.cuda.get_device_properties(0).multi_processor_count + 7) // 8 * 8


@pytest.mark.parametrize('capped', [False, True], ids=['uncapped', 'capped'])
def test_grouped_launch_at_the_benchmark_shape(ops, monkeypatch, capped):
    """(64, 80, 256, 300): the first layer of the benchmark step, K = 5120, 50 tiles x 5 slabs, accumulating as the step does."""
    calls = _grouped_launches(ops, monkeypatch)
    shape = (64, 80, 256, 300)
    dK, db, _ = _run(ops, shape, 1, capped, True, 1)
    assert calls == [True]
    e = _errors(shape, 1, dK, db)
    if capped:
        e_t = _errors(shape, 1, *_run(ops, shape, 1, True, True, 0)[:2])
        print('benchmark shape capped', e, 'separate capped', e_t)
        assert all(e[k] < max(2.0 * e_t[k], 2e-7) for k in ('wx', 'u_f', 'u_b')), (e, e_t)
    else:
        print('benchmark shape uncapped', e)
        assert max(e['wx'], e['u_f'], e['u_b']) < 1e-7, e
    assert e['db'] < 1e-6, e


_SAME_BITS_SCRIPT = r"""
import os, sys
import numpy as np
import torch
sys.path[:0] = [os.environ['AMS_ROOT'], os.path.join(os.environ['AMS_ROOT'], 'adaptive-multispeaker-separation_amd')]
from ams_hip import ops
from tests import test_gpu_blstm_wgrad_group as t
shape, s = t.SHAPES[2], int(os.environ['AMS_GEMM_SPLITS'])
items, grid = t._items(shape, s), t._resident_workgroups()
print('items', items, 'resident workgroups', grid)
bad = []
if os.environ['AMS_EXPECT_WRAP'] == '1' and not items > grid:
    bad.append(('the persistent walk does not wrap', items, grid))
for capped in (False, True):
    for acc in (0, 1):
        for f16 in (True, False):
            a = t._run(ops, shape, acc, capped, f16, 0)
            b = t._run(ops, shape, acc, capped, f16, 1)
            if not (torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])):
                bad.append(('bits', capped, acc, f16, float((a[0] - b[0]).abs().max()), float((a[1] - b[1]).abs().max())))
            e, e_t = t._errors(shape, acc, b[0], b[1]), t._errors(shape, acc, a[0], a[1])
            print('grouped', capped, acc, f16, e, 'separate', e_t)
            lim = {k: (max(2.0 * e_t[k], 2e-7) if capped else 1e-7) for k in ('wx', 'u_f', 'u_b')}
            if any(not e[k] < lim[k] for k in lim) or not e['db'] < 1e-6:
                bad.append(('float64', capped, acc, f16, e, e_t))
print('cases that fail:', bad)
sys.exit(1 if bad else 0)
"""


@pytest.mark.parametrize('splits,wraps', [('4', False), ('8', True)], ids=['4-slabs', '7-slabs-walk-wraps'])
def test_same_bits_as_the_separate_launches_at_equal_slab_count(tmp_path, splits, wraps):
    """AMS_GEMM_SPLITS is read once per process, hence a child: shape 3 through the separate launches and through the grouped one,
    capped and uncapped, both arithmetics -- the same partition of k, the same accumulation and slab order, the same bits; and the
    grouped results against float64 at the module's bounds.  AMS_GEMM_SPLITS=4: 4 slabs, 200 items.  =8: k_per_split 160 -> 7 slabs,
    350 items on 256 resident workgroups (asserted in the child): the uncapped launch's persistent walk WRAPS -- a workgroup's second
    item lies in another region than its first (wx -> u_b: other shape, other bound of A, no column sums), its operands are requested
    before the first item's stores.  (With the split model's own choice, 5 slabs, shape 3 has 250 items: no wrap.)"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    script = tmp_path / 'same_bits.py'
    script.write_text(_SAME_BITS_SCRIPT)
    env = dict(os.environ, AMS_GEMM_SPLITS=splits, AMS_EXPECT_WRAP='1' if wraps else '0', AMS_ROOT=root)
    r = subprocess.run([sys.executable, str(script)], env=env, capture_output=True, text=True, timeout=300)
    print(r.stdout[-3000:])
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
