"""GPU: every instantiated arm of the BLSTM ring recurrence kernels (csrc/lstm_ring.hip) against the float64 oracle.

ams_blstm_ring_fwd / _bwd choose among 21 + 12 separately compiled kernels from NW = ceil(H / 12) and the arithmetic
(tests/ring_arms.py).  Each NR of the forward kernel is a register layout of its own (3 NR k-slots packed into MFMAs of 8: NR = 2, 4
and 5 leave 2, 4 and 1 zero slots in the last one), each backward arm has its own number of tiles per wave and producers per group.
test_ring_arm runs one BLSTM layer, forward and backward, through the arm a hidden size reaches:

  * kernels uniform(+-lim) * 3, so that the recurrence matters; upstream gradients with one magnitude per batch row, 2^20 .. 2^-60;
  * out, dKf, dKb, dbf, dbb against the whole reference array, dx per batch row;
  * the bound word: ams_blstm_ring_bwd leaves max |da| in float word 2 of its sync head and ops.blstm_bwd_recurrent tags G with it --
    the fp16x3 operand bound of the three products that read dZ.  The kernel takes the maximum of the very values it stores (masked
    by `live`, as the stores are), so the word is held to be EXACTLY max |G|, which includes the condition word >= max |G|;
  * the ring error word zero.

Arithmetics.  'bf16x6_f32': no bound is passed -- lstm_ring_fwd_kernel<NR, 1> and lstm_ring_bwd_kernel<arm, arm, 0>.  'fp16x3':
amax = (max |x|, max |K|) to blstm_fwd and amax_u = max |K| to the backward -- <NR, 2> and <arm, arm, 2>.  The forward kernel on the
f32 pipe, <NR, 0>, is chosen by AMS_LSTM_RING_X6=0, read once per process: one child process runs the 'bf16x6_f32' sweep under it.

Tolerances are those of test_gpu_kernels.py (test_blstm_layer, test_backward_ring_as_fp16x3_one_scale_per_row): TOL for out, 5 TOL
for every gradient, relative to the reference array's (for dx: the reference row's) largest entry.

MEASURED on the MI355X, largest error over all cases of this file, relative as above (limits: out 2e-5, gradients 1e-4):
    arithmetic                               out       dx        dK        db
    bf16x6 forward, f32 backward             3.3e-7    4.5e-7    4.2e-7    2.9e-7
    fp16x3 forward and backward              4.8e-7    4.8e-7    4.1e-7    3.6e-7
    f32-pipe forward (child), f32 backward   4.5e-7    4.5e-7    3.7e-7    2.8e-7
The forward ring as fp16x3 meets TOL at every size, so it is held to TOL (not to test_gpu_benchshape.py's FWD_TOL).  The module takes
about 20 s, of which the child process 5.5 s.
"""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

from oracle import blstm as oblstm
from tests import ring_arms as RA

TOL = 2e-5                                  # tests/test_gpu_kernels.py
ARITHS = ('bf16x6_f32', 'fp16x3')
RING_ID = {'1': 'plain', 'safe': 'safe'}


def dev(x, dtype=np.float32):
    return torch.from_numpy(np.ascontiguousarray(x, dtype=dtype)).cuda()


def host(t):
    torch.cuda.synchronize()
    return t.detach().cpu().numpy().astype(np.float64)


def rel(a, b):
    b = np.asarray(b, np.float64)
    return np.abs(np.asarray(a, np.float64) - b).max() / max(np.abs(b).max(), 1e-30)


@pytest.fixture(scope='module')
def ops():
    from ams_hip import ops as o
    return o


@functools.lru_cache(maxsize=None)
def reference(B, T, D, H):
    """Inputs and float64 oracle results of one shape: computed once, shared by every case of that shape, read-only."""
    rng = np.random.RandomState(1000 * H + 10 * B + T)
    lim = np.sqrt(6.0 / (D + 5 * H))
    r = {'x': rng.randn(B, T, D)}
    r['Kf'], r['Kb'] = rng.uniform(-lim, lim, (D + H, 4 * H)) * 3, rng.uniform(-lim, lim, (D + H, 4 * H)) * 3
    r['bf'], r['bb'] = rng.randn(4 * H) * 0.1, rng.randn(4 * H) * 0.1
    r['out'], cache = oblstm.blstm_fwd(r['x'], r['Kf'], r['bf'], r['Kb'], r['bb'])
    row_scale = 2.0 ** (20 - 80.0 * rng.permutation(B) / max(B - 1, 1))            # one magnitude per batch row
    r['dout'] = rng.randn(B, T, 2 * H) * row_scale[:, None, None]
    r['dx'], (r['dKf'], r['dbf'], r['dKb'], r['dbb']) = oblstm.blstm_bwd(r['dout'], cache)
    for v in r.values():
        v.setflags(write=False)
    return r


def upload_kernels(ref, twin):
    """The two direction kernels on the device: two tensors, or the two planes of one [D + H, 2, 4H] block (ldu = 8H, what
    optim.FlatOptimizer stores)."""
    if not twin:
        return dev(ref['Kf']), dev(ref['Kb'])
    blk = torch.empty(ref['Kf'].shape[0], 2, ref['Kf'].shape[1], device='cuda')
    blk[:, 0].copy_(dev(ref['Kf']))
    blk[:, 1].copy_(dev(ref['Kb']))
    return blk[:, 0], blk[:, 1]


def ring_forward(ops, ref, xd, Kfd, Kbd, bound_w):
    return ops.blstm_fwd(xd, Kfd, dev(ref['bf']), Kbd, dev(ref['bb']), amax=None if bound_w is None else (ops.absmax(xd), bound_w))


def ring_arm_case(ops, monkeypatch, B, T, D, H, ring, arith, twin=False, rings=True):
    """One layer, forward and backward, against the oracle; returns the measured errors.  rings: the shape is one the ring takes
    (else the per-step kernels must have run: no bound word)."""
    assert arith in ARITHS and ring in RING_ID
    monkeypatch.setattr(ops, 'LSTM_RING', ring)
    monkeypatch.setattr(ops, 'F16X3', True)
    lib = ops.load()
    assert (lib.ams_blstm_ring_sync_bytes(B, H, 0) != 0) == rings and (lib.ams_blstm_ring_sync_bytes(B, H, 1) != 0) == rings
    ref = reference(B, T, D, H)
    xd = dev(ref['x'])
    Kfd, Kbd = upload_kernels(ref, twin)
    assert Kfd.stride(0) == (8 * H if twin else 4 * H)
    bound_w = None
    if arith == 'fp16x3':
        bound_w = ops.absmax(Kfd._base) if twin else torch.maximum(ops.absmax(Kfd), ops.absmax(Kbd))
    out, G, cst = ring_forward(ops, ref, xd, Kfd, Kbd, bound_w)
    assert (cst.dim() == 5) == rings
    errs = {'out': rel(host(out), ref['out'])}
    doutd = dev(ref['dout'])
    # ops.blstm_bwd, taken apart: the bound word is read between the recurrence and the products that use it
    syncs, ring_sync = [], ops._ring_sync

    def recorded_ring_sync(nbytes, like):
        syncs.append(ring_sync(nbytes, like))
        return syncs[-1]

    monkeypatch.setattr(ops, '_ring_sync', recorded_ring_sync)
    dbpart = ops.blstm_bwd_recurrent(xd, Kfd, Kbd, G, cst, doutd, amax_u=bound_w)
    monkeypatch.setattr(ops, '_ring_sync', ring_sync)
    assert (dbpart is not None) == rings and len(syncs) == int(rings)
    if rings:
        tag = ops.amax_of(G)
        # the tag is word 2 of the launch's sync buffer (a private one, or a slot of the pass arena), not a fresh measurement
        assert tag is G._ams_amax[0] and tag is ops.amax_of(G)
        assert tag.numel() == 1 and tag.dtype == torch.float32 and tag.data_ptr() == syncs[0][0].data_ptr() + 8
        word, da_max = float(tag), float(G.abs().max())
        assert np.isfinite(word)
        assert word >= da_max, (word, da_max)                   # the condition: a smaller bound lets the dW products overflow fp16
        assert word == da_max, (word, da_max)                   # and it is the maximum of the stored values themselves
    dKf = torch.empty(tuple(Kfd.shape), dtype=torch.float32, device='cuda')
    dKb = torch.empty(tuple(Kbd.shape), dtype=torch.float32, device='cuda')
    dbf = torch.empty(4 * H, dtype=torch.float32, device='cuda')
    dbb = torch.empty(4 * H, dtype=torch.float32, device='cuda')
    ops.blstm_bwd_weights(xd, out, G, dKf, dbf, dKb, dbb, False, dbpart=dbpart)
    dx = ops.blstm_bwd_dx(G, Kfd, Kbd, B, T, D)
    dxh = host(dx)
    errs['dx'] = max(rel(dxh[b], ref['dx'][b]) for b in range(B))
    errs['dK'] = max(rel(host(dKf), ref['dKf']), rel(host(dKb), ref['dKb']))
    errs['db'] = max(rel(host(dbf), ref['dbf']), rel(host(dbb), ref['dbb']))
    print('ring_arm B=%d T=%d D=%d H=%d ring=%s arith=%s twin=%d rings=%d fwd<%d> bwd<%d>: out %.3e dx %.3e dK %.3e db %.3e'
          % (B, T, D, H, ring, arith, twin, rings, RA.fwd_arm(H), RA.bwd_arm(H), errs['out'], errs['dx'], errs['dK'], errs['db']))
    assert errs['out'] < TOL, errs
    for b in range(B):                                           # every batch row to the tolerance of the whole
        assert rel(dxh[b], ref['dx'][b]) < 5 * TOL, (b, rel(dxh[b], ref['dx'][b]))
    assert errs['dK'] < 5 * TOL and errs['db'] < 5 * TOL, errs
    assert ops.persist_errors() == 0                            # no bounded in-launch wait timed out
    ops.raise_on_ring_errors()
    return errs


# ------------------------------------------------------------------------------------------------------------------------- the cases
SWEEP_SHAPE = (17, 6, 8)        # two chains per direction (a full one, one with a single live row); both phases of the tile buffers twice
SWEEP = [SWEEP_SHAPE + (H, ring, arith) for H in RA.H_CASES for ring in ('1', 'safe') for arith in ARITHS]

# batch and time geometry at (forward arm 2, backward arm 2) and (5, 4): a single row, a chain short of one row, a full chain, a
# one-row chain, 8 chains, and 10 chains padded to 16 (six chains' worth of workgroups leave without touching anything); one, two and
# three steps (no hand-off, one, one per tile buffer)
GEOMETRY_H = (61, 193)
GEOMETRY = ([(B, 5, 8, H, '1', arith) for H in GEOMETRY_H for B in (1, 15, 16, 17, 64, 65, 80) for arith in ARITHS] +
            [(17, T, 8, H, '1', arith) for H in GEOMETRY_H for T in (1, 2, 3) for arith in ARITHS])

# what the fenced table (tests/test_gpu_fenced.py) runs again between red zones, and one more arm of each kernel
FENCED = [(65, 5, 8, 61, '1', 'bf16x6_f32'), (65, 5, 8, 61, '1', 'fp16x3'), (17, 6, 8, 97, '1', 'fp16x3'), (17, 6, 8, 336, '1', 'bf16x6_f32')]

CASES = SWEEP + [c for c in GEOMETRY if c not in SWEEP]
assert all(c in CASES for c in FENCED)

# the sweep cases the child process runs under AMS_LSTM_RING_X6=0: lstm_ring_fwd_kernel<NR, 0>
F32_PIPE = [c for c in SWEEP if c[4] == '1' and c[5] == 'bf16x6_f32']


def case_id(c):
    return '%s-B%d-T%d-H%d-%s-%s' % ('sweep' if c in SWEEP else 'geometry', c[0], c[1], c[3], RING_ID[c[4]], c[5])


@pytest.mark.parametrize('B,T,D,H,ring,arith', CASES, ids=[case_id(c) for c in CASES])
def test_ring_arm(ops, monkeypatch, B, T, D, H, ring, arith):
    ring_arm_case(ops, monkeypatch, B, T, D, H, ring, arith)


@pytest.mark.parametrize('arith', ARITHS)
@pytest.mark.parametrize('H', [61, 241])
def test_twin_interleaved_kernels(ops, monkeypatch, H, arith):
    """Kf / Kb as the two planes of one [D + H, 2, 4H] block: the ring reads its recurrent weights with ldu = 8H."""
    ring_arm_case(ops, monkeypatch, 17, 6, 8, H, '1', arith, twin=True)


def ring_batch_limit(H):
    """The largest batch the ring takes at hidden size H on this device, as ring_shape (csrc/lstm_ring.hip) decides: whole groups of 8
    chains of NW workgroups within 2 x CUs, at most 512 live workgroups, two chains per 16 rows."""
    cus = torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count
    cus = int(os.environ.get('AMS_LSTM_RING_CUS', cus))
    chains = min(8 * ((2 * cus) // (8 * RA.nw(H))), 512 // RA.nw(H))
    chains -= chains % 2
    assert chains >= 2, 'no ring at H = %d on %d CUs' % (H, cus)
    return 8 * chains


@pytest.mark.parametrize('arith', ARITHS)
@pytest.mark.parametrize('over', [0, 1])
def test_capacity_edge(ops, monkeypatch, over, arith):
    """H = 300 on 256 CUs: B = 128 is 16 chains x 25 = 400 workgroups, the largest ring; B = 129 pads 18 chains to 24 = 600 and takes
    the per-step kernels.  Both match the oracle."""
    B = ring_batch_limit(300) + over
    assert B == 128 + over or torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count != 256
    assert (ops.load().ams_blstm_ring_sync_bytes(B, 300, 0) != 0) == (over == 0)
    ring_arm_case(ops, monkeypatch, B, 3, 8, 300, '1', arith, rings=(over == 0))


@pytest.mark.parametrize('H', [61, 170, 301])
def test_the_bounds_change_the_arithmetic(ops, monkeypatch, H):
    """The same inputs with and without the bounds differ bit-wise: the forward output (fwd<NR, 2> against <NR, 1>), and, from ONE
    forward state, what the backward ring leaves in G (bwd<arm, arm, 2> against <arm, arm, 0>)."""
    monkeypatch.setattr(ops, 'LSTM_RING', '1')
    monkeypatch.setattr(ops, 'F16X3', True)
    B, T, D = SWEEP_SHAPE
    ref = reference(B, T, D, H)
    xd = dev(ref['x'])
    Kfd, Kbd = upload_kernels(ref, False)
    bound_w = torch.maximum(ops.absmax(Kfd), ops.absmax(Kbd))
    out16, _, _ = ring_forward(ops, ref, xd, Kfd, Kbd, bound_w)
    out6, G, cst = ring_forward(ops, ref, xd, Kfd, Kbd, None)
    assert rel(host(out16), ref['out']) < TOL and rel(host(out6), ref['out']) < TOL
    assert not torch.equal(out16, out6)
    doutd = dev(ref['dout'])
    G16, G32 = G.clone(), G.clone()
    ops.blstm_bwd_recurrent(xd, Kfd, Kbd, G16, cst, doutd, amax_u=bound_w)
    ops.blstm_bwd_recurrent(xd, Kfd, Kbd, G32, cst, doutd, amax_u=None)
    assert not torch.equal(G16, G32)
    assert bool(torch.isfinite(G16).all()) and bool(torch.isfinite(G32).all())
    assert ops.persist_errors() == 0
    ops.raise_on_ring_errors()


def test_forward_arms_on_the_f32_pipe():
    """AMS_LSTM_RING_X6=0 (read once per process) puts the forward ring's product on v_mfma_f32_16x16x4_f32: lstm_ring_fwd_kernel<NR, 0>
    for all seven NR, in ONE child process that runs the 'bf16x6_f32' half of the sweep with the plain hand-off."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, '-m', 'pytest', os.path.join(root, 'tests', 'test_gpu_ring_arms.py'), '-q', '-x', '-k',
                        'test_ring_arm and sweep and plain and bf16x6_f32'], env=dict(os.environ, AMS_LSTM_RING_X6='0'),
                       capture_output=True, text=True, timeout=900, cwd=root)
    assert len(F32_PIPE) == len(RA.H_CASES)
    assert r.returncode == 0 and '\n%d passed' % len(F32_PIPE) in r.stdout and 'failed' not in r.stdout, r.stdout[-1500:]


def test_every_instantiation_is_reached():
    """The parametrisation above, recomputed through tests/ring_arms.py, contains each of the 21 forward and 12 backward kernels."""
    arith_f = {'bf16x6_f32': 1, 'fp16x3': 2}
    arith_b = {'bf16x6_f32': 0, 'fp16x3': 2}
    assert all(RA.takes_ring(c[3]) for c in CASES)
    fwd = {(RA.fwd_arm(c[3]), arith_f[c[5]]) for c in SWEEP} | {(RA.fwd_arm(c[3]), 0) for c in F32_PIPE}
    bwd = {(RA.bwd_arm(c[3]), arith_b[c[5]]) for c in SWEEP}
    assert fwd == {(nr, a) for nr in RA.FWD_ARMS for a in RA.FWD_ARITH} and len(fwd) == 21
    assert bwd == {(arm, a) for arm in RA.BWD_ARMS for a in RA.BWD_ARITH} and len(bwd) == 12
    # ... each of them with both hand-offs, and at the first and the last hidden size of its arm
    for ring in ('1', 'safe'):
        assert {(RA.fwd_arm(c[3]), arith_f[c[5]]) for c in SWEEP if c[4] == ring} == {(nr, a) for nr in RA.FWD_ARMS for a in (1, 2)}
        assert {(RA.bwd_arm(c[3]), arith_b[c[5]]) for c in SWEEP if c[4] == ring} == {(arm, a) for arm in RA.BWD_ARMS for a in (0, 2)}
    for ring in ('1', 'safe'):
        for arith in ARITHS:
            swept = {c[3] for c in SWEEP if c[4] == ring and c[5] == arith}
            for arm_of, arms in ((RA.fwd_arm, RA.FWD_ARMS), (RA.bwd_arm, RA.BWD_ARMS)):
                for arm in arms:
                    sizes = [H for H in range(2, RA.RING_MAX_H + 1) if arm_of(H) == arm]
                    assert sizes[-1] in swept and (arm == 1 or sizes[0] in swept), (ring, arith, arm_of.__name__, arm)
            for nr in RA.FWD_ARMS[1:]:                           # inside the arm: a partial last workgroup, granule and group of four
                assert any(RA.fwd_arm(H - 1) == RA.fwd_arm(H + 1) == nr and H % 12 > 1 and H % 3 and RA.nw(H) % 4 for H in swept), \
                    (ring, arith, nr)
