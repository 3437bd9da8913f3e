"""GPU: the 128 x 320 instance of the backward dX products (csrc/gemm_ps.hip: gemm_ps_a320_kernel) and the one rule that gives both forms
their tile and k-partition (include/ams.h: ams_gemm_ps_a_plan; csrc/gemm.hip: dx_plan).

The rule is a cost model: it takes the wider tile where the launch is bound by its rounds (many row tiles: the step's 5120 x 600 shapes)
and keeps the 128 x 256 tile for a product of a few tiles, where every workgroup has a CU to itself either way and the wider tile only
makes its k-tiles longer.  The small shapes that probe the instance's edges (M = 5, 129, 257, ...) therefore run in a child process with
AMS_GEMM_DX_TILE=320 -- the switch is read once per process and holds for BOTH forms, so the in-product form follows the same partition
there; every case asserts through the plan query that it ran the 320 instance.  The shapes the model itself gives to the wide tile (1, 2, 3
and 6 slabs) run in this process."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _plan(M, N, K, ws_bytes=None):
    from ams_hip import ops
    lib = ops.load()
    if ws_bytes is None:
        ws_bytes = lib.ams_gemm_ps_a_workspace_bytes(M, N, K)
    t, s, k = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    ops.check(lib.ams_gemm_ps_a_plan(M, N, K, ws_bytes, ctypes.byref(t), ctypes.byref(s), ctypes.byref(k)), 'ams_gemm_ps_a_plan')
    return t.value, s.value, k.value


def _direct(dUd, Wd, am, out=None):
    """ams_gemm_ps_a_f32 itself, its workspace sized as the query says."""
    from ams_hip import ops
    lib = ops.load()
    M, K = dUd.shape
    N = Wd.shape[0]
    if out is None:
        out = torch.empty((M, N), dtype=torch.float32, device='cuda')
    img = ops.ps_pack_rows(Wd, am[1])
    nb = lib.ams_gemm_ps_a_workspace_bytes(M, N, K)
    assert nb == (_plan(M, N, K)[1] * M * N * 4 if _plan(M, N, K)[1] > 1 else 0)
    ws = torch.empty(max(nb, 16) // 4, dtype=torch.float32, device='cuda')
    ops.check(lib.ams_gemm_ps_a_f32(M, N, K, ops._p(dUd), dUd.stride(0), ops._p(img), ops._p(out), out.stride(0), ops._p(am[0]),
                                    ops._p(am[1]), ops._p(ws), nb, ops._s()), 'ams_gemm_ps_a_f32')
    return out


def _gpu_operands(M, N, K, seed):
    g = torch.Generator(device='cuda')
    g.manual_seed(seed)
    dU = torch.randn((M, K), device='cuda', generator=g) * torch.exp(torch.randn((M, K), device='cuda', generator=g))
    W = torch.randn((N, K), device='cuda', generator=g) * 0.05
    return dU, W


# shapes the model gives to the 320 tile, by slab count (many row tiles: the launch is bound by its rounds)
MODEL_PICKS = {1: (15360, 600, 2400), 2: (7680, 600, 2400), 3: (5120, 600, 2400), 6: (2560, 600, 2400)}


@pytest.fixture(scope='module')
def picks():
    """operands, bounds and the in-product form's result of each MODEL_PICKS shape, computed once and left unchanged"""
    from ams_hip import ops
    res = {}
    for slabs, (M, N, K) in MODEL_PICKS.items():
        dU, W = _gpu_operands(M, N, K, slabs)
        am = (ops.absmax(dU), ops.absmax(W))
        if slabs == 1:
            # 360 tiles of 128 x 256 are more than the CUs: ops.gemm would share the second round's k-tiles between workgroups
            # (stream-K, another k-partition: such products were outside the equal-bits class before the plan too).  The one-slab
            # bits of the in-product form are those of the entry point without slab workspace and without stream-K scratch.
            ref = torch.empty((M, N), dtype=torch.float32, device='cuda')
            ops.check(ops.load().ams_gemm_f32(0, 1, M, N, K, ops._p(dU), K, ops._p(W), K, ops._p(ref), N, None, 0, 0, 0, ops._p(am[0]),
                                              ops._p(am[1]), 0, None, 0, None, 0, ops._s()), 'ams_gemm_f32')
        else:
            ref = ops.gemm(dU, W, transB=True, amax=am).clone()
        res[slabs] = (dU, W, am, ref)
    torch.cuda.synchronize()
    return res


@pytest.mark.parametrize('slabs', sorted(MODEL_PICKS))
def test_model_picks_equal_the_in_product_form_and_match_float64(picks, slabs):
    from ams_hip import ops
    M, N, K = MODEL_PICKS[slabs]
    tile, s, kps = _plan(M, N, K)
    assert (tile, s) == (320, slabs) and kps % 32 == 0 and (s - 1) * kps < K <= s * kps, (tile, s, kps)
    dU, W, am, ref_gemm = picks[slabs]
    got = _direct(dU, W, am)
    assert torch.equal(got, ref_gemm)
    ops.load().ams_gemm_set_arith(0)
    try:
        f32 = ops.gemm(dU, W, transB=True)                          # native f32 MFMA on the whole product: the 1.5x yardstick of test_gpu_gemm_ps_dx.py
    finally:
        ops.load().ams_gemm_set_arith(1)
    rows = torch.linspace(0, M - 1, 128, device='cuda').long().unique()
    f32 = f32[rows]
    a64, w64 = dU[rows].double(), W.double()
    ref = a64 @ w64.t()
    scale = a64.norm(dim=1)[:, None] * w64.norm(dim=1)[None, :]
    err = float(((got[rows].double() - ref).abs() / scale).max())
    err_g = float(((ref_gemm[rows].double() - ref).abs() / scale).max())
    err_f32 = float(((f32.double() - ref).abs() / scale).max())
    print('320 tile %s: %d slabs of %d, error %.3g (in-product %.3g, native f32 %.3g)' % ((M, N, K), s, kps, err, err_g, err_f32))
    assert err <= err_g and err <= 1.5 * err_f32, (err, err_g, err_f32)


@pytest.mark.parametrize('M,N,K', [(640, 512, 600), (640, 768, 600), (5120, 1024, 2400)])
def test_shapes_the_model_leaves_on_the_256_tile_still_equal_the_in_product_form(M, N, K):
    from ams_hip import ops
    assert _plan(M, N, K)[0] == 256
    dU, W = _gpu_operands(M, N, K, M + N)
    am = (ops.absmax(dU), ops.absmax(W))
    assert torch.equal(_direct(dU, W, am), ops.gemm(dU, W, transB=True, amax=am))


def test_the_plan_is_consistent_and_a_small_workspace_keeps_the_256_tile():
    """kps a multiple of 32 that covers K in `splits` ranges; the wide tile only where all its slabs fit the workspace that is lent."""
    for (M, N, K) in list(MODEL_PICKS.values()) + [(5, 600, 2400), (129, 324, 72), (257, 604, 600), (640, 600, 2400), (5120, 600, 10240)]:
        for ws in (None, 0, M * N * 4 * 2):
            tile, s, kps = _plan(M, N, K, ws)
            assert tile in (256, 320) and s >= 1 and kps % 32 == 0 and (s - 1) * kps < K <= s * kps, (M, N, K, ws, tile, s, kps)
            if ws is not None:
                assert s == 1 or s * M * N * 4 <= ws
    assert _plan(5120, 600, 10240) == (320, 3, 3424) and _plan(5120, 600, 2400) == (320, 3, 800)        # the step's launches
    assert _plan(5120, 600, 2400, 2 * 5120 * 600 * 4) == (256, 2, 1216)                                 # two slabs lent: the 256 tile's plan


def test_hand_counted_waits_hold_under_memory_pressure(picks):
    """vmcnt(5) of the 320 instance (A of k-tile t + 1 and B of t have landed, the five DMAs of B(t + 1) may be in flight) and one barrier
    per k-tile: a miscount shows as rare wrong tiles when a load lands late, not as a hang -- no workgroup waits for another.  25 - 75
    k-tiles per workgroup in 3, 2 and 1 slabs while a second stream streams a 256 MB buffer; every output equals the in-product bits."""
    from ams_hip import ops
    noise_stream = torch.cuda.Stream()
    big = torch.empty(64 * 1024 * 1024, device='cuda')
    outs = {s: torch.empty_like(picks[s][3]) for s in (1, 2, 3)}
    bad = 0
    for rep in range(25):
        with torch.cuda.stream(noise_stream):
            big.add_(1.0)
            big.mul_(0.5)
        for s in (3, 2, 1):
            dU, W, am, ref = picks[s]
            _direct(dU, W, am, out=outs[s])
            bad += int(not torch.equal(outs[s], ref))
    torch.cuda.synchronize()
    assert bad == 0, '%d of 75 launches differed from the in-product form' % bad


# ---- the instance's edges, and a training step, with the tile forced (child processes: the switch is read once) ----------------------
_CHILD = r'''
import ctypes, gc, os, sys, tempfile
import numpy as np
root = os.environ['AMS_ROOT']
sys.path[:0] = [root, os.path.join(root, 'adaptive-multispeaker-separation_amd')]
import torch
from ams_hip import functional as F, ops as K
lib = K.load()
out = {}

def plan(M, N, Kk, nb):
    t, s, k = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    K.check(lib.ams_gemm_ps_a_plan(M, N, Kk, nb, ctypes.byref(t), ctypes.byref(s), ctypes.byref(k)), 'ams_gemm_ps_a_plan')
    return t.value, s.value, k.value

if os.environ.get('AMS_TILE_CASES'):
    from tests.fenced import Fence
    cases = [tuple(int(v) for v in c.split('x')) for c in os.environ['AMS_TILE_CASES'].split(',')]
    for i, (M, N, Kk, lda) in enumerate(cases):
        rng = np.random.RandomState(7 * M + Kk + N)
        dU = (rng.randn(M, lda) * np.exp(rng.randn(M, lda))).astype(np.float32)
        dU[:, Kk:] = 1e30
        W = (rng.randn(N, Kk) * 0.05).astype(np.float32)
        with Fence() as fence:
            dUd, Wd = fence.dev(dU), fence.dev(W)
            view = dUd[:, :Kk]
            am = (K.absmax(view.contiguous()), K.absmax(Wd))
            img = K.ps_pack_rows(Wd, am[1])
            nb = lib.ams_gemm_ps_a_workspace_bytes(M, N, Kk)
            tile, s, kps = plan(M, N, Kk, nb)
            ws = torch.empty(max(nb, 16) // 4, dtype=torch.float32, device='cuda')      # fenced, NaN-filled, exactly the query's size
            got = torch.empty((M, N), dtype=torch.float32, device='cuda')               # fenced, NaN-filled
            K.check(lib.ams_gemm_ps_a_f32(M, N, Kk, K._p(view), lda, K._p(img), K._p(got), N, K._p(am[0]), K._p(am[1]), K._p(ws), nb, K._s()),
                    'ams_gemm_ps_a_f32')
            fence.check()
            ref_gemm = K.gemm(view, Wd, transB=True, amax=am, M=M, N=N, K=Kk, lda=lda, ldb=Kk)
            lib.ams_gemm_set_arith(0)
            f32 = K.gemm(view, Wd, transB=True, M=M, N=N, K=Kk, lda=lda, ldb=Kk)
            lib.ams_gemm_set_arith(1)
            torch.cuda.synchronize()
            g = got.cpu().numpy()
            ref = dU[:, :Kk].astype(np.float64) @ W.astype(np.float64).T
            scale = np.linalg.norm(dU[:, :Kk].astype(np.float64), axis=1)[:, None] * np.linalg.norm(W.astype(np.float64), axis=1)[None, :]
            e = lambda y: float((np.abs(y - ref) / scale).max())
            out['case%d' % i] = np.array([M, N, Kk, lda, tile, s, kps, nb, int(torch.equal(got, ref_gemm)), int(np.isfinite(g).all())], np.int64)
            out['err%d' % i] = np.array([e(g), e(ref_gemm.cpu().numpy()), e(f32.cpu().numpy())])
    # ten launches back to back
    M, N, Kk = 640, 600, 2400
    g_ = torch.Generator(device='cuda'); g_.manual_seed(3)
    dU = torch.randn((M, Kk), device='cuda', generator=g_) * torch.exp(torch.randn((M, Kk), device='cuda', generator=g_))
    W = torch.randn((N, Kk), device='cuda', generator=g_) * 0.05
    am = (K.absmax(dU), K.absmax(W))
    class Owner(object):
        pass
    owner = Owner()
    first = K.backward_product(dU, W, am, owner).clone()
    same = sum(int(torch.equal(K.backward_product(dU, W, am, owner), first)) for _ in range(10))
    out['determinism'] = np.array([same, plan(M, N, Kk, lib.ams_gemm_ps_a_workspace_bytes(M, N, Kk))[0],
                                   int(torch.equal(first, K.gemm(dU, W, transB=True, amax=am)))], np.int64)

# a front_DPCL step whose dX products are 192 x 600 x 2400 (the second BLSTM layer) and 192 x 600 x 128 (the dense layer)
from tests.smoke_step import build_front_dpcl
import utils.ops
K.PS_AUTOTUNE = False
gc.disable()
B, L, hop, LS, NF, E = 3, 1024, 16, 600, 16, 8
Mtok = B * (L // hop)
out['step_plans'] = np.array([plan(Mtok, LS, 4 * LS, lib.ams_gemm_ps_a_workspace_bytes(Mtok, LS, 4 * LS)),
                              plan(Mtok, LS, NF * E, lib.ams_gemm_ps_a_workspace_bytes(Mtok, LS, NF * E))], np.int64)
for graph in (False, True):
    utils.ops.rng.seed(42)
    torch.manual_seed(0)
    np.random.seed(0)
    calls0 = K.PS_LAUNCHES[0]
    trainer, tfds = build_front_dpcl(tempfile.mkdtemp(prefix='ams_dxt_'), B=B, L=L, W=64, N=NF, hop=hop, E=E, hip_graph=graph,
                                     no_summaries=True, layer_size=LS, nb_layers=2)
    g, model = trainer.graph, trainer.model
    steps = 5 if graph else 3                            # captured: two eager steps, the capture, replays
    costs = []
    with g.as_default():
        feed = {tfds.handle: tfds.get_handle(tfds.TRAIN), tfds.chunk_size: L}
        tfds.initialize(tfds.TRAIN)
        for i in range(steps):
            costs.append(np.float32(float(model.train(feed, i))))
    torch.cuda.synchronize()
    K.raise_on_ring_errors()
    k = 'g%d' % int(graph)
    out['cost_' + k] = np.array(costs[:3] if not graph else costs, np.float32)
    for v in model.trainable_variables:
        out['var_%s_%s' % (k, v.ams_name.replace('/', '.'))] = v.detach().cpu().numpy()
    del trainer, tfds, g, model
    gc.collect()
    torch.cuda.synchronize()
np.savez(sys.argv[1], **out)
'''

# M x N x K x lda: rows ending inside a tile (5, 129, 257), N = 320 (one tile exactly), 324 (four columns into the second), 600, 604;
# K = 4 (one k-tile), 36, 72, 300, 400, 600, 2400; lda > K with 1e30 in the row tails.  Slabs (asserted below): 1 (K <= 72), 2 (K = 300:
# the last slab is 140 = 4 k-tiles + 12), 3 (K = 400), 4 (K = 600: the last slab is 120 = 3 k-tiles + 24), 15 (K = 2400)
EDGE_CASES = [(5, 600, 2400, 2404), (129, 604, 600, 604), (257, 600, 72, 76), (257, 604, 36, 40), (129, 600, 4, 4), (5, 604, 300, 304),
              (257, 600, 400, 404), (129, 320, 72, 72), (257, 324, 36, 40), (5, 320, 4, 8), (257, 320, 600, 604), (129, 324, 2400, 2400)]
EDGE_SLABS = [15, 4, 1, 1, 1, 2, 3, 1, 1, 1, 4, 15]


@pytest.fixture(scope='module')
def arms(tmp_path_factory):
    tmp = tmp_path_factory.mktemp('dx_tile')
    script = tmp / 'child.py'
    script.write_text(_CHILD)
    res = {}
    for tile in ('320', '256'):
        out = tmp / ('tile%s.npz' % tile)
        e = dict(os.environ, AMS_ROOT=ROOT, AMS_LOG_DIR=str(tmp / 'log'), AMS_GEMM_DX_TILE=tile)
        e.pop('AMS_TILE_CASES', None)
        if tile == '320':
            e['AMS_TILE_CASES'] = ','.join('x'.join(str(v) for v in c) for c in EDGE_CASES)
        subprocess.run([sys.executable, str(script), str(out)], check=True, env=e, timeout=600)
        res[tile] = dict(np.load(out))
    return res


@pytest.mark.parametrize('i', range(len(EDGE_CASES)))
def test_edges_on_the_320_tile_inside_fences(arms, i):
    """Output and slab workspace NaN-filled between red zones (tests/fenced.py; the entry point wants 16-byte bases, so the payloads
    start on their 256-byte boundaries), the workspace exactly as large as the query says: every output word is written, no zone word
    is, the row tails past K do not count.  Same bits as the in-product form where that form runs the 128 x 256 configuration under the
    same plan (N = 600, 604) or both take a single slab; not worse than it against float64, and within 1.5 x the native-f32 error.
    K = 4 has no accumulation error for the arithmetic to be measured by: what is left is the operands' own resolution, 22 bits each in
    the fp16 pairs (tests/test_gpu_gemm_ps.py) against 24 in f32, so every fp16x3 form, the in-product one included, is 2 - 2.5 x the
    native product there (measured 3.39e-07 against 1.50e-07 and 2.12e-07 against 9.2e-08, the in-product form bit for bit the same).
    There the bound is the format's: two operands cut to 2^-22 of their size each, |error| <= 2^-21 |a| |w| by Cauchy-Schwarz."""
    a = arms['320']
    M, N, K, lda, tile, s, kps, nb, equal, finite = (int(v) for v in a['case%d' % i])
    err, err_g, err_f32 = (float(v) for v in a['err%d' % i])
    print('edge %s: tile %d, %d slabs of %d, equal %d, error %.3g (in-product %.3g, native f32 %.3g)' % (EDGE_CASES[i], tile, s, kps, equal, err, err_g, err_f32))
    assert (M, N, K, lda) == EDGE_CASES[i] and tile == 320 and s == EDGE_SLABS[i] and nb == (s * M * N * 4 if s > 1 else 0)
    assert finite
    in_class = (N + 255) // 256 * 256 <= 1.30 * N          # the in-product form is on its 128 x 256 configuration and follows the plan
    if in_class or s == 1:
        assert equal
    assert err <= err_g, (err, err_g)
    if K >= 32:
        assert err <= 1.5 * err_f32, (err, err_g, err_f32)
    else:
        assert err <= 2.0 ** -21, (err, err_g, err_f32)


def test_ten_launches_back_to_back_are_identical(arms):
    same, tile, equal = (int(v) for v in arms['320']['determinism'])
    assert tile == 320 and same == 10 and equal


def test_a_step_on_the_320_tile_eager_equals_captured_and_agrees_with_the_256_arm(arms):
    """front_DPCL with layer size 600 (dX products 192 x 600 x 2400 and 192 x 600 x 128), three steps: costs and variables identical
    eager and captured on the 320 tile; against AMS_GEMM_DX_TILE=256 (other slab counts: not the same bits, by design) within 2e-6 of an
    array's largest value, the bound tests/test_gpu_gemm_ps.py holds the two forward forms to."""
    a, b = arms['320'], arms['256']
    assert [int(p[0]) for p in a['step_plans']] == [320, 320] and [int(p[0]) for p in b['step_plans']] == [256, 256]
    assert a['cost_g0'].tobytes() == a['cost_g1'][:3].tobytes() and len(set(a['cost_g0'].tolist())) > 2
    names = [k[len('var_g0_'):] for k in a if k.startswith('var_g0_')]
    assert len(names) > 8
    worst = 0.0
    for n in names:
        x, y = a['var_g0_' + n], b['var_g0_' + n]
        assert np.all(np.isfinite(x)) and x.shape == y.shape
        d = float(np.abs(x.astype(np.float64) - y).max() / max(float(np.abs(y).max()), 1e-30))
        worst = max(worst, d)
        assert d <= 2e-6, (n, d)
    dc = float(np.abs(a['cost_g0'].astype(np.float64) - b['cost_g0']).max() / np.abs(b['cost_g0']).max())
    print('320 against 256 arm after three steps: largest variable difference %.3g of its array, cost %.3g' % (worst, dc))
    assert dc <= 2e-6
