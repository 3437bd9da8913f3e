"""GPU: the backward input-gradient products dX = dU . W^T from a PS32 image of W with dU cut inside the product (csrc/gemm_ps.hip,
include/ams.h: ams_gemm_ps_a_f32; ops.backward_product) against float64 and against the in-product fp16x3 form of ams_gemm_f32 with the
same bounds -- same terms, MFMA order, accumulator sets, k-split and reduce order: the same bits."""
import numpy as np
import pytest

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()


class _Owner(object):
    pass


def _operands(M, N, K, seed, lda=None):
    rng = np.random.RandomState(seed)
    lda = K if lda is None else lda
    dU = (rng.randn(M, lda) * np.exp(rng.randn(M, lda))).astype(np.float32)
    W = (rng.randn(N, K) * 0.05).astype(np.float32)
    return dU, W


def _direct(dUd, Wd, am, out=None):
    """ams_gemm_ps_a_f32 itself (backward_product could fall back to the in-product form)."""
    from ams_hip import ops
    lib = ops.load()
    M, K = dUd.shape
    N = Wd.shape[0]
    if out is None:
        out = torch.empty((M, N), dtype=torch.float32, device='cuda')
    img = ops.ps_pack_rows(Wd, am[1])
    nb = lib.ams_gemm_ps_a_workspace_bytes(M, N, K)
    ws = torch.empty(max(nb, 16) // 4, dtype=torch.float32, device='cuda')
    ops.check(lib.ams_gemm_ps_a_f32(M, N, K, ops._p(dUd), dUd.stride(0), ops._p(img), ops._p(out), out.stride(0), ops._p(am[0]),
                                    ops._p(am[1]), ops._p(ws), nb, ops._s()), 'ams_gemm_ps_a_f32')
    return out


@pytest.mark.parametrize('M,N,K', [(5120, 600, 10240), (5120, 600, 2400)])
def test_step_shapes_match_float64_and_equal_the_in_product_form(M, N, K):
    from ams_hip import ops
    dU, W = _operands(M, N, K, M + N + K)
    dUd, Wd = dev(dU), dev(W)
    am = (ops.absmax(dUd), ops.absmax(Wd))
    got = _direct(dUd, Wd, am)
    ref_gemm = ops.gemm(dUd, Wd, transB=True, amax=am)
    ops.load().ams_gemm_set_arith(0)
    try:
        f32 = ops.gemm(dUd, Wd, transB=True)                  # native f32 MFMA: the 1.5x yardstick of test_gpu_gemm_f16.py
    finally:
        ops.load().ams_gemm_set_arith(1)
    torch.cuda.synchronize()
    assert torch.equal(got, ref_gemm)
    rows = np.unique(np.linspace(0, M - 1, 256).astype(int))
    ref = dU[rows].astype(np.float64) @ W.astype(np.float64).T
    scale = np.linalg.norm(dU[rows].astype(np.float64), axis=1)[:, None] * np.linalg.norm(W.astype(np.float64), axis=1)[None, :]
    err = (np.abs(got.cpu().numpy()[rows] - ref) / scale).max()
    err_g = (np.abs(ref_gemm.cpu().numpy()[rows] - ref) / scale).max()
    err_f32 = (np.abs(f32.cpu().numpy()[rows] - ref) / scale).max()
    assert err <= err_g and err <= 1.5 * err_f32, (err, err_g, err_f32)


@pytest.mark.parametrize('M,N,K,lda', [(129, 260, 70, 72), (100, 40, 45, 48), (5, 4, 1, 4), (300, 604, 33, 36), (257, 8, 600, 604),
                                       (130, 600, 2400, 2404)])
def test_edges_are_zeros_not_neighbours(M, N, K, lda):
    """M, N, K that end inside a tile, lda > K with large values in the row tails: only dU[:, :K] counts, and nothing is stored past
    the edge of C (a guard band stays untouched).  Equal to the in-product form at the same bounds."""
    from ams_hip import ops
    dU, W = _operands(M, N, K, 7 * M + K, lda)
    dU[:, K:] = 1e30
    dUd, Wd = dev(dU), dev(W)
    view = dUd[:, :K]
    am = (ops.absmax(view.contiguous()), ops.absmax(Wd))
    big = torch.full((M + 2, N + 8), 7.0, device='cuda')
    out = big[1:M + 1, 4:N + 4]
    _direct(view, Wd, am, out=out)
    ref_gemm = ops.gemm(view, Wd, transB=True, amax=am, M=M, N=N, K=K, lda=lda, ldb=K)
    torch.cuda.synchronize()
    g = big.cpu().numpy()
    ref = dU[:, :K].astype(np.float64) @ W.astype(np.float64).T
    assert np.abs(g[1:M + 1, 4:N + 4] - ref).max() <= 1e-5 * np.abs(ref).max()
    # the in-product form is fp16x3 on the 128 x 256 tile as well: 16-byte fetches (K % 4 == 0) and csrc/gemm.hip: x6_choose_cfg
    if K % 4 == 0 and (N + 255) // 256 * 256 <= 1.30 * N:
        assert torch.equal(out, ref_gemm)
    g[1:M + 1, 4:N + 4] = 7.0
    assert (g == 7.0).all()


def test_launches_back_to_back_are_deterministic():
    from ams_hip import ops
    M, N, K = 5120, 600, 2400
    dU, W = _operands(M, N, K, 3)
    dUd, Wd = dev(dU), dev(W)
    am = (ops.absmax(dUd), ops.absmax(Wd))
    owner = _Owner()
    first = ops.backward_product(dUd, Wd, am, owner).clone()
    for _ in range(10):
        assert torch.equal(ops.backward_product(dUd, Wd, am, owner), first)


def test_the_pipeline_is_race_free_under_memory_pressure():
    """The main loop rests on hand-counted waits (vmcnt(4): B of tile t and A of tile t + 1 have landed) and one barrier per k-tile; a
    miscount shows up as RARE wrong tiles whenever a load lands late.  Many launches of several shapes (one round, several rounds per
    workgroup, one k-tile, a K tail, k-splits) while another stream thrashes HBM: every output equals the in-product form's bits."""
    from ams_hip import ops
    shapes = [(5120, 600, 10240), (5120, 600, 2400), (4096, 1024, 512), (640, 512, 32), (384, 768, 100), (128, 256, 3000)]
    cases = []
    for i, (M, N, K) in enumerate(shapes):
        dU, W = _operands(M, N, K, 100 + i)
        dUd, Wd = dev(dU), dev(W)
        am = (ops.absmax(dUd), ops.absmax(Wd))
        ref = ops.gemm(dUd, Wd, transB=True, amax=am).clone()
        owner = _Owner()
        cases.append((dUd, Wd, am, owner, ref, torch.empty_like(ref)))
    noise_stream = torch.cuda.Stream()
    big = torch.empty(64 * 1024 * 1024, device='cuda')                 # 256 MB: does not fit the Infinity Cache either
    bad = 0
    for rep in range(25):
        with torch.cuda.stream(noise_stream):
            big.add_(1.0)
            big.mul_(0.5)
        for dUd, Wd, am, owner, ref, out in cases:
            ops.backward_product(dUd, Wd, am, owner, out=out)
            bad += int(not torch.equal(out, ref))
    torch.cuda.synchronize()
    assert bad == 0, '%d of %d launches differed from the in-product form' % (bad, 25 * len(cases))
