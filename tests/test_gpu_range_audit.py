"""The fp16x3 range audit (ops.F16_AUDIT, include/ams.h: ams_range_share) against every product that takes operand bounds.

fp16x3 scales each operand by ONE power of two from its bound; an entry 2^-30 below the bound lands in the fp16 subnormals and keeps a
handful of bits.  The audit is the only guard: it measures both operands of every bounded launch of one eager step and sends a class
whose operands leave the range back to bf16x6.  These tests hold it to that:
  - the header's bounded entry points are exactly this file's table plus named exclusions (CPU);
  - every bounded launch of an audited step of each recipe is audited, and after a denial no form of the step (eager pre-split,
    eager in-product, re-captured graph) makes a bounded launch of a denied class;
  - for each product that used to escape the audit (the unaligned BLSTM input projection, the dilated conv layers, path B's conv +
    max-pool): fp16x3 really is off on quiet slices of real-looking data, one audited call denies exactly that class, and the denied
    class then meets float64 on quiet and loud slices alike within 1.5x the native f32 MFMA's error."""
import contextlib
import os
import re
import tempfile

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'ams.h')

QUIET = 2.0 ** -30          # quiet slices, relative to the loud ones: below the bound * 2^-17 range of fp16x3

# Entry points of include/ams.h that take a pair of operand bounds (const float* amax_*): fp16x3 products.  Every launch of one of
# them with both bounds given must be covered by the audit.
BOUNDED = ('ams_front_conv_fwd', 'ams_front_maxpool_fwd', 'ams_gemm_f32', 'ams_gemm_ps', 'ams_gemm_ps_a_f32', 'ams_gemm_f32_at_b_colsum',
           'ams_dilated_conv2d_fwd', 'ams_dilated_conv2d_bwd_data', 'ams_dilated_conv2d_bwd_filter', 'ams_gemm_f32_batched')
# Entry points with a bound that the audit does not cover, and why.
EXCLUDED = {
    'ams_blstm_ring_fwd': 'one bound (amax_u) of the recurrent kernels only: h_{t-1} (|h| < 1) is scaled by a fixed 2^13',
    'ams_blstm_ring_bwd': 'one bound (amax_u) of the recurrent kernels only: da_t gets a power-of-two scale per batch row inside the ring',
}


def bound_arguments(path=HEADER):
    """{entry point: [positions of its `const float* amax_*` arguments]} over the prototypes of include/ams.h."""
    src = re.sub(r'/\*.*?\*/', ' ', open(path).read(), flags=re.S)
    out = {}
    for m in re.finditer(r'\b(?:ams_status|size_t|int|long|void)\s+(ams_\w+)\s*\(([^)]*)\)\s*;', src):
        args = [a.strip() for a in m.group(2).split(',')]
        pos = [i for i, a in enumerate(args) if re.match(r'const\s+float\s*\*\s*amax_\w+$', a)]
        if pos:
            out[m.group(1)] = pos
    return out


def test_header_bounded_entry_points_are_the_table():
    """A new entry point with operand bounds fails here until it is placed in BOUNDED (and the audit covers it) or in EXCLUDED."""
    found = bound_arguments()
    assert sorted(n for n, pos in found.items() if len(pos) == 2) == sorted(BOUNDED)
    assert sorted(n for n, pos in found.items() if len(pos) != 2) == sorted(EXCLUDED)
    assert all(len(found[n]) == 1 for n in EXCLUDED)


# ------------------------------------------------------------------ launch recorder
def _ptr(v):
    v = getattr(v, 'value', v)
    return int(v) if v else 0


class _Recorder(object):
    """Stands in for the ctypes library: calls of the BOUNDED entry points with both bounds given are recorded (name, bound of A, bound
    of B, inside a graph capture), everything is passed through."""

    def __init__(self, lib):
        import torch
        self._lib, self._torch, self.calls = lib, torch, []
        self._pos = {n: p for n, p in bound_arguments().items() if n in BOUNDED}

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        pos = self._pos.get(name)
        if pos is None:
            return fn

        def call(*a):
            pa, pb = _ptr(a[pos[0]]), _ptr(a[pos[1]])
            if pa and pb:
                self.calls.append((name, pa, pb, self._torch.cuda.is_current_stream_capturing()))
            return fn(*a)
        return call


@contextlib.contextmanager
def recording():
    from ams_hip import _lib
    lib = _lib.load()
    rec = _Recorder(lib)
    _lib._lib = rec
    try:
        yield rec
    finally:
        _lib._lib = lib


def audited_pairs(records):
    """{(address of A's bound, address of B's bound): {keys}} of the audit's records (appended A, B per launch by ops._bounds)."""
    pairs = {}
    for i in range(0, len(records), 2):
        (ka, ra, _, ba, _), (kb, rb, _, bb, _) = records[i], records[i + 1]
        assert ka == kb and (ra, rb) == ('A', 'B'), (ka, ra, kb, rb)
        pairs.setdefault((ba.data_ptr(), bb.data_ptr()), set()).add(ka)
    return pairs


# ------------------------------------------------------------------ recipes at reduced geometry
def _seed():
    import torch
    import utils.ops
    from ams_hip import ops
    np.random.seed(1234)
    torch.manual_seed(1234)
    utils.ops.rng.seed(42)          # the reference's module-level initialiser RNG (tests/smoke_step.py)
    ops.PASS[0] += 10


def _front_dpcl(hip_graph):
    from tests.smoke_step import build_front_dpcl
    trainer, tfds = build_front_dpcl(tempfile.mkdtemp(prefix='ams_ra_'), no_summaries=True, hip_graph=hip_graph)
    return trainer, tfds, 1024


def _stft(hip_graph, dilated):
    from models.dpcl import DPCL
    from utils.trainer import STFT_Separator_Trainer
    from tests.test_gpu_recipes import base_args
    B, L, W, hop = 2, 4096, 512, 256                    # F = 257 bins
    a = base_args(batch_size=B, nb_speakers=2, chunk_size=L, window_size=W, hop_size=hop, layer_size=12, nb_layers=2, embedding_size=8,
                  model_folder=None, learning_rate=1e-3, add_dilated=dilated, hip_graph=hip_graph)
    a.pop('type')
    tr = STFT_Separator_Trainer(DPCL, 'STFT_DPCL', **a)
    dist, tfds = tr.prepare()
    return tr, tfds, L


def _stft_enhance(hip_graph):
    from models.dpcl import DPCL
    from utils.trainer import STFT_Separator_enhance_Trainer
    from tests.test_gpu_recipes import base_args, _full_checkpoint
    tmp = tempfile.mkdtemp(prefix='ams_ra_enh_')
    rng = np.random.RandomState(41)
    B, S, L, W, hop, LS, NL, E, tries, steps = 2, 2, 4096, 512, 256, 12, 2, 8, 2, 3
    Fq = W // 2 + 1                                     # the enhance stack reads 2F = 514
    folder, params, P = _full_checkpoint(tmp, rng, W, None, hop, L, B, S, LS, NL, E, Fq, Fq, front=False)
    T = 1 + (L - W) // hop
    # fixed k-means seeds are staged from the host in every pass, which a graph capture refuses: a captured step draws its own
    idx = None if hip_graph else np.stack([rng.choice(T * Fq, S, replace=False) for _ in range(B * tries)]).astype(np.int32)
    a = base_args(**params)
    a.update(model_folder=folder, nb_tries=tries, nb_steps=steps, end_assign=True, kmeans_init_indices=idx, layer_size_enhance=8,
             nb_layers_enhance=2, nonlinearity='softmax', learning_rate=1e-3, pretraining=False, hip_graph=hip_graph)
    a.pop('type')
    tr = STFT_Separator_enhance_Trainer(DPCL, 'STFT_DPCL_enhance', **a)
    dist, tfds = tr.prepare()
    return tr, tfds, L


def _max_pool(hip_graph):
    from utils.trainer import Adapt_Pretrainer
    from tests.test_gpu_recipes import base_args
    B, S, L, W, N, hop, Pool = 2, 2, 1024, 64, 16, 128, 128
    a = base_args(batch_size=B, nb_speakers=S, chunk_size=L, window_size=W, filters=N, hop_size=hop, max_pool=Pool, with_max_pool=True,
                  loss='l2', separation='perfect', overlap_coef=0.0, optimizer='Adam', learning_rate=1e-3, pretraining=True,
                  hip_graph=hip_graph)
    a.pop('type')
    tr = Adapt_Pretrainer(**a)
    dist, tfds = tr.prepare()
    return tr, tfds, L


def _front_finetuning(hip_graph):
    from models.dpcl import DPCL
    from utils.trainer import Front_Separator_Finetuning_Trainer
    from tests.test_gpu_recipes import base_args, _full_checkpoint
    tmp = tempfile.mkdtemp(prefix='ams_ra_ft_')
    rng = np.random.RandomState(21)
    B, S, L, W, N, hop, LS, NL, E, tries, steps, beta = 2, 2, 1024, 64, 16, 16, 12, 2, 8, 1, 3, 4.0
    folder, params, P = _full_checkpoint(tmp, rng, W, N, hop, L, B, S, LS, NL, E, N, N)
    T = -(-L // hop)
    idx = np.stack([rng.choice(T * N, S, replace=False) for _ in range(B * tries)]).astype(np.int32)
    a = base_args(**params)
    a.update(model_folder=folder, nb_tries=tries, nb_steps=steps, beta_kmeans=beta, with_silence=True, threshold=2.0, end_assign=True,
             kmeans_init_indices=idx, loss='sdr+l2', optimizer='RMSProp', learning_rate=1e-4, pretraining=False, hip_graph=hip_graph)
    a.pop('type')
    tr = Front_Separator_Finetuning_Trainer(DPCL, 'front_L41_finetuning', **a)
    dist, tfds = tr.prepare()
    return tr, tfds, L


RECIPES = {
    'front_dpcl': _front_dpcl,                                  # aligned control
    'stft_f257': lambda hg: _stft(hg, False),                   # BLSTM_0 reads D = 257
    'stft_dilated': lambda hg: _stft(hg, True),                 # the conv stack (BLSTM_0 reads 4F = 1028)
    'stft_enhance_2f514': _stft_enhance,                        # the enhance stack reads 2F = 514
    'max_pool': _max_pool,                                      # path B
    'front_finetuning': _front_finetuning,
}


def _build(name, hip_graph=False):
    _seed()
    tr, tfds, L = RECIPES[name](hip_graph)
    feed = {tfds.handle: tfds.get_handle(tfds.TRAIN), tfds.chunk_size: L}
    return tr, tfds, feed


def _audited_step(model, feed, step, monkeypatch):
    """model.train_audited with every bounded launch recorded and the audit's records kept: (cost, new, calls, pairs)."""
    from ams_hip import ops
    kept = []
    finish = ops.F16_AUDIT.finish

    def keep_and_finish():
        kept.extend(ops.F16_AUDIT.records)
        return finish()
    monkeypatch.setattr(ops.F16_AUDIT, 'finish', keep_and_finish)
    try:
        with recording() as rec:
            c, new = model.train_audited(feed, step)
    finally:
        monkeypatch.setattr(ops.F16_AUDIT, 'finish', finish)
    return c, new, rec.calls, audited_pairs(kept)


@pytest.mark.gpu
@pytest.mark.parametrize('recipe', sorted(RECIPES))
def test_every_bounded_launch_of_an_audited_step_is_audited(recipe, monkeypatch):
    from ams_hip import ops
    tr, tfds, feed = _build(recipe)
    before = set(ops.F16_AUDIT.denied)
    try:
        with tr.graph.as_default():
            tfds.initialize(tfds.TRAIN)
            float(tr.model.train(feed, 0))
            c, new, calls, pairs = _audited_step(tr.model, feed, 1, monkeypatch)
        assert np.isfinite(float(c))
        assert calls, 'no bounded launch in the step: fp16x3 is not what it runs'
        missed = sorted(set(n for n, pa, pb, cap in calls if (pa, pb) not in pairs))
        assert not missed, 'bounded launches the audit did not measure: %s' % missed
    finally:
        ops.F16_AUDIT.denied.intersection_update(before)
    ops.raise_on_ring_errors()


@pytest.mark.gpu
@pytest.mark.parametrize('recipe', ['stft_f257', 'stft_enhance_2f514', 'stft_dilated', 'max_pool'])
def test_a_denial_holds_in_every_form_of_the_step(recipe, monkeypatch):
    """limit = -1 denies every audited class.  The eager step under presplit(True) and presplit(False) and the re-captured graph then make
    no bounded launch at all and no pre-split product; costs stay within 1e-4 of a run without the audit."""
    from ams_hip import ops
    steps, audit_at = 10, 2
    costs = {}
    before = set(ops.F16_AUDIT.denied)
    old_limit = ops.F16_AUDIT.limit
    for mode in ('plain', 'denied'):
        tr, tfds, feed = _build(recipe, hip_graph=True)
        model = tr.model
        cs = []
        try:
            with tr.graph.as_default():
                tfds.initialize(tfds.TRAIN)
                for i in range(steps):
                    if mode == 'plain' or i < audit_at:
                        cs.append(float(model.train(feed, i)))
                        continue
                    if i == audit_at:
                        ops.F16_AUDIT.limit = -1.0
                        c, new, calls, pairs = _audited_step(model, feed, i, monkeypatch)
                        ops.F16_AUDIT.limit = old_limit
                        assert new and set(new) == set().union(*pairs.values()), (new, pairs)
                        assert '_cg_state' not in model.__dict__
                        n_ps = ops.PS_LAUNCHES[0]
                        cs.append(float(c))
                        continue
                    with recording() as rec:
                        if i in (audit_at + 1, audit_at + 2):       # eager, in both forms of the forward products
                            hg, model.args['hip_graph'] = model.args.get('hip_graph'), False
                            try:
                                with ops.presplit(i == audit_at + 1):
                                    c = model.train(feed, i)
                            finally:
                                model.args['hip_graph'] = hg
                        else:                                       # warm-ups, the re-capture, replays
                            c = model.train(feed, i)
                        cs.append(float(c))
                    assert not rec.calls, 'step %d: bounded launches of denied classes %s' % (i, sorted(set(r[0] for r in rec.calls)))
                    assert ops.PS_LAUNCHES[0] == n_ps, 'step %d: pre-split products after the denial' % i
                if mode == 'denied':
                    assert '_cg_state' in model.__dict__          # the step was captured again
        finally:
            ops.F16_AUDIT.limit = old_limit
            ops.F16_AUDIT.denied.intersection_update(before)
        costs[mode] = np.array(cs)
        ops.raise_on_ring_errors()
    assert np.isfinite(costs['denied']).all()
    assert np.abs(costs['denied'] - costs['plain']).max() <= 1e-4 * np.abs(costs['plain']).max(), costs


# ------------------------------------------------------------------ kernels against float64 at the range edge
def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()


class _Owner(object):
    pass


@contextlib.contextmanager
def native_f32():
    from ams_hip._lib import load
    lib = load()
    old = lib.ams_gemm_get_arith()
    lib.ams_gemm_set_arith(0)
    try:
        yield
    finally:
        lib.ams_gemm_set_arith(old)


def edge_checks(run, per_slice, key, quiet, forms=(None,)):
    """run(form) -> numpy result; per_slice(result) -> error of every output slice relative to its own scale.
    (i) fp16x3 before any audit is off by > 2^-16 on the quiet slices (the data sits at the edge); (ii) one audited call denies exactly
    `key`; (iii) the denied class, in every form, meets float64 within 1.5x the native f32 MFMA's error, on quiet and on loud slices."""
    from ams_hip import ops
    assert key not in ops.F16_AUDIT.denied
    loud = ~quiet
    report = {}
    try:
        for form in forms:
            e = per_slice(run(form))
            report['fp16x3', form] = (float(np.median(e[quiet])), float(e[loud].max()))
            assert np.median(e[quiet]) > 2.0 ** -16, ('no teeth', form, report)
        ops.F16_AUDIT.begin()
        try:
            run(forms[0])
        finally:
            new = ops.F16_AUDIT.finish()
        assert new == [key], (new, key)
        with native_f32():
            e32 = per_slice(run(forms[0]))
        for form in forms:
            e = per_slice(run(form))
            report['denied', form] = (float(e[quiet].max()), float(e[loud].max()))
            for grp in (quiet, loud):
                assert e[grp].max() <= 1.5 * e32[grp].max(), (form, float(e[grp].max()), float(e32[grp].max()), report)
    finally:
        ops.F16_AUDIT.denied.discard(key)
    print('%s: (median error of the quiet slices | worst of the quiet slices, worst of the loud slices) %r' % (key, report))
    return report


@pytest.mark.gpu
@pytest.mark.parametrize('D', [257, 514, 600])
def test_blstm_input_projection_at_the_range_edge(D):
    """The hoisted BLSTM input projection x . [Wx_f | Wx_b] (ops.blstm_input_projection) with half of the frames 2^-30 quiet: the padded
    product an audit runs (D = 257, 514), the pre-split form and the in-product form are ONE class; 600 is the aligned control."""
    import torch
    from ams_hip import ops
    M, H = 64 * 80, 300
    N = 8 * H
    rng = np.random.RandomState(D)
    x = rng.randn(M, D).astype(np.float32)
    quiet = np.zeros(M, bool)
    quiet[rng.permutation(M)[:M // 2]] = True
    x[quiet] *= QUIET
    W = (rng.randn(D, N) / np.sqrt(D)).astype(np.float32)
    xd, Wd, bias = dev(x), dev(W), torch.zeros(N, device='cuda')
    amax = (ops.absmax(xd), ops.absmax(Wd))
    owner = _Owner()
    x64, W64 = x.astype(np.float64), W.astype(np.float64)
    ref = x64 @ W64
    scale = np.linalg.norm(x64, axis=1)[:, None] * np.linalg.norm(W64, axis=0)[None, :]

    def run(presplit):
        G = torch.empty((M, N), dtype=torch.float32, device='cuda')
        with ops.presplit(presplit):
            ops.blstm_input_projection(xd, Wd, bias, G, amax, owner)
        return G.cpu().numpy()

    def per_slice(G):
        return (np.abs(G - ref) / scale).max(axis=1)

    key = ('gemm', 'blstm_input_gemm', M, N, D, False, False)
    n0 = ops.PS_LAUNCHES[0]
    edge_checks(run, per_slice, key, quiet, forms=(True, False))
    assert ops.PS_LAUNCHES[0] == n0 + 1                 # the pre-split form ran before the denial, and only then


def _dilated_geometry(spec):
    from tests import dilated_ref as ref
    (kh, kw), rate, cout = ref.SPECS[spec]
    return kh, kw, rate, cout


def _patch_norm(a4, kh, kw, rate):
    """|| patch of pixel p ||: sqrt of the sum over channels and the taps of p's dilated SAME window of a4 [B,T,F,C]^2 (float64)."""
    import torch
    sq = torch.as_tensor(np.asarray(a4, np.float64) ** 2).sum(-1)[:, None]
    ones = torch.ones((1, 1, kh, kw), dtype=torch.float64)
    s = torch.nn.functional.conv2d(sq, ones, padding=((kh - 1) // 2 * rate[0], (kw - 1) // 2 * rate[1]), dilation=tuple(rate))
    return np.sqrt(s[:, 0].numpy())


@pytest.mark.gpu
@pytest.mark.parametrize('spec', [2, 8], ids=['rate_r1', 'rate_rr'])
@pytest.mark.parametrize('op', ['fwd', 'bwd_data', 'bwd_filter'])
def test_dilated_conv_layer_at_the_range_edge(op, spec):
    """One 128 -> 128 5x5 layer of the dilated stack at B = 2, T = 79, F = 257.  fwd and dX: the second half of the frames is 2^-30
    quiet, an output pixel is a slice; dW: half of the input channels are quiet, an input channel (all taps, all cout) is a slice."""
    import torch
    from ams_hip import ops
    from tests.dilated_ref import conv_pre
    kh, kw, rate, cout = _dilated_geometry(spec)
    B, T, Fq, cin = 2, 79, 257, 128
    rng = np.random.RandomState(100 + 10 * spec + ['fwd', 'bwd_data', 'bwd_filter'].index(op))
    w = (rng.randn(kh, kw, cin, cout) / np.sqrt(kh * kw * cin)).astype(np.float32)
    a = rng.randn(B, T, Fq, cin).astype(np.float32)            # x (fwd, dW) or dy (dX)
    g = (B, T, Fq, cin, cout, kh, kw, int(rate[0]), int(rate[1]))
    wd = dev(w)
    w64 = torch.as_tensor(w.astype(np.float64))
    pad = ((kh - 1) // 2 * rate[0], (kw - 1) // 2 * rate[1])
    if op == 'bwd_filter':
        a[..., cin // 2:] *= QUIET
        dy = rng.randn(B, T, Fq, cout).astype(np.float32)
        ad, dyd = dev(a), dev(dy)
        amax = (ops.absmax(ad), ops.absmax(dyd))
        x64, dy64 = torch.as_tensor(a.astype(np.float64)), torch.as_tensor(dy.astype(np.float64))
        ref = torch.nn.grad.conv2d_weight(x64.permute(0, 3, 1, 2), (cout, cin, kh, kw), dy64.permute(0, 3, 1, 2), padding=pad,
                                          dilation=tuple(rate)).permute(2, 3, 1, 0).numpy()
        scale = (np.linalg.norm(a.reshape(-1, cin).astype(np.float64), axis=0)[:, None]
                 * np.linalg.norm(dy.reshape(-1, cout).astype(np.float64), axis=0)[None, :])[None, None]
        quiet = np.arange(cin) >= cin // 2

        def run(_):
            return ops.dilated_conv2d_bwd_filter(ad, dyd, wd, rate, amax=amax)[0].cpu().numpy()

        def per_slice(dw):
            return (np.abs(dw - ref) / scale).max(axis=(0, 1, 3))
    else:
        a[:, T // 2:] *= QUIET
        ad = dev(a)
        amax = (ops.absmax(ad), ops.absmax(wd))
        a64 = torch.as_tensor(a.astype(np.float64))
        patch = _patch_norm(a, kh, kw, rate)                        # [B, T, F] (the window is symmetric: dX reads the same patch)
        if op == 'fwd':
            bd = torch.zeros(cout, device='cuda')
            ref = torch.relu(conv_pre(a64, w64, torch.zeros(cout, dtype=torch.float64), rate)).numpy()
            wn = np.linalg.norm(w.reshape(-1, cout).astype(np.float64), axis=0)           # || filter column co ||

            def run(_):
                return ops.dilated_conv2d_fwd(ad, wd, bd, rate, amax=amax, want_amax=False)[0].cpu().numpy()
        else:
            ref = torch.nn.grad.conv2d_input((B, cin, T, Fq), w64.permute(3, 2, 0, 1), a64.permute(0, 3, 1, 2), padding=pad,
                                             dilation=tuple(rate)).permute(0, 2, 3, 1).numpy()
            wn = np.linalg.norm(w.transpose(2, 0, 1, 3).reshape(cin, -1).astype(np.float64), axis=1)   # || w[:, :, ci, :] ||

            def run(_):
                return ops.dilated_conv2d_bwd_data(ad, wd, None, rate, amax=amax, want_amax=False)[0].cpu().numpy()
        scale = patch[..., None] * wn[None, None, None, :]
        t = np.arange(T)
        rt = (kh - 1) // 2 * rate[0]
        qt = t - rt >= T // 2                                       # frames whose whole window is quiet
        lt = t + rt < T // 2                                        # ... loud
        sel = qt | lt
        quiet = np.broadcast_to(qt[None, :, None], (B, T, Fq))[:, sel].reshape(-1)

        def per_slice(y):
            return (np.abs(y - ref) / scale)[:, sel].max(axis=-1).reshape(-1)
    key = ('dilated_' + op,) + g
    edge_checks(run, per_slice, key, quiet)


@pytest.mark.gpu
def test_front_maxpool_at_the_range_edge():
    """Path B's stride-1 conv + max-pool (pooling.front_maxpool_fwd) where the pre-split form applies (L % 128 == 0, N % 4 == 0): the
    second half of every waveform is 2^-30 quiet; a slice is one pooled frame of one signal, all filters; the pooled maxima against
    oracle/front.py in float64."""
    from ams_hip import ops, pooling
    from oracle import front as ofront
    Bt, L, W, N, P, hop = 4, 4096, 256, 64, 128, 128
    rng = np.random.RandomState(77)
    x = rng.randn(Bt, L).astype(np.float32)
    x[:, L // 2:] *= QUIET
    f = (rng.randn(W, N) / np.sqrt(W)).astype(np.float32)
    xd, fd = dev(x), dev(f)
    x64, f64 = x.astype(np.float64), f.astype(np.float64)
    y_ref, _ = ofront.front_maxpool(x64, f64, P, hop)
    T = y_ref.shape[1]
    _, pl, _ = ofront.same_pads(L, W, 1)
    lo = np.arange(T) * hop - pl                                    # sample span of pooled frame t: [lo, hi)
    hi = lo + P + W - 1
    xp = np.concatenate([np.zeros((Bt, pl)), x64, np.zeros((Bt, W))], axis=1)
    span = np.stack([np.linalg.norm(xp[:, l + pl:h + pl], axis=1) for l, h in zip(lo, hi)], axis=1)    # [Bt, T]
    scale = span[:, :, None] * np.linalg.norm(f64, axis=0)[None, None, :]
    qt, lt = lo >= L // 2, hi <= L // 2
    sel = qt | lt
    quiet = np.broadcast_to(qt[None, :], (Bt, T))[:, sel].reshape(-1)

    def run(_):
        return pooling.front_maxpool_fwd(xd, fd, P, hop)[0].cpu().numpy()

    def per_slice(y):
        return (np.abs(y - y_ref) / scale)[:, sel].max(axis=-1).reshape(-1)
    edge_checks(run, per_slice, ('front_maxpool', Bt, L, W, N, P, hop), quiet)


@pytest.mark.gpu
def test_dense_fwd_of_a_transposed_view():
    """dense_fwd on a 2-D input that is a transposed view (stride(1) != 1): float64 result, in both arithmetic classes; forward_product
    itself refuses such an operand instead of reading it with the wrong pitch."""
    import torch
    from ams_hip import ops
    rng = np.random.RandomState(5)
    xt = rng.randn(64, 300).astype(np.float32)
    W = (rng.randn(64, 40) / 8).astype(np.float32)
    b = rng.randn(40).astype(np.float32)
    x = dev(xt).t()
    assert x.stride(1) != 1
    Wd, bd = dev(W), dev(b)
    ref = xt.T.astype(np.float64) @ W.astype(np.float64) + b
    for amax in (None, (ops.absmax(x.contiguous()), ops.absmax(Wd))):
        u = ops.dense_fwd(x, Wd, bd, amax=amax).cpu().numpy()
        assert np.abs(u - ref).max() <= 1e-6 * np.abs(ref).max(), amax is not None
    with pytest.raises(ops.AmsError):
        ops.forward_product(x, Wd, bd, torch.empty((300, 40), device='cuda'), None, '', Wd)
