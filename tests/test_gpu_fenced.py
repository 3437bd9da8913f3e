"""GPU: the oracle tests of the neighbouring modules, run again inside a fence (tests/fenced.py).

Every row of ROWS calls one existing test function, unchanged, with
  * its inputs uploaded into fenced payloads where the called module uploads through a module-level `dev` (UPLOADS; the rows of
    INPUTS_NOT_FENCED upload by other means and keep ordinary inputs),
  * every torch.empty / zeros / ... of ams_hip.ops, ams_hip.functional and utils.bss_eval fenced and, for `empty`, NaN-filled,
  * the persistent scratch of ams_hip.ops created afresh inside the fence.
The called test's own assertions are the oracle comparison: an output word a kernel did not store is a NaN there.  fence.check() then
asserts that no word within 64 KiB of any operand, output or workspace changed.

ODD_ROWS runs a subset with every input `base` bytes past a 256-byte boundary (row b of a [B, L] batch with L % 4 != 0, a slice of a
flat buffer): the launch-time choices made on a pointer's alignment take their other arm.  Each row states its outcome: 'passes', or
'refuses' (AmsError from an argument check, before any launch).

The last section checks the scratch buffers that are specified 'zero before the first launch, left zero' (include/ams.h): the
optimizers' amax_slots at ragged grids, the ams_stage_inputs ticket, the hard k-means row tickets, the stream-K flags.

No graph-capturing test is in the tables: fills recorded into a capture are not what this is about."""
import importlib
import inspect

import numpy as np
import pytest

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

from oracle import optim as ooptim
from tests import test_gpu_dispatch_arms as arms
from tests.fenced import Fence

E_ = 'test_gpu_edge_cases'
K1 = 'test_gpu_kernels'
K2 = 'test_gpu_kernels2'
DA = 'test_gpu_danet'
DC = 'test_gpu_dilated_conv'
KS = 'test_gpu_kmeans_soft'
KT = 'test_gpu_kmeans_tries'
MS = 'test_gpu_many_speakers_kernels'
PS = 'test_gpu_gemm_ps'
DX = 'test_gpu_gemm_ps_dx'
BB = 'test_gpu_bss_batch'
DP = 'test_gpu_dispatch_arms'
RA = 'test_gpu_ring_arms'


def _arm(cases, *head):
    """The row of a case table of tests/test_gpu_dispatch_arms.py that starts with `head` (its seed comes with it)."""
    found = [c for c in cases if tuple(c[:len(head)]) == head]
    assert len(found) == 1, (head, found)
    return tuple(found[0])


DANET_SMALLEST = [(3, 50, 8, 2, 'binary'), (3, 50, 8, 2, 'fractional')]          # tests/test_gpu_danet.py: CASES[0], CASES[1]

# (module, test function, its parametrised arguments in the order of its signature)
ROWS = [
    (E_, 'test_gemm_smallest_shapes', (1, 1, 1)), (E_, 'test_gemm_smallest_shapes', (1, 300, 7)),
    (E_, 'test_gemm_smallest_shapes', (129, 1, 129)), (E_, 'test_gemm_smallest_shapes', (2, 2, 4097)),
    (E_, 'test_blstm_single_step_single_row', ()),
    (E_, 'test_dpcl_single_point_and_single_utterance', ()),
    (E_, 'test_front_conv_signal_shorter_than_window', ()),
    (E_, 'test_kmeans_tiny_and_empty_cluster_nan', ()),

    (K1, 'test_gemm', (33, 17, 5, 0, 0)), (K1, 'test_gemm', (4, 8, 12, 1, 1)),
    (K1, 'test_gemm', (130, 70, 45, 0, 0)), (K1, 'test_gemm', (130, 70, 45, 0, 1)),
    (K1, 'test_gemm', (130, 70, 45, 1, 0)), (K1, 'test_gemm', (130, 70, 45, 1, 1)),
    (K1, 'test_gemm', (132, 260, 604, 0, 0)), (K1, 'test_gemm', (132, 260, 603, 0, 1)),
    (K1, 'test_gemm', (131, 260, 604, 1, 0)), (K1, 'test_gemm', (132, 262, 604, 0, 0)),
    (K1, 'test_gemm_strided_and_masked', ()),
    (K1, 'test_front_conv_and_filter', (3, 1000, 128, 8, 48)),
    (K1, 'test_model_front_conv_at_shapes_the_16_byte_fetch_does_not_take', (3, 1001, 128, 8, 48)),
    (K1, 'test_model_front_conv_at_shapes_the_16_byte_fetch_does_not_take', (2, 1000, 126, 8, 48)),
    (K1, 'test_model_front_conv_at_shapes_the_16_byte_fetch_does_not_take', (2, 1000, 128, 6, 48)),
    (K1, 'test_make_masks', ()),
    (K1, 'test_make_masks_counted_for_the_fused_loss', (5, 2, 77, 8, 1.0, 0.25)),
    (K1, 'test_make_masks_counted_for_the_fused_loss', (2, 3, 4097, 40, 1.0, 0.0)),
    (K1, 'test_blstm_layer', (5, 7, 12, 8, '1')), (K1, 'test_blstm_layer', (5, 7, 12, 8, '0')),
    (K1, 'test_blstm_layer', (33, 12, 8, 37, '1')), (K1, 'test_blstm_layer', (33, 12, 8, 37, '0')),
    (K1, 'test_blstm_layer', (4, 5, 6, 336, '1')), (K1, 'test_blstm_layer', (4, 5, 6, 336, '0')),
    (K1, 'test_blstm_layer', (2, 3, 4, 340, '1')), (K1, 'test_blstm_layer', (2, 3, 4, 340, '0')),
    (K1, 'test_backward_ring_as_fp16x3_one_scale_per_row', (5, 7, 12, 8, '1')),
    (K1, 'test_backward_ring_as_fp16x3_one_scale_per_row', (18, 5, 16, 130, '1')),
    (K1, 'test_l2norm_dpcl', (2, 77, 3, 2)), (K1, 'test_l2norm_dpcl', (2, 300, 8, 2)), (K1, 'test_l2norm_dpcl', (2, 2049, 40, 3)),
    (K1, 'test_l2norm_dpcl', (1, 700, 20, 4)), (K1, 'test_l2norm_dpcl', (2, 2561, 40, 8)),
    (K1, 'test_optimizers', ()),
    (K1, 'test_global_norm_clip_and_weight_bound_stay_on_the_device', ()),
    (K1, 'test_gemm_at_b_colsum', (64, 128, 40)), (K1, 'test_gemm_at_b_colsum', (132, 388, 777)),
    (K1, 'test_blstm_under_dropout_wrappers', (5, 7, 12, 10, False)), (K1, 'test_blstm_under_dropout_wrappers', (33, 6, 8, 12, True)),

    (K2, 'test_synth_strided', (3, 640, 64, 6, 16)), (K2, 'test_synth_strided', (2, 1000, 128, 8, 48)),
    (K2, 'test_pair_stats_and_costs', (2,)), (K2, 'test_pair_stats_and_costs', (3,)),
    (K2, 'test_overlap_metric', ()),
    (K2, 'test_apply_masks', ()),
    (K2, 'test_stft_istft', (2, 1500, 128, 32, 1)), (K2, 'test_stft_istft', (4, 2048, 256, 128, 2)),
    (K2, 'test_l41_loss', (True,)), (K2, 'test_l41_loss', (False,)),
    (K2, 'test_l41_loss_from_the_unnormalised_embeddings', (3, 50, None, 2, 0)),
    (K2, 'test_l41_loss_from_the_unnormalised_embeddings', (3, 50, 'k-nearest', 2, 5)),
    (K2, 'test_l41_loss_from_the_unnormalised_embeddings', (20, 33, None, 2, 0)),
    (K2, 'test_l41_loss_from_the_unnormalised_embeddings', (20, 33, 'k-nearest', 2, 5)),
    (K2, 'test_l41_loss_negative_sampling', (True, 'k-nearest', 3, 4)),
    (K2, 'test_kmeans_hard_bit_exact', (2, 4100, 40, 3, 3, True, False)),
    (K2, 'test_kmeans_soft_forward', ()),
    (K2, 'test_maxpool_front_and_sparse_synthesis', (2, 300, 32, 5, 40, 24, 1)),
    (K2, 'test_maxpool_front_and_sparse_synthesis', (4, 512, 64, 16, 128, 128, 2)),
    (K2, 'test_enhance_output_stage', (3, 3, 777, 'tanh')), (K2, 'test_enhance_output_stage', (2, 4, 513, 'softmax')),
    (K2, 'test_l41_speaker_vectors', (True,)),
    (K2, 'test_input_conditioning_matches_oracle', ('sqrt', 'meanstd', 0)),
    (K2, 'test_mask_weighting_and_silence_weights', ('sqrt', 2.0)),
    (K2, 'test_sparsity_kl_and_regulariser_kernels', (5, 7, 3, 0.3)), (K2, 'test_sparsity_kl_and_regulariser_kernels', (9, 64, 16, 0.02)),

    (DA, 'test_reconstruction_cost_and_gradient', DANET_SMALLEST[0]), (DA, 'test_reconstruction_cost_and_gradient', DANET_SMALLEST[1]),
    (DA, 'test_silence_mask_folded_into_the_attractor_pass', (8, 2, 3, 50, 'binary')),
    (DA, 'test_silence_mask_folded_into_the_attractor_pass', (40, 2, 9, 257, 'binary')),
    # the next six rows and the two test_gpu_bss_batch.py rows: INPUTS NOT FENCED (see UPLOADS); outputs, workspaces and scratch are
    # geometry B3T37F65; layers 0 and 12 are the direct f32 kernels that carry no bounds
    (DC, 'test_layer', (0, (3, 37, 65))), (DC, 'test_layer', (6, (3, 37, 65))), (DC, 'test_layer', (12, (3, 37, 65))),
    (KS, 'test_soft_kmeans_backward', (2, 2500, 8, 3, 1, 4, True, False)),
    (KT, 'test_five_tries_per_read_is_bit_exact', (3, 197, 5, 3, False)), (KT, 'test_five_tries_per_read_is_bit_exact', (2, 64, 5, 2, True)),
    (MS, 'test_pair_stats_and_costs', (6,)),
    (MS, 'test_equal_costs_keep_the_lowest_permutation_index', (1, 6, 517)),
    (MS, 'test_equal_costs_keep_the_lowest_permutation_index', (260, 5, 67)),
    (MS, 'test_dpcl_loss', (5, 8)),
    (MS, 'test_soft_kmeans_backward', (2, 2500, 8, 6, 1, 4, True, False)),                  # inputs not fenced (see UPLOADS)
    (PS, 'test_product_matches_float64_and_the_in_product_cut', (100, 40, 45, True)),
    (PS, 'test_product_matches_float64_and_the_in_product_cut', (130, 260, 33, True)),
    (DX, 'test_edges_are_zeros_not_neighbours', (5, 4, 1, 4)),
    # inputs not fenced; their float64 workspaces come from torch.empty in utils/bss_eval.py: fenced by the patch alone
    (BB, 'test_edge_tiles', (37,)),
    (BB, 'test_potrf_depends_on_its_matrix_only', (100,)),
    # the arms whose vector width, row pitch or ownership differ from E = 40's (tests/test_gpu_dispatch_arms.py): five and two float4 per
    # point in the k-means passes, one and four per point in the L41 loss, four Gram tiles and the 4-byte staging of an odd E in the
    # deep-clustering loss
    (DP, 'test_hard_kmeans', _arm(arms.HARD_CASES, 20, 3, 8449, 3, True)), (DP, 'test_hard_kmeans', _arm(arms.HARD_CASES, 8, 4, 8449, 3, True)),
    (DP, 'test_soft_kmeans_forward', _arm(arms.SOFT_FORWARD_CASES, 20, 3, 8449)),
    (DP, 'test_soft_kmeans_forward', _arm(arms.SOFT_FORWARD_CASES, 8, 4, 197)),
    (DP, 'test_l41_loss', (4, 4, True, True)), (DP, 'test_l41_loss', (16, 6, False, False)),
    (DP, 'test_dpcl_from_the_network_output', (60, 4, 2561)), (DP, 'test_dpcl_from_the_network_output', (45, 5, 77)),
    # arms of the ring recurrence (tests/test_gpu_ring_arms.py), plain hand-off: 10 chains padded to 16 (six chains' worth of workgroups
    # must leave without touching anything) in both arithmetics, a last workgroup of one unit, and the largest ring
    (RA, 'test_ring_arm', (65, 5, 8, 61, '1', 'bf16x6_f32')), (RA, 'test_ring_arm', (65, 5, 8, 61, '1', 'fp16x3')),
    (RA, 'test_ring_arm', (17, 6, 8, 97, '1', 'fp16x3')),
    (RA, 'test_ring_arm', (17, 6, 8, 336, '1', 'bf16x6_f32')),
]

# (module, test function, arguments, base, outcome)
ODD_ROWS = [
    (K1, 'test_l2norm_dpcl', (2, 300, 8, 2), 4, 'passes'),
    (K1, 'test_l2norm_dpcl', (2, 2049, 40, 3), 4, 'passes'),
    (K1, 'test_l2norm_dpcl', (2, 2049, 40, 3), 12, 'passes'),
    (K2, 'test_l41_loss', (True,), 4, 'passes'),
    (DA, 'test_reconstruction_cost_and_gradient', DANET_SMALLEST[0], 4, 'passes'),
    (K1, 'test_gemm', (132, 260, 604, 0, 0), 4, 'passes'),
    (K1, 'test_gemm', (4, 8, 12, 1, 1), 4, 'passes'),
    (K1, 'test_gemm_at_b_colsum', (64, 128, 40), 4, 'passes'),
    (K1, 'test_front_conv_and_filter', (3, 1000, 128, 8, 48), 4, 'passes'),
    (K2, 'test_kmeans_hard_bit_exact', (2, 4100, 40, 3, 3, True, False), 4, 'passes'),
    (K2, 'test_kmeans_soft_forward', (), 4, 'passes'),
    (K2, 'test_sparsity_kl_and_regulariser_kernels', (9, 64, 16, 0.02), 4, 'passes'),
    (K1, 'test_blstm_layer', (5, 7, 12, 8, '1'), 4, 'passes'),
    (K1, 'test_blstm_layer', (5, 7, 12, 8, '0'), 4, 'passes'),
    (K1, 'test_optimizers', (), 4, 'passes'),
    (DP, 'test_hard_kmeans', _arm(arms.HARD_CASES, 20, 3, 8449, 3, True), 4, 'passes'),
    (DP, 'test_l41_loss', (4, 4, True, True), 4, 'passes'),
    # rows of 4H = 244 floats stay 16-byte multiples, so x, the kernels and dout are all 4 bytes off as a slice of a flat buffer would be
    (RA, 'test_ring_arm', (65, 5, 8, 61, '1', 'bf16x6_f32'), 4, 'passes'),
]


def _id(row):
    return '%s.%s%s%s' % (row[0].replace('test_gpu_', ''), row[1].replace('test_', ''),
                          '[%s]' % '-'.join(str(a).replace(' ', '') for a in row[2]) if row[2] else '',
                          '@%d' % row[3] if len(row) > 3 else '')


@pytest.fixture(scope='module')
def ops():
    from ams_hip import ops as o
    return o


@pytest.fixture(scope='module')
def F():
    from ams_hip import functional as f
    return f


def host(t):
    torch.cuda.synchronize()
    return t.detach().cpu().numpy()


# How a module's inputs reach the device.  'dev': through its module-level dev(x[, dtype]), replaced by fence.dev for the call -- these
# inputs are fenced and can be given an odd base.  'not fenced': the module has no dev; it uploads with torch.from_numpy(a).cuda() /
# .to(d) (test_gpu_dilated_conv.py, test_gpu_kmeans_soft.py, test_gpu_kmeans_tries.py) or hands numpy arrays to utils/bss_eval.py
# (test_gpu_bss_batch.py), which the fence does not reach: in those rows the INPUTS ARE ORDINARY UPLOADS, and only the outputs, the
# workspaces and the persistent scratch are fenced and NaN-filled.  A load past the end of an input of conv2d.hip, of the soft k-means
# backward or of the five-tries kernels is therefore not seen by these rows (the hard and soft k-means FORWARD kernels read fenced
# inputs in the test_gpu_kernels2.py rows).  test_gpu_many_speakers_kernels.py::test_soft_kmeans_backward calls
# test_gpu_kmeans_soft.py's test and is 'not fenced' in the same way.
UPLOADS = {E_: 'dev', K1: 'dev', K2: 'dev', DA: 'dev', PS: 'dev', DX: 'dev', MS: 'dev', DP: 'dev', RA: 'dev',
           DC: 'not fenced', KS: 'not fenced', KT: 'not fenced', BB: 'not fenced'}
INPUTS_NOT_FENCED = [(DC, 'test_layer'), (KS, 'test_soft_kmeans_backward'), (KT, 'test_five_tries_per_read_is_bit_exact'),
                     (MS, 'test_soft_kmeans_backward'), (BB, 'test_edge_tiles'), (BB, 'test_potrf_depends_on_its_matrix_only')]


SK_ENTRIES = [0]


def _stream_k_flags(ops, what):
    """The flag area of every stream-K scratch made inside the current fence (ops._sk: 'every launch leaves them zero')."""
    torch.cuda.synchronize()
    dirty = [key for key, t in ops._SK.items() if bool(t[:2048].view(torch.int32).ne(0).any())]
    SK_ENTRIES[0] += len(ops._SK)
    assert not dirty, (what, dirty)


def _run(row, ops, F, monkeypatch, base=0):
    mod = importlib.import_module('tests.' + row[0])
    fn = getattr(mod, row[1])
    given = {'ops': ops, 'F': F, 'monkeypatch': monkeypatch}
    names = list(inspect.signature(fn).parameters)
    free = [n for n in names if n not in given]
    assert len(free) == len(row[2]), (free, row[2])
    kw = dict(zip(free, row[2]))
    kw.update((n, given[n]) for n in names if n in given)
    uploaded = [0]

    def dev(x, dtype=np.float32):
        uploaded[0] += 1
        return fence.dev(x, dtype, base=base)

    with Fence() as fence:
        assert hasattr(mod, 'dev') == (UPLOADS[row[0]] == 'dev'), row[0]
        if UPLOADS[row[0]] == 'dev':
            monkeypatch.setattr(mod, 'dev', dev)
        else:
            assert base == 0, 'these inputs cannot be given a base'
        fn(**kw)
        assert (uploaded[0] == 0) == ((row[0], row[1]) in INPUTS_NOT_FENCED), (row[0], row[1], uploaded[0])
        fence.check()
        _stream_k_flags(ops, _id(row))


@pytest.mark.parametrize('row', ROWS, ids=_id)
def test_inside_a_fence(row, ops, F, monkeypatch):
    _run(row, ops, F, monkeypatch)


def test_stream_k_flags_were_left_zero_in_every_fence(ops, F, monkeypatch):
    """Every row above asserted, before its fence closed, that the first 2048 words of each ops._SK entry made inside it were zero; this
    one holds that there were such entries at all.  (One product that takes the scratch is run here too, so that the statement is not
    empty when this test is selected alone.)"""
    _run((K1, 'test_gemm', (132, 260, 604, 0, 0)), ops, F, monkeypatch)
    assert SK_ENTRIES[0] > 0


@pytest.mark.parametrize('row', ODD_ROWS, ids=_id)
def test_from_an_odd_base(row, ops, F, monkeypatch):
    from ams_hip._lib import AmsError
    assert row[4] in ('passes', 'refuses')
    if row[4] == 'refuses':
        with pytest.raises(AmsError):
            _run(row, ops, F, monkeypatch, base=row[3])
    else:
        _run(row, ops, F, monkeypatch, base=row[3])


@pytest.mark.parametrize('base', [0, 4, 8, 12])
def test_absmax_from_every_base(ops, base):
    """ams_absmax_f32 chooses between 16-byte and 4-byte loads on its pointer; n = 4099 = one 16-byte body of 1024 and a tail of 3."""
    x = np.random.RandomState(base).randn(4099).astype(np.float32)
    x[4098 - base] = -7.5                                            # the maximum sits in the tail / near it
    with Fence() as fence:
        xd = fence.dev(x, base=base)
        assert xd.data_ptr() % 16 == base
        got = ops.absmax(xd)
        assert float(host(got)[0]) == float(np.abs(x).max())
        fence.check()


# ---------------------------------------------------------------------------------------------------------- persistent scratch
def _rel(a, b):
    b = np.asarray(b, np.float64)
    return np.abs(np.asarray(a, np.float64) - b).max() / max(np.abs(b).max(), 1e-30)


@pytest.mark.parametrize('n', [200, 16128, 16384, 16385, 25601, 524301])
def test_optimizer_bound_fold_at_ragged_grids(ops, n):
    """amax_slots / bound_out of the three optimizer entry points (include/ams.h) at 1, 63, 64, 65, 101 and the capped 2048 workgroups
    (csrc/elementwise.hip: stream_blocks): the in-launch fold counts ragged groups of workgroups per slot.  Three steps on the same
    slots; after each: p against the float64 oracle (the 1e-5 of test_gpu_kernels.py::test_optimizers), the bound exactly max |p|, all
    192 slot words zero.  Then a step with the skip word set changes nothing."""
    lib = ops.load()
    rng = np.random.RandomState(n)
    p0, g = rng.randn(n), rng.randn(3, n)
    _p, _s = ops._p, ops._s
    with Fence() as fence:
        for kind in ('amsgrad', 'rmsprop', 'momentum'):
            p = fence.dev(p0)
            pr = p0.copy()
            slots = torch.zeros(192, dtype=torch.int32, device='cuda')
            bound = torch.zeros(1, dtype=torch.float32, device='cuda')
            skip = torch.zeros(1, dtype=torch.int32, device='cuda')
            if kind == 'amsgrad':
                ref = ooptim.AMSGrad(0.01)
                state = [torch.zeros_like(p), torch.zeros_like(p), torch.zeros_like(p)]
            elif kind == 'rmsprop':
                ref = ooptim.RMSProp(0.01)
                state = [torch.ones(n, dtype=torch.float32, device='cuda')]
            else:
                ref = ooptim.Momentum(0.01)
                state = [torch.zeros(n, dtype=torch.float32, device='cuda')]
            b1p, b2p = [0.9], [0.99]

            def step(gd):
                if kind == 'amsgrad':
                    lr_t = 0.01 * np.sqrt(1 - b2p[0]) / (1 - b1p[0])
                    ops.check(lib.ams_opt_amsgrad(_p(p), _p(gd), _p(state[0]), _p(state[1]), _p(state[2]), n, lr_t, 0.9, 0.99, 1e-3, 1.0,
                                                  _p(skip), _p(slots), _p(bound), _p(None), _s()), 'ams_opt_amsgrad')
                elif kind == 'rmsprop':
                    ops.check(lib.ams_opt_rmsprop(_p(p), _p(gd), _p(state[0]), n, 0.01, 0.9, 1e-10, 1.0, _p(skip), _p(slots), _p(bound),
                                                  _p(None), _s()), 'ams_opt_rmsprop')
                else:
                    ops.check(lib.ams_opt_momentum(_p(p), _p(gd), _p(state[0]), n, 0.01, 0.9, 1.0, _p(skip), _p(slots), _p(bound),
                                                   _p(None), _s()), 'ams_opt_momentum')

            for k in range(3):
                step(fence.dev(g[k]))
                b1p[0] *= 0.9
                b2p[0] *= 0.99
                ref.apply([pr], [g[k]])
                got = host(p)
                assert _rel(got, pr) < 1e-5, (kind, k)
                assert float(host(bound)[0]) == float(np.abs(got).max()), (kind, k)
                assert not host(slots).any(), (kind, k, np.nonzero(host(slots))[0])
            skip.fill_(1)
            before = [host(t).copy() for t in [p, bound, slots] + state]
            step(fence.dev(g[0]))
            after = [host(t) for t in [p, bound, slots] + state]
            for a, b in zip(before, after):
                assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), kind
            fence.check()


@pytest.mark.parametrize('want_amax', [True, False])
def test_stage_inputs_copies_bounds_and_leaves_its_ticket_zero(ops, monkeypatch, want_amax):
    """ops.stage_inputs (ams_stage_inputs: one launch stages a batch into the static buffers of a captured step): four sizes in turn on
    the same destination -- the same cache entry, the same scratch -- with a 7-byte second pair."""
    monkeypatch.setattr(ops, 'F16X3', True)
    rng = np.random.RandomState(11)
    with Fence() as fence:
        dst = torch.empty(300000, dtype=torch.float32, device='cuda')
        dst2 = torch.empty(7, dtype=torch.uint8, device='cuda')
        for n in (1000, 1003, 300000, 1000):
            x = (rng.randn(n) * np.exp(rng.randn(n))).astype(np.float32)
            b2 = rng.randint(0, 256, 7).astype(np.uint8)
            dst.fill_(7.0)
            dst2.fill_(0)
            am = ops.stage_inputs(fence.dev(x), dst[:n], fence.dev(b2, np.uint8), dst2, want_amax=want_amax)
            got = host(dst)
            assert np.array_equal(got[:n].view(np.uint32), x.view(np.uint32)), n
            assert (got[n:] == 7.0).all(), n
            assert np.array_equal(host(dst2), b2), n
            if want_amax:
                assert float(host(am)[0]) == float(np.abs(x).max()), n
            else:
                assert am is None
            assert list(ops._STAGE) == [(dst.device.index, dst.data_ptr())]
            scratch = ops._STAGE[(dst.device.index, dst.data_ptr())][0]
            assert int(host(scratch)[0]) == 0, n
            fence.check()


def test_hard_kmeans_leaves_its_row_tickets_zero(ops):
    """ops.kmeans_run on the persistent row tickets (ops._KM_TICKETS, include/ams.h: zero before the first use and left zero): a shape,
    another shape with five restarts per read, and the first shape again -- same labels, centroids and best restart as the first time."""
    def data(seed, b, tries, L, E, C):
        rng = np.random.RandomState(seed)
        centers = rng.randn(C, E).astype(np.float32) * 2.0
        X = (centers[rng.randint(0, C, (b, L))] + rng.randn(b, L, E).astype(np.float32) * 0.7).astype(np.float32)
        idx = np.stack([rng.choice(L, C, replace=False) for _ in range(b * tries)]).astype(np.int32)
        return X, idx

    runs = []
    with Fence() as fence:
        for seed, (b, tries, L) in ((1, (2, 2, 4100)), (2, (3, 5, 197)), (1, (2, 2, 4100))):
            X, idx = data(seed, b, tries, L, 40, 3)
            xn = ops.kmeans_normalize(fence.dev(X))
            for end in (True, False):
                cent, lab, best, _ = ops.kmeans_run(xn, fence.dev(idx, np.int32), 3, tries, 3, assign_at_end=end)
                runs.append((host(cent), host(lab), host(best)))
                assert runs[-1][1].min() >= 0 and runs[-1][1].max() < 3
                assert 0 <= runs[-1][2].min() and runs[-1][2].max() < tries
                assert len(ops._KM_TICKETS) == 1
                for t in ops._KM_TICKETS.values():
                    assert not host(t).any()
            fence.check()
    for first, third in zip(runs[0:2], runs[4:6]):
        for a, b in zip(first, third):
            assert a.shape == b.shape and a.tobytes() == b.tobytes()     # (bit for bit: an empty cluster's NaN centroid included)
