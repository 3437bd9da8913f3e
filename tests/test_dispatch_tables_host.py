"""CPU: an (embedding_size, nb_speakers) pair outside a kernel family's table (include/ams.h; ams_hip/ops.py states them once on the
host side) is refused when the model is CONSTRUCTED, with the table in the message -- not as AMS_E_INVALID_ARG at the first inference
of a model that trained to the end, nor in the first backward() of a fine-tuning step whose forward ran.  No kernel is launched.
(tests/test_gpu_dispatch_arms.py holds the same tables against the library's answers.)"""
import os
import re

import pytest

from tests.test_many_speakers_host import KMEANS, _args

HEADER = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'include', 'ams.h')


def _trainer(separator, typ, E, S, **kw):
    from utils.trainer import STFT_Separator_Trainer
    a = _args(batch_size=2, nb_speakers=S, chunk_size=2048, window_size=64, hop_size=32, layer_size=12, nb_layers=2, embedding_size=E,
              model_folder=None, learning_rate=1e-3, **kw)
    tr = STFT_Separator_Trainer(separator, typ, **a)
    tr.prepare()
    return tr


def _separates(model):
    """What the inference recipes touch (utils/trainer.py WIRING: ('touch', 'separate')): builds the k-means."""
    with model.graph.as_default():
        model.separate
    return model


def test_host_tables_are_the_headers():
    """The three sentences of include/ams.h the host tables restate; a change of either side without the other fails here."""
    from ams_hip import ops
    src = re.sub(r'\s*\n\s*\*\s*', ' ', open(HEADER).read())
    assert '1 <= S <= 6 (ABI 9; was 4), E in {3, 4, 8, 16, 20, 32, 40}: all four entry points.' in src
    assert 'ams_kmeans_iterate / ams_kmeans_assign: (E, C) in {40, 8} x {2 .. 6} or {20} x {2, 3}' in src
    assert 'ams_kmeans_soft_bwd: (40, 2 .. 6), (8, 2 | 3 | 5 | 6), (20, 2)' in src
    assert ops.LOSS_E == (3, 4, 8, 16, 20, 32, 40) and ops.L41_MAX_S == 6 and ops.DANET_MAX_S == 4
    assert ops.KMEANS_PAIRS == {(E, C) for E in (40, 8) for C in range(2, 7)} | {(20, 2), (20, 3)}
    assert ops.KMEANS_SOFT_FWD_PAIRS == ops.KMEANS_PAIRS
    assert ops.KMEANS_SOFT_BWD_PAIRS == {(40, C) for C in range(2, 7)} | {(8, 2), (8, 3), (8, 5), (8, 6), (20, 2)}
    assert ops.KMEANS_SOFT_BWD_PAIRS < ops.KMEANS_SOFT_FWD_PAIRS
    assert (ops.DPCL_MAX_S, ops.DPCL_MAX_E_PLUS_S) == (8, 64)


@pytest.mark.parametrize('kmeans', ['hard', 'soft'])
@pytest.mark.parametrize('S', [2, 3, 4, 5, 6])
@pytest.mark.parametrize('E', [40, 8])
def test_recipe_sizes_construct_and_separate(E, S, kmeans):
    from models.dpcl import DPCL
    from models.L41 import L41Model
    for sep, typ in ((DPCL, 'STFT_DPCL'), (L41Model, 'STFT_L41')):
        m = _separates(_trainer(sep, typ, E, S, **KMEANS[kmeans]).model)
        assert (m.embedding_size, m.S, m.kmeans.nb_clusters) == (E, S, S)


@pytest.mark.parametrize('S', [2, 3, 4])
@pytest.mark.parametrize('E', [40, 8])
def test_danet_sce_sizes_construct_and_separate(E, S):
    from models.SC_V2 import L41ModelV2
    m = _separates(_trainer(L41ModelV2, 'STFT_DANet_SCE', E, S, **KMEANS['hard']).model)
    assert (m.embedding_size, m.S) == (E, S)


def test_twenty_wide_embeddings_separate_two_and_three_speakers_only():
    from models.dpcl import DPCL
    for S in (2, 3):
        assert _separates(_trainer(DPCL, 'STFT_DPCL', 20, S, **KMEANS['hard']).model).kmeans.nb_clusters == S
    m = _trainer(DPCL, 'STFT_DPCL', 20, 4, **KMEANS['hard']).model          # the loss takes (20, 4): a training model constructs
    with pytest.raises(ValueError, match=r'--embedding_size 20 --nb_speakers 4: no k-means kernel') as e:
        _separates(m)
    assert '(40, 2|3|4|5|6), (20, 2|3), (8, 2|3|4|5|6)' in str(e.value)


def test_fifty_wide_embeddings_train_and_are_refused_where_they_would_separate():
    from models.dpcl import DPCL
    m = _trainer(DPCL, 'STFT_DPCL', 50, 2, **KMEANS['hard']).model          # a loss (E + S <= 64) and no k-means
    assert m.embedding_size == 50 and not hasattr(m, 'kmeans')
    with pytest.raises(ValueError, match='no k-means kernel'):
        _separates(m)
    with pytest.raises(ValueError, match=r'embedding_size \+ nb_speakers <= 64'):
        _trainer(DPCL, 'STFT_DPCL', 62, 3, **KMEANS['hard'])


def test_l41_and_danet_refuse_an_embedding_size_without_a_kernel():
    from models.L41 import L41Model
    from models.SC_V2 import L41ModelV2
    with pytest.raises(ValueError, match=r'--embedding_size 5 --nb_speakers 2: the L41 loss kernels') as e:
        _trainer(L41Model, 'STFT_L41', 5, 2, **KMEANS['hard'])
    assert '3, 4, 8, 16, 20, 32, 40' in str(e.value)
    with pytest.raises(ValueError, match='the DANet reconstruction kernels'):
        _trainer(L41ModelV2, 'STFT_DANet_SCE', 64, 2, **KMEANS['hard'])
    assert _trainer(L41Model, 'STFT_L41', 32, 1, **KMEANS['hard']).model.embedding_size == 32


@pytest.mark.parametrize('E,S', [(8, 4), (20, 3)])
def test_soft_kmeans_under_a_finetuning_cost_needs_the_backward_table(E, S):
    """The forward/backward seam: the soft forward takes (8, 4) and (20, 3), ams_kmeans_soft_bwd refuses both.  Such a model separates
    (no gradient), and is refused where a fine-tuning cost is wired on top of its k-means."""
    from models.dpcl import DPCL
    m = _separates(_trainer(DPCL, 'STFT_DPCL', E, S, **KMEANS['soft']).model)
    assert m.kmeans.beta == KMEANS['soft']['beta_kmeans']
    from ams_hip import separate_host
    with pytest.raises(ValueError, match='has no backward kernel') as e:
        separate_host.require_soft_kmeans_backward(m)
    assert 'ams_kmeans_soft_bwd' in str(e.value) and 'ams_kmeans_iterate' in str(e.value)
    with pytest.raises(ValueError, match='has no backward kernel'):
        with m.graph.as_default():
            m.cost_finetuning
    hard = _separates(_trainer(DPCL, 'STFT_DPCL', E, S, **KMEANS['hard']).model)
    separate_host.require_soft_kmeans_backward(hard)                        # a hard k-means has no backward


def test_functional_kmeans_checks_the_backward_table_before_any_launch():
    """F.kmeans on CPU tensors: with gradient the refusal comes first (AmsError naming both tables); without, the call goes on to the
    kernels and fails on the CPU tensor instead -- the table check is not what stopped it."""
    import torch
    from ams_hip import functional as F
    from ams_hip._lib import AmsError
    X = torch.randn(2, 64, 8)
    idx = torch.zeros(2, 4, dtype=torch.int32)
    with pytest.raises(AmsError, match=r'\(E, C\) = \(8, 4\)') as e:
        F.kmeans(X.clone().requires_grad_(), idx, 4, 1, 2, 3.0, None, True)
    assert 'ams_kmeans_soft_bwd' in str(e.value) and 'ams_kmeans_iterate' in str(e.value)
    with pytest.raises(AmsError, match='device tensors'):
        F.kmeans(X, idx, 4, 1, 2, 3.0, None, True)
