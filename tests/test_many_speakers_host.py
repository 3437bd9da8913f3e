"""CPU: five and six speakers on the host side -- every separator but the DANet-SCE one constructs (with hard and with soft k-means
settings), seven is refused with the limit and its reason, L41ModelV2 stops at four, and the permutation table the PIT search reads
is the oracle's: 720 rows in lexicographic order.  No kernel is launched."""
import os
import tempfile

import numpy as np
import pytest

os.environ.setdefault('AMS_LOG_DIR', tempfile.mkdtemp(prefix='ams_log_'))

KMEANS = {'hard': dict(beta_kmeans=None, nb_tries=2, nb_steps=3, end_assign=True),
          'soft': dict(beta_kmeans=4.0, nb_tries=1, nb_steps=3, end_assign=True, with_silence=True, threshold=2.0)}


def _args(**kw):
    from ams_hip import testing
    a = dict(testing.ADAPT_DEFAULTS)
    a.update(testing.SEPARATOR_DEFAULTS)
    a.update(testing.ENHANCE_DEFAULTS)
    a.update(kw)
    a.pop('type', None)
    return a


def _stft_trainer(separator, typ, S, **kw):
    from utils.trainer import STFT_Separator_Trainer
    a = _args(batch_size=2, nb_speakers=S, chunk_size=2048, window_size=64, hop_size=32, layer_size=12, nb_layers=2, embedding_size=8,
              model_folder=None, learning_rate=1e-3, **kw)
    tr = STFT_Separator_Trainer(separator, typ, **a)
    tr.prepare()
    return tr


def _pretrainer(S):
    from utils.trainer import Adapt_Pretrainer
    a = _args(batch_size=2, nb_speakers=S, chunk_size=1024, window_size=64, filters=16, hop_size=16, loss='sdr+l2', separation='mask',
              overlap_coef=1.0, optimizer='Adam', learning_rate=1e-3, pretraining=True)
    tr = Adapt_Pretrainer(**a)
    tr.prepare()
    return tr


@pytest.mark.parametrize('S', [5, 6])
def test_adapt_constructs(S):
    tr = _pretrainer(S)
    assert tr.model.S == S


@pytest.mark.parametrize('kmeans', ['hard', 'soft'])
@pytest.mark.parametrize('S', [5, 6])
def test_dpcl_and_l41_construct(S, kmeans):
    from models.dpcl import DPCL
    from models.L41 import L41Model
    for sep, typ in ((DPCL, 'STFT_DPCL'), (L41Model, 'STFT_L41')):
        tr = _stft_trainer(sep, typ, S, **KMEANS[kmeans])
        assert tr.model.S == S and isinstance(tr.model, sep)
        assert tr.model.beta == KMEANS[kmeans]['beta_kmeans']


def test_seven_speakers_are_refused_with_the_limit_and_its_reason():
    from models.dpcl import DPCL
    with pytest.raises(ValueError, match='at most 6') as e:
        _stft_trainer(DPCL, 'STFT_DPCL', 7)
    assert 'BSS-eval' in str(e.value) and 'permutation' in str(e.value)
    with pytest.raises(ValueError, match='at most 6'):
        _pretrainer(7)


def test_l41modelv2_stops_at_four():
    from models.SC_V2 import L41ModelV2
    with pytest.raises(ValueError, match='L41ModelV2.*at most 4'):
        _stft_trainer(L41ModelV2, 'STFT_DANet_SCE', 5)
    assert _stft_trainer(L41ModelV2, 'STFT_DANet_SCE', 4).model.S == 4


def test_permutation_table_is_the_oracles():
    from ams_hip import functional as F
    from oracle import losses as olosses
    ref = np.asarray(olosses.perms(6))
    tab = F._perm_table(6, 'cpu').numpy()
    assert tab.shape == ref.shape == (720, 6)
    assert np.array_equal(tab, ref)
    assert all(tuple(tab[i]) < tuple(tab[i + 1]) for i in range(719))            # lexicographic: index order is the tie rule's order
    t32 = F._perm_table32(6, 'cpu')
    assert t32.dtype.is_floating_point is False and t32.element_size() == 4 and np.array_equal(t32.numpy(), ref)
