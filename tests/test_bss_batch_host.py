"""CPU: the batched BSS-eval's boundary -- include/ams_bss_batch.h against the library's exports, the argument checks of
utils.bss_eval.bss_eval_pairs_batch (made before the device is touched), the permutation rule of bss_eval_sources_batch, and
experiments.evaluation.eval.evaluate_batched against evaluate with both library entry points replaced by the numpy oracle."""
import ctypes
import os
import re

import numpy as np
import pytest

from oracle import bss_eval as obss

torch = pytest.importorskip('torch')

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {'ams_bssb_abi_version', 'ams_bssb_create', 'ams_bssb_destroy', 'ams_bssb_workspace_bytes', 'ams_bssb_eval', 'ams_bssb_potrf'}


def test_batch_header_and_exports():
    src = open(os.path.join(ROOT, 'include', 'ams_bss_batch.h')).read()
    src = re.sub(r'/\*.*?\*/', ' ', src, flags=re.S)
    assert set(re.findall(r'\b(ams_\w+)\s*\(', src)) == NAMES
    path = os.path.join(ROOT, 'adaptive-multispeaker-separation_amd', 'ams_hip', 'libams_bss.so')
    if not os.path.exists(path):
        import __graft_entry__
        __graft_entry__.build()
    lib = ctypes.CDLL(path)
    for n in NAMES:
        assert hasattr(lib, n), n
    assert lib.ams_bssb_abi_version() == 1
    assert lib.ams_bss_abi_version() == 1                       # the per-utterance ABI did not move


def test_batch_symbols_stay_out_of_the_product_library():
    import subprocess
    from ams_hip import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    out = subprocess.run(['nm', '-D', '--defined-only', _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert 'ams_bssb_' not in out


@pytest.mark.parametrize('rs,es', [((2, 2, 100), (2, 2, 101)),          # length
                                   ((2, 2, 100), (3, 2, 100)),          # utterances
                                   ((2, 2, 100), (2, 3, 100)),          # sources
                                   ((2, 2, 100), (2, 2, 3, 100)),       # sources, with a set axis
                                   ((2, 100), (2, 100)),                # no utterance axis
                                   ((2, 2, 100), (2, 100)),
                                   ((0, 2, 100), (0, 2, 100))])         # empty batch
def test_pairs_batch_rejects_mismatched_shapes(rs, es, monkeypatch):
    from utils import bss_eval as hb

    def touched(*a, **k):
        raise AssertionError('the device was touched before the shapes were checked')
    monkeypatch.setattr(hb, '_batch_context', touched)
    monkeypatch.setattr(hb, '_load_batch', touched)
    with pytest.raises(hb.BssError):
        hb.bss_eval_pairs_batch(np.zeros(rs), np.zeros(es))
    with pytest.raises(hb.BssError):
        hb.bss_eval_pairs_batch(torch.zeros(rs), torch.zeros(es))


def test_pairs_batch_raises_without_a_gpu():
    from utils import bss_eval as hb
    if torch.cuda.is_available():
        return                                                   # asserted only where there is no GPU
    with pytest.raises(hb.BssError):
        hb.bss_eval_pairs_batch(np.ones((2, 2, 100)), np.ones((2, 2, 100)))
    with pytest.raises(hb.BssError):
        hb.bss_eval_sources_batch(np.ones((2, 2, 100)), np.ones((2, 2, 2, 100)))


def test_sources_batch_permutation_rule(monkeypatch):
    """Best mean SIR; on a tie the first permutation in itertools order wins (np.argmax), as in bss_eval_sources_cupy."""
    from utils import bss_eval as hb
    U, K, S = 2, 2, 3
    rng = np.random.RandomState(3)
    crit = rng.randn(U, K, 3, S, S)
    # (0, 0): estimate e matches reference (e + 1) % 3, i.e. perm[j] = (j - 1) % 3 = [2, 0, 1]
    sir = np.zeros((S, S))
    for e in range(S):
        sir[e, (e + 1) % S] = 30.0
    crit[0, 0, 1] = sir
    # (0, 1): a tie between the identity and the swap of the first two -> the identity (earlier in itertools order) wins
    crit[0, 1, 1] = np.array([[5.0, 5.0, 0.0], [5.0, 5.0, 0.0], [0.0, 0.0, 9.0]])
    # (1, 0): all equal -> identity
    crit[1, 0, 1] = 1.0
    # (1, 1): swap of the last two
    crit[1, 1, 1] = np.array([[9.0, 0.0, 0.0], [0.0, 0.0, 7.0], [0.0, 8.0, 0.0]])
    monkeypatch.setattr(hb, 'bss_eval_pairs_batch', lambda r, e, flen=hb.FLEN, max_utt=hb.MAX_UTT: (crit.copy(), np.zeros(U, np.int32)))
    sdr, sir_o, sar, perm = hb.bss_eval_sources_batch(None, None)
    assert sdr.shape == sir_o.shape == sar.shape == perm.shape == (U, K, S)
    assert perm[0, 0].tolist() == [2, 0, 1] and perm[0, 1].tolist() == [0, 1, 2]
    assert perm[1, 0].tolist() == [0, 1, 2] and perm[1, 1].tolist() == [0, 2, 1]
    dum = np.arange(S)
    for u in range(U):
        for k in range(K):
            for got, c in ((sdr, 0), (sir_o, 1), (sar, 2)):
                assert np.array_equal(got[u, k], crit[u, k, c][perm[u, k], dum])
    out = hb.bss_eval_sources_batch(None, None, compute_permutation=False)
    assert np.array_equal(out[3], np.broadcast_to(dum, (U, K, S)))
    assert np.array_equal(out[1][0, 0], np.diag(crit[0, 0, 1]))


def test_evaluate_batched_matches_evaluate_on_the_oracle(monkeypatch):
    """Both library entry points replaced by stubs on the numpy oracle that return NaN for one chosen utterance: the batched
    loop returns the same means and the same per-utterance array as the per-utterance loop, and skips the same utterance."""
    from experiments.evaluation import eval as ev
    rng = np.random.RandomState(11)
    S, L, flen = 2, 700, 24
    sizes = (3, 2)
    batches = []
    for B in sizes:
        nm = rng.randn(B, S, L)
        for b in range(B):
            for k in range(S):
                nm[b, k] = np.convolve(nm[b, k], rng.randn(6), mode='same')
        batches.append((nm.sum(1), nm, nm + 0.1 * rng.randn(B, S, L)))
    bad = batches[0][1][1]                                       # references of utterance 1 of batch 0

    def stub_single(refs, ests, compute_permutation=True, nsrc=2):
        refs, ests = np.asarray(refs, np.float64).reshape(nsrc, -1), np.asarray(ests, np.float64).reshape(nsrc, -1)
        out = obss.bss_eval_sources(refs, ests, compute_permutation=compute_permutation, flen=flen)
        if np.array_equal(refs, bad):
            return tuple(np.full(nsrc, np.nan) for _ in range(3)) + (out[3],)
        return out

    calls = []

    def stub_batch(refs, ests, compute_permutation=True, **kw):
        refs, ests = np.asarray(refs, np.float64), np.asarray(ests, np.float64)
        U, K, nsrc, _ = ests.shape
        calls.append((U, K))
        res = [np.empty((U, K, nsrc)) for _ in range(3)] + [np.empty((U, K, nsrc), np.int64)]
        for u in range(U):
            for k in range(K):
                o = stub_single(refs[u], ests[u, k], compute_permutation, nsrc)
                for dst, v in zip(res, o):
                    dst[u, k] = v
        return tuple(res)

    monkeypatch.setattr(ev, 'bss_eval_sources_cupy', stub_single)
    monkeypatch.setattr(ev, 'bss_eval_sources_batch', stub_batch)
    means, arr = ev.evaluate(batches, nsrc=S, verbose=False)
    means_b, arr_b = ev.evaluate_batched(batches, nsrc=S, verbose=False)
    assert calls == [(B, 2) for B in sizes]                      # ONE call per batch, two sets
    assert arr.shape == (sum(sizes) - 1, 2, S)                   # the chosen utterance was skipped ...
    assert np.array_equal(arr, arr_b) and means == means_b       # ... by both, and everything else is identical
    assert np.all(np.isfinite(arr_b))
    # the same on CPU tensors (the path device tensors take)
    tb = [tuple(torch.tensor(x) for x in b) for b in batches]
    del calls[:]
    means_t, arr_t = ev.evaluate_batched(tb, nsrc=S, verbose=False)
    assert np.array_equal(arr, arr_t) and means == means_t
