"""What the BSS-eval tests share -- test infrastructure only: the pinned reference vectors, the dB rule, the coloured test mixtures and
the numpy oracle run per (recording, set).

dB rule: 1e-6 dB where the expected value is below 100 dB, "stays above 100 dB" above."""
import os

import numpy as np

from oracle import bss_eval as obss

G = np.load(os.path.join(os.path.dirname(__file__), 'golden', 'bss_eval.npz'))
TOL_DB = 1e-6


def close_db(got, ref, tol=TOL_DB):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    small = ref < 100.0
    err = np.abs(got[small] - ref[small]).max(initial=0.0)
    print('max |dB error| below 100 dB: %.3e (tol %.1e); min above: %s' % (err, tol, got[~small].min(initial=np.inf)))
    assert err < tol, (got, ref)
    assert (got[~small] > 100.0).all(), (got, ref)
    return err


def cupy_db(name):
    """The reference's GPU-path dB convention (_safe_db_cupy, utils/bss_eval.py:742-748) from the stored reference energies."""
    e = G[name + '/energies']
    ea = G[name + '/e_artif_energy']
    db = lambda num, den: 10.0 * np.log10(num / (den + 1e-12))      # noqa: E731
    return np.stack([db(e[..., 0], e[..., 1]), db(e[..., 0], e[..., 2]), db(e[..., 3], ea)])


def mix(rng, nsrc, L):
    s = rng.randn(nsrc, L)
    for i in range(nsrc):                                     # colour the sources so the Gram matrices are not near-identity
        s[i] = np.convolve(s[i], rng.randn(8 + 3 * i), mode='same')
    a = rng.randn(nsrc, nsrc) * 0.3 + np.eye(nsrc)
    est = a.dot(s) + 0.05 * rng.randn(nsrc, L)
    return s, est


def oracle(refs, ests, flen):
    """refs[r]: [S, L_r], ests[r]: [K, S, L_r] (a list, or arrays with a leading axis) -> crit [R, K, 3, S, S] and perm [R, K, S] from
    oracle/bss_eval.py on each recording alone."""
    R, (K, S, _) = len(refs), ests[0].shape
    crit, perm = np.empty((R, K, 3, S, S)), np.empty((R, K, S), np.int64)
    for r in range(R):
        for k in range(K):
            o = obss.bss_eval_sources(refs[r], ests[r][k], flen=flen, return_matrices=True)
            crit[r, k], perm[r, k] = np.stack(o[4]), o[3]
    return crit, perm
