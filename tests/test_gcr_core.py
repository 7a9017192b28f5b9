"""The coefficient core that the three host GCRs share (csrc/gcr_core.h) through its host hook qudaAmdGcrBackSubstitute: the symbol is exported
and declared, and the back substitution solves T delta = alpha, T = diag(gamma) + the strict upper triangle of beta, no GPU needed.

Bound: substitution is componentwise backward stable, |T delta - alpha| <= gamma_k (|T| |delta|) elementwise with gamma_k ~ k u, u = 2^-52
(Higham, Accuracy and Stability of Numerical Algorithms, theorem 8.5), and a factor 4 for complex products and quotients.  The residual
itself is formed in extended precision, so that the check adds no rounding of the size it bounds."""
import importlib
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
qa = importlib.import_module("quda-qkxtm-multigrid_amd")

HOOK = "qudaAmdGcrBackSubstitute"
NK = 20
U = 2.0 ** -52


def test_hook_is_exported_and_declared():
    assert hasattr(qa.lib(), HOOK)
    assert HOOK in qa.EXT_H_SYMBOLS
    header = open(os.path.join(ROOT, "include", "quda_amd_ext.h")).read()
    proto = re.search(r"\bvoid %s\s*\(int k, int nK, const double \*alpha, const double \*beta, const double \*gamma, double \*delta\)" % HOOK, header)
    assert proto
    fn = getattr(qa.lib(), HOOK)
    assert len(fn.argtypes) == proto.group(0).count(",") + 1 and fn.restype is None


def _coefficients(k, seed):
    """alpha[k] complex normal, beta[NK][NK] with |beta_ij| <= 1 everywhere (also below the diagonal and beyond k, which must not be read),
    gamma[k] in [0.5, 2]"""
    rng = np.random.default_rng(seed)
    alpha = rng.standard_normal(k) + 1j * rng.standard_normal(k)
    beta = rng.uniform(0.0, 1.0, (NK, NK)) * np.exp(2j * np.pi * rng.uniform(0.0, 1.0, (NK, NK)))
    gamma = rng.uniform(0.5, 2.0, k)
    return alpha, beta, gamma


def _backward_error(alpha, beta, gamma, delta, keep=None):
    """largest |T delta - alpha|_i / (|T| |delta|)_i over the rows in `keep` (all of them by default) of the k x k system"""
    k = alpha.shape[0]
    keep = np.arange(k) if keep is None else keep
    T = (np.diag(gamma) + np.triu(beta[:k, :k], 1))[np.ix_(keep, keep)].astype(np.clongdouble)
    d = delta[keep].astype(np.clongdouble)
    res = np.abs(T @ d - alpha[keep].astype(np.clongdouble))
    scale = np.abs(T) @ np.abs(d)
    return float(np.max(res / scale))


@pytest.mark.parametrize("k", [1, 2, 10, 20])
def test_back_substitution_solves_the_triangular_system(k):
    alpha, beta, gamma = _coefficients(k, 100 + k)
    delta = qa.gcr_back_substitute(alpha, beta, gamma)
    assert delta.shape == (k,) and np.all(np.isfinite(delta))
    err = _backward_error(alpha, beta, gamma, delta)
    print("k = %d of nK = %d: componentwise backward error %.3e (bound %.3e)" % (k, NK, err, 4 * k * U))
    assert err <= 4 * k * U


@pytest.mark.parametrize("a", [0, 4, 9])
def test_a_direction_with_zero_norm_gets_a_zero_coefficient(a):
    """an all-zero padding column of the lockstep GCR on block fields: gamma_a = alpha_a = 0 and no overlap with any other direction"""
    k = 10
    alpha, beta, gamma = _coefficients(k, 200 + a)
    gamma[a] = 0.0
    alpha[a] = 0.0
    beta[a, :] = 0.0
    beta[:, a] = 0.0
    delta = qa.gcr_back_substitute(alpha, beta, gamma)
    assert delta[a] == 0
    assert not np.any(np.isnan(delta.real)) and not np.any(np.isnan(delta.imag))
    keep = np.array([i for i in range(k) if i != a])
    err = _backward_error(alpha, beta, gamma, delta, keep)
    print("k = %d without direction %d: componentwise backward error %.3e (bound %.3e)" % (k, a, err, 4 * (k - 1) * U))
    assert err <= 4 * (k - 1) * U
