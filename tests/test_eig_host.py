"""Host side of the exact deflation of the loops: the new symbols are exported, and qudaAmdHostSymmetricEig (cyclic Jacobi, what the
Lanczos eigensolver diagonalises its projected matrix with) against numpy.linalg.eigh.

Bounds, with ||a|| the Frobenius norm and n the dimension: eigenvalues agree to n * 2^-52 * ||a||; |q^T a q - diag(w)| and
|q^T q - 1| (largest element) stay below n * 2^-50 * ||a|| and n * 2^-50: the backward-error bound of Jacobi rotations
(every rotation perturbs the matrix by a few ulps of its norm, a sweep touches every element n times) with a factor 4 for the sweeps."""
import importlib

import numpy as np
import pytest

qa = importlib.import_module("quda-qkxtm-multigrid_amd")

NEW_SYMBOLS = ["qudaAmdNewDeflation", "qudaAmdDestroyDeflation", "qudaAmdDeflationInfo", "qudaAmdDeflationTimings", "qudaAmdDeflationGetVector", "qudaAmdDeflationProject",
               "qudaAmdDeflationExactLoop", "qudaAmdHostSymmetricEig", "qudaAmdRotateBasis", "qudaAmdBlockDot", "qudaAmdBlockAxpy", "qudaAmdLastEigenvalues"]


def test_new_symbols_are_exported():
    L = qa.lib()
    missing = [s for s in NEW_SYMBOLS if not hasattr(L, s)]
    assert not missing, missing
    assert set(NEW_SYMBOLS) <= set(qa.EXT_H_SYMBOLS)


def _random_symmetric(n, seed):
    a = np.random.default_rng(seed).standard_normal((n, n))
    return 0.5 * (a + a.T)


def _arrowhead_tridiagonal(n, keep, seed):
    """the projected matrix after a thick restart: `keep` Ritz values on the diagonal, their couplings to vector `keep` in one row and
    column, tridiagonal from there on"""
    rng = np.random.default_rng(seed)
    a = np.zeros((n, n))
    a[np.arange(keep), np.arange(keep)] = np.sort(rng.uniform(0.5, 1.0, keep))[::-1]
    a[keep, :keep] = a[:keep, keep] = rng.standard_normal(keep) * 1e-3
    for j in range(keep, n):
        a[j, j] = rng.uniform(-0.05, 0.3)
        if j + 1 < n:
            a[j, j + 1] = a[j + 1, j] = rng.uniform(0.05, 0.2)
    return a


def _repeated(n, seed):
    """eigenvalues 1 (four times), 2 (three times) and distinct ones, in a random orthogonal frame"""
    rng = np.random.default_rng(seed)
    w = np.concatenate([np.full(4, 1.0), np.full(3, 2.0), rng.uniform(-3.0, 3.0, n - 7)])
    q, _ = np.linalg.qr(rng.standard_normal((n, n)))
    a = (q * w) @ q.T
    return 0.5 * (a + a.T)


CASES = {"random 37": _random_symmetric(37, 1), "arrowhead + tridiagonal 32": _arrowhead_tridiagonal(32, 22, 2), "repeated eigenvalue 24": _repeated(24, 3),
         "one by one": np.array([[-2.5]])}


@pytest.mark.parametrize("name", sorted(CASES))
def test_host_symmetric_eig_matches_numpy(name):
    a = CASES[name]
    n = a.shape[0]
    w, q = qa.host_symmetric_eig(a)
    norm = np.linalg.norm(a)
    want = np.linalg.eigh(a)[0]
    e_w = np.max(np.abs(w - want))
    e_d = np.max(np.abs(q.T @ a @ q - np.diag(w)))
    e_o = np.max(np.abs(q.T @ q - np.eye(n)))
    print("%s: |w - eigh| %.3e (bound %.3e), |q^T a q - w| %.3e (bound %.3e), |q^T q - 1| %.3e (bound %.3e)"
          % (name, e_w, n * 2.0 ** -52 * norm, e_d, n * 2.0 ** -50 * norm, e_o, n * 2.0 ** -50))
    assert np.all(np.diff(w) >= 0)
    assert e_w <= n * 2.0 ** -52 * norm
    assert e_d <= n * 2.0 ** -50 * norm
    assert e_o <= n * 2.0 ** -50


def test_host_symmetric_eig_reads_the_upper_triangle():
    a = _random_symmetric(9, 5)
    b = np.triu(a) + np.tril(np.full((9, 9), 7.0), -1)
    assert np.array_equal(qa.host_symmetric_eig(a)[0], qa.host_symmetric_eig(b)[0])
