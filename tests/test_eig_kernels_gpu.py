"""The panel kernels of the Lanczos eigensolver (csrc/eig.hip) through their test hooks, against numpy.

Lattice 6 x 4 x 2 x 8: 9216 real rows, 4608 complex numbers in two segments of 2304 (one full tile of the dot kernel and a tail of 256).
A second lattice of six sites (144 rows, two segments of 72) has a last panel of 16 rows and a panel that straddles the two segments.

qudaAmdRotateBasis (v_mfma_f64_16x16x4_f64): every element within 4 m 2^-53 sum_j |V_rj| |Q_jc| of numpy's V @ Q, the bound of an fp64
FMA chain of length m (twice: the reference product has the same bound); the vectors k .. m-1 unchanged bit for bit.
qudaAmdBlockDot / qudaAmdBlockAxpy: 1e-12 |v_j| |w| and 1e-12 max |w|, the bounds of the contraction tests."""
import importlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

X = (6, 4, 2, 8)
XSMALL = (2, 3, 1, 1)


@pytest.fixture(scope="module")
def qa():
    mod = importlib.import_module("quda-qkxtm-multigrid_amd")
    mod.init(0)
    yield mod
    mod.end()


def _cplx(a):
    return a[..., 0::2] + 1j * a[..., 1::2]


@pytest.mark.parametrize("lattice,m,k", [(X, 23, 9), (X, 32, 16), (X, 64, 33), (XSMALL, 23, 9), (XSMALL, 7, 7)])
def test_rotate_basis_matches_numpy(qa, lattice, m, k):
    n = int(np.prod(lattice)) * 24
    rng = np.random.default_rng(100 * m + k)
    V = rng.standard_normal((m, n))
    Q = rng.standard_normal((m, k))
    got = qa.rotate_basis(V, Q, lattice)
    want = Q.T @ V                      # new vector c = sum_j Q[j, c] v_j
    bound = 4.0 * m * 2.0 ** -53 * (np.abs(Q).T @ np.abs(V))
    ratio = np.max(np.abs(got[:k] - want) / bound)
    print("m = %d, k = %d, %d rows: largest error / bound = %.3f" % (m, k, n, ratio))
    assert ratio <= 1.0
    assert np.array_equal(got[k:], V[k:])


def test_rotate_basis_exact_integers(qa):
    """small integers are exact in fp64: any wrong lane-to-element map of the matrix-core operands shows as a wrong integer"""
    m, k = 37, 21
    n = int(np.prod(X)) * 24
    rng = np.random.default_rng(9)
    V = rng.integers(-8, 9, (m, n)).astype(np.float64)
    Q = rng.integers(-8, 9, (m, k)).astype(np.float64)
    got = qa.rotate_basis(V, Q, X)
    assert np.array_equal(got[:k], Q.T @ V)
    assert np.array_equal(got[k:], V[k:])


@pytest.mark.parametrize("lattice,m", [(X, 1), (X, 21), (X, 64), (XSMALL, 5)])
def test_block_dot_and_axpy_match_numpy(qa, lattice, m):
    n = int(np.prod(lattice)) * 24
    rng = np.random.default_rng(7 + m)
    V = rng.standard_normal((m, n))
    w = rng.standard_normal(n)
    Vc, wc = _cplx(V), _cplx(w)
    c = qa.block_dot(V, w, lattice)
    want = Vc.conj() @ wc
    scale = np.linalg.norm(Vc, axis=1) * np.linalg.norm(wc)
    print("m = %d: dot error / (|v||w|) = %.3e" % (m, np.max(np.abs(c - want) / scale)))
    assert np.all(np.abs(c - want) <= 1e-12 * scale)
    assert np.array_equal(c, qa.block_dot(V, w, lattice))   # fixed order of the partial sums
    coef = rng.standard_normal(m) + 1j * rng.standard_normal(m)
    got = _cplx(qa.block_axpy(w, coef, V, lattice))
    want = wc - coef @ Vc
    print("m = %d: axpy error / max|w| = %.3e" % (m, np.max(np.abs(got - want)) / np.max(np.abs(want))))
    assert np.max(np.abs(got - want)) <= 1e-12 * np.max(np.abs(want))


def test_gram_schmidt_pass_orthogonalises(qa):
    """the two kernels as the eigensolver uses them: w - V (V^+ w) is orthogonal to an orthonormal V to rounding"""
    m = 48
    n = int(np.prod(X)) * 24
    rng = np.random.default_rng(3)
    q, _ = np.linalg.qr(rng.standard_normal((n // 2, m)) + 1j * rng.standard_normal((n // 2, m)))
    V = np.ascontiguousarray(np.stack([q.T.real, q.T.imag], axis=-1).reshape(m, n))
    w = rng.standard_normal(n)
    for _ in range(2):
        w = qa.block_axpy(w, qa.block_dot(V, w, X), V, X)
    left = np.max(np.abs(qa.block_dot(V, w, X))) / np.linalg.norm(w)
    print("|V^+ w| / |w| after two passes: %.3e" % left)
    assert left <= 1e-14
