"""The thick-restart Lanczos eigensolver on the device and the deflation object built on it (qudaAmdNewDeflation), twisted mass on
4^4 at kappa 0.124, mu 0.005, against the dense spectrum of the ORACLE's operator (tm_mat applied to the 3072 unit vectors, M^+ M,
numpy.linalg.eigh), which shares no code with the device operator.

Warm start, smooth_gauge(X, 0.35): nEv 12, nKv 32, Chebyshev degree 20 on [0.2, 4.0], tol 1e-10.  Findings on the CPU: the twelve lowest
values of the dense spectrum are 0.0204 .. 0.0230, then a gap to 0.1107; the largest value is 3.586 < (1 + 8 kappa)^2 = 3.97 < amax; a
numpy prototype of the same process converged within the first cycle with 640 applications of A and residuals up to 9.5e-13.
Hot start, make_gauge(X): nEv 8, nKv 32, degree 20 on [0.4, 3.2]: the dense spectrum starts at 0.159, the prototype took 4 cycles
(3 restarts, residuals 2e-14); the cap is 12.  This is the case that runs eig_rotate inside the solver.

Checks: residuals recomputed on the host with the oracle <= 1e-10 (the requested tolerance); |lambda_i - w_i| <= r_i + 1e-13 (residual
theorem for Hermitian matrices); ascending, lambda >= (2 kappa mu)^2; |U^+ U - 1| <= 1e-12; the restart caps; the projector against
numpy with the device's vectors (1e-12 |x|) and against the dense eigenvectors (1e-8 |x|: Davis-Kahan, sqrt(12) 1e-10 / 0.087 = 4e-9);
the exact part of the loops against sum_i contract_loop(v_i) / lambda_i (1e-12 of each block's maximum) and, for the Scalar block at zero
momentum summed over t, the entries that make the building block v^+ v against -sum_i 1 / w_i of the dense eigenvalues (1e-9 relative)."""
import importlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from synth import make_gauge, smooth_gauge  # noqa: E402

X = (4, 4, 4, 4)
V = int(np.prod(X))
KAPPA, MU, QSQ = 0.124, 0.005, 2


@pytest.fixture(scope="module")
def qa():
    mod = importlib.import_module("quda-qkxtm-multigrid_amd")
    mod.init(0)
    yield mod
    mod.end()


def _cplx(v):
    return v[0::2] + 1j * v[1::2]


def _dense(oracle, gauge):
    """(ascending eigenvalues, eigenvectors) of M^+ M, M the oracle's full operator on even-odd DeGrand-Rossi vectors"""
    n = V * 12
    M = np.zeros((n, n), dtype=complex)
    for k in range(n):
        e = np.zeros(V * 24)
        e[2 * k] = 1.0
        M[:, k] = _cplx(oracle.tm_mat(gauge, e, list(X), KAPPA, MU, +1, 0))
    return np.linalg.eigh(M.conj().T @ M)


def _A(oracle, gauge, v):
    return oracle.tm_mat(gauge, oracle.tm_mat(gauge, v, list(X), KAPPA, MU, +1, 0), list(X), KAPPA, MU, +1, 1)


def _ip(qa):
    # full-field host vectors in the device's own basis and order: what the oracle's tm_mat takes
    return qa.invert_param(qa.QUDA_TWISTED_MASS_DSLASH, KAPPA, MU, +1, "ee", 0, cuda_prec=8, solution_type=qa.QUDA_MAT_SOLUTION)


class Case:
    def __init__(self, qa, oracle, gauge, tb, nEv, amin, amax):
        self.qa, self.gauge, self.tb, self.nEv = qa, gauge, tb, nEv
        self.load()
        self.ip = _ip(qa)
        self.defl = qa.Deflation(self.ip, nEv, 32, 20, amin, amax, 1e-10, isACC=True, maxRestarts=100)
        self.U = np.stack([self.defl.vector(i, V) for i in range(nEv)])
        self.w, self.W = _dense(oracle, gauge)
        self.res = np.array([np.linalg.norm(_A(oracle, gauge, self.U[i]) - self.defl.evals[i] * self.U[i]) for i in range(nEv)])

    def load(self):
        self.qa.load_gauge(self.gauge, self.qa.gauge_param(X, t_boundary=self.tb))


@pytest.fixture(scope="module")
def warm(qa, oracle):
    c = Case(qa, oracle, smooth_gauge(X, 0.35), qa.QUDA_PERIODIC_T, 12, 0.2, 4.0)
    yield c
    c.defl.close()


@pytest.fixture(scope="module")
def hot(qa, oracle):
    c = Case(qa, oracle, make_gauge(X), qa.QUDA_ANTI_PERIODIC_T, 8, 0.4, 3.2)
    yield c
    c.defl.close()


def _check_pairs(c, cap):
    d = c.defl
    print("restarts %d, applications of A %d" % (d.restarts, d.matvecs))
    print("lambda:", d.evals)
    print("host residuals |A v - lambda v| with the oracle: max %.3e; the solver's own: max %.3e" % (c.res.max(), d.residuals.max()))
    print("|lambda - w|: max %.3e" % np.max(np.abs(d.evals - c.w[:c.nEv])))
    assert np.all(c.res <= 1e-10)
    assert np.all(np.abs(d.evals - c.w[:c.nEv]) <= c.res + 1e-13)
    assert np.all(np.diff(d.evals) >= 0) and np.all(d.evals >= (2 * KAPPA * MU) ** 2)
    Uc = c.U[:, 0::2] + 1j * c.U[:, 1::2]
    orth = np.max(np.abs(Uc.conj() @ Uc.T - np.eye(c.nEv)))
    print("|U^+ U - 1| = %.3e" % orth)
    assert orth <= 1e-12
    assert d.restarts <= cap


def test_warm_start_pairs(warm):
    _check_pairs(warm, 3)
    if warm.defl.restarts == 0:
        assert warm.defl.matvecs == 32 * 20 + 12   # one cycle of 32 filtered steps, then A on every returned vector


def test_hot_start_pairs_with_restarts(hot):
    _check_pairs(hot, 12)
    assert hot.defl.restarts >= 1   # otherwise this case would not cover the basis compression


@pytest.mark.parametrize("n", [12, 4])
def test_projection_matches_numpy(warm, n):
    x = np.random.default_rng(5).standard_normal(V * 24)
    xc = _cplx(x)
    got = _cplx(warm.defl.project(x, n))
    Uc = (warm.U[:, 0::2] + 1j * warm.U[:, 1::2])[:n]
    own = xc - Uc.T @ (Uc.conj() @ xc)
    e_own = np.linalg.norm(got - own) / np.linalg.norm(xc)
    Wn = warm.W[:, :n]
    dense = xc - Wn @ (Wn.conj().T @ xc)
    e_dense = np.linalg.norm(got - dense) / np.linalg.norm(xc)
    print("n = %d: against the device's vectors %.3e, against the dense eigenvectors %.3e" % (n, e_own, e_dense))
    assert e_own <= 1e-12
    if n == 12:
        assert e_dense <= 1e-8   # the twelve lowest values are 0.087 away from the rest; the first four are not separated from the fifth
    else:
        U12 = warm.U[:, 0::2] + 1j * warm.U[:, 1::2]
        assert np.linalg.norm(got - (xc - U12.T @ (U12.conj() @ xc))) > 1e-3 * np.linalg.norm(own)   # the first four only, not all twelve


@pytest.mark.parametrize("n", [4, 12])
def test_exact_loop(warm, oracle, n):
    qa = warm.qa
    warm.load()
    got = warm.defl.exact_loop(n, QSQ, X[:3])
    ipl = qa.invert_param(qa.QUDA_TWISTED_MASS_DSLASH, KAPPA, MU, +1, "ee", 0, cuda_prec=8, solution_type=qa.QUDA_MAT_SOLUTION,
                          gamma_basis=qa.QUDA_UKQCD_GAMMA_BASIS)
    want = 0
    for i in range(n):
        lex = oracle.dr_to_ukqcd(oracle.eo_to_lex(warm.U[i], list(X), 24).reshape(-1, 24)).reshape(-1)
        want = want + qa.contract_loop(lex, ipl, QSQ, X[:3]) / warm.defl.evals[i]
    errs = [np.max(np.abs(got[k] - want[k])) / np.max(np.abs(want[k])) for k in range(18)]
    print("n = %d: largest deviation of a block, relative to its maximum: %.3e" % (n, max(errs)))
    assert max(errs) <= 1e-12
    # Scalar block = -C[v, v], C[4a + b] = sum_c conj(v[(a + 2) mod 4, c]) v[b, c]: the entries b = (a + 2) mod 4 add up to -v^+ v = -1 per vector
    moms = qa.loop_momenta(X[:3], QSQ)
    zero = [i for i, m in enumerate(moms) if not np.any(m)][0]
    anchor = sum(got[0, :, zero, 4 * a + (a + 2) % 4].sum() for a in range(4))
    ref = -np.sum(1.0 / warm.w[:n])
    print("n = %d: Scalar anchor %.12e %+.3e i, -sum 1 / w = %.12e" % (n, anchor.real, anchor.imag, ref))
    assert abs(anchor - ref) <= 1e-9 * abs(ref)
