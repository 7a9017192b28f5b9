"""The numpy reference of the twisted-clover force (tests/clover_force_ref.py) against things that do not depend on it: the oracle's clover
term, central differences of L_T, of -|Mh(U) x|^2 with Mh from the oracle's tmc_matpc on a clover term rebuilt from the links, and of
log det(A^2 + a^2), and the order of the leapfrog integrator.  No GPU.  The leapfrog inputs (clover_force_ref.LEAPFROG) are the ones
tests/test_clover_force_gpu.py runs through the C ABI.

The finite-difference checks are those of tests/test_ferm_force_ref.py: central differences at eps = 1e-2 and 5e-3, the discrepancy must
fall to a quarter (0.3 allowed) and at eps = 1e-2 be within three times what this reference itself gives on these inputs (the
*_MEASURED constants, printed by the tests)."""
import numpy as np
import pytest

import clover_force_ref as cf
import ferm_force_ref as ff
import gauge_md_ref as md
import gauge_obs_ref as ob
from synth import smooth_gauge

LATTICES = [(4, 4, 4, 4), (6, 4, 2, 8)]
KAPPA, MU, CSW = 0.13, 0.2, 0.13 * 1.57551

OPS = {}
for _m in ("ee", "oo", "eeasym", "ooasym"):
    for _f in (+1, -1):
        OPS["tmc_%s_%s" % (_m, "plus" if _f > 0 else "minus")] = cf.Op(KAPPA, MU, _f, CSW, matpc=_m)
OPS["tmc_ee_mu0"] = cf.Op(KAPPA, 0.0, +1, CSW, matpc="ee")
OPS["tmc_ooasym_mu0"] = cf.Op(KAPPA, 0.0, +1, CSW, matpc="ooasym")
OPS["tmc_ee_plus_mass"] = cf.Op(KAPPA, MU, +1, CSW, matpc="ee", norm="mass")
OPS["tmc_ooasym_minus_asym_mass"] = cf.Op(KAPPA, MU, -1, CSW, matpc="ooasym", norm="asym_mass")

# largest |central difference - analytic| / |analytic| at eps = 1e-2 that this reference gives on these inputs (printed by the tests):
# L_T over both lattices (3.97e-4 and 7.27e-4); -|Mh x|^2 over all OPS, both lattices, hot and smooth links (3.1e-5 ... 4.19e-3, the
# largest where the derivative itself is small: tmc_eeasym_minus on 4^4 hot links, dS = -1.41 next to tens elsewhere); log det over both
# lattices, parities and twists (6.4e-5 ... 2.43e-3)
FD_DERIV_MEASURED = 7.28e-4
FD_FORCE_MEASURED = 4.19e-3
FD_LOGDET_MEASURED = 2.43e-3


@pytest.fixture(scope="module")
def fields(oracle):
    """per lattice: hot and smooth links with the anti-periodic sign, lexicographic, and a parity spinor.  Never modified"""
    out = {}
    for X in LATTICES:
        hot, spinor, _ = oracle.make_fields(list(X), seed=41, antiperiodic_t=True, clover=False)
        rng = np.random.default_rng(5)
        out[X] = {"hot": ob.from_qdp(oracle, hot, X),
                  "smooth": ob.flip_time_boundary(ob.from_qdp(oracle, smooth_gauge(X, 0.35), X)),
                  "x1": rng.standard_normal(spinor.size // 2)}
    return out


def _fd(action, U, analytic_of, seed=2):
    """(analytic, [discrepancy at 1e-2, at 5e-3]) of sum Re tr(Theta F) against the central difference of action along a random Theta"""
    Theta = md.random_momentum(np.random.default_rng(seed), U.shape[:-2])
    analytic = analytic_of(Theta)
    disc = []
    for eps in (1e-2, 5e-3):
        disc.append(abs((action(md.update(U, Theta, eps)) - action(md.update(U, Theta, -eps))) / (2 * eps) - analytic))
    return analytic, disc


def _pair(Theta, F):
    return np.sum(np.einsum("...ij,...ji->...", Theta, F).real)


@pytest.mark.parametrize("X", LATTICES)
def test_clover_matrix_is_the_oracles(oracle, fields, X):
    """1 + i c sum_f sigma_f (x) F_f with sigma from ferm_force_ref.GAMMA against oracle.clover_compute unpacked: pins sigma, the plane
    order and the spin basis"""
    U = fields[X]["hot"]
    want = cf.unpack_clover(oracle, oracle.clover_compute(ob.to_qdp(oracle, U, X), CSW, list(X)), X)
    got = cf.clover_matrix(U, CSW)
    assert np.max(np.abs(got - want)) <= 1e-14
    assert np.max(np.abs(got - np.eye(12))) > 1e-2
    # sigma commutes with gamma5 and the layouts round-trip
    g5 = ff.GAMMA[0] @ ff.GAMMA[1] @ ff.GAMMA[2] @ ff.GAMMA[3]
    for s in cf.SIGMA:
        assert np.array_equal(s @ g5, g5 @ s) and np.array_equal(s, np.conj(s.T))
    rng = np.random.default_rng(1)
    h = rng.standard_normal((int(np.prod(X)), 6, 3, 3, 2))
    assert np.array_equal(cf.tensor_to_host(oracle, cf.tensor_from_host(oracle, h, X), X), h)


@pytest.mark.parametrize("X", LATTICES)
def test_derivative_is_the_force_of_l_t(oracle, fields, X):
    """G[T] against the central difference of L_T = sum Re tr(T_f F_f) for a random general complex T, hot links with the anti-periodic
    sign.  Measured discrepancy at eps = 1e-2: see FD_DERIV_MEASURED"""
    U = fields[X]["hot"]
    rng = np.random.default_rng(9)
    T = rng.standard_normal((6,) + U.shape[1:]) + 1j * rng.standard_normal((6,) + U.shape[1:])
    G = cf.deriv_force(U, np.zeros_like(U), T, 1.0)
    analytic, disc = _fd(lambda V: cf.l_t(V, T), U, lambda Th: _pair(Th, G))
    print("%s: dL = %.6e, discrepancy %.3e (%.3e of dL) at 1e-2, %.3e at 5e-3, ratio %.3f" % (X, analytic, disc[0], disc[0] / abs(analytic), disc[1], disc[1] / disc[0]))
    assert disc[1] <= 0.3 * disc[0]
    assert disc[0] <= 3.0 * FD_DERIV_MEASURED * abs(analytic)
    # only the anti-Hermitian part of T counts, G is linear in T, traceless and anti-Hermitian, and accumulates
    Ta = [0.5 * (t - ob._dag(t)) for t in T]
    scale = np.max(np.abs(G))
    assert np.max(np.abs(cf.deriv_force(U, np.zeros_like(U), Ta, 1.0) - G)) <= 1e-13 * scale
    A0 = md.random_momentum(rng, U.shape[:-2])
    assert np.max(np.abs(cf.deriv_force(U, A0, T, -0.7) - (A0 - 0.7 * G))) <= 1e-13 * scale
    assert np.max(np.abs(G + ob._dag(G))) <= 1e-13 * scale and np.max(np.abs(np.trace(G, axis1=-2, axis2=-1))) <= 1e-13 * scale


@pytest.mark.parametrize("name", sorted(OPS))
@pytest.mark.parametrize("X", LATTICES)
def test_force_is_the_derivative_of_the_action(oracle, fields, X, name):
    """sum Re tr(Theta F) against the central difference of -|Mh(exp(eps Theta) U) x|^2, Mh the oracle's tmc_matpc with the clover term
    and its twisted inverse recomputed from the moved links.  Measured discrepancy at eps = 1e-2: see FD_FORCE_MEASURED"""
    op = OPS[name]
    c = fields[X]
    x = c["x1"]
    for links in ("hot", "smooth"):
        U = c[links]
        F = cf.tmc_force(oracle, U, np.zeros_like(U), [x], [1.0], 1.0, op, X)
        analytic, disc = _fd(lambda V: cf.minus_norm2_mx(oracle, V, x, op, X), U, lambda Th: _pair(Th, F))
        print("%s %s %s: dS = %.6e, discrepancy %.3e (%.3e of dS) at 1e-2, %.3e at 5e-3, ratio %.3f"
              % (name, X, links, analytic, disc[0], disc[0] / abs(analytic), disc[1], disc[1] / disc[0]))
        assert disc[1] <= 0.3 * disc[0]
        assert disc[0] <= 3.0 * FD_FORCE_MEASURED * abs(analytic)


@pytest.mark.parametrize("a", [2 * KAPPA * MU, -2 * KAPPA * MU, 0.0])
@pytest.mark.parametrize("X", LATTICES)
def test_logdet_force_is_the_derivative_of_logdet(oracle, fields, X, a):
    """per parity: the force of L_p = sum_(x of parity p) log det(A^2 + a^2) against its central difference; L_p itself against the
    trlogA convention (log det of the 12 x 12 matrix).  Measured discrepancy at eps = 1e-2: see FD_LOGDET_MEASURED"""
    U = fields[X]["hot"]
    for p in (0, 1):
        coeff = [1.0 - p, float(p)]
        F = cf.logdet_force(U, np.zeros_like(U), CSW, a, 1.0, coeff)
        analytic, disc = _fd(lambda V: cf.logdet(V, CSW, a)[p], U, lambda Th: _pair(Th, F))
        print("%s a %.3f parity %d: dL = %.6e, discrepancy %.3e (%.3e of dL) at 1e-2, %.3e at 5e-3, ratio %.3f"
              % (X, a, p, analytic, disc[0], disc[0] / abs(analytic), disc[1], disc[1] / disc[0]))
        assert disc[1] <= 0.3 * disc[0]
        assert disc[0] <= 3.0 * FD_LOGDET_MEASURED * abs(analytic)


def test_leapfrog_energy_violation_is_second_order(oracle):
    """H = momentum action + Wilson gauge action + phi^dag (Mh^dag Mh)^-1 phi - sum_x log det(A(x)^2 + a^2) on the inputs of
    clover_force_ref.LEAPFROG (those of ferm_force_ref.LEAPFROG with clover_coeff = 0.12 x 1.57551): measured
    dH = -7.369122 at dt = 0.05 and -1.869385 at 0.025, ratio 3.94;
    the ratio must lie in [3.7, 4.3]"""
    p = cf.LEAPFROG
    X = p["X"]
    U, A, phi, op = cf.leapfrog_inputs(oracle)
    H0 = cf.hamiltonian(oracle, U, A, phi, op, X, p["beta"], p["tol"], p["cdet"])
    dH = []
    for dt in p["dt"]:
        U1, A1 = cf.leapfrog(oracle, U, A, phi, op, X, p["beta"], dt, int(round(p["tau"] / dt)), p["tol"], p["cdet"])
        dH.append(cf.hamiltonian(oracle, U1, A1, phi, op, X, p["beta"], p["tol"], p["cdet"]) - H0)
    print("dH = %.6e, %.6e, ratio %.4f" % (dH[0], dH[1], dH[0] / dH[1]))
    assert 3.7 <= dH[0] / dH[1] <= 4.3
