"""The numpy reference of the fermion force (tests/ferm_force_ref.py) against things that do not depend on it: the oracle's hop, the
finite-difference derivative of -|Mh(U) x|^2 with Mh from the oracle's own even-odd operators, gauge covariance, the boundary sign,
linearity, and the order of the leapfrog integrator with a pseudofermion.  No GPU.  The leapfrog inputs (ferm_force_ref.LEAPFROG) are the
ones tests/test_ferm_force_gpu.py runs through the C ABI."""
import numpy as np
import pytest

import ferm_force_ref as ff
import gauge_md_ref as md
import gauge_obs_ref as ob
from synth import smooth_gauge

LATTICES = [(4, 4, 4, 4), (6, 4, 2, 8)]
KAPPA, MU, EPSILON = 0.13, 0.2, 0.15

# the operators of the finite-difference test: the four matpc types with both twist signs, Wilson, the doublet, and the two mass
# normalisations next to the kappa normalisation of all the others
OPS = {}
for _m in ("ee", "oo", "eeasym", "ooasym"):
    for _f in (+1, -1):
        OPS["tm_%s_%s" % (_m, "plus" if _f > 0 else "minus")] = ff.Op("tm", KAPPA, MU, _f, matpc=_m)
    OPS["ndeg_%s" % _m] = ff.Op("ndeg", KAPPA, MU, epsilon=EPSILON, matpc=_m)
for _m in ("ee", "oo"):
    OPS["wilson_%s" % _m] = ff.Op("wilson", KAPPA, matpc=_m)
OPS["tm_ee_plus_mass"] = ff.Op("tm", KAPPA, MU, +1, matpc="ee", norm="mass")
OPS["tm_ooasym_minus_asym_mass"] = ff.Op("tm", KAPPA, MU, -1, matpc="ooasym", norm="asym_mass")
OPS["ndeg_eeasym_mass"] = ff.Op("ndeg", KAPPA, MU, epsilon=EPSILON, matpc="eeasym", norm="mass")

# largest |central difference - analytic| / |analytic| at eps = 1e-2 that this reference gives on these inputs, over all OPS, both
# lattices, hot and smooth links (printed by the test); the test allows three times this
FD_MEASURED = 1.13e-3


@pytest.fixture(scope="module")
def fields(oracle):
    """per lattice: hot and smooth links with the anti-periodic sign, lexicographic; and a parity spinor / doublet.  Never modified"""
    out = {}
    for X in LATTICES:
        hot, spinor, _ = oracle.make_fields(list(X), seed=41, antiperiodic_t=True, clover=False)
        rng = np.random.default_rng(5)
        out[X] = {"hot": ob.from_qdp(oracle, hot, X),
                  "smooth": ob.flip_time_boundary(ob.from_qdp(oracle, smooth_gauge(X, 0.35), X)),
                  "x1": rng.standard_normal(spinor.size // 2), "x2": rng.standard_normal(spinor.size)}
    return out


def _x(c, op):
    return c["x2"] if op.nflavor == 2 else c["x1"]


@pytest.mark.parametrize("X", LATTICES)
def test_gamma_matrices_and_projectors_are_the_oracles(oracle, fields, X):
    """the hop written with GAMMA, np.roll and einsum against oracle.wil_dslash on both parities, with and without dagger"""
    c = fields[X]
    gauge = ob.to_qdp(oracle, c["hot"], X)
    full = np.random.default_rng(3).standard_normal(int(np.prod(X)) * 24)
    h = full.size // 2
    psi = ff.lex_spinor(oracle, full, X)
    assert np.array_equal(ff.host_spinor(oracle, psi, X), full)
    for dagger in (0, 1):
        got = ff.host_spinor(oracle, ff.dslash(c["hot"], psi, bool(dagger)), X)
        want = np.concatenate([oracle.wil_dslash(gauge, np.ascontiguousarray(full[h:]), list(X), 0, dagger),
                               oracle.wil_dslash(gauge, np.ascontiguousarray(full[:h]), list(X), 1, dagger)])
        assert np.max(np.abs(got - want)) <= 1e-13 * np.max(np.abs(want))
    for mu in range(4):
        g = ff.GAMMA[mu]
        assert np.array_equal(g @ g, ff.EYE4) and np.array_equal(g, np.conj(g.T))


@pytest.mark.parametrize("name", sorted(OPS))
@pytest.mark.parametrize("X", LATTICES)
def test_force_is_the_derivative_of_the_action(oracle, fields, X, name):
    """sum Re tr(T F) against the central difference of -|Mh(exp(eps T) U) x|^2, Mh from the oracle's tm_matpc / wil_matpc and the doublet's
    ndeg_matpc.  Central differences are exact to O(eps^2): halving eps must cut the discrepancy to a quarter (0.3 allowed).  The
    discrepancy at eps = 1e-2 measured with this reference on these inputs is at most 1.13e-3 of the derivative (FD_MEASURED; between
    6.8e-6 and 1.126e-3 over the cases); three times that is allowed."""
    op = OPS[name]
    c = fields[X]
    x = _x(c, op)
    zero = np.zeros(c["hot"].shape, dtype=np.complex128)
    for links in ("hot", "smooth"):
        U = c[links]
        F = ff.tm_force(oracle, U, zero, [x], [1.0], 1.0, op, X)
        T = md.random_momentum(np.random.default_rng(2), U.shape[:-2])
        analytic = np.sum(np.einsum("...ij,...ji->...", T, F).real)
        disc = []
        for eps in (1e-2, 5e-3):
            Sp = ff.minus_norm2_mx(oracle, md.update(U, T, eps), x, op, X)
            Sm = ff.minus_norm2_mx(oracle, md.update(U, T, -eps), x, op, X)
            disc.append(abs((Sp - Sm) / (2 * eps) - analytic))
        print("%s %s %s: dS = %.6e, discrepancy %.3e (%.3e of dS) at eps = 1e-2, %.3e at 5e-3, ratio %.3f"
              % (name, X, links, analytic, disc[0], disc[0] / abs(analytic), disc[1], disc[1] / disc[0]))
        assert disc[1] <= 0.3 * disc[0]
        assert disc[0] <= 3.0 * FD_MEASURED * abs(analytic)


@pytest.mark.parametrize("name", ["tm_ee_plus", "tm_ooasym_minus", "wilson_oo", "ndeg_ee", "ndeg_eeasym"])
@pytest.mark.parametrize("X", LATTICES)
def test_force_is_gauge_covariant(oracle, fields, X, name):
    """U_mu(x) -> g(x) U_mu(x) g(x + mu)^dag, x -> g x: F_mu(x) -> g(x) F_mu(x) g(x)^dag"""
    op = OPS[name]
    c = fields[X]
    U, x = c["hot"], _x(c, op)
    zero = np.zeros(U.shape, dtype=np.complex128)
    g = ob.random_su3(np.random.default_rng(5), U.shape[1:-2])
    h = x.size // op.nflavor
    gx = np.concatenate([ff.host_spinor(oracle, np.einsum("...ab,...sb->...sa", g, ff.lex_spinor(oracle, ff.embed(x[f * h:(f + 1) * h], op.p0), X)), X)
                         [op.p0 * h:(op.p0 + 1) * h] for f in range(op.nflavor)])
    F = ff.tm_force(oracle, U, zero, [x], [1.0], 1.0, op, X)
    Fg = ff.tm_force(oracle, ob.gauge_transform(U, g), zero, [gx], [1.0], 1.0, op, X)
    err = np.max(np.abs(Fg - g @ F @ ob._dag(g)))
    print("%s %s: covariance %.3e of max|F| = %.3e" % (name, X, err, np.max(np.abs(F))))
    assert err <= 1e-12 * np.max(np.abs(F))


@pytest.mark.parametrize("X", LATTICES)
def test_boundary_sign_and_linearity_of_the_outer_product(oracle, fields, X):
    c = fields[X]
    U = c["hot"]                                 # carries the anti-periodic sign
    rng = np.random.default_rng(8)
    shape = U.shape[1:-2] + (4, 3)
    fld = lambda: rng.standard_normal(shape) + 1j * rng.standard_normal(shape)
    pairs = [(fld(), fld()), ([fld(), fld()], [fld(), fld()]), (fld(), fld())]   # the second pair has two flavours
    coeff = [0.3, -1.1, 0.7]
    A0 = md.random_momentum(rng, U.shape[:-2])
    F = ff.oprod_force(U, A0, pairs, coeff)
    scale = np.max(np.abs(F))
    # the sign on the links of the last time slice is the sign anti-periodic fields pick up across the boundary on links without it
    Fb = ff.oprod_force(ob.flip_time_boundary(U), A0, pairs, coeff, antiperiodic=True)
    assert np.max(np.abs(Fb - F)) <= 1e-14 * scale
    assert np.max(np.abs(ff.oprod_force(ob.flip_time_boundary(U), A0, pairs, coeff) - F)) > 1e-3 * scale
    # linear in the coefficients, and in the momentum it accumulates onto
    zero = np.zeros_like(A0)
    parts = sum(cf * ff.oprod_force(U, zero, [p], [1.0]) for p, cf in zip(pairs, coeff))
    assert np.max(np.abs(md.ta(A0) + parts - F)) <= 1e-13 * scale
    assert np.max(np.abs(ff.oprod_force(U, A0, pairs, [2.0 * cf for cf in coeff]) - (2.0 * (F - A0) + A0))) <= 1e-13 * scale
    # traceless and anti-Hermitian
    assert np.max(np.abs(F + ob._dag(F))) <= 1e-14 * scale and np.max(np.abs(np.trace(F, axis1=-2, axis2=-1))) <= 1e-14 * scale


def test_force_is_linear_in_the_coefficients_and_sums_over_solutions(oracle, fields):
    X = LATTICES[1]
    c = fields[X]
    op = OPS["tm_eeasym_plus"]
    U = c["hot"]
    zero = np.zeros(U.shape, dtype=np.complex128)
    xs = [c["x1"], c["x1"][::-1].copy(), np.roll(c["x1"], 7)]
    coeff = [0.5, -0.25, 1.5]
    A0 = md.random_momentum(np.random.default_rng(4), U.shape[:-2])
    F = ff.tm_force(oracle, U, A0, xs, coeff, 0.1, op, X)
    parts = sum(cf * ff.tm_force(oracle, U, zero, [x], [1.0], 1.0, op, X) for x, cf in zip(xs, coeff))
    assert np.max(np.abs(A0 + 0.1 * parts - F)) <= 1e-13 * np.max(np.abs(F))


def test_leapfrog_energy_violation_is_second_order(oracle):
    """H = momentum action + Wilson gauge action + phi^dag (Mh^dag Mh)^-1 phi on the inputs of ferm_force_ref.LEAPFROG (4^4, smooth_gauge(0.35) with
    the anti-periodic sign, beta = 5.5, twisted mass kappa = 0.12, mu = 0.2, even-even symmetric, tau = 0.5, CG to 1e-12): measured
    dH = -6.430630 at dt = 0.05 and -1.633566 at 0.025, ratio 3.94; the ratio must lie in [3.7, 4.3]"""
    p = ff.LEAPFROG
    X = p["X"]
    U, A, phi, op = ff.leapfrog_inputs(oracle)
    H0 = ff.hamiltonian(oracle, U, A, phi, op, X, p["beta"], p["tol"])
    dH = []
    for dt in p["dt"]:
        U1, A1 = ff.leapfrog(oracle, U, A, phi, op, X, p["beta"], dt, int(round(p["tau"] / dt)), p["tol"])
        dH.append(ff.hamiltonian(oracle, U1, A1, phi, op, X, p["beta"], p["tol"]) - H0)
    print("dH = %.6e, %.6e, ratio %.4f" % (dH[0], dH[1], dH[0] / dH[1]))
    assert 3.7 <= dH[0] / dH[1] <= 4.3
