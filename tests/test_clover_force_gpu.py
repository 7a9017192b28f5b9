"""The twisted-clover force on the GPU (qudaAmdCloverSigmaOprod, qudaAmdCloverSigmaTrace, qudaAmdCloverDerivativeForce, qudaAmdCloverLogDetForce and
qudaAmdComputeTMForce with a twisted-clover inv_param) against the numpy reference tests/clover_force_ref.py, which takes neighbours by np.roll,
walks every plaquette link by link, contracts explicit 4x4 sigma matrices by einsum and inverts dense 12x12 site matrices, so it shares
nothing with the device formulation.  Lattices 4^4 and 6x4x2x8: odd half-extent in x, extent 2 in z (x + nu and x - nu are the same site).
Hot links with the anti-periodic sign.

Bounds.  Derivative kernel on fp64 links (18 and 12 reals): 1e-12 x max|reference|, the bound of the project's fp64 gauge kernels.  fp32 12-real
links: the reference on links rounded the same way against the reference on the fp64 links, times 4 for operation order, recomputed by the
test from its own inputs as test_ferm_force_gpu.py does.  The other bounds are counted in the docstrings of their tests in units of 1e-12 x
max|reference|, the fp64 operator bound of tests/test_dslash_gpu.py."""
import importlib
import os
import subprocess
import sys

import numpy as np
import pytest

import clover_force_ref as cf
import ferm_force_ref as ff
import gauge_md_ref as md
import gauge_obs_ref as ob

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

LATTICES = [(4, 4, 4, 4), (6, 4, 2, 8)]
KAPPA, MU, CSW = 0.13, 0.2, 0.13 * 1.57551
COEFF = [0.3, -1.1, 0.7]
LINKS = {"fp64-18": (8, 18), "fp64-12": (8, 12), "fp32-12": (4, 12)}
DERIV_COEFF = -0.7

OPS = {}
for _m in ("ee", "oo", "eeasym", "ooasym"):
    for _f in (+1, -1):
        OPS["tmc_%s_%s" % (_m, "plus" if _f > 0 else "minus")] = cf.Op(KAPPA, MU, _f, CSW, matpc=_m)
OPS["tmc_ee_mu0"] = cf.Op(KAPPA, 0.0, +1, CSW, matpc="ee")
OPS["tmc_ooasym_mu0"] = cf.Op(KAPPA, 0.0, +1, CSW, matpc="ooasym")
OPS["tmc_ee_plus_mass"] = cf.Op(KAPPA, MU, +1, CSW, matpc="ee", norm="mass")
OPS["tmc_ooasym_minus_asym_mass"] = cf.Op(KAPPA, MU, -1, CSW, matpc="ooasym", norm="asym_mass")


def _driver_units(op):
    """1e-12 units of the driver bound: the three operator applications in front of the hop product that the 4e-12 of
    test_ferm_force_gpu.test_driver_matches_the_reference counts (R^-1 D x, Mh x, R^-dag D^dag y), one more inverse (R^-dag on Mh x) under
    symmetric preconditioning, the construction of the clover term and its twisted inverse on the device (one each), and the three
    kernels (hop outer product, sigma outer product, derivative): 8 asymmetric, 9 symmetric"""
    return 8 if op.asym else 9


@pytest.fixture(scope="module")
def qa():
    mod = importlib.import_module("quda-qkxtm-multigrid_amd")
    mod.init(0)
    yield mod
    mod.end()


@pytest.fixture(scope="module")
def cases(oracle):
    """per lattice: hot links with the anti-periodic sign, a momentum, a random complex tensor field, three pairs of random full fields,
    three parity fields, the clover matrix and the references of the derivative; computed once and never modified"""
    out = {}
    for X in LATTICES:
        V = int(np.prod(X))
        hot, _, _ = oracle.make_fields(list(X), seed=31, antiperiodic_t=True, clover=False)
        U = ob.from_qdp(oracle, hot, X)
        rng = np.random.default_rng(23)
        A0 = md.random_momentum(rng, (4, X[3], X[2], X[1], X[0]))
        hT = rng.standard_normal((V, 6, 3, 3, 2))
        T = cf.tensor_from_host(oracle, hT, X)
        c = {"hot": hot, "U": U, "A0": A0, "mom0": md.mom_to_host(oracle, A0, X), "hT": hT, "T": T, "x1": rng.standard_normal((3, V * 12)),
             "xs": rng.standard_normal((3, V * 24)), "ys": rng.standard_normal((3, V * 24)), "A": cf.clover_matrix(U, CSW)}
        c["acc"] = cf.deriv_force(U, A0, T, DERIV_COEFF)
        c["over"] = cf.deriv_force(U, np.zeros_like(A0), T, DERIV_COEFF)
        c["fp32"] = np.max(np.abs(cf.deriv_force(ob.fp32_recon12(U, True), A0, T, DERIV_COEFF) - c["acc"]))
        c["S"] = [cf.sigma_oprod(ff.lex_spinor(oracle, x, X), ff.lex_spinor(oracle, y, X)) for x, y in zip(c["xs"], c["ys"])]
        c["par"] = cf.parity_mask((X[3], X[2], X[1], X[0]))
        out[X] = c
    return out


def _load(qa, gauge, X, mask=0, prec=8, recon=18):
    qa.lib().qudaAmdSetPartitionMask(mask)
    gp = qa.gauge_param(X, cuda_prec=prec, recon=recon, t_boundary=qa.QUDA_ANTI_PERIODIC_T)
    qa.load_gauge(gauge, gp)
    return gp


def _ip(qa, op):
    ip = qa.invert_param(qa.QUDA_TWISTED_CLOVER_DSLASH, op.kappa, op.mu, op.flavor, op.matpc, 0, solution_type=qa.QUDA_MATPCDAG_MATPC_SOLUTION)
    ip.solve_type = qa.QUDA_NORMOP_PC_SOLVE
    ip.mass_normalization = {"kappa": qa.QUDA_KAPPA_NORMALIZATION, "mass": qa.QUDA_MASS_NORMALIZATION, "asym_mass": qa.QUDA_ASYMMETRIC_MASS_NORMALIZATION}[op.norm]
    ip.clover_coeff = op.c
    return ip


def _full_ip(qa):
    return qa.invert_param(qa.QUDA_TWISTED_CLOVER_DSLASH, KAPPA, MU, qa.QUDA_TWIST_PLUS, "ee", 0, solution_type=qa.QUDA_MAT_SOLUTION)


@pytest.mark.parametrize("X", LATTICES)
@pytest.mark.parametrize("links", sorted(LINKS))
def test_derivative_kernel_matches_the_reference(qa, oracle, cases, X, links):
    """a random general complex tensor field, accumulation onto a non-zero momentum and overwrite_mom; 12-real links take the anti-periodic
    sign through tsign, 18-real links carry it"""
    c = cases[X]
    prec, recon = LINKS[links]
    gp = _load(qa, c["hot"], X, 0, prec, recon)
    want = c["acc"]
    scale = np.max(np.abs(want))
    tol = 1e-12 * scale if prec == 8 else 4.0 * c["fp32"]
    raw = qa.clover_derivative_force(gp, c["hT"], DERIV_COEFF, mom=c["mom0"])
    err = np.max(np.abs(md.mom_from_host(oracle, raw, X) - want))
    print("%s %s: max|delta| = %.3e, max|ref| = %.3e, max|ref - mom| = %.3e, rounded-link reference %.3e" % (X, links, err, scale, np.max(np.abs(want - c["A0"])), c["fp32"]))
    assert err <= tol
    over = qa.clover_derivative_force(gp, c["hT"], DERIV_COEFF, overwrite=True)
    assert np.max(np.abs(md.mom_from_host(oracle, over, X) - c["over"])) <= tol
    # the packed momentum is traceless and its tenth real is 0
    assert np.all(raw[..., 9] == 0) and np.max(np.abs(raw[..., 6:9].sum(axis=-1))) <= 1e-14 * scale


@pytest.mark.parametrize("X", LATTICES)
@pytest.mark.parametrize("mask", [0, 0b1010])
@pytest.mark.parametrize("nv", [1, 3, 17])
def test_sigma_outer_product_matches_the_reference(qa, oracle, cases, X, mask, nv):
    """nvector 1 and 3 with distinct even and odd coefficients, and 17 pairs (one launch holds 16; the second accumulates onto the first):
    the three pairs of the fixture in turn, with their own coefficients"""
    c = cases[X]
    V = int(np.prod(X))
    coeff = np.array([[0.05 * (k + 1) * (-1) ** k, -0.03 * (k + 2)] for k in range(nv)]) if nv > 3 else np.array([[COEFF[k], -0.5 * COEFF[k] + 0.1] for k in range(nv)])
    want = 0.0
    for k in range(min(nv, 3)):
        w = np.where(c["par"] == 0, coeff[k::3, 0].sum(), coeff[k::3, 1].sum())[..., None, None]
        want = want + w * c["S"][k]
    try:
        _load(qa, c["hot"], X, mask)
        got = qa.clover_sigma_oprod(_full_ip(qa), [c["xs"][k % 3] for k in range(nv)], [c["ys"][k % 3] for k in range(nv)], coeff, V)
    finally:
        qa.lib().qudaAmdSetPartitionMask(0)
    err, scale = np.max(np.abs(cf.tensor_from_host(oracle, got, X) - want)), np.max(np.abs(want))
    print("%s mask %d nvector %d: max|delta| = %.3e, max|ref| = %.3e" % (X, mask, nv, err, scale))
    assert err <= 1e-12 * scale


@pytest.mark.parametrize("X", LATTICES)
@pytest.mark.parametrize("flavor,mu", [(+1, MU), (-1, MU), (+1, 0.0)])
def test_sigma_trace_matches_the_reference(qa, oracle, cases, X, flavor, mu):
    """B = A (A^2 + a^2)^-1 from the clover term built on the device from the links.  Bound 3e-12 x max|reference|: the fp64 operator bound
    1e-12 once for the construction of the clover term, once for its (twisted) inverse and once for the product and trace"""
    c = cases[X]
    V = int(np.prod(X))
    _load(qa, c["hot"], X)
    ip = _ip(qa, cf.Op(KAPPA, mu, flavor, CSW))
    qa.load_clover(None, None, ip)
    got = cf.tensor_from_host(oracle, qa.clover_sigma_trace(ip, 0.8, -1.3, V), X)
    want = cf.sigma_trace(c["A"], 2 * KAPPA * mu * flavor, (0.8, -1.3))
    err, scale = np.max(np.abs(got - want)), np.max(np.abs(want))
    print("%s flavor %d mu %.2f: max|delta| = %.3e, max|ref| = %.3e" % (X, flavor, mu, err, scale))
    assert scale > 1e-3
    assert err <= 3e-12 * scale


@pytest.mark.parametrize("X", LATTICES)
@pytest.mark.parametrize("which", ["even", "odd", "both"])
def test_logdet_force_matches_the_reference(qa, oracle, cases, X, which):
    """mom + dt (c_e F[L_even] + c_o F[L_odd]).  Bound 4e-12 x max|reference|: the three of the sigma trace and one for the derivative kernel"""
    c = cases[X]
    ce, co = {"even": (1.0, 0.0), "odd": (0.0, -1.0), "both": (0.6, -1.4)}[which]
    dt = 0.3
    gp = _load(qa, c["hot"], X)
    ip = _ip(qa, OPS["tmc_ee_plus"])
    qa.load_clover(None, None, ip)
    got = md.mom_from_host(oracle, qa.clover_logdet_force(gp, ip, dt, ce, co, mom=c["mom0"]), X)
    want = cf.logdet_force(c["U"], c["A0"], CSW, 2 * KAPPA * MU, dt, (ce, co))
    err, scale = np.max(np.abs(got - want)), np.max(np.abs(want))
    print("%s %s: max|delta| = %.3e, max|ref| = %.3e, max|ref - mom| = %.3e" % (X, which, err, scale, np.max(np.abs(want - c["A0"]))))
    assert np.max(np.abs(want - c["A0"])) > 1e-4
    assert err <= 4e-12 * scale
    # the determinant itself: trlogA of loadCloverQuda is L_p
    ld = cf.logdet(c["U"], CSW, 2 * KAPPA * MU)
    assert np.max(np.abs(np.array([ip.trlogA[0], ip.trlogA[1]]) - ld)) <= 1e-12 * np.max(np.abs(ld)) * 3


@pytest.mark.parametrize("X", LATTICES)
@pytest.mark.parametrize("name", sorted(OPS))
def test_driver_matches_the_reference(qa, oracle, cases, X, name):
    """tm_force with a twisted-clover inv_param: mom + dt sum_i coeff_i F[x_i] for three solutions, hop and clover part, X and Y built on the
    device by the Dirac classes on a clover term built on the device.  The four matpc types, both flavours, mu = 0, the two extra
    normalisations.  Bound: _driver_units (8 or 9) x 1e-12 x max|reference|, counted there"""
    op = OPS[name]
    c = cases[X]
    xs = list(c["x1"])
    dt, coeff = 0.1, [0.8, -0.35, 0.5]
    want = cf.tmc_force(oracle, c["U"], c["A0"], xs, coeff, dt, op, X)
    gp = _load(qa, c["hot"], X)
    ip = _ip(qa, op)
    qa.load_clover(None, None, ip)
    got = md.mom_from_host(oracle, qa.tm_force(gp, ip, xs, coeff, dt, mom=c["mom0"]), X)
    err, scale = np.max(np.abs(got - want)), np.max(np.abs(want))
    hop_only = ff.oprod_force(c["U"], c["A0"], [op.force_fields(oracle, c["hot"], x, X)[:2] for x in xs], [-dt * cc * op.force_coeff() for cc in coeff])
    print("%s %s: max|delta| = %.3e, max|ref| = %.3e, max|ref - mom| = %.3e, clover part %.3e" % (name, X, err, scale, np.max(np.abs(want - c["A0"])), np.max(np.abs(want - hop_only))))
    assert np.max(np.abs(want - hop_only)) > 1e-6 * scale
    assert err <= _driver_units(op) * 1e-12 * scale


def test_resident_momentum(qa, oracle, cases):
    """gauge force, twisted-clover force and determinant force chained through make_resident_mom / use_resident_mom: the sum of the references
    and the derivative of a
    tensor field on top, within the sum of their bounds (1 + 8 + 4 + 1) x 1e-12 x max|reference|, and the same bits as passing the host momentum from call to call"""
    X = LATTICES[1]
    c = cases[X]
    op = OPS["tmc_eeasym_plus"]
    xs, coeff, dt = list(c["x1"][:2]), [0.8, -0.35], 0.1
    paths, pc = md.wilson_paths()
    eb3 = dt * 5.5 / 3.0
    want = md.force(c["U"], c["A0"], paths, pc, eb3)
    want = cf.tmc_force(oracle, c["U"], want, xs, coeff, dt, op, X)
    want = cf.logdet_force(c["U"], want, CSW, op.a, dt, (0.0, -1.0))
    want = cf.deriv_force(c["U"], want, c["T"], DERIV_COEFF)
    gp = _load(qa, c["hot"], X)
    ip = _ip(qa, op)
    qa.load_clover(None, None, ip)
    qa.gauge_force(gp, paths, pc, eb3, mom=c["mom0"], make_resident_mom=True, return_mom=False)
    qa.tm_force(gp, ip, xs, coeff, dt, make_resident_mom=True, return_mom=False)
    qa.clover_logdet_force(gp, ip, dt, 0.0, -1.0, make_resident_mom=True, return_mom=False)
    got = qa.clover_derivative_force(gp, c["hT"], DERIV_COEFF, make_resident_mom=True)
    err, scale = np.max(np.abs(md.mom_from_host(oracle, got, X) - want)), np.max(np.abs(want))
    print("chained: max|delta| = %.3e, max|ref| = %.3e" % (err, scale))
    assert err <= 14e-12 * scale
    assert qa.mom_action(gp) == qa.mom_action(gp, got)
    host = qa.gauge_force(gp, paths, pc, eb3, mom=c["mom0"])
    host = qa.tm_force(gp, ip, xs, coeff, dt, mom=host)
    host = qa.clover_logdet_force(gp, ip, dt, 0.0, -1.0, mom=host)
    host = qa.clover_derivative_force(gp, c["hT"], DERIV_COEFF, mom=host)
    assert np.array_equal(got, host)


def test_hop_outer_product_takes_a_clover_inv_param(qa, cases):
    """qudaAmdFermionOprodForce does not depend on the action: the same bits under a twisted-clover and a twisted-mass inv_param"""
    X = LATTICES[1]
    c = cases[X]
    gp = _load(qa, c["hot"], X)
    tm = qa.invert_param(qa.QUDA_TWISTED_MASS_DSLASH, KAPPA, MU, qa.QUDA_TWIST_PLUS, "ee", 0, solution_type=qa.QUDA_MAT_SOLUTION)
    a = qa.ferm_oprod_force(gp, tm, list(c["xs"][:2]), list(c["ys"][:2]), COEFF[:2], mom=c["mom0"])
    b = qa.ferm_oprod_force(gp, _full_ip(qa), list(c["xs"][:2]), list(c["ys"][:2]), COEFF[:2], mom=c["mom0"])
    assert np.array_equal(a, b) and np.max(np.abs(a - c["mom0"])) > 1e-3


@pytest.mark.parametrize("case,message", [("partitioned_derivative", "unpartitioned lattices only (partitioned directions y t, mask 0xa)"),
                                          ("partitioned_tm_force", "unpartitioned lattices only (partitioned directions y t, mask 0xa)"),
                                          ("partitioned_logdet", "unpartitioned lattices only (partitioned directions y t, mask 0xa)"),
                                          ("clover_from_the_host", "its coefficient is unknown"),
                                          ("another_clover_coeff", "the resident clover term was built with"),
                                          ("another_mu", "the resident clover inverse was computed with"),
                                          ("clover_not_fp64", "clover_cuda_prec must be fp64"),
                                          ("no_clover_term", "no resident clover term"),
                                          ("doublet", "no doublet")])
def test_refusals(case, message):
    """the refusals of DESIGN section 3 "Twisted-clover force" and section 7 in the library's error convention (message, exit status 1), each case
    in a child process (tools/clover_force_error_cases.py)"""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "clover_force_error_cases.py"), case], capture_output=True, text=True, timeout=300)
    out = r.stdout + r.stderr
    assert r.returncode == 1, (r.returncode, out[-1500:])
    assert "ERROR:" in out and message in out and "NOT REACHED" not in out, out[-1500:]


def test_leapfrog_through_the_c_abi(qa, oracle):
    """The inputs of clover_force_ref.LEAPFROG; every step is update_gauge with make_resident_gauge, loadCloverQuda(NULL, NULL), a CG
    QUDA_NORMOP_PC_SOLVE to 1e-12, the gauge force, tm_force and clover_logdet_force, links and momenta resident throughout.  The device's
    dH(dt) / dH(dt/2) must lie in [3.7, 4.3].  The final momentum must agree with the reference's within ten times the difference of the
    reference's own final momenta with its CG run to 1e-12 and to 1e-11, the construction of
    test_ferm_force_gpu.test_leapfrog_through_the_c_abi; the test recomputes it."""
    p = cf.LEAPFROG
    X, beta, cdet = p["X"], p["beta"], p["cdet"]
    V = int(np.prod(X))
    U0, A0, phi, op = cf.leapfrog_inputs(oracle)
    paths, coeff = md.wilson_paths()
    host_links, host_mom = ob.to_qdp(oracle, U0, X), md.mom_to_host(oracle, A0, X)
    ip = _ip(qa, op)
    ip.inv_type, ip.tol, ip.maxiter = qa.QUDA_CG_INVERTER, p["tol"], 2000

    def hamiltonian(gp):
        qa.load_clover(None, None, ip)
        return (qa.mom_action(gp) - 6.0 * beta * V * qa.plaquette()[0] + float(np.dot(phi, qa.invert(phi, ip)))
                - cdet[0] * ip.trlogA[0] - cdet[1] * ip.trlogA[1])

    def kick(gp, h, mom=None, last=False):
        qa.load_clover(None, None, ip)
        x = qa.invert(phi, ip)
        qa.gauge_force(gp, paths, coeff, h * beta / 3.0, mom=mom, make_resident_mom=True, return_mom=False)
        qa.tm_force(gp, ip, [x], [1.0], h, make_resident_mom=True, return_mom=False)
        return qa.clover_logdet_force(gp, ip, h, -cdet[0], -cdet[1], make_resident_mom=True, return_mom=last)

    dH = []
    for dt in p["dt"]:
        n = int(round(p["tau"] / dt))
        gp = _load(qa, host_links, X)
        qa.mom_action(gp, host_mom, make_resident_mom=True)
        H0 = hamiltonian(gp)
        kick(gp, 0.5 * dt, mom=host_mom)
        for step in range(n):
            qa.update_gauge(gp, dt, make_resident_gauge=True, make_resident_mom=True, return_gauge=False)
            last = step == n - 1
            mom1 = kick(gp, 0.5 * dt if last else dt, last=last)
        dH.append(hamiltonian(gp) - H0)
        _, Ar = cf.leapfrog(oracle, U0, A0, phi, op, X, beta, dt, n, 1e-12, cdet)
        _, Ar11 = cf.leapfrog(oracle, U0, A0, phi, op, X, beta, dt, n, 1e-11, cdet)
        measured = np.max(np.abs(Ar - Ar11))
        bound = 10.0 * measured
        err = np.max(np.abs(md.mom_from_host(oracle, mom1, X) - Ar))
        print("dt %.3f, %d steps: dH = %.9e, momenta %.3e (bound %.3e: reference 1e-12 vs 1e-11 %.3e, max %.3e)" % (dt, n, dH[-1], err, bound, measured, np.max(np.abs(Ar))))
        assert err <= bound
    print("dH ratio %.4f" % (dH[0] / dH[1]))
    assert 3.7 <= dH[0] / dH[1] <= 4.3
