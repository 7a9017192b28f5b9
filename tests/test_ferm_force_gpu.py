"""The fermion force on the GPU (qudaAmdFermionOprodForce, qudaAmdComputeTMForce) against the numpy reference tests/ferm_force_ref.py, which
takes neighbours by np.roll and contracts explicit 4x4 projectors by einsum, so it shares neither the gather, the ghost zones nor the half-spinor
form with the device.  Lattices 4^4 and 6x4x2x8: odd half-extent in x, extent 2 in z (x + mu and x - mu are the same site).

Bounds.  Kernel on fp64 18-real links: 1e-12 x max|reference|, the bound of the project's fp64 gauge kernels.  fp32 12-real links: the
reference on links rounded the same way (rows 0 and 1 to fp32, row 2 rebuilt from them in fp32) against the reference on the fp64 links, times 4
for operation order, recomputed by the test from its own inputs as test_gauge_md_gpu.py does.  Driver: 4e-12 x max|reference|, the fp64 operator
parity bound of tests/test_dslash_gpu.py once for each of the three operator applications in front of the product and once for the product.
Leapfrog: see test_leapfrog_through_the_c_abi."""
import importlib

import numpy as np
import pytest

import ferm_force_ref as ff
import gauge_md_ref as md
import gauge_obs_ref as ob

pytestmark = pytest.mark.gpu

LATTICES = [(4, 4, 4, 4), (6, 4, 2, 8)]
KAPPA, MU, EPSILON = 0.13, 0.2, 0.15
COEFF = [0.3, -1.1, 0.7]
LINKS = {"fp64-18": (8, 18), "fp32-12": (4, 12)}

OPS = {}
for _m in ("ee", "oo", "eeasym", "ooasym"):
    for _f in (+1, -1):
        OPS["tm_%s_%s" % (_m, "plus" if _f > 0 else "minus")] = ff.Op("tm", KAPPA, MU, _f, matpc=_m)
    OPS["ndeg_%s" % _m] = ff.Op("ndeg", KAPPA, MU, epsilon=EPSILON, matpc=_m)
for _m in ("ee", "oo"):
    OPS["wilson_%s" % _m] = ff.Op("wilson", KAPPA, matpc=_m)
OPS["tm_ee_plus_mass"] = ff.Op("tm", KAPPA, MU, +1, matpc="ee", norm="mass")
OPS["ndeg_ooasym_asym_mass"] = ff.Op("ndeg", KAPPA, MU, epsilon=EPSILON, matpc="ooasym", norm="asym_mass")


@pytest.fixture(scope="module")
def qa():
    mod = importlib.import_module("quda-qkxtm-multigrid_amd")
    mod.init(0)
    yield mod
    mod.end()


def _flavours(oracle, full, X, nf):
    """a full host field ([even][odd], a doublet [flavour 1][flavour 2] within each parity) -> per flavour psi[t, z, y, x, 4, 3]"""
    h = full.size // 2
    q = h // nf
    return [ff.lex_spinor(oracle, np.concatenate([full[f * q:(f + 1) * q], full[h + f * q:h + (f + 1) * q]]), X) for f in range(nf)]


@pytest.fixture(scope="module")
def cases(oracle):
    """per lattice: hot links with the anti-periodic sign, a momentum, three pairs of random full fields of one and of two flavours, and the
    references of the kernel-level operation; computed once and never modified"""
    out = {}
    for X in LATTICES:
        V = int(np.prod(X))
        hot, _, _ = oracle.make_fields(list(X), seed=31, antiperiodic_t=True, clover=False)
        U = ob.from_qdp(oracle, hot, X)
        rng = np.random.default_rng(17)
        A0 = md.random_momentum(rng, (4, X[3], X[2], X[1], X[0]))
        c = {"hot": hot, "U": U, "A0": A0, "mom0": md.mom_to_host(oracle, A0, X), "x1": rng.standard_normal((2, V * 12)), "x2": rng.standard_normal((2, V * 24))}
        zero = np.zeros_like(A0)
        rounded = ob.fp32_recon12(U, True)
        for nf in (1, 2):
            xs, ys = rng.standard_normal((3, nf * V * 24)), rng.standard_normal((3, nf * V * 24))
            c["xs", nf], c["ys", nf] = xs, ys
            pairs = [(_flavours(oracle, x, X, nf), _flavours(oracle, y, X, nf)) for x, y in zip(xs, ys)]
            for nv in (1, 3):
                c["acc", nf, nv] = ff.oprod_force(U, A0, pairs[:nv], COEFF[:nv])
                c["over", nf, nv] = ff.oprod_force(U, zero, pairs[:nv], COEFF[:nv])
                c["fp32", nf, nv] = np.max(np.abs(ff.oprod_force(rounded, A0, pairs[:nv], COEFF[:nv]) - c["acc", nf, nv]))
        out[X] = c
    return out


def _load(qa, gauge, X, mask=0, prec=8, recon=18):
    qa.lib().qudaAmdSetPartitionMask(mask)
    gp = qa.gauge_param(X, cuda_prec=prec, recon=recon, t_boundary=qa.QUDA_ANTI_PERIODIC_T)
    qa.load_gauge(gauge, gp)
    return gp


def _ip(qa, op):
    kind = {"wilson": qa.QUDA_WILSON_DSLASH, "tm": qa.QUDA_TWISTED_MASS_DSLASH, "ndeg": qa.QUDA_TWISTED_MASS_DSLASH}[op.kind]
    flavor = qa.QUDA_TWIST_NONDEG_DOUBLET if op.kind == "ndeg" else op.flavor
    ip = qa.invert_param(kind, op.kappa, op.mu, flavor, op.matpc, 0, solution_type=qa.QUDA_MATPCDAG_MATPC_SOLUTION, epsilon=op.epsilon)
    ip.solve_type = qa.QUDA_NORMOP_PC_SOLVE
    ip.mass_normalization = {"kappa": qa.QUDA_KAPPA_NORMALIZATION, "mass": qa.QUDA_MASS_NORMALIZATION, "asym_mass": qa.QUDA_ASYMMETRIC_MASS_NORMALIZATION}[op.norm]
    return ip


def _full_ip(qa, nf):
    ip = qa.invert_param(qa.QUDA_TWISTED_MASS_DSLASH, KAPPA, MU, qa.QUDA_TWIST_NONDEG_DOUBLET if nf == 2 else qa.QUDA_TWIST_PLUS, "ee", 0,
                         solution_type=qa.QUDA_MAT_SOLUTION, epsilon=EPSILON if nf == 2 else 0.0)
    return ip


@pytest.mark.parametrize("X", LATTICES)
@pytest.mark.parametrize("mask", [0, 0b0111, 0b1010])
@pytest.mark.parametrize("links", sorted(LINKS))
@pytest.mark.parametrize("nf", [1, 2])
def test_kernel_matches_the_reference(qa, oracle, cases, X, mask, links, nf):
    """random full fields, nvector 1 and 3, accumulation onto a non-zero momentum and overwrite_mom, one and two flavours"""
    c = cases[X]
    prec, recon = LINKS[links]
    try:
        gp = _load(qa, c["hot"], X, mask, prec, recon)
        ip = _full_ip(qa, nf)
        for nv in (1, 3):
            want = c["acc", nf, nv]
            scale = np.max(np.abs(want))
            tol = 1e-12 * scale if prec == 8 else 4.0 * c["fp32", nf, nv]
            xs, ys = list(c["xs", nf][:nv]), list(c["ys", nf][:nv])
            raw = qa.ferm_oprod_force(gp, ip, xs, ys, COEFF[:nv], mom=c["mom0"])
            err = np.max(np.abs(md.mom_from_host(oracle, raw, X) - want))
            print("%s mask %d %s nf %d nvector %d: max|delta| = %.3e, max|ref| = %.3e, rounded-link reference %.3e" % (X, mask, links, nf, nv, err, scale, c["fp32", nf, nv]))
            assert err <= tol
            over = qa.ferm_oprod_force(gp, ip, xs, ys, COEFF[:nv], overwrite=True)
            assert np.max(np.abs(md.mom_from_host(oracle, over, X) - c["over", nf, nv])) <= tol
            # the packed momentum is traceless and its tenth real is 0
            assert np.all(raw[..., 9] == 0) and np.max(np.abs(raw[..., 6:9].sum(axis=-1))) <= 1e-14 * scale
    finally:
        qa.lib().qudaAmdSetPartitionMask(0)


@pytest.mark.parametrize("nf,nv", [(1, 17), (2, 9)])
def test_more_pairs_than_one_launch_holds(qa, oracle, cases, nf, nv):
    """one launch takes 16 (X, Y) pairs, a doublet counting two: 17 single-flavour pairs and 9 doublets are chunked on the host, the
    second launch accumulating onto the result of the first.  The pairs are the three of the fixture in turn, with their own coefficients"""
    X = LATTICES[0]
    c = cases[X]
    coeff = [0.05 * (k + 1) * (-1) ** k for k in range(nv)]
    xs, ys = [c["xs", nf][k % 3] for k in range(nv)], [c["ys", nf][k % 3] for k in range(nv)]
    pairs = [(_flavours(oracle, x, X, nf), _flavours(oracle, y, X, nf)) for x, y in zip(xs[:3], ys[:3])]
    want = ff.oprod_force(c["U"], c["A0"], pairs, [sum(coeff[k::3]) for k in range(3)])
    try:
        gp = _load(qa, c["hot"], X, 0b1010)
        got = md.mom_from_host(oracle, qa.ferm_oprod_force(gp, _full_ip(qa, nf), xs, ys, coeff, mom=c["mom0"]), X)
    finally:
        qa.lib().qudaAmdSetPartitionMask(0)
    err, scale = np.max(np.abs(got - want)), np.max(np.abs(want))
    print("nf %d nvector %d: max|delta| = %.3e, max|ref| = %.3e" % (nf, nv, err, scale))
    assert err <= 1e-12 * scale


@pytest.mark.parametrize("X", LATTICES)
@pytest.mark.parametrize("mask", [0, 0b1010])
@pytest.mark.parametrize("name", sorted(OPS))
def test_driver_matches_the_reference(qa, oracle, cases, X, mask, name):
    """mom + dt sum_i coeff_i F[x_i] for two solutions, X and Y built on the device by the Dirac classes"""
    op = OPS[name]
    c = cases[X]
    xs = list(c["x2"] if op.nflavor == 2 else c["x1"])
    dt, coeff = 0.1, [0.8, -0.35]
    want = ff.tm_force(oracle, c["U"], c["A0"], xs, coeff, dt, op, X)
    try:
        gp = _load(qa, c["hot"], X, mask)
        got = md.mom_from_host(oracle, qa.tm_force(gp, _ip(qa, op), xs, coeff, dt, mom=c["mom0"]), X)
    finally:
        qa.lib().qudaAmdSetPartitionMask(0)
    err, scale = np.max(np.abs(got - want)), np.max(np.abs(want))
    print("%s %s mask %d: max|delta| = %.3e, max|ref| = %.3e, max|ref - mom| = %.3e" % (name, X, mask, err, scale, np.max(np.abs(want - c["A0"]))))
    assert err <= 4e-12 * scale


def test_resident_momentum(qa, oracle, cases):
    """make_resident_mom, then use_resident_mom: the same bits as passing the host momentum"""
    X = LATTICES[1]
    c = cases[X]
    op = OPS["tm_eeasym_plus"]
    xs = list(c["x1"])
    gp = _load(qa, c["hot"], X)
    ip = _ip(qa, op)
    one = qa.tm_force(gp, ip, xs, [0.8, -0.35], 0.1, mom=c["mom0"], make_resident_mom=True)
    two = qa.tm_force(gp, ip, xs[:1], [0.5], 0.2, make_resident_mom=True)            # use_resident_mom
    host = qa.tm_force(gp, ip, xs[:1], [0.5], 0.2, mom=one)
    assert np.array_equal(two, host)
    assert qa.mom_action(gp) == qa.mom_action(gp, host)
    # the kernel-level call honours the flags in the same way
    fip = _full_ip(qa, 1)
    a = qa.ferm_oprod_force(gp, fip, [c["xs", 1][0]], [c["ys", 1][0]], [0.3], make_resident_mom=True)
    assert np.array_equal(a, qa.ferm_oprod_force(gp, fip, [c["xs", 1][0]], [c["ys", 1][0]], [0.3], mom=host))
    # overwrite with a resident momentum starts from zero and leaves the result resident
    b = qa.ferm_oprod_force(gp, fip, [c["xs", 1][0]], [c["ys", 1][0]], [0.3], overwrite=True, make_resident_mom=True)
    assert np.array_equal(b, qa.ferm_oprod_force(gp, fip, [c["xs", 1][0]], [c["ys", 1][0]], [0.3], mom=np.zeros_like(host)))
    assert qa.mom_action(gp) == qa.mom_action(gp, b)


def test_leapfrog_through_the_c_abi(qa, oracle):
    """The inputs of ferm_force_ref.LEAPFROG; every step is update_gauge with make_resident_gauge, a CG QUDA_NORMOP_PC_SOLVE to 1e-12, the gauge
    force and tm_force, links and momenta resident throughout.  dH(dt) / dH(dt/2) must lie in [3.5, 4.5].  The final momentum must agree
    with the reference's within ten times the difference of the reference's own final momenta with its CG run to 1e-12 and to 1e-11 (ten for
    the solver's different path), or N_steps x 4e-12 x max|momentum| where that is larger.  Measured on the CPU: the difference is
    1.30e-11 at dt = 0.05 (10 steps; ten times it 1.30e-10, floor 1.33e-10) and 1.30e-11 at dt = 0.025 (20 steps, floor 2.67e-10), so the
    floor is the bound in both; the test recomputes all of it."""
    p = ff.LEAPFROG
    X, beta = p["X"], p["beta"]
    V = int(np.prod(X))
    U0, A0, phi, op = ff.leapfrog_inputs(oracle)
    paths, coeff = md.wilson_paths()
    host_links, host_mom = ob.to_qdp(oracle, U0, X), md.mom_to_host(oracle, A0, X)
    ip = _ip(qa, op)
    ip.inv_type, ip.tol, ip.maxiter = qa.QUDA_CG_INVERTER, p["tol"], 2000

    def hamiltonian(gp):
        return qa.mom_action(gp) - 6.0 * beta * V * qa.plaquette()[0] + float(np.dot(phi, qa.invert(phi, ip)))

    def kick(gp, h, mom=None, last=False):
        x = qa.invert(phi, ip)
        qa.gauge_force(gp, paths, coeff, h * beta / 3.0, mom=mom, make_resident_mom=True, return_mom=False)
        return qa.tm_force(gp, ip, [x], [1.0], h, make_resident_mom=True, return_mom=last)

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
        _, Ar = ff.leapfrog(oracle, U0, A0, phi, op, X, beta, dt, n, 1e-12)
        _, Ar11 = ff.leapfrog(oracle, U0, A0, phi, op, X, beta, dt, n, 1e-11)
        measured = np.max(np.abs(Ar - Ar11))
        bound = max(10.0 * measured, n * 4e-12 * np.max(np.abs(Ar)))
        err = np.max(np.abs(md.mom_from_host(oracle, mom1, X) - Ar))
        print("dt %.3f, %d steps: dH = %.9e, momenta %.3e (bound %.3e: reference 1e-12 vs 1e-11 %.3e, max %.3e)" % (dt, n, dH[-1], err, bound, measured, np.max(np.abs(Ar))))
        assert err <= bound
    print("dH ratio %.4f" % (dH[0] / dH[1]))
    assert 3.5 <= dH[0] / dH[1] <= 4.5
