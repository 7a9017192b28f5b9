"""Gauge molecular dynamics on the GPU (computeGaugeForceQuda, updateGaugeFieldQuda, momActionQuda, projectSU3Quda) against the numpy
reference tests/gauge_md_ref.py, which walks paths by np.roll, exponentiates by eigh and projects by SVD, so it shares neither the
gather, the transport formulation, the Cayley-Hamilton form nor the polar iteration with the device.

Bounds.  fp64: 1e-12 x max|reference| (the bound of the project's fp64 gauge kernels, test_gauge_obs_gpu.py).  fp32 12-real
resident links: the reference on links rounded the same way (rows 0 and 1 to fp32, row 2 rebuilt from them in fp32) against the
reference on the fp64 links, times 4 for operation order; measured on the CPU for the hot fields with eb3 = 0.3
(max|reference| 3.4 to 3.8): Wilson 7.4e-8 (4^4) and 7.2e-8 (6x4x2x8), Symanzik 1.25e-7 and 1.22e-7.  The test recomputes the figure
from its own inputs; the device came within 8.0e-8 / 9.2e-8 (Wilson) and 1.37e-7 / 1.47e-7 (Symanzik) of the fp64 reference.
Leapfrog of N steps: N x 1e-12, the per-application bound accumulated linearly."""
import importlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import gauge_md_ref as md
import gauge_obs_ref as ob
from synth import smooth_gauge

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LATTICES = [(4, 4, 4, 4), (6, 4, 2, 8)]
EB3 = 0.3
TABLES = {"wilson": md.wilson_paths(), "symanzik": md.symanzik_paths()}


@pytest.fixture(scope="module")
def qa():
    mod = importlib.import_module("quda-qkxtm-multigrid_amd")
    mod.init(0)
    yield mod
    mod.end()


def _dag(a):
    return np.conj(np.swapaxes(a, -1, -2))


@pytest.fixture(scope="module")
def cases(oracle):
    """per lattice: host arrays, momenta and references, computed once and never modified"""
    out = {}
    for X in LATTICES:
        hot, _, _ = oracle.make_fields(list(X), seed=31, antiperiodic_t=True, clover=False)
        warm = smooth_gauge(X, 0.35)
        c = {"hot": hot, "warm": warm}
        A0 = md.random_momentum(np.random.default_rng(17), (4, X[3], X[2], X[1], X[0]))
        c["A0"] = A0
        c["mom0"] = md.mom_to_host(oracle, A0, X)
        zero = np.zeros_like(A0)
        for kind in ("hot", "warm"):
            U = ob.from_qdp(oracle, c[kind], X)
            c[kind + "_lex"] = U
            for name, (paths, coeff) in TABLES.items():
                c[kind, name, "acc"] = md.force(U, A0, paths, coeff, EB3)
                c[kind, name, "over"] = md.force(U, zero, paths, coeff, EB3)
        for name, (paths, coeff) in TABLES.items():
            rounded = md.force(ob.fp32_recon12(c["hot_lex"], True), A0, paths, coeff, EB3)
            c["fp32", name] = np.max(np.abs(rounded - c["hot", name, "acc"]))
        out[X] = c
    return out


def _load(qa, gauge, X, mask=0, prec=8, recon=18, periodic=False):
    qa.lib().qudaAmdSetPartitionMask(mask)
    gp = qa.gauge_param(X, cuda_prec=prec, recon=recon, t_boundary=qa.QUDA_PERIODIC_T if periodic else qa.QUDA_ANTI_PERIODIC_T)
    qa.load_gauge(gauge, gp)
    return gp


def _mom(oracle, host, X):
    return md.mom_from_host(oracle, host, X)


@pytest.mark.parametrize("X", LATTICES)
@pytest.mark.parametrize("mask,prec,recon", [(0, 8, 18), (0b0111, 8, 18), (0b1010, 4, 12)])
@pytest.mark.parametrize("table", sorted(TABLES))
def test_force_matches_the_reference(qa, oracle, cases, X, mask, prec, recon, table):
    """hot anti-periodic links, resident: accumulation onto a non-zero momentum, and overwrite_mom.  Mask 0 runs the direct
    gather (length-5 paths wrap the extent-2 dimension of 6x4x2x8 more than once), the other masks the transport formulation"""
    c = cases[X]
    paths, coeff = TABLES[table]
    want = c["hot", table, "acc"]
    scale = np.max(np.abs(want))
    tol = 1e-12 * scale if prec == 8 else 4.0 * c["fp32", table]
    try:
        gp = _load(qa, c["hot"], X, mask, prec, recon)
        got = _mom(oracle, qa.gauge_force(gp, paths, coeff, EB3, mom=c["mom0"]), X)
        err = np.max(np.abs(got - want))
        print("%s force, mask %d prec %d: max|delta| = %.3e, max|ref| = %.3e, rounded-link reference %.3e" % (table, mask, prec, err, scale, c["fp32", table]))
        assert err <= tol
        over = _mom(oracle, qa.gauge_force(gp, paths, coeff, EB3, overwrite=True), X)
        assert np.max(np.abs(over - c["hot", table, "over"])) <= tol
        # the packed momentum is traceless and its tenth real is 0
        raw = qa.gauge_force(gp, paths, coeff, EB3, mom=c["mom0"])
        assert np.all(raw[..., 9] == 0) and np.max(np.abs(raw[..., 6:9].sum(axis=-1))) <= 1e-14 * scale
    finally:
        qa.lib().qudaAmdSetPartitionMask(0)


@pytest.mark.parametrize("X", LATTICES)
def test_force_host_links_boundaries_and_transport(qa, oracle, cases, X):
    c = cases[X]
    for table in sorted(TABLES):
        paths, coeff = TABLES[table]
        want = c["warm", table, "acc"]
        tol = 1e-12 * np.max(np.abs(want))
        # warm links, host-gauge path, periodic; and the same links with the anti-periodic sign: closed loops give the same force
        gp = qa.gauge_param(X, t_boundary=qa.QUDA_PERIODIC_T)
        qa.lib().freeGaugeQuda()
        direct = qa.gauge_force(gp, paths, coeff, EB3, gauge=c["warm"], mom=c["mom0"])
        assert np.max(np.abs(_mom(oracle, direct, X) - want)) <= tol
        gpa = qa.gauge_param(X, t_boundary=qa.QUDA_ANTI_PERIODIC_T)
        flipped = ob.to_qdp(oracle, ob.flip_time_boundary(c["warm_lex"]), X)
        got = qa.gauge_force(gpa, paths, coeff, EB3, gauge=flipped, mom=c["mom0"])
        assert np.max(np.abs(_mom(oracle, got, X) - want)) <= tol
        # fp32 12-real links loaded from the host with the sign: the sign goes back on the rebuilt third row
        gp12 = qa.gauge_param(X, cuda_prec=4, recon=12, t_boundary=qa.QUDA_ANTI_PERIODIC_T)
        got = qa.gauge_force(gp12, paths, coeff, EB3, gauge=flipped, mom=c["mom0"])
        assert np.max(np.abs(_mom(oracle, got, X) - want)) <= 4.0 * np.max(np.abs(md.force(ob.fp32_recon12(ob.flip_time_boundary(c["warm_lex"]), True), c["A0"], paths, coeff, EB3) - want))
        # the transport formulation on one rank against the direct kernel
        os.environ["QUDA_AMD_GAUGE_FORCE_TRANSPORT"] = "1"
        try:
            transport = qa.gauge_force(gp, paths, coeff, EB3, gauge=c["warm"], mom=c["mom0"])
        finally:
            del os.environ["QUDA_AMD_GAUGE_FORCE_TRANSPORT"]
        d = np.max(np.abs(transport - direct))
        print("%s: transport vs direct max|delta| = %.3e" % (table, d))
        assert d <= tol
        assert np.max(np.abs(_mom(oracle, transport, X) - want)) <= tol
        # a zero coefficient skips its path
        c2 = list(coeff)
        c2[2] = 0.0
        p2 = [[p for i, p in enumerate(paths[mu]) if i != 2] for mu in range(4)]
        a = qa.gauge_force(gp, paths, c2, EB3, gauge=c["warm"], mom=c["mom0"])
        b = qa.gauge_force(gp, p2, coeff[:2] + coeff[3:], EB3, gauge=c["warm"], mom=c["mom0"])
        assert np.array_equal(a, b)


def test_resident_momentum_accumulates(qa, oracle, cases):
    X = LATTICES[1]
    c = cases[X]
    paths, coeff = TABLES["symanzik"]
    gp = _load(qa, c["warm"], X, periodic=True)
    qa.gauge_force(gp, paths, coeff, 0.1, mom=c["mom0"], make_resident_mom=True, return_mom=False)
    two = qa.gauge_force(gp, paths, coeff, 0.2, make_resident_mom=True)          # use_resident_mom
    one = qa.gauge_force(gp, paths, coeff, 0.1 + 0.2, mom=c["mom0"])
    scale = np.max(np.abs(one))
    assert np.max(np.abs(two - one)) <= 1e-12 * scale
    assert np.max(np.abs(_mom(oracle, one, X) - md.force(c["warm_lex"], c["A0"], paths, coeff, 0.1 + 0.2))) <= 1e-12 * scale
    # host links made resident by the force call: the plaquette sees them
    qa.lib().freeGaugeQuda()
    qa.gauge_force(qa.gauge_param(X), paths, coeff, 0.1, gauge=c["hot"], mom=c["mom0"], make_resident_gauge=True)
    assert np.max(np.abs(np.array(qa.plaquette()) - ob.plaq(c["hot_lex"]))) <= 1e-12


@pytest.mark.parametrize("X", LATTICES)
@pytest.mark.parametrize("exact", [1, 0])
@pytest.mark.parametrize("conj", [0, 1])
def test_link_update_matches_the_reference(qa, oracle, cases, X, exact, conj):
    c = cases[X]
    dt = 0.07
    gp = _load(qa, c["hot"], X)
    loaded = qa.save_gauge(qa.gauge_param(X))
    got = ob.from_qdp(oracle, qa.update_gauge(gp, dt, mom=c["mom0"], conj_mom=conj, exact=exact), X)
    want = md.update(c["hot_lex"], c["A0"], dt, bool(conj), bool(exact))
    err = np.max(np.abs(got - want))
    print("update exact=%d conj=%d: max|delta| = %.3e" % (exact, conj, err))
    assert err <= 1e-12 * np.max(np.abs(want))
    if exact:
        assert np.max(np.abs(got @ _dag(got) - np.eye(3))) <= 1e-13
        assert np.max(np.abs(np.linalg.det(ob.flip_time_boundary(got)) - 1.0)) <= 1e-13
    # host-gauge path gives the same bits as the resident fp64 links
    assert np.array_equal(qa.update_gauge(gp, dt, gauge=c["hot"], mom=c["mom0"], conj_mom=conj, exact=exact), ob.to_qdp(oracle, got, X))
    # no time, no motion
    assert np.array_equal(qa.update_gauge(gp, 0.0, mom=c["mom0"], conj_mom=conj, exact=exact), loaded)
    assert np.array_equal(qa.save_gauge(qa.gauge_param(X)), loaded)   # nothing was made resident


def test_update_makes_the_new_links_resident_and_drops_the_smeared_field(qa, oracle, cases):
    X = LATTICES[0]
    c = cases[X]
    gp = _load(qa, c["hot"], X)
    qa.stout_smear(2, 0.12, True)
    q_smeared = qa.q_charge()
    new = qa.update_gauge(gp, 0.07, mom=c["mom0"], make_resident_gauge=True)
    U = ob.from_qdp(oracle, new, X)
    assert np.array_equal(qa.save_gauge(qa.gauge_param(X)), new)
    assert np.max(np.abs(np.array(qa.plaquette()) - ob.plaq(U))) <= 1e-12
    q_ref = ob.qdensity(U)
    assert abs(qa.q_charge() - q_ref.sum()) <= 1e-12 * np.sum(np.abs(q_ref))     # the thin new links, not the old smeared field
    assert abs(qa.q_charge() - q_smeared) > 1e-6 * np.sum(np.abs(q_ref))


@pytest.mark.parametrize("X", LATTICES)
@pytest.mark.parametrize("mask", [0, 0b1010])
def test_momentum_action(qa, oracle, cases, X, mask):
    c = cases[X]
    terms = md.mom_action_terms(c["A0"])
    try:
        qa.lib().qudaAmdSetPartitionMask(mask)
        gp = qa.gauge_param(X)
        got = qa.mom_action(gp, c["mom0"])
        print("momentum action %.15e, reference %.15e, sum|terms| %.3e" % (got, terms.sum(), np.abs(terms).sum()))
        assert abs(got - terms.sum()) <= 1e-12 * np.abs(terms).sum()
        assert qa.mom_action(gp, c["mom0"]) == got
        assert qa.mom_action(gp, c["mom0"], make_resident_mom=True) == got and qa.mom_action(gp) == got
        assert qa.mom_action(gp, np.zeros_like(c["mom0"])) == -4.0 * 4 * int(np.prod(X))
    finally:
        qa.lib().qudaAmdSetPartitionMask(0)


@pytest.mark.parametrize("X", LATTICES)
def test_projection_matches_the_svd(qa, oracle, cases, X):
    c = cases[X]
    noise = np.random.default_rng(9).standard_normal(c["hot_lex"].shape + (2,))
    bent = c["hot_lex"] @ (np.eye(3) + 1e-3 * (noise[..., 0] + 1j * noise[..., 1]))
    want = ob.flip_time_boundary(md.project(ob.flip_time_boundary(bent)))       # the anti-periodic sign is not part of the SU(3) matrix
    gp = qa.gauge_param(X)
    got = ob.from_qdp(oracle, qa.project_su3(gp, 1e-13, gauge=ob.to_qdp(oracle, bent, X), make_resident_gauge=True), X)
    assert np.max(np.abs(got @ _dag(got) - np.eye(3))) <= 1e-13
    assert np.max(np.abs(np.linalg.det(ob.flip_time_boundary(got)) - 1.0)) <= 1e-13
    err = np.max(np.abs(got - want))
    print("projection: max|delta| = %.3e" % err)
    assert err <= 1e-12
    assert np.array_equal(qa.save_gauge(qa.gauge_param(X)), ob.to_qdp(oracle, got, X))
    # SU(3) links are a fixed point to rounding, resident path
    again = ob.from_qdp(oracle, qa.project_su3(gp, 1e-13), X)
    assert np.max(np.abs(again - got)) <= 1e-14


def _device_leapfrog(qa, gp, paths, coeff, beta, dt, n, mom):
    """half force, (update, force) ..., update, half force, links and momenta resident throughout"""
    eb3 = dt * beta / 3.0
    qa.gauge_force(gp, paths, coeff, 0.5 * eb3, mom=mom, make_resident_mom=True, return_mom=False)
    for step in range(n):
        qa.update_gauge(gp, dt, make_resident_gauge=True, make_resident_mom=True, return_gauge=False)
        last = step == n - 1
        out = qa.gauge_force(gp, paths, coeff, 0.5 * eb3 if last else eb3, make_resident_mom=True, return_mom=last)
    return out


def test_leapfrog_through_the_c_abi(qa, oracle):
    p = md.LEAPFROG
    X, beta = p["X"], p["beta"]
    V = int(np.prod(X))
    U0, A0 = md.leapfrog_inputs(oracle)
    paths, coeff = md.wilson_paths()
    host_links, host_mom = ob.to_qdp(oracle, U0, X), md.mom_to_host(oracle, A0, X)

    def hamiltonian(gp):
        return qa.mom_action(gp), -6.0 * beta * V * qa.plaquette()[0]

    mom_scale = np.abs(md.mom_action_terms(A0)).sum()
    dH_dev, dH_ref = [], []
    for dt in p["dt"]:
        n = int(round(p["tau"] / dt))
        gp = _load(qa, host_links, X, periodic=True)
        qa.mom_action(gp, host_mom, make_resident_mom=True)
        K0, S0 = hamiltonian(gp)
        mom1 = _device_leapfrog(qa, gp, paths, coeff, beta, dt, n, host_mom)
        K1, S1 = hamiltonian(gp)
        U1 = ob.from_qdp(oracle, qa.save_gauge(qa.gauge_param(X)), X)
        Ur, Ar = md.leapfrog(U0, A0, paths, coeff, beta, dt, n)
        eU, eA = np.max(np.abs(U1 - Ur)), np.max(np.abs(_mom(oracle, mom1, X) - Ar))
        print("dt %.3f, %d steps: links %.3e, momenta %.3e (max %.3e)" % (dt, n, eU, eA, np.max(np.abs(Ar))))
        assert eU <= n * 1e-12 * np.max(np.abs(Ur))
        assert eA <= n * 1e-12 * np.max(np.abs(Ar))
        dH_dev.append((K1 + S1) - (K0 + S0))
        dH_ref.append(md.mom_action(Ar) + md.wilson_action(Ur, beta) - md.mom_action(A0) - md.wilson_action(U0, beta))
        print("dH device %.9e, reference %.9e" % (dH_dev[-1], dH_ref[-1]))
        assert abs(dH_dev[-1] - dH_ref[-1]) <= n * 1e-12 * (abs(S0) + mom_scale)
        if dt == p["dt"][0]:
            # reversibility: the momenta negated, n steps back
            _device_leapfrog(qa, gp, paths, coeff, beta, dt, n, -mom1)
            back = ob.from_qdp(oracle, qa.save_gauge(qa.gauge_param(X)), X)
            print("reversibility: %.3e" % np.max(np.abs(back - U0)))
            assert np.max(np.abs(back - U0)) <= 2 * n * 1e-12
    assert 3.0 <= dH_dev[0] / dH_dev[1] <= 5.0


@pytest.mark.parametrize("case,message", [("force_without_resident_gauge", "No resident gauge field"),
                                          ("action_without_resident_momentum", "No resident momentum field"),
                                          ("milc_gauge_order", "only QUDA_QDP_GAUGE_ORDER"),
                                          ("path_longer_than_the_cap", "exceeds the cap of 8"),
                                          ("projection_to_zero_tolerance", "failures")])
def test_error_cases(case, message):
    """the library's error convention (message, exit status 1), each case in a child process (tools/gauge_md_error_cases.py)"""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gauge_md_error_cases.py"), case], capture_output=True, text=True, timeout=300)
    out = r.stdout + r.stderr
    assert r.returncode == 1, (r.returncode, out[-1500:])
    assert "ERROR:" in out and message in out and "NOT REACHED" not in out, out[-1500:]


def test_two_ranks_return_the_global_result(qa, oracle, tmp_path):
    """force, link update and momentum action on 4x4x4x8 split in t over two processes sharing the GPU (tools/gauge_md_ranks.sh,
    each rank under its own time limit), against the reference on the global lattice"""
    X = (4, 4, 4, 8)
    gauge, _, _ = oracle.make_fields(list(X), seed=9, antiperiodic_t=True, clover=False)
    U = ob.from_qdp(oracle, gauge, X)
    A = md.random_momentum(np.random.default_rng(23), U.shape[:-2])
    paths, coeff = md.symanzik_paths()
    eb3, dt = 0.2, 0.07
    inp = tmp_path / "inputs.npz"
    np.savez(str(inp), X=np.array(X), gauge=gauge, mom=md.mom_to_host(oracle, A, X), paths=json.dumps(paths), coeff=np.array(coeff), eb3=eb3, dt=dt,
             t_boundary=qa.QUDA_ANTI_PERIODIC_T)
    r = subprocess.run(["bash", os.path.join(ROOT, "tools", "gauge_md_ranks.sh"), str(inp), str(tmp_path)], capture_output=True, text=True, timeout=300)
    logs = "".join(open(str(tmp_path / ("rank%d.log" % k))).read()[-1500:] for k in range(2) if (tmp_path / ("rank%d.log" % k)).exists())
    assert r.returncode == 0, r.stdout + r.stderr + logs
    import multi_gpu as mg
    V = int(np.prod(X))
    force, links = np.zeros(V * 40), np.zeros((4, V * 18))
    F_ref = md.force(U, A, paths, coeff, eb3)
    U_ref = md.update(U, F_ref, dt)
    terms = md.mom_action_terms(F_ref)
    for rank in range(2):
        d = np.load(str(tmp_path / ("rank%d.npz" % rank)))
        coords = [int(v) for v in d["coords"]]
        mg.gather_field(d["force"].reshape(-1), list(X), [1, 1, 1, 2], coords, 40, force)
        for mu in range(4):
            mg.gather_field(d["links"][mu], list(X), [1, 1, 1, 2], coords, 18, links[mu])
        assert abs(float(d["action"]) - terms.sum()) <= 1e-12 * np.abs(terms).sum()
        assert np.max(np.abs(d["plaq"] - ob.plaq(U_ref))) <= 1e-12
    assert np.max(np.abs(_mom(oracle, force.reshape(V, 4, 10), X) - F_ref)) <= 1e-12 * np.max(np.abs(F_ref))
    assert np.max(np.abs(ob.from_qdp(oracle, links, X) - U_ref)) <= 1e-12 * np.max(np.abs(U_ref))
