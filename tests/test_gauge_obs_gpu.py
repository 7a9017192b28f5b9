"""Stout smearing and the topological charge on the GPU (performSTOUTnStep, qChargeCuda, qudaAmdStoutSmear, qudaAmdQCharge,
qudaAmdSu3ExpIQ) against the numpy reference tests/gauge_obs_ref.py, which evaluates exp(iQ) by eigen-decomposition and the
clover leaves by direct gathers, so it shares neither the Cayley-Hamilton form nor the transport formulation with the device.

Bounds: fp64 links 1e-12 and fp32 12-real links 2e-5 on the smeared links (the APE test's own); the exponential 1e-13 (a numpy
restatement of the device formula against eigh gave 4e-15 on this input set; the margin covers operation order and FMA
contraction); the charge 1e-12 relative to sum|q| (Q) and max|q| (q(x))."""
import importlib
import os
import subprocess
import sys

import numpy as np
import pytest

import gauge_obs_ref as ref
from synth import smooth_gauge

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LATTICES = [(4, 4, 4, 4), (6, 4, 2, 8)]


@pytest.fixture(scope="module")
def qa():
    mod = importlib.import_module("quda-qkxtm-multigrid_amd")
    mod.init(0)
    yield mod
    mod.end()


@pytest.fixture(scope="module")
def cases(oracle):
    """per lattice: the host arrays and their references, computed once and never modified"""
    out = {}
    for X in LATTICES:
        hot, _, _ = oracle.make_fields(list(X), seed=31, antiperiodic_t=True, clover=False)
        warm = smooth_gauge(X, 0.35)
        c = {"hot": hot, "warm": warm}
        for kind in ("hot", "warm"):
            U = ref.from_qdp(oracle, c[kind], X)
            c[kind + "_lex"] = U
            c[kind + "_q"] = ref.qdensity(U)
        c["hot_stout3"] = ref.stout(c["hot_lex"], 0.1, 3, 3)
        c["hot_stout4"] = ref.stout(c["hot_lex"], 0.12, 2, 4)
        c["warm_stout4"] = ref.stout(c["warm_lex"], 0.12, 2, 4)
        out[X] = c
    return out


def _dag(a):
    return np.conj(np.swapaxes(a, -1, -2))


def _load(qa, gauge, X, mask=0, prec=8, recon=18, periodic=False):
    qa.lib().qudaAmdSetPartitionMask(mask)
    gp = qa.gauge_param(X, cuda_prec=prec, recon=recon, t_boundary=qa.QUDA_PERIODIC_T if periodic else qa.QUDA_ANTI_PERIODIC_T)
    qa.load_gauge(gauge, gp)
    return gp


def _exp_inputs():
    rng = np.random.default_rng(1)
    qs = [ref.random_hermitian_traceless(rng, 32, s) for s in (1e-9, 1e-4, 1e-2, 0.3, 1.0, 3.0)]
    V = ref.random_su3(rng, (8,))
    for lam in (1e-6, 0.1, 1.0, 2.5):
        for d in ((1, 1, -2), (-1, -1, 2), (1, -1, 0)):     # c0 = +c0max and -c0max (w = 0), c0 = 0
            for split in (0.0, 1e-7):
                D = np.diag(np.array(d, dtype=np.float64) + split * np.array((1.0, -1.0, 0.0)))
                qs.append(lam * V @ D @ _dag(V))
    qs.append(np.zeros((1, 3, 3), dtype=np.complex128))
    q = np.concatenate(qs)
    return 0.5 * (q + _dag(q))


def test_exponential_matches_the_eigen_decomposition(qa):
    q = _exp_inputs()
    got = qa.su3_exp_iq(q)
    assert got.shape == q.shape
    assert not np.isnan(got).any()
    err = np.max(np.abs(got - ref.exp_eigh(q)))
    uni = np.max(np.abs(got @ _dag(got) - np.eye(3)))
    print("exp(iQ): max|delta| = %.3e, unitarity = %.3e over %d matrices" % (err, uni, len(q)))
    assert err <= 1e-13
    assert uni <= 1e-13
    assert np.array_equal(got[-1], np.eye(3))   # Q = 0: the unit matrix, exactly


@pytest.mark.parametrize("X", LATTICES)
@pytest.mark.parametrize("mask,prec,recon", [(0, 8, 18), (0b0111, 8, 18), (0b1010, 4, 12)])
def test_stout_matches_the_reference(qa, oracle, cases, X, mask, prec, recon):
    c = cases[X]
    V = int(np.prod(X))
    tol = 1e-12 if prec == 8 else 2e-5
    try:
        _load(qa, c["hot"], X, mask, prec, recon)
        loaded = ref.from_qdp(oracle, qa.save_gauge(qa.gauge_param(X)), X)
        # performSTOUTnStep: spatial links from spatial staples, time links as loaded
        qa.perform_stout(3, 0.1)
        got = ref.from_qdp(oracle, qa.save_smeared_gauge(V), X)
        err = np.max(np.abs(got - c["hot_stout3"]))
        print("stout(3, 0.1) spatial: max|delta| = %.3e" % err)
        assert err < tol
        assert np.max(np.abs(got[3] - loaded[3])) <= 1e-15
        # exp(iQ) is unitary with determinant 1, so the smeared links are as unitary as the loaded ones: to rounding in fp64
        # (fp32 12-real links are unitary to fp32 rounding only, and are compared with the reference alone)
        if prec == 8:
            assert np.max(np.abs(got @ _dag(got) - np.eye(3))) < 1e-13
            assert np.max(np.abs(np.linalg.det(ref.flip_time_boundary(got)) - 1.0)) < 1e-13
        # the smearing smooths the hot field: the spatial plaquette rises
        assert ref.plaq(got)[1] > qa.plaquette()[1]
        # all four directions, staples of all six planes: the anti-periodic time links must come back with one sign
        qa.stout_smear(2, 0.12, True)
        got = ref.from_qdp(oracle, qa.save_smeared_gauge(V), X)
        err = np.max(np.abs(got - c["hot_stout4"]))
        print("stout(2, 0.12) all directions: max|delta| = %.3e, time links %.3e" % (err, np.max(np.abs(got[3] - c["hot_stout4"][3]))))
        assert err < tol
        assert np.max(np.abs(got[3] - c["hot_stout4"][3])) < tol
        if prec == 8:
            assert np.max(np.abs(got @ _dag(got) - np.eye(3))) < 1e-13
            assert np.max(np.abs(np.linalg.det(ref.flip_time_boundary(got)) - 1.0)) < 1e-13
        # no steps, and no weight: the loaded links
        for n, rho, st in ((0, 0.1, False), (0, 0.1, True), (2, 0.0, False), (2, 0.0, True)):
            qa.stout_smear(n, rho, st)
            back = ref.from_qdp(oracle, qa.save_smeared_gauge(V), X)
            assert np.max(np.abs(back - loaded)) <= 1e-15, (n, rho, st)
    finally:
        qa.lib().qudaAmdSetPartitionMask(0)


@pytest.mark.parametrize("X", LATTICES)
def test_stout_of_the_warm_field_and_of_the_unit_gauge(qa, oracle, cases, X):
    c = cases[X]
    V = int(np.prod(X))
    _load(qa, c["warm"], X, periodic=True)
    qa.stout_smear(2, 0.12, True)
    got = ref.from_qdp(oracle, qa.save_smeared_gauge(V), X)
    assert np.max(np.abs(got - c["warm_stout4"])) < 1e-12
    unit = np.zeros((4, V, 9, 2))
    unit[:, :, [0, 4, 8], 0] = 1.0
    unit = unit.reshape(4, -1)
    _load(qa, unit, X, periodic=True)
    for st in (False, True):
        qa.stout_smear(3, 0.1, st)
        assert np.array_equal(qa.save_smeared_gauge(V), unit)
    Q, q = qa.q_charge(density=True, which=0)
    assert Q == 0.0 and np.all(q == 0.0)
    assert qa.q_charge() == 0.0   # the smeared unit gauge


def _check_charge(Q, q, q_ref):
    sum_abs, max_abs = np.sum(np.abs(q_ref)), np.max(np.abs(q_ref))
    dQ, dq = abs(Q - q_ref.sum()), np.max(np.abs(q - q_ref))
    print("charge: Q = %.15e, |dQ| = %.3e (sum|q| = %.3e), max|dq| = %.3e (max|q| = %.3e)" % (Q, dQ, sum_abs, dq, max_abs))
    assert dQ <= 1e-12 * sum_abs
    assert dq <= 1e-12 * max_abs


@pytest.mark.parametrize("X", LATTICES)
@pytest.mark.parametrize("mask", [0, 0b0111])
@pytest.mark.parametrize("kind", ["hot", "warm"])
def test_charge_matches_the_reference(qa, oracle, cases, X, mask, kind):
    c = cases[X]
    q_ref = c[kind + "_q"]
    try:
        _load(qa, c[kind], X, mask, periodic=kind == "warm")
        Q, q_lex = qa.q_charge(density=True, lexicographic=True, which=0)
        _check_charge(Q, q_lex.reshape(q_ref.shape), q_ref)
        Q2, q_eo = qa.q_charge(density=True, lexicographic=False, which=0)
        assert np.array_equal(oracle.eo_to_lex(q_eo, list(X), 1), q_lex)
        # a fixed summation order: the same bits from every call and every entry point
        assert Q2 == Q and qa.q_charge(which=0) == Q and qa.q_charge() == Q
        assert np.array_equal(qa.q_charge(density=True, lexicographic=True, which=-1)[1], q_lex)
        # gauge invariance: a random gauge transformation, loaded as a new field
        g = ref.random_su3(np.random.default_rng(5), q_ref.shape)
        Ug = ref.to_qdp(oracle, ref.gauge_transform(c[kind + "_lex"], g), X)
        _load(qa, Ug, X, mask, periodic=kind == "warm")
        Qg, qg = qa.q_charge(density=True, lexicographic=True, which=0)
        assert np.max(np.abs(qg - q_lex)) <= 1e-12 * np.max(np.abs(q_ref))
        assert abs(Qg - Q) <= 1e-12 * np.sum(np.abs(q_ref))
    finally:
        qa.lib().qudaAmdSetPartitionMask(0)


@pytest.mark.parametrize("X", LATTICES)
def test_charge_follows_the_resident_smeared_field(qa, oracle, cases, X):
    """qChargeCuda measures the smeared field if one is resident (from stout or APE), else the resident links"""
    c = cases[X]
    _load(qa, c["hot"], X)
    Q_thin = c["hot_q"].sum()
    scale = np.sum(np.abs(c["hot_q"]))
    assert abs(qa.q_charge() - Q_thin) <= 1e-12 * scale
    qa.perform_stout(3, 0.1)
    q_ref = ref.qdensity(c["hot_stout3"])
    Q, q = qa.q_charge(density=True, lexicographic=True, which=-1)
    _check_charge(Q, q.reshape(q_ref.shape), q_ref)
    assert qa.q_charge() == Q and qa.q_charge(which=1) == Q
    assert abs(qa.q_charge(which=0) - Q_thin) <= 1e-12 * scale
    qa.perform_ape(3, 0.5)
    q_ref = ref.qdensity(ref.from_qdp(oracle, oracle.ape_smear(c["hot"], list(X), 0.5, 3), X))
    Q, q = qa.q_charge(density=True, lexicographic=True, which=-1)
    _check_charge(Q, q.reshape(q_ref.shape), q_ref)
    assert qa.q_charge() == Q
    qa.lib().freeGaugeQuda()
    _load(qa, c["hot"], X)
    assert abs(qa.q_charge() - Q_thin) <= 1e-12 * scale


# max |plaquette - reference| over (total, spatial, temporal) of the hot 4^4 field, measured on the commit before the link-type
# dispatcher (forLinkType) existed, three loads each with the same figure; fp64 gave 0, 2.8e-17 and 2.8e-17 (18, 12, 8 reals)
PLAQ_DEVIATION = {(4, 18): 2.025643e-10, (4, 12): 9.265036e-10, (4, 8): 2.406853e-08,
                  (2, 18): 5.678953e-07, (2, 12): 1.874196e-07, (2, 8): 8.310244e-07}


@pytest.mark.parametrize("recon", [18, 12, 8])
@pytest.mark.parametrize("prec", [8, 4, 2])
def test_plaquette_of_every_link_type(qa, oracle, cases, prec, recon):
    """Every (precision, reconstruct) pair walks its own branch of the link-type dispatcher (through extractForwardLinks) and of the
    loader; a swapped branch reads the links in the wrong format and moves the plaquette by 0.1 or more.  Bounds: fp64 1e-12, as the
    other fp64 comparisons of this file; fp32 and 16-bit four times the measured deviation of that pair (the atomicAdd of the
    plaquette sum lets the last bits vary from run to run)"""
    X = LATTICES[0]
    c = cases[X]
    want = np.array(ref.plaq(c["hot_lex"]))
    _load(qa, c["hot"], X, prec=prec, recon=recon)
    err = np.max(np.abs(np.array(qa.plaquette()) - want))
    tol = 1e-12 if prec == 8 else 4.0 * PLAQ_DEVIATION[prec, recon]
    print("plaquette, precision %d, %d reals: max|delta| = %.6e (bound %.3e)" % (prec, recon, err, tol))
    assert err <= tol


@pytest.mark.parametrize("case,message", [("charge_of_missing_smeared_field", "no smeared field"), ("stout_without_gauge", "Gauge field must be loaded"),
                                          ("charge_without_gauge", "Gauge field must be loaded")])
def test_error_cases(case, message):
    """the library's error convention (message, exit status 1), each case in a child process (tools/gauge_obs_error_cases.py)"""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gauge_obs_error_cases.py"), case], capture_output=True, text=True, timeout=300)
    out = r.stdout + r.stderr
    assert r.returncode == 1, (r.returncode, out[-1500:])
    assert "ERROR:" in out and message in out and "NOT REACHED" not in out, out[-1500:]
