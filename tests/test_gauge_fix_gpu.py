"""Gauge fixing by overrelaxation on the GPU (computeGaugeFixingOVRQuda, qudaAmdGaugeFixOVR, qudaAmdGaugeFixQuality) against the numpy
reference tests/gauge_fix_ref.py, which sweeps whole-lattice arrays under a parity mask with np.roll neighbours and projects by SVD,
so it shares neither the lane map, the shuffles, the transport formulation nor the polar iteration with the device.

Bounds.  Links and G: 1e-12 x max|U| (the bound of the project's fp64 gauge kernels); F: 1e-12; theta: 1e-9 relative.  On the CPU
prototype a 2e-16 relative perturbation of the input moved the links by at most 1.0e-14 after 10 iterations and by 1.2e-13 through a
1692-iteration run to convergence: the sweeps do not amplify round-off.  Unitarity of the result: 1e-13.

Lattices: 4^4; 6x4x2x8 (an extent of 2: x + mu and x - mu are the same site); 6x2x2x6 (Vh = 72: one full wave of sites and a partial
one, and with eight lanes a site a partial block: the smallest shape on which a lane that left before the shuffles would show)."""
import importlib
import os
import subprocess
import sys

import numpy as np
import pytest

import gauge_fix_ref as gf
import gauge_md_ref as md
import gauge_obs_ref as ob
from synth import smooth_gauge

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LATTICES = [(4, 4, 4, 4), (6, 4, 2, 8), (6, 2, 2, 6)]
OMEGA = 1.5
EYE = np.eye(3)


@pytest.fixture(scope="module")
def qa():
    mod = importlib.import_module("quda-qkxtm-multigrid_amd")
    mod.init(0)
    yield mod
    mod.end()


def _dag(a):
    return np.conj(np.swapaxes(a, -1, -2))


def _g_lex(oracle, G, X):
    lex = oracle.eo_to_lex(np.ascontiguousarray(G, dtype=np.float64).reshape(-1), [int(v) for v in X], 18).reshape(X[3], X[2], X[1], X[0], 3, 3, 2)
    return lex[..., 0] + 1j * lex[..., 1]


@pytest.fixture(scope="module")
def cases(oracle):
    """per lattice: host arrays and the references of the ten-iteration runs, computed once and never modified.  hot: anti-periodic;
    warm: periodic, smooth links behind a random gauge transformation"""
    out = {}
    for X in LATTICES:
        hot, _, _ = oracle.make_fields(list(X), seed=31, antiperiodic_t=True, clover=False)
        c = {"hot": hot, "hot_lex": ob.from_qdp(oracle, hot, X)}
        smooth = ob.from_qdp(oracle, smooth_gauge(X, 0.35), X)
        c["warm_lex"] = ob.gauge_transform(smooth, ob.random_su3(np.random.default_rng(41), smooth.shape[1:5]))
        c["warm"] = ob.to_qdp(oracle, c["warm_lex"], X)
        for kind in ("hot", "warm"):
            for D in (4, 3):
                c[kind, D] = gf.fix(c[kind + "_lex"], D, OMEGA, 0.0, 10, 4, 1, transform=True, antiperiodic=kind == "hot")
        out[X] = c
    return out


def _gp(qa, X, kind, **kw):
    return qa.gauge_param(X, t_boundary=qa.QUDA_ANTI_PERIODIC_T if kind == "hot" else qa.QUDA_PERIODIC_T, **kw)


def _check(oracle, X, got, want, label):
    """device (links, G, info) against the reference's (U, G, (iterations, F, theta, delta))"""
    links, G, info = got
    U, Gr, (it, F, theta, _) = want
    eU = np.max(np.abs(ob.from_qdp(oracle, links, X) - U))
    eG = np.max(np.abs(_g_lex(oracle, G, X) - Gr)) if G is not None else 0.0
    print("%s: links %.3e, G %.3e, F %.15e (ref %.15e), theta %.9e (ref %.9e), %d iterations" % (label, eU, eG, info["F"], F, info["theta"], theta, info["iterations"]))
    assert info["iterations"] == it
    assert eU <= 1e-12 * np.max(np.abs(U))
    assert eG <= 1e-12
    assert abs(info["F"] - F) <= 1e-12
    assert abs(info["theta"] - theta) <= 1e-9 * theta


def _run(qa, X, kind, D, host, **kw):
    return qa.gauge_fix_ovr(_gp(qa, X, kind), 3 if D == 3 else 4, 10, OMEGA, 0.0, 4, 1, gauge=host, transform=True, **kw)


@pytest.mark.parametrize("X", LATTICES)
def test_ten_iterations_match_the_reference_element_wise(qa, oracle, cases, X):
    """the direct sweep; reunit_interval 4: the projection inside the loop (iterations 4 and 8) and the final one both run"""
    c = cases[X]
    qa.lib().qudaAmdSetPartitionMask(0)
    for kind in ("hot", "warm"):
        for D in (4, 3):
            _check(oracle, X, _run(qa, X, kind, D, c[kind]), c[kind, D], "direct %s D=%d" % (kind, D))


@pytest.mark.parametrize("X", LATTICES)
@pytest.mark.parametrize("mode", ["env", 0b0111, 0b1010])
def test_transport_matches_the_reference_and_the_direct_sweep(qa, oracle, cases, X, mode):
    """the transport formulation, forced on one rank by the environment variable or chosen by a partition mask"""
    c = cases[X]
    for kind in ("hot", "warm"):
        for D in (4, 3):
            qa.lib().qudaAmdSetPartitionMask(0)
            direct = _run(qa, X, kind, D, c[kind])
            try:
                if mode == "env":
                    os.environ["QUDA_AMD_GAUGE_FIX_TRANSPORT"] = "1"
                else:
                    qa.lib().qudaAmdSetPartitionMask(mode)
                got = _run(qa, X, kind, D, c[kind])
            finally:
                os.environ.pop("QUDA_AMD_GAUGE_FIX_TRANSPORT", None)
                qa.lib().qudaAmdSetPartitionMask(0)
            _check(oracle, X, got, c[kind, D], "transport(%s) %s D=%d" % (mode, kind, D))
            d = max(np.max(np.abs(got[0] - direct[0])), np.max(np.abs(got[1] - direct[1])))
            print("transport vs direct: %.3e" % d)
            assert d <= 1e-12
            assert abs(got[2]["F"] - direct[2]["F"]) <= 1e-12 and abs(got[2]["theta"] - direct[2]["theta"]) <= 1e-9 * direct[2]["theta"]


@pytest.fixture(scope="module")
def converged(cases):
    """the reference runs to tolerance 1e-10 on the warm fields, with their history"""
    out = {}
    for X in LATTICES[:2]:
        for D in (4, 3):
            for stop_theta in (1, 0):
                hist = []
                out[X, D, stop_theta] = gf.fix(cases[X]["warm_lex"], D, OMEGA, 1e-10, 400, 4, stop_theta, history=hist) + (hist,)
    return out


@pytest.mark.parametrize("X", LATTICES[:2])
@pytest.mark.parametrize("D", [4, 3])
@pytest.mark.parametrize("stop_theta", [1, 0])
def test_convergence_and_stopping(qa, oracle, cases, converged, X, D, stop_theta):
    tol = 1e-10
    c = cases[X]
    U, _, (it, F, theta, delta), hist = converged[X, D, stop_theta]
    # the reference alone: it stops before 400, and the figure it stops on is not within 1 % of the tolerance at the stopping
    # iteration or the one before, so that rounding cannot move the stop
    k = 1 if stop_theta else 2
    assert it < 400
    assert hist[it - 1][k] < 0.99 * tol and hist[it - 2][k] > 1.01 * tol, (hist[it - 2], hist[it - 1])
    qa.lib().qudaAmdSetPartitionMask(0)
    gp = _gp(qa, X, "warm")
    links, _, info = qa.gauge_fix_ovr(gp, 3 if D == 3 else 4, 400, OMEGA, tol, 4, stop_theta, gauge=c["warm"], make_resident_gauge=True)
    got = ob.from_qdp(oracle, links, X)
    print("D=%d stop_theta=%d: %d iterations (ref %d), F %.15e, theta %.6e (ref %.6e), delta %.3e (ref %.3e), links %.3e"
          % (D, stop_theta, info["iterations"], it, info["F"], info["theta"], theta, info["delta"], delta, np.max(np.abs(got - U))))
    assert info["iterations"] == it
    assert abs(info["F"] - F) <= 1e-12 and abs(info["theta"] - theta) <= 1e-9 * theta
    if stop_theta:
        assert info["theta"] < tol
    else:
        assert info["delta"] < tol
    Fq, thq = qa.gauge_fix_quality(3 if D == 3 else 4)   # of the fixed, projected links, now resident
    Fr, thr = gf.quality(U, D)
    assert abs(Fq - Fr) <= 1e-12 and abs(thq - thr) <= 1e-9 * thr
    assert qa.gauge_fix_quality(3 if D == 3 else 4) == (Fq, thq)   # a fixed summation order: the same bits
    assert np.max(np.abs(got - U)) <= 1e-12
    assert np.max(np.abs(ob.plaq(got) - ob.plaq(c["warm_lex"]))) <= 1e-12
    assert np.max(np.abs(got @ _dag(got) - EYE)) <= 1e-13


def test_residency(qa, oracle, cases):
    X = LATTICES[1]
    c = cases[X]
    want = c["hot", 4]
    qa.lib().qudaAmdSetPartitionMask(0)
    gp = _gp(qa, X, "hot")
    qa.load_gauge(c["hot"], gp)
    loaded = qa.save_gauge(qa.gauge_param(X))
    # resident links in, nothing made resident: the same result as from host links, and the resident links untouched
    res = qa.gauge_fix_ovr(gp, 4, 10, OMEGA, 0.0, 4, 1, transform=True)
    host = _run(qa, X, "hot", 4, c["hot"])
    _check(oracle, X, res, want, "resident")
    assert np.array_equal(res[0], host[0]) and np.array_equal(res[1], host[1])
    assert np.array_equal(qa.save_gauge(qa.gauge_param(X)), loaded)
    # a smeared field is dropped when the fixed links become resident; the plaquette does not change, saveGaugeQuda returns them
    plaq0 = np.array(qa.plaquette())
    qa.stout_smear(2, 0.12, True)
    q_smeared = qa.q_charge()
    fixed, _, _ = qa.gauge_fix_ovr(gp, 4, 10, OMEGA, 0.0, 4, 1, make_resident_gauge=True)
    assert np.array_equal(fixed, res[0])
    assert np.array_equal(qa.save_gauge(qa.gauge_param(X)), fixed)
    assert np.max(np.abs(np.array(qa.plaquette()) - plaq0)) <= 1e-12
    assert np.max(np.abs(np.array(qa.plaquette()) - ob.plaq(want[0]))) <= 1e-12
    q_ref = ob.qdensity(want[0])
    assert abs(qa.q_charge() - q_ref.sum()) <= 1e-12 * np.sum(np.abs(q_ref))     # the thin fixed links, not the old smeared field
    assert abs(qa.q_charge() - q_smeared) > 1e-6 * np.sum(np.abs(q_ref))
    # the plain entry point of quda.h: the same links, timeinfo filled
    out = np.array(c["hot"], dtype=np.float64).reshape(4, -1).copy()
    q = qa._md_param(gp, return_result_gauge=True)
    import ctypes as C
    secs = (C.c_double * 3)(-1, -1, -1)
    assert qa.lib().computeGaugeFixingOVRQuda(qa._qdp_ptrs(out), 4, 10, 0, OMEGA, 0.0, 4, 1, C.byref(q), secs) == 0
    assert np.array_equal(out, res[0]) and min(secs) >= 0


@pytest.mark.parametrize("X", LATTICES[:2])
def test_fp32_recon12_resident_links_as_input(qa, oracle, cases, X):
    """arithmetic is fp64 on the links as the resident field holds them.  Those links are fp32_recon12 of the host links: rows 0 and 1
    bit for bit, row 2 up to the rounding of its fp32 reconstruction, where the device's fused multiply-adds and numpy's complex64
    products differ in the last bits (measured 2.5e-7 in the fixed links when the reference started from numpy's row 2).  The
    reference therefore starts from the links saveGaugeQuda returns for that field, which are checked against fp32_recon12 first"""
    c = cases[X]
    qa.lib().qudaAmdSetPartitionMask(0)
    gp = _gp(qa, X, "hot", cuda_prec=4, recon=12)
    qa.load_gauge(c["hot"], gp)
    held = ob.from_qdp(oracle, qa.save_gauge(_gp(qa, X, "hot")), X)
    restated = ob.fp32_recon12(c["hot_lex"], True)
    assert np.array_equal(held[..., :2, :], restated[..., :2, :])
    assert np.max(np.abs(held[..., 2, :] - restated[..., 2, :])) <= 8 * 2.0 ** -24   # a sum of four fp32 products of magnitude <= 1
    got = qa.gauge_fix_ovr(gp, 4, 10, OMEGA, 0.0, 4, 1, transform=True)
    want = gf.fix(held, 4, OMEGA, 0.0, 10, 4, 1, transform=True, antiperiodic=True)
    _check(oracle, X, got, want, "fp32 recon-12")


@pytest.mark.parametrize("case,message", [("reunit_interval_zero", "reunit_interval = 0"),
                                          ("without_resident_gauge", "No resident gauge field"),
                                          ("milc_gauge_order", "only QUDA_QDP_GAUGE_ORDER"),
                                          ("singular_input_link", "Error in the unitarization")])
def test_error_cases(case, message):
    """the library's error convention (message, exit status 1), each case in a child process (tools/gauge_fix_error_cases.py)"""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gauge_fix_error_cases.py"), case], capture_output=True, text=True, timeout=300)
    out = r.stdout + r.stderr
    assert r.returncode == 1, (r.returncode, out[-1500:])
    assert "ERROR:" in out and message in out and "NOT REACHED" not in out, out[-1500:]


def test_two_ranks_return_the_global_result(qa, oracle, tmp_path):
    """4x4x4x8 split in t over two processes sharing the GPU (tools/gauge_fix_ranks.sh, each rank under its own time limit),
    anti-periodic, so the sign sits on one rank only: ten iterations with the transformation against the global reference"""
    X = (4, 4, 4, 8)
    gauge, _, _ = oracle.make_fields(list(X), seed=9, antiperiodic_t=True, clover=False)
    U, G, (it, F, theta, _) = gf.fix(ob.from_qdp(oracle, gauge, X), 4, OMEGA, 0.0, 10, 4, 1, transform=True, antiperiodic=True)
    inp = tmp_path / "inputs.npz"
    np.savez(str(inp), X=np.array(X), gauge=gauge, gauge_dir=4, n_steps=10, omega=OMEGA, tolerance=0.0, reunit_interval=4, stop_theta=1,
             t_boundary=qa.QUDA_ANTI_PERIODIC_T)
    r = subprocess.run(["bash", os.path.join(ROOT, "tools", "gauge_fix_ranks.sh"), str(inp), str(tmp_path)], capture_output=True, text=True, timeout=300)
    logs = "".join(open(str(tmp_path / ("rank%d.log" % k))).read()[-1500:] for k in range(2) if (tmp_path / ("rank%d.log" % k)).exists())
    assert r.returncode == 0, r.stdout + r.stderr + logs
    import multi_gpu as mg
    V = int(np.prod(X))
    links, Gdev, infos = np.zeros((4, V * 18)), np.zeros(V * 18), []
    for rank in range(2):
        d = np.load(str(tmp_path / ("rank%d.npz" % rank)))
        coords = [int(v) for v in d["coords"]]
        for mu in range(4):
            mg.gather_field(d["links"][mu], list(X), [1, 1, 1, 2], coords, 18, links[mu])
        mg.gather_field(d["G"].reshape(-1), list(X), [1, 1, 1, 2], coords, 18, Gdev)
        infos.append((d["info"], d["quality"]))
    assert np.array_equal(infos[0][0], infos[1][0]) and np.array_equal(infos[0][1], infos[1][1])   # identical on both ranks
    info, quality = infos[0]
    assert int(info[0]) == it and abs(info[1] - F) <= 1e-12 and abs(info[2] - theta) <= 1e-9 * theta
    Fr, thr = gf.quality(ob.flip_time_boundary(U), 4)
    assert abs(quality[0] - Fr) <= 1e-12 and abs(quality[1] - thr) <= 1e-9 * thr
    assert np.max(np.abs(ob.from_qdp(oracle, links, X) - U)) <= 1e-12 * np.max(np.abs(U))
    assert np.max(np.abs(_g_lex(oracle, Gdev, X) - G)) <= 1e-12
