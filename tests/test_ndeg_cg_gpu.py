"""Solvers on the non-degenerate twisted-mass doublet: CG, multi-shift CG and GCR through invertQuda / invertMultiShiftQuda, against textbook fp64
CG in numpy on the host doublet operator of tests/test_ndeg_golden.py (nothing hard-coded).

Conventions of tests/test_cg_gpu.py: smooth_gauge(X, 0.35), periodic t, kappa = 0.124, mu = 0.005, source default_rng(5).random(n), tol = 1e-10,
lattices 4^3 x 8 and 6x4x2x8; host residual with the host operator <= 1.1 tol; iteration counts within 2 (even-odd) / 3 (full, multi-shift) of the
numpy reference; mixed precision capped at maxiter = 10 x the fp64 count.  epsilon = 0.2: (2 kappa epsilon)^2 = 0.0025 < 1 + (2 kappa mu)^2, so the
twist is invertible and M^dag M is positive definite (the numpy CG converges on it).  The solvers see a doublet as a parity field of twice the sites.
The measured iteration counts are printed."""
import importlib

import numpy as np
import pytest

import test_ndeg_golden as ng

pytestmark = pytest.mark.gpu

from synth import smooth_gauge  # noqa: E402

TOL, KAPPA, MU, EPS = 1e-10, 0.124, 0.005, 0.2
X0, X1 = (4, 4, 4, 8), (6, 4, 2, 8)


@pytest.fixture(scope="module")
def qa():
    mod = importlib.import_module("quda-qkxtm-multigrid_amd")
    mod.init(0)
    yield mod
    mod.end()


_gauges, _refs, _resident = {}, {}, {}


def _gauge(X):
    if X not in _gauges:
        _gauges[X] = smooth_gauge(X, 0.35)
    return _gauges[X]


def _load(qa, X, sloppy=8):
    if _resident.get("key") != (X, sloppy):
        qa.load_gauge(_gauge(X), qa.gauge_param(X, cuda_prec=8, prec_sloppy=sloppy, t_boundary=qa.QUDA_PERIODIC_T))
        _resident["key"] = (X, sloppy)


def _source(X, pc):
    n = 2 * int(np.prod(X)) * 24 // (2 if pc else 1)
    return np.random.default_rng(5).random(n)


def _operator(oracle, X, pc, matpc="ee"):
    """A(v, dagger): the host doublet operator, periodic t as the gauge field is loaded"""
    g = _gauge(X)
    if pc:
        return lambda v, dag: ng.ndeg_matpc(oracle, g, v, X, KAPPA, MU, EPS, matpc, dag)
    return lambda v, dag: ng.ndeg_mat(oracle, g, v, X, KAPPA, MU, EPS, dag)


def _normal(A, shift=0.0):
    return lambda v: A(A(v, 0), 1) + shift * v


def _numpy_cg(N, b, tol, maxiter=5000):
    x, r = np.zeros_like(b), b.copy()
    p, r2, k = r.copy(), float(b @ b), 0
    stop = tol * tol * r2
    while r2 > stop and k < maxiter:
        Ap = N(p)
        alpha = r2 / float(p @ Ap)
        x += alpha * p
        r -= alpha * Ap
        r2_new = float(r @ r)
        p = r + (r2_new / r2) * p
        r2 = r2_new
        k += 1
    return x, k, float(np.linalg.norm(b - N(x)) / np.linalg.norm(b))


def _reference(oracle, X, pc, matpc="ee", shift=0.0):
    key = (X, pc, matpc, shift)
    if key not in _refs:
        _, k, res = _numpy_cg(_normal(_operator(oracle, X, pc, matpc), shift), _source(X, pc), TOL)
        print("numpy CG doublet %s %s shift %g: %d iterations, true residual %.3e" % (X, "even-odd " + matpc if pc else "full", shift, k, res))
        _refs[key] = (k, res)
    return _refs[key]


def _res(N, x, b):
    return float(np.linalg.norm(b - N(x)) / np.linalg.norm(b))


def _param(qa, pc, solution, matpc="ee", sloppy=8, maxiter=2000, delta=1e-4):
    ip = qa.invert_param(qa.QUDA_TWISTED_MASS_DSLASH, KAPPA, MU, qa.QUDA_TWIST_NONDEG_DOUBLET, matpc, 0, cuda_prec=8, prec_sloppy=sloppy,
                         solution_type=solution, epsilon=EPS)
    ip.solve_type = qa.QUDA_NORMOP_PC_SOLVE if pc else qa.QUDA_NORMOP_SOLVE
    ip.inv_type, ip.tol, ip.maxiter, ip.reliable_delta = qa.QUDA_CG_INVERTER, TOL, maxiter, delta
    return ip


@pytest.mark.parametrize("X,matpc", [(X0, "ee"), (X0, "ooasym"), (X1, "ee")])
def test_cg_even_odd(qa, oracle, X, matpc):
    _load(qa, X)
    b = _source(X, True)
    ref_iter, _ = _reference(oracle, X, True, matpc)
    ip = _param(qa, True, qa.QUDA_MATPCDAG_MATPC_SOLUTION, matpc)
    x = qa.invert(b, ip)
    res = _res(_normal(_operator(oracle, X, True, matpc)), x, b)
    print("doublet CG even-odd %s %s: %d iterations (numpy %d), host residual %.3e, reported %.3e, %.1f Gflop/s" % (X, matpc, ip.iter, ref_iter, res, ip.true_res, ip.gflops / max(ip.secs, 1e-9)))
    assert res <= 1.1 * TOL
    assert abs(ip.iter - ref_iter) <= 2
    assert ip.gflops > 0


@pytest.mark.parametrize("fused", [1, 0], ids=["fused", "composed"])
def test_cg_full_operator(qa, oracle, fused):
    X = X0
    _load(qa, X)
    b = _source(X, False)
    ref_iter, _ = _reference(oracle, X, False)
    ip = _param(qa, False, qa.QUDA_MATDAG_MAT_SOLUTION)
    qa.lib().qudaAmdSetDslashTune(b"ndeg_fused", fused)
    try:
        x = qa.invert(b, ip)
    finally:
        qa.lib().qudaAmdSetDslashTune(b"ndeg_fused", -1)
    res = _res(_normal(_operator(oracle, X, False)), x, b)
    print("doublet CG full %s: %d iterations (numpy %d), host residual %.3e" % (X, ip.iter, ref_iter, res))
    assert res <= 1.1 * TOL
    assert abs(ip.iter - ref_iter) <= 3


@pytest.mark.parametrize("pc", [False, True], ids=["NORMOP", "NORMOP_PC-prepare-reconstruct"])
def test_mat_solution_through_the_normal_equations(qa, oracle, pc):
    """a full MAT solution: from QUDA_NORMOP_SOLVE the normal-equation residual is checked on the host; from QUDA_NORMOP_PC_SOLVE the system goes
    through prepare / reconstruct, the solver's own true residual of the even-odd normal equations is the checked quantity (as tests/test_cg_gpu.py)
    and the full system's residual is bounded by that tolerance times the condition of the reconstruction, printed"""
    X = X0
    _load(qa, X)
    b = _source(X, False)
    A = _operator(oracle, X, False)
    ip = _param(qa, pc, qa.QUDA_MAT_SOLUTION)
    x = qa.invert(b, ip)
    full = _res(lambda v: A(v, 0), x, b)
    print("doublet CG MAT solution, %s: %d iterations, reported %.3e, |b - M x| / |b| = %.3e" % ("NORMOP_PC" if pc else "NORMOP", ip.iter, ip.true_res, full))
    if pc:
        assert ip.true_res <= 1.1 * TOL
        assert full < 1e-7   # a wrong prepare / reconstruct leaves an O(1) residual
    else:
        Adb = A(b, 1)
        assert float(np.linalg.norm(Adb - A(A(x, 0), 1)) / np.linalg.norm(Adb)) <= 1.1 * TOL


@pytest.mark.parametrize("sloppy,delta", [(8, 1e-4), (2, 0.1)], ids=["fp64", "16-bit-sloppy"])
@pytest.mark.parametrize("X", [X0, X1])
def test_multi_shift(qa, oracle, X, sloppy, delta):
    offsets, tols = [0.0, 0.01, 0.1, 1.0], [TOL] * 4
    ref_iter, _ = _reference(oracle, X, True)
    _load(qa, X, sloppy)
    b = _source(X, True)
    ip = _param(qa, True, qa.QUDA_MATPCDAG_MATPC_SOLUTION, sloppy=sloppy, maxiter=2000 if sloppy == 8 else 10 * ref_iter, delta=delta)
    xs = qa.invert_multi_shift(b, ip, offsets, tols)
    A = _operator(oracle, X, True)
    print("doublet multi-shift %s sloppy %d: %d iterations (numpy CG on offset 0: %d)" % (X, sloppy, ip.iter, ref_iter))
    for i, s in enumerate(offsets):
        res = _res(_normal(A, s), xs[i], b)
        print("  offset %-6g host residual %.3e, reported true %.3e" % (s, res, ip.true_res_offset[i]))
        assert res <= 1.1 * TOL, (i, s, res)
    if sloppy == 8:
        assert abs(ip.iter - ref_iter) <= 3


def test_gcr_direct_pc(qa, oracle):
    X = X0
    _load(qa, X)
    b = _source(X, True)
    ip = _param(qa, True, qa.QUDA_MATPC_SOLUTION)
    ip.solve_type, ip.inv_type, ip.gcrNkrylov = qa.QUDA_DIRECT_PC_SOLVE, qa.QUDA_GCR_INVERTER, 20
    x = qa.invert(b, ip)
    A = _operator(oracle, X, True)
    res = _res(lambda v: A(v, 0), x, b)
    print("doublet GCR DIRECT_PC %s: %d iterations, host residual %.3e, reported %.3e" % (X, ip.iter, res, ip.true_res))
    assert res <= 1.1 * TOL


def test_partitioned_directions_change_nothing(qa, oracle):
    """y and t through the ghost-zone path (self-neighbour emulation): the same iteration count, solutions equal to 1e-12"""
    X = X0
    _load(qa, X)
    b = _source(X, True)
    out = {}
    for mask in (0, 0b1010):
        qa.lib().qudaAmdSetPartitionMask(mask)
        try:
            ip = _param(qa, True, qa.QUDA_MATPCDAG_MATPC_SOLUTION)
            x = qa.invert(b, ip)
        finally:
            qa.lib().qudaAmdSetPartitionMask(0)
        out[mask] = (ip.iter, x)
    print("doublet CG: mask 0 %d iterations, mask 0b1010 %d" % (out[0][0], out[0b1010][0]))
    assert out[0][0] == out[0b1010][0]
    assert np.linalg.norm(out[0][1] - out[0b1010][1]) <= 1e-12 * np.linalg.norm(out[0][1])
