"""CG and multi-shift CG through invertQuda / invertMultiShiftQuda (csrc/inv_cg.cpp, csrc/solve_interface.cpp) against textbook fp64 CG in
numpy on the oracle's operators, computed here (nothing hard-coded).

Inputs: synth.smooth_gauge(X, 0.35), periodic t, twisted mass kappa = 0.124, mu = 0.005, flavour +, source default_rng(5).random(n),
tol = 1e-10; lattices 4^3 x 8 and 6x4x2x8.

Bounds:
  * every solution's residual is recomputed on the HOST with the oracle's operator and must be <= 1.1 tol: CG stops on the iterated
    residual, whose drift from the true one over ~140 fp64 iterations is ~1e-13, and the numpy reference's own true residual comes as
    close as 0.6 % to the tolerance;
  * iteration counts within 2 (even-odd) / 3 (full operator, multi-shift) of the numpy reference: the residual falls by a factor 0.6 / 0.83
    per iteration near the end, so rounding cannot move the crossing of the tolerance further;
  * the reported true residuals within 1 % + 1e-12 of the host values;
  * mixed precision: maxiter = 10 x the fp64 reference count — a condition that makes stagnation fail, not an expected value.
The measured iteration counts are printed (DESIGN.md "CG and multi-shift CG" quotes them)."""
import importlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from synth import smooth_gauge  # noqa: E402

TOL, KAPPA, MU = 1e-10, 0.124, 0.005
X0, X1 = (4, 4, 4, 8), (6, 4, 2, 8)
CSW_COEFF = KAPPA * 1.57551   # as tests/test_mg_tmc_gpu.py


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
    """one gauge load per lattice and precision set"""
    if _resident.get("key") != (X, sloppy):
        qa.load_gauge(_gauge(X), qa.gauge_param(X, cuda_prec=8, prec_sloppy=sloppy, t_boundary=qa.QUDA_PERIODIC_T))
        _resident["key"] = (X, sloppy)


def _source(X, pc):
    n = int(np.prod(X)) * 24 // (2 if pc else 1)
    return np.random.default_rng(5).random(n)


def _operator(oracle, X, pc, matpc="ee", clover=None):
    """A(v, dagger) of the oracle: tm_matpc / tm_mat, or tmc_matpc with clover = (clover, inverse)"""
    g, L = _gauge(X), list(X)
    if clover is not None:
        return lambda v, dag: oracle.tmc_matpc(g, v, clover[0], clover[1], L, KAPPA, MU, +1, matpc, dag)
    if pc:
        return lambda v, dag: oracle.tm_matpc(g, v, L, KAPPA, MU, +1, matpc, dag)
    return lambda v, dag: oracle.tm_mat(g, v, L, KAPPA, MU, +1, dag)


def _normal(A, shift=0.0):
    return lambda v: A(A(v, 0), 1) + shift * v


def _numpy_cg(N, b, tol, maxiter=5000):
    """textbook CG in fp64: (x, iterations, true relative residual)"""
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


def _reference(oracle, X, pc, matpc="ee", shift=0.0, tol=TOL):
    """the numpy reference of one system, computed once and shared"""
    key = (X, pc, matpc, shift, tol)
    if key not in _refs:
        _, k, res = _numpy_cg(_normal(_operator(oracle, X, pc, matpc), shift), _source(X, pc), tol)
        print("numpy CG %s %s %s shift %g tol %g: %d iterations, true residual %.3e" % (X, "even-odd " + matpc if pc else "full", "", shift, tol, k, res))
        _refs[key] = (k, res)
    return _refs[key]


def _res(N, x, b):
    return float(np.linalg.norm(b - N(x)) / np.linalg.norm(b))


def _cg_param(qa, pc, solution, matpc="ee", sloppy=8, dslash=None, maxiter=2000, delta=1e-4):
    ip = qa.invert_param(qa.QUDA_TWISTED_MASS_DSLASH if dslash is None else dslash, KAPPA, MU, +1, matpc, 0, cuda_prec=8, prec_sloppy=sloppy,
                         solution_type=solution)
    ip.solve_type = qa.QUDA_NORMOP_PC_SOLVE if pc else qa.QUDA_NORMOP_SOLVE
    ip.inv_type, ip.tol, ip.maxiter, ip.reliable_delta = qa.QUDA_CG_INVERTER, TOL, maxiter, delta
    return ip


# ---- 1. fp64 CG ----
@pytest.mark.parametrize("X,matpc", [(X0, "ee"), (X0, "oo"), (X0, "eeasym"), (X0, "ooasym"), (X1, "ee")])
def test_cg_fp64_even_odd(qa, oracle, X, matpc):
    _load(qa, X)
    b = _source(X, True)
    ref_iter, _ = _reference(oracle, X, True, matpc)
    ip = _cg_param(qa, True, qa.QUDA_MATPCDAG_MATPC_SOLUTION, matpc)
    x = qa.invert(b, ip)
    res = _res(_normal(_operator(oracle, X, True, matpc)), x, b)
    print("CG fp64 even-odd %s %s: %d iterations (numpy %d), host residual %.3e, reported %.3e" % (X, matpc, ip.iter, ref_iter, res, ip.true_res))
    assert res <= 1.1 * TOL
    assert abs(ip.iter - ref_iter) <= 2
    assert abs(ip.true_res - res) <= 0.01 * res + 1e-12


@pytest.mark.parametrize("X", [X0, X1])
def test_cg_fp64_full_operator(qa, oracle, X):
    _load(qa, X)
    b = _source(X, False)
    ref_iter, _ = _reference(oracle, X, False)
    ip = _cg_param(qa, False, qa.QUDA_MATDAG_MAT_SOLUTION)
    x = qa.invert(b, ip)
    res = _res(_normal(_operator(oracle, X, False)), x, b)
    print("CG fp64 full %s: %d iterations (numpy %d), host residual %.3e, reported %.3e" % (X, ip.iter, ref_iter, res, ip.true_res))
    assert res <= 1.1 * TOL
    assert abs(ip.iter - ref_iter) <= 3
    assert abs(ip.true_res - res) <= 0.01 * res + 1e-12


# ---- 2. MAT / MATPC solutions through the normal equations ----
@pytest.mark.parametrize("pc", [False, True], ids=["MAT-NORMOP", "MATPC-NORMOP_PC"])
def test_mat_solutions_through_the_normal_equations(qa, oracle, pc):
    X = X0
    _load(qa, X)
    b = _source(X, pc)
    A = _operator(oracle, X, pc)
    ip = _cg_param(qa, pc, qa.QUDA_MATPC_SOLUTION if pc else qa.QUDA_MAT_SOLUTION)
    x = qa.invert(b, ip)
    Adb = A(b, 1)
    res_normal = float(np.linalg.norm(Adb - A(A(x, 0), 1)) / np.linalg.norm(Adb))
    print("CG %s: %d iterations, |A^dag b - A^dag A x| / |A^dag b| = %.3e, |b - A x| / |b| = %.3e" % ("MATPC" if pc else "MAT", ip.iter, res_normal, _res(lambda v: A(v, 0), x, b)))
    assert res_normal <= 1.1 * TOL


def test_mat_solution_through_the_even_odd_normal_equations(qa, oracle):
    """a full MAT solution from QUDA_NORMOP_PC_SOLVE: prepare / reconstruct around the even-odd normal equations; the solver's own true
    residual of that system is the checked quantity, the residual of the full system is printed"""
    X = X0
    _load(qa, X)
    b = _source(X, False)
    ip = _cg_param(qa, True, qa.QUDA_MAT_SOLUTION)
    x = qa.invert(b, ip)
    A = _operator(oracle, X, False)
    print("CG MAT solution, NORMOP_PC solve: %d iterations, reported normal-equation residual %.3e, |b - M x| / |b| = %.3e" % (ip.iter, ip.true_res, _res(lambda v: A(v, 0), x, b)))
    assert ip.true_res <= 1.1 * TOL


# ---- 3. twisted clover ----
def test_cg_twisted_clover(qa, oracle):
    X, matpc = X0, "ee"
    _load(qa, X)
    ip = _cg_param(qa, True, qa.QUDA_MATPCDAG_MATPC_SOLUTION, matpc, dslash=qa.QUDA_TWISTED_CLOVER_DSLASH)
    ip.clover_coeff = CSW_COEFF
    qa.load_clover(None, None, ip)   # built on the device from the resident links, as the QKXTM drivers do
    clover = oracle.clover_compute(_gauge(X), CSW_COEFF, list(X))
    cinv = oracle.clover_twisted_inverse(clover, 4 * KAPPA * KAPPA * MU * MU)
    N = _normal(_operator(oracle, X, True, matpc, clover=(clover, cinv)))
    b = _source(X, True)
    _, ref_iter, ref_res = _numpy_cg(N, b, TOL)
    x = qa.invert(b, ip)
    res = _res(N, x, b)
    print("CG fp64 twisted clover %s: %d iterations (numpy %d, its residual %.3e), host residual %.3e, reported %.3e" % (X, ip.iter, ref_iter, ref_res, res, ip.true_res))
    assert res <= 1.1 * TOL
    assert abs(ip.iter - ref_iter) <= 2
    assert abs(ip.true_res - res) <= 0.01 * res + 1e-12


# ---- 4. mixed precision ----
MIXED = [(4, 1e-4), (2, 0.1)]   # (sloppy precision, reliable_delta): fp32 with the binding's default, 16-bit


@pytest.mark.parametrize("sloppy,delta", MIXED, ids=["fp32", "16-bit"])
@pytest.mark.parametrize("X", [X0, X1])
def test_cg_mixed_precision(qa, oracle, X, sloppy, delta):
    ref_iter, _ = _reference(oracle, X, True)
    _load(qa, X, sloppy)
    b = _source(X, True)
    ip = _cg_param(qa, True, qa.QUDA_MATPCDAG_MATPC_SOLUTION, sloppy=sloppy, maxiter=10 * ref_iter, delta=delta)
    x = qa.invert(b, ip)
    res = _res(_normal(_operator(oracle, X, True)), x, b)
    print("CG fp64 / sloppy %d, delta %g, %s: %d iterations (fp64 numpy %d), host residual %.3e, reported %.3e" % (sloppy, delta, X, ip.iter, ref_iter, res, ip.true_res))
    assert res <= 1.1 * TOL


# ---- 5. multi-shift ----
def _check_multi_shift(qa, oracle, X, pc, offsets, tols, sloppy=8, delta=1e-4, count=True):
    ref_iter, _ = _reference(oracle, X, pc, shift=float(offsets[0]), tol=float(tols[0]))
    _load(qa, X, sloppy)
    b = _source(X, pc)
    ip = _cg_param(qa, pc, qa.QUDA_MATPCDAG_MATPC_SOLUTION if pc else qa.QUDA_MATDAG_MAT_SOLUTION, sloppy=sloppy,
                   maxiter=2000 if sloppy == 8 else 10 * ref_iter, delta=delta)
    xs = qa.invert_multi_shift(b, ip, offsets, tols)
    A = _operator(oracle, X, pc)
    print("multi-shift %s %s sloppy %d: %d offsets, %d iterations (numpy CG on offset %g: %d)" % (X, "even-odd" if pc else "full", sloppy, len(offsets), ip.iter, offsets[0], ref_iter))
    for i, (s, t) in enumerate(zip(offsets, tols)):
        res = _res(_normal(A, float(s)), xs[i], b)
        print("  offset %-8g tol %g: host residual %.3e, reported true %.3e, iterated %.3e" % (s, t, res, ip.true_res_offset[i], ip.iter_res_offset[i]))
        assert res <= 1.1 * t, (i, s, res)
        assert abs(ip.true_res_offset[i] - res) <= 0.01 * res + 1e-12, (i, ip.true_res_offset[i], res)
    for i in range(len(offsets)):
        assert ip.offset[i] == float(offsets[i])   # restored on exit
    if count:
        assert abs(ip.iter - ref_iter) <= 3
    return ip, xs


SYSTEMS = [(X0, True), (X1, True), (X0, False)]
SYSTEM_IDS = ["4x4x4x8-even-odd", "6x4x2x8-even-odd", "4x4x4x8-full"]


@pytest.mark.parametrize("X,pc", SYSTEMS, ids=SYSTEM_IDS)
@pytest.mark.parametrize("case", ["four", "single", "KB+1"])
def test_multi_shift_fp64(qa, oracle, X, pc, case):
    offsets = {"four": [0.0, 0.01, 0.1, 1.0], "single": [0.05], "KB+1": list(np.geomspace(1e-3, 1.0, qa.multi_shift_chunk() + 1))}[case]
    _check_multi_shift(qa, oracle, X, pc, offsets, [TOL] * len(offsets))


@pytest.mark.parametrize("X,pc", SYSTEMS, ids=SYSTEM_IDS)
def test_multi_shift_per_shift_tolerances(qa, oracle, X, pc):
    _check_multi_shift(qa, oracle, X, pc, [0.0, 0.01, 0.1, 1.0], [1e-10, 1e-6, 1e-6, 1e-4])


@pytest.mark.parametrize("sloppy,delta", MIXED, ids=["fp32", "16-bit"])
@pytest.mark.parametrize("X", [X0, X1])
def test_multi_shift_mixed_precision_with_refinement(qa, oracle, X, sloppy, delta):
    """the iteration count includes the CG refinement of the shifts that miss their tolerance, so it is not compared with the fp64 one;
    maxiter = 10 x the fp64 count caps the multi-shift solve and every refinement"""
    _check_multi_shift(qa, oracle, X, True, [0.0, 0.01, 0.1, 1.0], [TOL] * 4, sloppy=sloppy, delta=delta, count=False)


# ---- 6. partition mask ----
def test_partitioned_directions_change_nothing(qa, oracle):
    """y and t through the ghost-zone path (self-neighbour emulation of a decomposed lattice): same iteration counts, solutions equal to
    1e-12 — the BLAS sums keep their order, only the stencil's neighbour path differs"""
    X = X0
    _load(qa, X)
    b = _source(X, True)
    offsets, tols = [0.0, 0.01, 0.1, 1.0], [TOL] * 4
    out = {}
    for mask in (0, 0b1010):
        qa.lib().qudaAmdSetPartitionMask(mask)
        try:
            ip = _cg_param(qa, True, qa.QUDA_MATPCDAG_MATPC_SOLUTION)
            x = qa.invert(b, ip)
            ipm = _cg_param(qa, True, qa.QUDA_MATPCDAG_MATPC_SOLUTION)
            xs = qa.invert_multi_shift(b, ipm, offsets, tols)
        finally:
            qa.lib().qudaAmdSetPartitionMask(0)
        out[mask] = (ip.iter, x, ipm.iter, xs)
    print("mask 0: CG %d, multi-shift %d iterations; mask 0b1010: CG %d, multi-shift %d" % (out[0][0], out[0][2], out[0b1010][0], out[0b1010][2]))
    assert out[0][0] == out[0b1010][0] and out[0][2] == out[0b1010][2]
    assert np.linalg.norm(out[0][1] - out[0b1010][1]) <= 1e-12 * np.linalg.norm(out[0][1])
    for a, c in zip(out[0][3], out[0b1010][3]):
        assert np.linalg.norm(a - c) <= 1e-12 * np.linalg.norm(a)
