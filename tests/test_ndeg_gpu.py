"""The non-degenerate twisted-mass doublet on the GPU, through the C ABI and the resident-field extension, against (1) the golden vectors of the
reference's own host operators (tests/golden/ndeg_*.npz) and (2) the host doublet reference of tests/test_ndeg_golden.py on seeded lattices.

Two forms of the doublet operators are checked, selected by the tune key "ndeg_fused": the fused doublet stencil (ndeg_dslash_kernel: both flavours
in one launch, every link read once, the flavours mixed across the half-waves in the epilogue; the default where no direction is partitioned) and the
composed one (the single-flavour stencil on the two flavour views of a doublet field plus the flavour-mixing site kernel ndeg_twist_kernel; always used
on partitioned lattices).  Tolerances are those of tests/test_dslash_gpu.py: 1e-12 / 2e-5 / 1e-2 per site for fp64 / fp32 / 16-bit, twice that for the
matpc and mat cases (two stencils in a row)."""
import importlib
import os
import subprocess
import sys

import numpy as np
import pytest

import qa_cases as qc
import test_ndeg_golden as ng

pytestmark = pytest.mark.gpu

TOL = {8: 1e-12, 4: 2e-5, 2: 1e-2}
KAPPA, MU, EPS = 0.12, 0.3, 0.2
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def qa():
    mod = importlib.import_module("quda-qkxtm-multigrid_amd")
    mod.init(0)
    yield mod
    mod.end()


def _load_gauge(qa, gauge, X, prec, recon):
    qa.load_gauge(gauge, qa.gauge_param(X, cuda_prec=prec, recon=recon))


def _ip(qa, prec, matpc="ee", dagger=0, sol=None, kappa=KAPPA, mu=MU, eps=EPS):
    return qa.invert_param(qa.QUDA_TWISTED_MASS_DSLASH, kappa, mu, qa.QUDA_TWIST_NONDEG_DOUBLET, matpc, dagger, cuda_prec=prec,
                           solution_type=qa.QUDA_MATPC_SOLUTION if sol is None else sol, epsilon=eps)


def run_abi(qa, name, spinor2, prec, kappa=KAPPA, mu=MU, eps=EPS):
    """golden case `name` through dslashQuda / MatQuda with twist_flavor = QUDA_TWIST_NONDEG_DOUBLET; the gauge field must be resident"""
    t = name.split("_")
    nd = spinor2.size // 2
    if t[1] == "dslash":
        return qa.dslash(spinor2[:nd].copy(), _ip(qa, prec, t[2], int(t[3][1]), kappa=kappa, mu=mu, eps=eps), int(t[4][1]))
    if t[1] == "matpc":
        p0 = qc.P0[t[2]]
        return qa.mat(spinor2[p0 * nd:(p0 + 1) * nd].copy(), _ip(qa, prec, t[2], int(t[3][1]), kappa=kappa, mu=mu, eps=eps))
    if t[1] == "mat":
        return qa.mat(spinor2.copy(), _ip(qa, prec, "ee", int(t[2][1]), sol=qa.QUDA_MAT_SOLUTION, kappa=kappa, mu=mu, eps=eps))
    raise KeyError(name)


def _set_fused(qa, value):
    qa.lib().qudaAmdSetDslashTune(b"ndeg_fused", int(value))


def _tol(name, prec):
    return TOL[prec] if "_dslash_" in name else 2 * TOL[prec]


_golden = {}


def _gold(X):
    if X not in _golden:
        _golden[X] = ng.load_golden(X)
    return _golden[X]


@pytest.mark.parametrize("fused", [1, 0], ids=["fused", "composed"])
@pytest.mark.parametrize("X", ng.LATTICES, ids=["4x4x4x4", "6x4x2x8"])
@pytest.mark.parametrize("prec,recon", [(8, 18), (8, 12), (8, 8), (4, 18), (4, 12), (4, 8), (2, 18), (2, 12), (2, 8)])
def test_all_golden_cases_through_c_abi(qa, X, prec, recon, fused):
    z, gauge, _ = _gold(X)
    _load_gauge(qa, gauge, X, prec, recon)
    worst = {}
    try:
        _set_fused(qa, fused)
        for name in ng.case_names(z):
            err = qc.rel_err(run_abi(qa, name, z["spinor2"], prec), z[name])
            worst[name] = err
            assert err < _tol(name, prec), "%s prec=%d recon=%d fused=%d: %g" % (name, prec, recon, fused, err)
    finally:
        _set_fused(qa, -1)
    assert len(worst) == 26


@pytest.mark.parametrize("prec", [8, 4, 2])
def test_matdagmat_through_c_abi(qa, oracle, prec):
    """MatDagMatQuda with the doublet, even-odd (ee, ooasym) and full, in both forms, against Mdag(M(.)) of the host reference on the 6x4x2x8
    golden inputs; four stencils in a row: twice the tolerance of the matpc and mat cases"""
    X = (6, 4, 2, 8)
    z, gauge, _ = _gold(X)
    src = z["spinor2"]
    nd = src.size // 2
    _load_gauge(qa, gauge, X, prec, 18)
    want = {m: ng.ndeg_matpc(oracle, gauge, ng.ndeg_matpc(oracle, gauge, src[qc.P0[m] * nd:(qc.P0[m] + 1) * nd], X, KAPPA, MU, EPS, m, 0), X, KAPPA, MU, EPS, m, 1)
            for m in ("ee", "ooasym")}
    want["full"] = ng.ndeg_mat(oracle, gauge, ng.ndeg_mat(oracle, gauge, src, X, KAPPA, MU, EPS, 0), X, KAPPA, MU, EPS, 1)
    try:
        for fused in (1, 0):
            _set_fused(qa, fused)
            for m in ("ee", "ooasym"):
                got = qa.matdagmat(src[qc.P0[m] * nd:(qc.P0[m] + 1) * nd].copy(), _ip(qa, prec, m, 0))
                assert qc.rel_err(got, want[m]) < 4 * TOL[prec], (m, prec, fused)
            got = qa.matdagmat(src.copy(), _ip(qa, prec, "ee", 0, sol=qa.QUDA_MAT_SOLUTION))
            assert qc.rel_err(got, want["full"]) < 4 * TOL[prec], ("full", prec, fused)
    finally:
        _set_fused(qa, -1)


SEEDED_CASES = ("ndeg_dslash_ee_d0_p0", "ndeg_dslash_oo_d1_p1", "ndeg_dslash_ooasym_d1_p0", "ndeg_matpc_oo_d1", "ndeg_matpc_eeasym_d0", "ndeg_mat_d1")
_seeded = {}


def _seeded_fields(oracle, X):
    """gauge, full doublet source and the host reference of SEEDED_CASES, computed once per lattice"""
    if X not in _seeded:
        gauge, _, _ = oracle.make_fields(list(X), clover=False)
        src = np.random.default_rng(11).random(2 * int(np.prod(X)) * 24)
        oracle.set_threads(8)
        try:
            want = {n: ng.host_case(oracle, n, gauge, src, X, KAPPA, MU, EPS) for n in SEEDED_CASES}
        finally:
            oracle.set_threads(1)
        _seeded[X] = (gauge, src, want)
    return _seeded[X]


@pytest.mark.parametrize("X", [(2, 2, 2, 2), (4, 2, 2, 8), (12, 6, 10, 4), (16, 16, 8, 24)])
def test_host_reference_on_seeded_lattices(qa, oracle, X):
    """2^4: every neighbour wraps and the site kernel's only block has 8 live threads; (12, 6, 10, 4): Vh = 1440 is no multiple of the block
    size of either kernel; (16, 16, 8, 24): several blocks per plane, 24 time slices"""
    gauge, src, want = _seeded_fields(oracle, X)
    try:
        for prec in (8, 4, 2):
            _load_gauge(qa, gauge, X, prec, 18)
            for fused in (1, 0):
                _set_fused(qa, fused)
                for name in SEEDED_CASES:
                    err = qc.rel_err(run_abi(qa, name, src, prec), want[name])
                    assert err < _tol(name, prec), (name, prec, fused, err)
    finally:
        _set_fused(qa, -1)


@pytest.mark.parametrize("prec,recon", [(8, 18), (4, 12), (2, 8)])
def test_fused_against_composed(qa, oracle, prec, recon):
    """the same inputs through both forms at (12, 6, 10, 4): Vh = 1440 is no multiple of a 128-site block, so the last block of the fused
    kernel has a tail.  All 26 cases: the two forms agree within the tolerance of the case, and each is within it of the host reference"""
    X = (12, 6, 10, 4)
    gauge, src, want = _seeded_fields(oracle, X)
    _load_gauge(qa, gauge, X, prec, recon)
    names = ["ndeg_dslash_%s_d%d_p%d" % (m, d, p) for m in ng.MPC for d in (0, 1) for p in (0, 1)]
    names += ["ndeg_matpc_%s_d%d" % (m, d) for m in ng.MPC for d in (0, 1)] + ["ndeg_mat_d0", "ndeg_mat_d1"]
    assert len(names) == 26
    got = {}
    try:
        for fused in (1, 0):
            _set_fused(qa, fused)
            got[fused] = {n: run_abi(qa, n, src, prec) for n in names}
    finally:
        _set_fused(qa, -1)
    oracle.set_threads(8)
    try:
        for n in names:
            host = want[n] if n in want else ng.host_case(oracle, n, gauge, src, X, KAPPA, MU, EPS)
            errs = (qc.rel_err(got[1][n], got[0][n]), qc.rel_err(got[1][n], host), qc.rel_err(got[0][n], host))
            assert max(errs) < _tol(n, prec), (n, prec, recon, errs)
    finally:
        oracle.set_threads(1)


def test_block_orders_do_not_change_the_doublet(qa, oracle):
    """the stencil's block orders (tests/test_dslash_gpu.py::test_block_orders_on_odd_shapes) with the 128-site blocks of the fused kernel
    ({"block": 128}: 64-site blocks) and under the flavour views of the composed form, whose base is offset by Vh sites inside the doublet's planes"""
    X = (16, 16, 8, 24)
    gauge, src, want = _seeded_fields(oracle, X)
    L = qa.lib()
    reset = dict(block=0, tiled=-1, nxz=0, tz=0, tt=0, ygroups=-1, ndeg_fused=-1, store_aux=-1, link_aux=-1)
    try:
        for prec in (8, 2):
            _load_gauge(qa, gauge, X, prec, 18)
            for fused in (1, 0):
                for setting in ({}, {"tiled": 0}, {"ygroups": 2}, {"block": 128}, {"store_aux": 2}, {"link_aux": 2}):
                    for k, v in reset.items():
                        L.qudaAmdSetDslashTune(k.encode(), v)
                    L.qudaAmdSetDslashTune(b"ndeg_fused", fused)
                    for k, v in setting.items():
                        L.qudaAmdSetDslashTune(k.encode(), v)
                    for name in ("ndeg_dslash_ee_d0_p0", "ndeg_matpc_oo_d1"):
                        err = qc.rel_err(run_abi(qa, name, src, prec), want[name])
                        assert err < _tol(name, prec), (name, prec, fused, setting, err)
    finally:
        for k, v in reset.items():
            L.qudaAmdSetDslashTune(k.encode(), v)


@pytest.mark.parametrize("prec", [8, 4, 2])
def test_site_kernel_against_numpy(qa, oracle, prec):
    """qudaAmdNdegTwist on resident parity doublets: direct and inverse, dagger 0 / 1, out of place and in place; inverse o direct is the
    identity (two passes, so twice the storage tolerance).  Vh = 1440: six blocks, the last one partly filled"""
    X = (12, 6, 10, 4)
    gauge, src, _ = _seeded_fields(oracle, X)
    _load_gauge(qa, gauge, X, prec, 18)
    nd = src.size // 2
    v = src[:nd] - 0.5
    ip = _ip(qa, prec)
    a, b = qa.Spinor(prec, flavor=qa.QUDA_TWIST_NONDEG_DOUBLET), qa.Spinor(prec, flavor=qa.QUDA_TWIST_NONDEG_DOUBLET)
    try:
        assert a.raw_info()["volumeCB"] == nd // 24 and a.raw_info()["twistFlavor"] == 2
        stored = a.load(v, ip).save(ip, v)     # the source as the storage precision holds it
        assert qc.rel_err(stored, v) < TOL[prec]
        for dagger in (0, 1):
            for inverse in (0, 1):
                want = ng.ndeg_twist(stored, KAPPA, MU, EPS, dagger, inverse)
                qa.ndeg_twist(b, a, KAPPA, MU, EPS, dagger, inverse)
                assert qc.rel_err(b.save(ip, v), want) < TOL[prec], (dagger, inverse)
                qa.ndeg_twist(b, b, KAPPA, MU, EPS, dagger, 1 - inverse)   # in place, the other direction
                assert qc.rel_err(b.save(ip, v), stored) < 2 * TOL[prec], (dagger, inverse)
    finally:
        a.free()
        b.free()


PARTITION_CASES = ("ndeg_dslash_ee_d0_p0", "ndeg_dslash_oo_d1_p0", "ndeg_matpc_ee_d0", "ndeg_matpc_ooasym_d1", "ndeg_mat_d0")


@pytest.mark.parametrize("fmt", [0, 1], ids=["flag-in-data", "atoms-16B"])
@pytest.mark.parametrize("mask", [6, 15])
def test_partitioned_self_neighbour(qa, mask, fmt):
    """the doublet through the halo path (pack, ghost exchange, interior + exterior kernels), one flavour after the other, as
    tests/test_dslash_gpu.py::test_partitioned_dslash_self_neighbour does for the degenerate operators"""
    X = (6, 4, 2, 8)
    z, gauge, _ = _gold(X)
    qa.lib().qudaAmdSetDslashTune(b"halo_format", fmt)
    os.environ["QUDA_AMD_FORCE_GAUGE_HALO"] = "1"
    try:
        _set_fused(qa, 1 if fmt else -1)   # the fused stencil asked for on a partitioned lattice: the composed form is taken silently
        for prec, recon in ((8, 18), (4, 12), (2, 18)):
            qa.lib().qudaAmdSetPartitionMask(mask)
            _load_gauge(qa, gauge, X, prec, recon)
            for name in PARTITION_CASES:
                err = qc.rel_err(run_abi(qa, name, z["spinor2"], prec), z[name])
                assert err < _tol(name, prec), (name, prec, mask, err)
            qa.lib().qudaAmdSetPartitionMask(0)
    finally:
        qa.lib().qudaAmdSetPartitionMask(0)
        qa.lib().qudaAmdSetDslashTune(b"halo_format", -1)
        _set_fused(qa, -1)
        os.environ.pop("QUDA_AMD_FORCE_GAUGE_HALO", None)


@pytest.mark.parametrize("matpc", ng.MPC)
def test_prepare_and_reconstruct_element_wise(qa, oracle, matpc):
    """with M = A - kappa D on doublets: src = [A^-1] (b_p + kappa D A^-1 b_q) and x_q = A^-1 (b_q + kappa D x_p), every site"""
    X = (8, 8, 8, 8)
    gauge, _, _ = oracle.make_fields(list(X), clover=False)
    rng = np.random.default_rng(3)
    n2 = 2 * int(np.prod(X)) * 24
    nd = n2 // 2
    b_h, x_h = rng.random(n2), rng.random(n2)
    Ainv = lambda v: ng.ndeg_twist(v, KAPPA, MU, EPS, 0, 1)
    D = lambda v, parity: ng._hop(oracle, gauge, v, X, parity, 0)
    _load_gauge(qa, gauge, X, 8, 18)
    ip = _ip(qa, 8, matpc, 0, sol=qa.QUDA_MAT_SOLUTION)
    ip.solve_type = qa.QUDA_DIRECT_PC_SOLVE
    d = qa.Dirac(ip, pc=True)
    dbl = qa.QUDA_TWIST_NONDEG_DOUBLET
    x, b, src = qa.Spinor(8, qa.QUDA_FULL_SITE_SUBSET, dbl), qa.Spinor(8, qa.QUDA_FULL_SITE_SUBSET, dbl), qa.Spinor(8, flavor=dbl)
    try:
        x.load(x_h, ip)
        b.load(b_h, ip)
        p = 0 if matpc.startswith("ee") else 1
        half = lambda v, par: v[:nd] if par == 0 else v[nd:]
        want = half(b_h, p) + KAPPA * D(Ainv(half(b_h, 1 - p)), p)
        if not matpc.endswith("asym"):
            want = Ainv(want)
        d.prepare(src, x, b, qa.QUDA_MAT_SOLUTION)
        assert qc.rel_err(src.save(ip, b_h[:nd]), want) < 1e-13
        x.load(x_h, ip)
        b.load(b_h, ip)
        d.reconstruct(x, b, qa.QUDA_MAT_SOLUTION)
        got = x.save(ip, x_h)
        assert np.array_equal(half(got, p), half(x_h, p))
        assert qc.rel_err(half(got, 1 - p), Ainv(half(b_h, 1 - p) + KAPPA * D(half(x_h, p), 1 - p))) < 1e-13
    finally:
        for f in (x, b, src):
            f.free()
        d.free()


def _cdot(qa, x, y):
    import ctypes as C
    r = (C.c_double * 2)()
    qa.lib().qudaAmdBlasCDot(x.h, y.h, r)
    return r[0], r[1]


_random_links = {}


@pytest.mark.parametrize("fused", [1, 0], ids=["fused", "composed"])
@pytest.mark.parametrize("pc,matpc", [(True, "ee"), (True, "ooasym"), (False, "ee")], ids=["even-odd-ee", "even-odd-ooasym", "full"])
def test_operator_properties_on_resident_fields(qa, pc, matpc, fused):
    """16^4 fp64: <y, M x> = <M^dag y, x> to 1e-12 of |y| |M x|, MdagM = Mdag(M(.)), and with epsilon = 0 the doublet operator is the two
    degenerate operators of flavours +1 / -1 on the flavour halves"""
    X = (16, 16, 16, 16)
    V = int(np.prod(X))
    rng = np.random.default_rng(7)
    if X not in _random_links:   # random SU(3) links by QR, made once
        g = rng.standard_normal((4, V, 3, 3)) + 1j * rng.standard_normal((4, V, 3, 3))
        q, r = np.linalg.qr(g)
        q = q * (np.diagonal(r, axis1=-2, axis2=-1) / np.abs(np.diagonal(r, axis1=-2, axis2=-1)))[..., None, :]
        q = q / np.linalg.det(q)[..., None, None] ** (1.0 / 3.0)
        _random_links[X] = np.ascontiguousarray(np.stack([q.real, q.imag], axis=-1)).reshape(4, V * 18)
    gauge = _random_links[X]
    _load_gauge(qa, gauge, X, 8, 18)
    sol = qa.QUDA_MATPC_SOLUTION if pc else qa.QUDA_MAT_SOLUTION
    subset = qa.QUDA_PARITY_SITE_SUBSET if pc else qa.QUDA_FULL_SITE_SUBSET
    ip = _ip(qa, 8, matpc, 0, sol=sol)
    n = 2 * V * 24 // (2 if pc else 1)
    x_h, y_h = rng.random(n) - 0.5, rng.random(n) - 0.5
    x, y, mx, my, t = [qa.Spinor(8, subset, qa.QUDA_TWIST_NONDEG_DOUBLET) for _ in range(5)]
    d = qa.Dirac(ip, pc=pc)
    try:
        _set_fused(qa, fused)
        x.load(x_h, ip)
        y.load(y_h, ip)
        d.M(mx, x)
        d.Mdag(my, y)
        r1, r2 = _cdot(qa, y, mx), _cdot(qa, my, x)
        scale = np.sqrt(y.norm2() * mx.norm2())
        assert abs(r1[0] - r2[0]) / scale < 1e-12 and abs(r1[1] - r2[1]) / scale < 1e-12
        d.MdagM(mx, y)
        d.M(t, y)
        d.Mdag(my, t)
        qa.lib().qudaAmdBlasAxpy(-1.0, my.h, mx.h)
        assert mx.norm2() / my.norm2() < 1e-24
        assert qa.lib().qudaAmdDiracFlops(d.h) > 0
        got = qa.mat(x_h.copy(), _ip(qa, 8, matpc, 0, sol=sol, eps=0.0))
    finally:
        _set_fused(qa, -1)
        for f in (x, y, mx, my, t):
            f.free()
        d.free()
    # epsilon = 0 through the C ABI against the degenerate operators (same kernels for the hop, different site arithmetic: rounding only)
    h = n // 2 if pc else n // 4
    for f, sign in ((0, +1), (1, -1)):
        ipd = qa.invert_param(qa.QUDA_TWISTED_MASS_DSLASH, KAPPA, MU, sign, matpc, 0, cuda_prec=8, solution_type=sol)
        pick = (lambda v: v[f * h:(f + 1) * h]) if pc else (lambda v: np.concatenate([v[f * h:(f + 1) * h], v[(2 + f) * h:(3 + f) * h]]))   # full: [even flavour f][odd flavour f]
        assert qc.rel_err(pick(got), qa.mat(pick(x_h).copy(), ipd)) < 1e-13, (f,)


def test_twist_flavour_of_a_field_is_fixed(qa):
    """changeTwist to or from the doublet on an existing field is an error (child process: the library ends the process)"""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "ndeg_error_cases.py"), "change_twist"], capture_output=True, text=True, timeout=300)
    out = r.stdout + r.stderr
    assert r.returncode == 1 and "ERROR:" in out and "doublet" in out and "NOT REACHED" not in out, out[-1500:]


@pytest.mark.parametrize("case", ["twisted_clover", "multigrid", "multi_src", "no_inverse"])
def test_error_cases(case):
    """each in a child process (tools/ndeg_error_cases.py): exit status 1 and an `ERROR:` line that names the doublet"""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "ndeg_error_cases.py"), case], capture_output=True, text=True, timeout=300)
    out = r.stdout + r.stderr
    assert r.returncode == 1, (r.returncode, out[-1500:])
    assert "ERROR:" in out and "doublet" in out and "NOT REACHED" not in out, out[-1500:]
