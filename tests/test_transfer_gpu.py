"""The transfer paths that only a solve reaches, element-wise against the single-source oracle (oracle/qo_mg.c mg_restrict / mg_prolongate
fed with the device's own V): the four-source restrictor / prolongator (Transfer::R4 / P4), their block-column variants (R4Block / P4Block,
columns 4..7 of an 8-column parity block field), the single-parity route of R and P (Transfer::setSiteSubset) and the fp16 mirror of V —
all through qudaAmdMultigridApplyTransfer.  A solver that still converges can hide a wrong column or a wrong parity; these cannot.

Shapes: the smallest at which the kernels take their different paths — four waves per aggregate without the x-neighbour aggregate order,
the same with that order (Xc[0] % 4 == 0 and 32 aggregates), two waves per aggregate with one parity per wave (parity-major order); Nvec 8,
24 and 32 are the three instantiations of the quad kernels.  Tolerance 2e-5 relative to the largest element: fp32 device sums against the
fp64 oracle, the figure of the single transfer kernels in test_mg_gpu.py."""
import importlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from synth import smooth_gauge  # noqa: E402

CASES = [((8, 8, 8, 8), (4, 4, 4, 4), 8), ((16, 8, 8, 8), (4, 4, 4, 4), 24), ((8, 8, 8, 8), (4, 4, 4, 2), 32)]
IDS = ["8x8x8x8-4x4x4x4-nvec8", "16x8x8x8-4x4x4x4-nvec24", "8x8x8x8-4x4x4x2-nvec32"]
TOL = 2e-5
ZERO = 2   # the source that is identically zero


@pytest.fixture(scope="module")
def qa():
    mod = importlib.import_module("quda-qkxtm-multigrid_amd")
    mod.init(0)
    yield mod
    mod.end()


def rel(a, b):
    return float(np.max(np.abs(a - b)) / np.max(np.abs(b)))


class Hier:
    pass


@pytest.fixture(scope="module", params=CASES, ids=IDS)
def hier(request, qa, oracle):
    """the hierarchy of one case with the oracle's answers for its four sources, computed once and only read by the tests"""
    X, bs, nvec = request.param
    kappa, mu = 0.124, 0.005
    qa.load_gauge(smooth_gauge(X, 0.35), qa.gauge_param(X, cuda_prec=8, prec_sloppy=4, prec_precondition=4, t_boundary=qa.QUDA_PERIODIC_T))
    ip = qa.invert_param(qa.QUDA_TWISTED_MASS_DSLASH, kappa, mu, +1, "ee", 0, cuda_prec=8, prec_sloppy=4, prec_precondition=4, solution_type=qa.QUDA_MAT_SOLUTION)
    ip.solve_type, ip.inv_type, ip.gcrNkrylov, ip.tol, ip.maxiter, ip.reliable_delta, ip.verbosity = qa.QUDA_DIRECT_SOLVE, qa.QUDA_GCR_INVERTER, 20, 1e-10, 2000, 1e-4, qa.QUDA_SILENT
    h = Hier()
    h.mg = qa.Multigrid(qa.multigrid_param(ip, n_level=2, geo_block=bs, n_vec=nvec, setup_maxiter=50, setup_tol=1e-3))
    try:
        i = h.mg.level_info(0)
        h.geom = (i["Xf"], i["geo_bs"], i["fineSpin"], i["fineColor"], i["Nvec"], i["spin_bs"])
        Xf, Xc = i["Xf"], i["Xc"]
        assert list(i["geo_bs"]) == list(bs) and i["Nvec"] == nvec
        h.xgroup = Xc[0] % 4 == 0 and int(np.prod(Xc)) % 32 == 0 and bs[0] == 4
        h.V, h.Vh = int(np.prod(Xf)), int(np.prod(Xf)) // 2
        h.Vd = h.mg.V(0).astype(np.complex128)
        rng = np.random.default_rng(31)
        h.phi = (rng.standard_normal((4, h.V, 4, 3)) + 1j * rng.standard_normal((4, h.V, 4, 3))).astype(np.complex64)
        h.eta = (rng.standard_normal((4, int(np.prod(Xc)), 2, nvec)) + 1j * rng.standard_normal((4, int(np.prod(Xc)), 2, nvec))).astype(np.complex64)
        h.phi[ZERO] = 0
        h.eta[ZERO] = 0
        h.preload = (rng.standard_normal((8, h.V, 4, 3)) + 1j * rng.standard_normal((8, h.V, 4, 3))).astype(np.complex64)
        oracle.set_threads(8)
        try:
            # restrictions of every source as a full field (-1) and with the other parity zeroed (0, 1); prolongations of every coarse source
            h.Rref = {}
            for par in (-1, 0, 1):
                for s in range(4):
                    src = h.phi[s].astype(np.complex128)
                    if par >= 0:
                        src[(1 - par) * h.Vh:(2 - par) * h.Vh] = 0
                    h.Rref[par, s] = oracle.mg_restrict(src, h.Vd, *h.geom)
            h.Pref = [oracle.mg_prolongate(h.eta[s].astype(np.complex128), h.Vd, *h.geom) for s in range(4)]
        finally:
            oracle.set_threads(1)
        for a in (h.Vd, h.phi, h.eta, h.preload, *h.Rref.values(), *h.Pref):
            a.setflags(write=False)
        yield h
    finally:
        h.mg.free()


def present(h, par):
    return slice(0, h.V) if par < 0 else slice(par * h.Vh, (par + 1) * h.Vh)


def absent(h, par):
    return slice((1 - par) * h.Vh, (2 - par) * h.Vh)


def check(got, want, what):
    if not np.any(want):
        assert not np.any(got), what   # the zero source: nothing may leak into it from its neighbours
        return
    r = rel(got, want)
    print("%s rel %.2e" % (what, r))
    assert r < TOL, (what, r)


def test_case_reaches_what_it_is_for(hier):
    assert hier.xgroup == (hier.geom[0][0] == 16)


@pytest.mark.parametrize("par", [-1, 0, 1], ids=["full", "even", "odd"])
def test_four_source_restrictor_and_prolongator(hier, par):
    h = hier
    got = h.mg.apply_transfer(0, "R4", h.phi, parity=par)
    for s in range(4):
        check(got[s], h.Rref[par, s], "R4 parity %d source %d" % (par, s))
    got = h.mg.apply_transfer(0, "P4", h.eta, parity=par)
    for s in range(4):
        check(got[s][present(h, par)], h.Pref[s][present(h, par)], "P4 parity %d source %d" % (par, s))
        if par >= 0:
            assert not np.any(got[s][absent(h, par)]), (par, s)


@pytest.mark.parametrize("par", [0, 1], ids=["even", "odd"])
def test_block_column_restrictor_and_prolongator(hier, par):
    h = hier
    got = h.mg.apply_transfer(0, "R4Block", h.phi, parity=par)
    for s in range(4):
        check(got[s], h.Rref[par, s], "R4Block parity %d source %d" % (par, s))
    here = present(h, par)
    for op, acc in (("P4Block", 0), ("P4Block+", 1)):
        got = h.mg.apply_transfer(0, op, h.eta, parity=par, preload=h.preload)
        assert got.shape[0] == 8
        for c in range(4):   # columns 0..3 are not the prolongator's
            assert np.array_equal(got[c][here], h.preload[c][here]), (op, par, c)
        for s in range(4):
            want = h.Pref[s][here] + (h.preload[4 + s][here].astype(np.complex128) if acc else 0)
            check(got[4 + s][here], want, "%s parity %d source %d" % (op, par, s))
        assert not np.any(got[:, absent(h, par)]), (op, par)


@pytest.mark.parametrize("par", [0, 1], ids=["even", "odd"])
def test_single_parity_restrictor_and_prolongator(hier, par):
    h = hier
    check(h.mg.apply_transfer(0, "R", h.phi[0], parity=par), h.Rref[par, 0], "R parity %d" % par)
    got = h.mg.apply_transfer(0, "P", h.eta[0], parity=par)
    check(got[present(h, par)], h.Pref[0][present(h, par)], "P parity %d" % par)
    assert not np.any(got[absent(h, par)]), par


TOL_HALF = 2e-5


@pytest.mark.parametrize("hier", CASES[:1], ids=IDS[:1], indirect=True)
def test_restrictor_and_prolongator_on_the_fp16_mirror_of_v(hier, oracle):
    """R and P streaming the fp16 mirror of V (set_half_storage) against the oracle fed with V rounded through fp16 the way v_to_half_kernel
    rounds it (complex64 parts through np.float16): only the fp32 summation order separates the two.  Measured before the transfer sources
    were split (8^4, 4^4 aggregates, Nvec 8): R rel 8.4e-08, P rel 1.0e-07 — twice that is below 1e-5, so the bar is the 2e-5 of the fp32 legs."""
    h = hier
    V32 = h.Vd.astype(np.complex64)
    V16 = V32.real.astype(np.float16).astype(np.float64) + 1j * V32.imag.astype(np.float16).astype(np.float64)
    h.mg.set_half_storage(True)
    try:
        gotR = h.mg.apply(0, "R", h.phi[0])
        gotP = h.mg.apply(0, "P", h.eta[0])
    finally:
        h.mg.set_half_storage(False)
    rR = rel(gotR, oracle.mg_restrict(h.phi[0].astype(np.complex128), V16, *h.geom))
    rP = rel(gotP, oracle.mg_prolongate(h.eta[0].astype(np.complex128), V16, *h.geom))
    print("fp16 V: R rel %.2e, P rel %.2e" % (rR, rP))
    assert rR < TOL_HALF and rP < TOL_HALF, (rR, rP)
