"""The transfer and set-up kernels BELOW level 0, element-wise against the fp64 oracle fed with the device's own vectors: level 1 of a 3-level
twisted-mass hierarchy (level-1 fields <-> level-2 fields) in all six coarse shapes of transfer.hip's forShape (fine spin x fine colour -> Nvec:
2x4->4, 2x8->8, 2x8->4, 2x24->24, 2x24->32, 2x32->32), through restrict_small_kernel / prolong_small_kernel at lane groups of 2, 4, 8, 16 and 32
lanes (one and two trips of the iteration loop, a 3- and a 24-site aggregate with idle lanes inside the shuffles) and through the general
restrict_kernel / prolong_kernel with NSF = 2 (64-site aggregates); the block orthonormalisation (block_cholqr_kernel<4 / 8 / 24 / 32> with
spin_bs = 1), the from-coarse Galerkin product (coarse.hip: the split restriction, DUAL, with and without partition masks), the fp16 mirror of V,
the single-parity route and the coarse operator of the level-2 lattice.  tests/test_mg_gpu.py reaches level 1 with 2-site aggregates and 2x8->8 only.

Cases (tests/transfer_ref.py CASES; tests/test_transfer_ref.py checks the table against the restated rules without a GPU).  a-f are the lattices
first proposed for these paths.  Transfer::Transfer halves a block extent until the coarse extent is even and never lets the x extent cover the
lattice (reference lib/transfer.cpp:31-44), so on their 2 x 2 x 2 x N level-1 lattices the blocks asked for shrink to 2, 3, 4 or 8 sites: they
reach every Shape, but not the aggregates of the production hierarchy.  A-F double every level-1 extent — the smallest lattices on which the
blocks asked for survive — and reach them: 16 sites (GS 16, 32 slots), 24 (GS 32, 16 slots, two trips at Nvec 32), 32 and 64 (general route).
What no hierarchy reaches: a coarse extent of 1 (MaskArg::single, every neighbour of coarse_apply_kernel the site itself) — the same rule forbids
it, and the even-odd site numbering (Xc[0] / 2 sites per row) has no room for it.

Bars: 2e-5 relative to the largest element for single kernels (fp32 sums against fp64, the project's figure), 1e-5 for |V^dag V - 1| per block
(CholeskyQR2, test_block_orthonormalisation_of_nearly_dependent_vectors), 1e-4 for verify.  V against the oracle's Gram-Schmidt: the bar comes
from the reference alone — the deviation of a complex64 modified Gram-Schmidt (transfer_ref.gram_schmidt) from the complex128 one on the device's
null vectors, worst case times four (DESIGN, coarse Schur section: the margin for chained fp32 pieces), and never below the 2e-4 of the 8-deep
recursion.  MEASURED on one MI355X, complex64 against complex128 Gram-Schmidt | device against oracle | max |V^dag V - 1|, no block of any
case handed to Gram-Schmidt:
  a 3.25e-06 | 7.16e-07 | 5.35e-07    b 5.33e-06 | 1.03e-06 | 5.35e-07    c 4.72e-06 | 1.86e-06 | 5.73e-07
  d 1.35e-07 | 1.43e-07 | 3.43e-07    e 1.83e-06 | 7.37e-07 | 5.01e-07    f 1.46e-07 | 1.07e-07 | 2.71e-07
  A 4.10e-06 | 8.70e-07 | 1.09e-06    B 4.10e-06 | 8.70e-07 | 1.09e-06    C 5.45e-06 | 1.03e-06 | 8.21e-07
  D 1.46e-07 | 1.82e-07 | 5.90e-07    E 2.78e-06 | 3.16e-07 | 8.83e-07    F 1.82e-07 | 3.07e-07 | 7.21e-07
The worst reference figure is 5.45e-06 (case C, 32 vectors on 768 rows); four times that is 2.2e-05 < 2e-4, so the bar stays 2e-4.
R, P, the Galerkin links and the level-2 operator came out at 5e-08 .. 3.1e-07 in every case and route (bar 2e-5), verify at <= 1.1e-06.

What the tests found: a 3-level hierarchy with 32 vectors on levels 0 and 1 (cases c, C) stopped in the set-up — blockCoarseSupported
(block.hip) promised the lockstep null-vector solve a 64 x 32 block kernel that applyCoarseBlock did not instantiate; it does now, and
test_block_coarse_operator_on_mfma[n64] holds it (and the other n = 64 batch sizes) to the oracle.  No wrong number anywhere."""
import importlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import transfer_ref as tr  # noqa: E402
from synth import smooth_gauge  # noqa: E402

TOL = 2e-5
GRAM = 1e-5
WORST_REFERENCE_FIGURE = 5.45e-6      # complex64 against complex128 Gram-Schmidt, worst case of the docstring (C)
ORTHO_BAR = max(2e-4, 4 * WORST_REFERENCE_FIGURE)
KAPPA, MU = 0.124, 0.005
ZERO = 1   # the source that is identically zero
NAMES = list(tr.CASES)


@pytest.fixture(scope="module")
def qa():
    mod = importlib.import_module("quda-qkxtm-multigrid_amd")
    mod.init(0)
    yield mod
    mod.end()


def rel(a, b):
    return float(np.max(np.abs(a - b)) / np.max(np.abs(b)))


def cvec(rng, shape):
    return (rng.standard_normal(shape) + 1j * rng.standard_normal(shape)).astype(np.complex64)


class Hier:
    pass


def build(qa, name):
    """the hierarchy of a case on the gauge field it loads; asserts from level_info(1) that level 1 is what the case table says"""
    X, req, nvec, maxiter, (got, rt, gs, slots, trips) = tr.CASES[name]
    qa.load_gauge(smooth_gauge(X, 0.35), qa.gauge_param(X, cuda_prec=8, prec_sloppy=4, prec_precondition=4, t_boundary=qa.QUDA_PERIODIC_T))
    ip = qa.invert_param(qa.QUDA_TWISTED_MASS_DSLASH, KAPPA, MU, +1, "ee", 0, cuda_prec=8, prec_sloppy=4, prec_precondition=4, solution_type=qa.QUDA_MAT_SOLUTION)
    ip.solve_type, ip.inv_type, ip.gcrNkrylov, ip.tol, ip.maxiter, ip.reliable_delta, ip.verbosity = qa.QUDA_DIRECT_SOLVE, qa.QUDA_GCR_INVERTER, 20, 1e-10, 2000, 1e-4, qa.QUDA_SILENT
    mp = qa.multigrid_param(ip, n_level=3, geo_block=[(4, 4, 4, 4), req, (2, 2, 2, 2)], n_vec=[nvec[0], nvec[1], nvec[1]], setup_maxiter=maxiter, setup_tol=1e-3)
    h = Hier()
    h.name, h.ip, h.mp = name, ip, mp
    h.mg = qa.Multigrid(mp)
    try:
        assert h.mg.levels() == 3
        i = h.mg.level_info(1)
        h.geom = (i["Xf"], i["geo_bs"], i["fineSpin"], i["fineColor"], i["Nvec"], i["spin_bs"])
        h.Xc, h.Nc, h.Nv = i["Xc"], i["fineColor"], i["Nvec"]
        # the reach: the Shape, the aggregate, and from transfer.hip's rule the route, the lane group, the slots and the trips of the iteration loop
        assert (i["fineSpin"], i["fineColor"], i["Nvec"], i["spin_bs"]) == (2, nvec[0], nvec[1], 1), i
        assert i["Xf"] == [X[d] // 4 for d in range(4)] and list(i["geo_bs"]) == list(got), i
        assert list(i["geo_bs"]) == tr.blocks_after_fallback(i["Xf"], req)
        h.blockVol = int(np.prod(i["geo_bs"]))
        assert tr.route(h.blockVol, i["Nvec"]) == (rt, gs, slots, trips)
        assert (rt == "small") == (h.blockVol <= 32)
    except BaseException:
        h.mg.free()
        raise
    return h


@pytest.fixture(scope="module", params=NAMES, ids=[tr.case_id(n) for n in NAMES])
def hier(request, qa, oracle):
    """the hierarchy of one case with the oracle's answers, computed once and only read by the tests.  Everything that needs the gauge field of
    the case (verify) is taken here, so that a test which loads another field cannot disturb the ones that follow"""
    h = build(qa, request.param)
    try:
        Xf, bs, Ns, Nc, Nv, sbs = h.geom
        V1, V2 = int(np.prod(Xf)), int(np.prod(h.Xc))
        h.V, h.Vh = V1, V1 // 2
        h.verify = h.mg.verify()
        h.fallback = h.mg.ortho_fallback_blocks(1)
        h.B = np.stack([h.mg.null_vector(1, k) for k in range(Nv)], axis=-1).astype(np.complex128)
        h.Vd = h.mg.V(1).astype(np.complex128)
        h.table = tr.aggregates(Xf, bs)
        rng = np.random.default_rng(37)
        h.phi, h.eta = cvec(rng, (3, V1, 2, Nc)), cvec(rng, (3, V2, 2, Nv))
        h.phi[ZERO] = 0
        h.eta[ZERO] = 0
        Y0, X0 = h.mg.coarse_links(0)
        h.Y1, h.X1 = h.mg.coarse_links(1)
        oracle.set_threads(8)
        try:
            h.Vo = oracle.mg_block_orthogonalize(h.B, *h.geom)
            h.Rref = {}
            for par in (-1, 0, 1):
                for s in range(3):
                    src = h.phi[s].astype(np.complex128)
                    if par >= 0:
                        src[(1 - par) * h.Vh:(2 - par) * h.Vh] = 0
                    h.Rref[par, s] = oracle.mg_restrict(src, h.Vd, *h.geom)
            h.Pref = [oracle.mg_prolongate(h.eta[s].astype(np.complex128), h.Vd, *h.geom) for s in range(3)]
            # the from-coarse Galerkin product from the device's level-1 links (the device stores -kappa Y) and the operator it defines on level 2
            h.Yo, h.Xo = oracle.mg_coarse_op_coarse(h.Vd, Y0.astype(np.complex128) / (-KAPPA), X0.astype(np.complex128), KAPPA, Xf, bs, Nc, Nv)
            h.Mref = [oracle.mg_coarse_apply(h.eta[s].astype(np.complex128), h.Y1.astype(np.complex128) / (-KAPPA), h.X1.astype(np.complex128), KAPPA, h.Xc, Nv) for s in range(3)]
        finally:
            oracle.set_threads(1)
        del Y0, X0
        for a in (h.B, h.Vd, h.Vo, h.phi, h.eta, h.Y1, h.X1, h.Yo, h.Xo, *h.Rref.values(), *h.Pref, *h.Mref):
            a.setflags(write=False)
        print("\ncase %s: set-up %.2f s" % (h.name, h.mp.secs))
        yield h
    finally:
        h.mg.free()


def check(got, want, what, tol=TOL):
    if not np.any(want):
        assert not np.any(got), what   # the zero source: nothing may leak into it
        return
    r = rel(got, want)
    print("%s rel %.2e" % (what, r))
    assert r < tol, (what, r)


def test_block_orthonormalisation(hier):
    h = hier
    Ns, Nc, Nv = h.geom[2], h.geom[3], h.geom[4]
    M = tr.block_matrices(h.Vd, h.table)
    gram = float(np.max(np.abs(np.einsum("bmi,bmj->bij", M.conj(), M) - np.eye(Nv))))
    Bm = tr.block_matrices(h.B, h.table)
    figure = rel(tr.gram_schmidt(Bm, np.complex64), tr.gram_schmidt(Bm, np.complex128))
    dev = rel(h.Vd, h.Vo)
    print("case %s orthonormalisation: %d blocks of %d x %d, %d to Gram-Schmidt, max |V^dag V - 1| %.2e, complex64 against complex128 Gram-Schmidt %.2e, device against oracle %.2e"
          % (h.name, len(M), M.shape[1], Nv, h.fallback, gram, figure, dev))
    assert h.fallback == 0
    assert gram < GRAM, gram
    assert dev < ORTHO_BAR, dev


def test_restrictor_and_prolongator_on_full_fields(hier):
    h = hier
    for s in range(3):
        check(h.mg.apply_transfer(1, "R", h.phi[s]), h.Rref[-1, s], "case %s R source %d" % (h.name, s))
        check(h.mg.apply_transfer(1, "P", h.eta[s]), h.Pref[s], "case %s P source %d" % (h.name, s))
    # the plain entry point (qudaAmdMultigridApply) takes the same kernels
    check(h.mg.apply(1, "R", h.phi[0]), h.Rref[-1, 0], "case %s R (apply)" % h.name)
    check(h.mg.apply(1, "P", h.eta[0]), h.Pref[0], "case %s P (apply)" % h.name)


@pytest.mark.parametrize("par", [0, 1], ids=["even", "odd"])
def test_restrictor_and_prolongator_on_one_parity(hier, par):
    """Transfer::setSiteSubset on a coarse level: in.v[other parity] == nullptr restricts as zero and is not written by the prolongator"""
    h = hier
    here, there = slice(par * h.Vh, (par + 1) * h.Vh), slice((1 - par) * h.Vh, (2 - par) * h.Vh)
    for s in range(3):
        check(h.mg.apply_transfer(1, "R", h.phi[s], parity=par), h.Rref[par, s], "case %s R parity %d source %d" % (h.name, par, s))
        got = h.mg.apply_transfer(1, "P", h.eta[s], parity=par)
        check(got[here], h.Pref[s][here], "case %s P parity %d source %d" % (h.name, par, s))
        assert not np.any(got[there]), (par, s)


def test_restrictor_and_prolongator_on_the_fp16_mirror_of_v(hier, oracle):
    """every level keeps a mirror (MG::makeHalfMirrors): R and P against the oracle fed with V rounded through fp16 part by part, the way
    v_to_half_kernel rounds it — only the fp32 summation order separates the two, hence the 2e-5 of the fp32 legs.  On every case (the
    hierarchy is there already; a, c, A, C are the ones the HALF variants were missing most: Nvec 24 / 32, one and two trips)"""
    h = hier
    V32 = h.Vd.astype(np.complex64)
    V16 = V32.real.astype(np.float16).astype(np.float64) + 1j * V32.imag.astype(np.float16).astype(np.float64)
    h.mg.set_half_storage(True)
    try:
        gotR = [h.mg.apply_transfer(1, "R", h.phi[s]) for s in range(3)]
        gotP = [h.mg.apply_transfer(1, "P", h.eta[s]) for s in range(3)]
    finally:
        h.mg.set_half_storage(False)
    assert not np.array_equal(gotR[0], h.mg.apply_transfer(1, "R", h.phi[0]))   # the mirror was streamed, not the fp32 master
    oracle.set_threads(8)
    try:
        for s in range(3):
            check(gotR[s], oracle.mg_restrict(h.phi[s].astype(np.complex128), V16, *h.geom), "case %s fp16 V: R source %d" % (h.name, s))
            check(gotP[s], oracle.mg_prolongate(h.eta[s].astype(np.complex128), V16, *h.geom), "case %s fp16 V: P source %d" % (h.name, s))
    finally:
        oracle.set_threads(1)


def test_from_coarse_galerkin_product(hier):
    h = hier
    check(h.X1, h.Xo, "case %s Galerkin X" % h.name)
    check(h.Y1, -KAPPA * h.Yo, "case %s Galerkin Y" % h.name)


def test_coarse_operator_on_the_level_2_lattice(hier):
    h = hier
    assert all(x % 2 == 0 for x in h.Xc)   # no extent of 1: see the module docstring
    for s in range(3):
        check(h.mg.apply(2, "M", h.eta[s]), h.Mref[s], "case %s M on %s source %d" % (h.name, "x".join(map(str, h.Xc)), s))


def test_verify_identities(hier):
    print("case %s verify %s" % (hier.name, ["%.2e" % d for d in hier.verify]))
    assert max(hier.verify) < 1e-4, hier.verify


@pytest.mark.parametrize("mask", [9, 15], ids=["self-neighbour-xt", "self-neighbour-xyzt"])
@pytest.mark.parametrize("name", ["a", "A"], ids=[tr.case_id("a"), tr.case_id("A")])
def test_from_coarse_galerkin_product_under_partition_masks(qa, oracle, name, mask):
    """a fresh hierarchy with the dimensions of the mask grid-decomposed (the process its own neighbour): the hermitian completion is off, all
    eight hops of a probe go through the split restriction (Transfer::RSplit, DUAL with mask_outside) and the ghost-aware hops of level 1"""
    qa.lib().qudaAmdSetPartitionMask(mask)
    h = None
    try:
        h = build(qa, name)
        Xf, bs, Ns, Nc, Nv, sbs = h.geom
        Vd = h.mg.V(1).astype(np.complex128)
        Y0, X0 = h.mg.coarse_links(0)
        Y1, X1 = h.mg.coarse_links(1)
        oracle.set_threads(8)
        try:
            Yo, Xo = oracle.mg_coarse_op_coarse(Vd, Y0.astype(np.complex128) / (-KAPPA), X0.astype(np.complex128), KAPPA, Xf, bs, Nc, Nv)
        finally:
            oracle.set_threads(1)
        check(X1, Xo, "case %s mask %d Galerkin X" % (name, mask))
        check(Y1, -KAPPA * Yo, "case %s mask %d Galerkin Y" % (name, mask))
    finally:
        if h is not None:
            h.mg.free()
        qa.lib().qudaAmdSetPartitionMask(0)
