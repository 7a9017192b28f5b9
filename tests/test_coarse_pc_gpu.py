"""The even-odd preconditioned coarse operator piece by piece, element-wise against tests/coarse_ref.py (numpy complex128 from the device's own
matrices): the batched inverse Xinv and the products Xinv H_d (coarse_invert_kernel / coarse_hat_kernel, also on synthetic batches that need
the row swap, at every n up to the 64 the kernels allow), applyCoarse on parity fields and with single matrices (with and without a partitioned
lattice), the Schur pieces M / prepare / reconstruct of DiracCoarsePC and of the block-field cycle (BlockCoarseCycle on the MFMA kernel), and the
fp16 mirror of both link sets.  Until here these were reached only from inside a solve, where a wrong Xinv or a wrong parity costs iterations,
not a test.

Cases: the smallest coarse lattices on which every dimension is at least once longer than 2 (at extent 2 the forward and the backward neighbour
are the same site and a swapped direction passes), with n = 2 Nvec = 16, 48 (Xh = 1) and 64.  What catches what (the reference catches the
same planted errors on the CPU, tests/test_coarse_ref.py):
  a swapped forward / backward neighbour   test_single_matrices_on_full_fields (bits 0..7 in the dimensions longer than 2), test_apply_on_parity_fields
  a parity field routed to the wrong half  test_apply_on_parity_fields (hops read the other parity, the local term its own), test_schur_pieces
  a skipped row swap                       test_synthetic_batches[swap] (the pivot search picks another row in almost every column)
  Xinv taken from the neighbour's site     test_hat_links (slots 0..7 against Xinv(A) H_d(A) of the same site), test_schur_pieces"""
import importlib

import numpy as np
import pytest

import coarse_ref as cr

pytestmark = pytest.mark.gpu

from synth import smooth_gauge  # noqa: E402

CASES = [((16, 8, 8, 16), (4, 4, 4, 4), 8), ((8, 16, 16, 8), (4, 4, 4, 4), 24), ((8, 8, 8, 8), (4, 4, 4, 2), 32)]
IDS = ["a-4x2x2x4-n16", "b-2x4x4x2-n48", "c-2x2x2x4-n64"]
KAPPA, MU = 0.124, 0.005
TOL = 2e-5    # relative to the largest element: the project's figure for single transfer / coarse kernels (test_mg_gpu.py, test_transfer_gpu.py)
ZERO = 2      # the vector (block column) that is identically zero


@pytest.fixture(scope="module")
def qa():
    mod = importlib.import_module("quda-qkxtm-multigrid_amd")
    mod.init(0)
    yield mod
    mod.end()


def rel(a, b):
    return float(np.max(np.abs(a - b)) / np.max(np.abs(b)))


def cnormal(rng, shape):
    return (rng.standard_normal(shape) + 1j * rng.standard_normal(shape)).astype(np.complex64)


class Hier:
    pass


@pytest.fixture(scope="module", params=CASES, ids=IDS)
def hier(request, qa, oracle):
    """the two-level hierarchy of one case, its site links as the device holds them, and the inputs; everything only read by the tests"""
    X, bs, nvec = request.param
    qa.load_gauge(smooth_gauge(X, 0.35), qa.gauge_param(X, cuda_prec=8, prec_sloppy=4, prec_precondition=4, t_boundary=qa.QUDA_PERIODIC_T))
    ip = qa.invert_param(qa.QUDA_TWISTED_MASS_DSLASH, KAPPA, MU, +1, "ee", 0, cuda_prec=8, prec_sloppy=4, prec_precondition=4, solution_type=qa.QUDA_MAT_SOLUTION)
    ip.solve_type, ip.inv_type, ip.gcrNkrylov, ip.tol, ip.maxiter, ip.reliable_delta, ip.verbosity = qa.QUDA_DIRECT_SOLVE, qa.QUDA_GCR_INVERTER, 20, 1e-10, 2000, 1e-4, qa.QUDA_SILENT
    h = Hier()
    h.qa = qa
    h.mg = qa.Multigrid(qa.multigrid_param(ip, n_level=2, geo_block=bs, n_vec=nvec, setup_maxiter=50, setup_tol=1e-3, smoother_pc=True))
    try:
        i = h.mg.level_info(0)
        h.Xc, h.nvec, h.n = tuple(i["Xc"]), nvec, 2 * nvec
        assert h.Xc == tuple(x // b for x, b in zip(X, bs)) and max(h.Xc) > 2
        h.V, h.Vh = cr.volume(h.Xc), cr.volume(h.Xc) // 2
        h.L = h.mg.coarse_site_links(0, "links")
        h.H = h.mg.coarse_site_links(0, "hat")
        # the site links are the links of coarse_links(): forward bit-identical, backward the dagger of the neighbour's, X the local matrix
        Y, Xm = h.mg.coarse_links(0)
        for mu in range(4):
            assert np.array_equal(Y[4 + mu], h.L[:, 2 * mu]), mu
            assert np.array_equal(Y[mu], np.conj(np.swapaxes(h.L[cr.neighbour(h.Xc, 2 * mu), 2 * mu + 1], -1, -2))), mu
        assert np.array_equal(Xm, h.L[:, 8])
        rng = np.random.default_rng(47)
        h.v = cnormal(rng, (4, h.V, 2, nvec))
        h.v[ZERO] = 0
        # ... and the numpy reference with them is the oracle's coarse operator: from here on it stands for the oracle
        want = oracle.mg_coarse_apply(h.v[0].astype(np.complex128), Y.astype(np.complex128) / (-KAPPA), Xm.astype(np.complex128), KAPPA, list(h.Xc), nvec)
        r = rel(cr.apply(h.L, h.v[0], h.Xc), want)
        print("coarse_ref.apply with the device's site links vs the oracle: rel %.2e" % r)
        assert r < 1e-12
        h.blocks = {}
        for nrhs in (8, 24):
            b = cnormal(rng, (nrhs, h.V, 2, nvec)) * (10.0 ** rng.integers(-2, 3, nrhs)).astype(np.float32)[:, None, None, None]
            b[ZERO] = 0
            h.blocks[nrhs] = b
        for a in (h.L, h.H, h.v, *h.blocks.values()):
            a.setflags(write=False)
        yield h
    finally:
        h.mg.free()


def check(got, want, what, tol=TOL):
    if not np.any(want):
        assert not np.any(got), what   # the zero vector: nothing may leak into it
        return 0.0
    r = rel(got, want)
    assert r < tol, (what, r, tol)
    return r


# ---------------------------------------------------------------------------------------------------------------------------------------------
# Xinv and Xinv H_d
# ---------------------------------------------------------------------------------------------------------------------------------------------
def hat_ratios(X, H, Xinv, hat):
    """worst element-wise error of the device's inverse and products in units of the forward-error bounds of coarse_ref"""
    X128, H128 = X.astype(np.complex128), H.astype(np.complex128)
    want = np.linalg.inv(X128)
    r_inv = cr.worst_ratio(Xinv, want, cr.inverse_bound(X128, want))
    r_hat = cr.worst_ratio(hat, want[:, None] @ H128, cr.product_bound(X128, want, H128))
    return r_inv, r_hat


def test_hat_links(hier):
    """which = 1 against coarse_ref.hat of the device's own links, element by element under c n 2^-24 |Xinv| |X| |Xinv| (Xinv) and the matching
    product bound (Xinv H_d): the forward-error form of an fp32 elimination.  c = C_HAT = 4 x the worst ratio a complex64 numpy Gauss-Jordan with
    partial pivoting shows under the same bound on the matrices of this file (coarse_ref.GJ_C64_WORST): the device's order of operations
    differs from numpy's, its arithmetic does not.
    MEASURED (complex64 numpy on the X of the cases a / b / c): 0.39 / 0.21 / 0.14; on the synthetic batches up to 1.49 (coarse_ref.py), so
    C_HAT = 5.96.  MEASURED (device on an MI355X, Xinv | Xinv H_d): a 0.39 | 0.28, b 0.19 | 0.08, c 0.15 | 0.05."""
    h = hier
    X = h.L[:, 8]
    c64 = cr.worst_ratio(cr.gauss_jordan_c64(X), np.linalg.inv(X.astype(np.complex128)), cr.inverse_bound(X.astype(np.complex128), np.linalg.inv(X.astype(np.complex128))))
    r_inv, r_hat = hat_ratios(X, h.L[:, :8], h.H[:, 8], h.H[:, :8])
    print("n %d: complex64 numpy Gauss-Jordan worst ratio %.3f; device worst ratio Xinv %.3f, Xinv H_d %.3f (allowed %.2f)" % (h.n, c64, r_inv, r_hat, cr.C_HAT))
    assert c64 <= cr.GJ_C64_WORST   # the calibration covers this case's matrices
    assert r_inv <= cr.C_HAT and r_hat <= cr.C_HAT


@pytest.mark.parametrize("n", [4, 16, 48, 64])
def test_synthetic_batches(qa, n):
    """qudaAmdCoarseInvertSites on 8 matrices per batch: (i) row-permuted P (D + 0.1 R), where the pivot search has to pick another row in almost
    every column (the X of a twisted-mass hierarchy is close to diagonal: it never does); (ii) the identity and diagonal matrices, whose
    inverse is exact; (iii) one site with an identically zero column among good ones: the flag; then good matrices again: nothing sticks.
    MEASURED (device worst ratio on the row-swap batch, Xinv | Xinv H_d, n = 4 / 16 / 48 / 64): 0.57 | 0.43, 0.56 | 0.03, 0.09 | 0.005,
    0.03 | 0.002, against 0.63 / 1.49 / 0.12 / 0.03 of complex64 numpy on the same matrices."""
    rng = np.random.default_rng(100 + n)
    swap, exact = cr.synthetic_batches(n, rng)
    assert np.max(np.linalg.cond(swap.astype(np.complex128))) <= 1e3
    H = cnormal(rng, (8, 8, n, n))
    Xinv, hat, fail = qa.coarse_invert_sites(swap, H)
    r_inv, r_hat = hat_ratios(swap, H, Xinv, hat)
    print("n %d row-swap batch: device worst ratio Xinv %.3f, Xinv H_d %.3f (allowed %.2f)" % (n, r_inv, r_hat, cr.C_HAT))
    assert fail == 0
    assert r_inv <= cr.C_HAT and r_hat <= cr.C_HAT
    exact_inv, _, fail = qa.coarse_invert_sites(exact, H)
    assert fail == 0
    assert np.array_equal(exact_inv, np.linalg.inv(exact.astype(np.complex128)).astype(np.complex64))
    singular = swap.copy()
    singular[3][:, n // 2] = 0
    _, _, fail = qa.coarse_invert_sites(singular, H)
    assert fail == 1
    again, hat_again, fail = qa.coarse_invert_sites(swap, H)
    assert fail == 0 and np.array_equal(again, Xinv) and np.array_equal(hat_again, hat)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# applyCoarse with parity fields and single matrices
# ---------------------------------------------------------------------------------------------------------------------------------------------
def links_of(h, which):
    return h.L if which == "links" else h.H


@pytest.mark.parametrize("mask", [0, 15], ids=["unpartitioned", "self-neighbour-xyzt"])
@pytest.mark.parametrize("which", ["links", "hat"])
@pytest.mark.parametrize("parity", [0, 1], ids=["even", "odd"])
def test_apply_on_parity_fields(hier, parity, which, mask):
    """Dslash (mmask 0xff: DiracCoarse::Dslash / DiracCoarsePC::Dslash) and the local term (1 << 8: Clover / CloverInv) with parity fields; the hook
    refuses a changed input.  mask 15: every dimension partitioned with the process as its own neighbour — the single-parity ghost zone."""
    h = hier
    before = h.qa.comm_stats()
    h.qa.lib().qudaAmdSetPartitionMask(mask)
    try:
        for mmask, in_par in ((cr.HOPS, 1 - parity), (cr.LOCAL, parity)):
            for s in (0, ZERO):
                src = cr.half(h.v[s], in_par)
                got = h.mg.coarse_apply(0, which, mmask, src, parity=parity)
                want = cr.half(cr.apply(links_of(h, which), cr.embed(src, in_par, h.Xc), h.Xc, mmask, parity), parity)
                r = check(got, want, (which, hex(mmask), parity, s))
                print("%s mmask 0x%x parity %d vector %d: rel %.2e" % (which, mmask, parity, s, r))
    finally:
        h.qa.lib().qudaAmdSetPartitionMask(0)
    after = h.qa.comm_stats()
    moved = sum(after[k] - before[k] for k in ("coarse_peer_store_exchanges", "coarse_staged_exchanges"))
    assert (moved > 0) == (mask != 0), (mask, moved)


@pytest.mark.parametrize("mask", [0, 15], ids=["unpartitioned", "self-neighbour-xyzt"])
@pytest.mark.parametrize("which", ["links", "hat"])
def test_single_matrices_on_full_fields(hier, which, mask):
    """each matrix of a site on its own (hopDir, localTerm): a forward / backward mix-up, invisible in the sum at extent 2, shows here"""
    h = hier
    h.qa.lib().qudaAmdSetPartitionMask(mask)
    try:
        for d in range(9):
            got = h.mg.coarse_apply(0, which, 1 << d, h.v[1])
            check(got, cr.apply(links_of(h, which), h.v[1], h.Xc, 1 << d), (which, d))
        assert not np.any(h.mg.coarse_apply(0, which, 1 << 3, h.v[ZERO]))
    finally:
        h.qa.lib().qudaAmdSetPartitionMask(0)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# the Schur pieces
# ---------------------------------------------------------------------------------------------------------------------------------------------
def schur_reference(h, p, x, b, dtype=np.complex128):
    """M x_p, prepare(b), reconstruct(x_p, b) from the device's links and preconditioned links"""
    par = (cr.parity_of_sites(h.Xc) == p).reshape(-1, 1, 1)
    xp = np.where(par, x, 0)
    return (cr.matpc(h.L, xp, h.Xc, p, hatlinks=h.H, dtype=dtype), cr.prepare(h.L, b, h.Xc, p, hatlinks=h.H, dtype=dtype),
            cr.reconstruct(h.L, xp, b, h.Xc, p, hatlinks=h.H, dtype=dtype))


def schur_tolerance(h, p, x, b):
    """four times the worst relative deviation of the same compositions in numpy complex64 from complex128, never less than the single-kernel figure"""
    dev = max(rel(a, w) for a, w in zip(schur_reference(h, p, x, b, np.complex64), schur_reference(h, p, x, b)))
    return max(TOL, 4 * dev), dev


@pytest.mark.parametrize("p", [0, 1], ids=["matpc-even", "matpc-odd"])
def test_schur_pieces(hier, p):
    """M, prepare and reconstruct of DiracCoarsePC (impl 0) and of BlockCoarseCycle on block fields (impl 1: 8 columns, 24 in case b) against the
    reference, and so against each other.  impl 1 runs with every work field preloaded with nonzero words on both parities — also the half of
    matpc's temporary that used to be trusted to "stay zero from its creation", which matpc now clears (its second application multiplies
    those words with Xinv and adds them to M); that half is zero afterwards and the absent parity of every output is exactly zero.  Tolerance: each piece chains up to three applications — four times the deviation of the same composition in numpy complex64
    from complex128, at least 2e-5.  MEASURED complex64 deviation (cases a / b / c, worse matpc): 1.8e-07 / 3.8e-07 / 3.4e-07, so the bar is 2e-5 everywhere;
    device on an MI355X: DiracCoarsePC at most 2.5e-07, block fields at most 4.7e-07."""
    h = hier
    q = 1 - p
    x, b = h.v[0], h.v[1]
    tol, dev = schur_tolerance(h, p, x, b)
    wM, wP, wR = schur_reference(h, p, x, b)
    gM, _ = h.mg.coarse_pc(0, 0, "M", p, x=cr.half(x, p))
    gP, _ = h.mg.coarse_pc(0, 0, "prepare", p, b=b)
    gR, _ = h.mg.coarse_pc(0, 0, "reconstruct", p, x=cr.half(x, p), b=b)
    worst0 = max(check(gM, wM, ("M", p), tol), check(gP, wP, ("prepare", p), tol), check(gR, wR, ("reconstruct", p), tol))
    assert not np.any(cr.half(gM, q)) and not np.any(cr.half(gP, q))
    zero = np.zeros_like(x)
    for op, kw in (("M", dict(x=cr.half(zero, p))), ("prepare", dict(b=zero)), ("reconstruct", dict(x=cr.half(zero, p), b=zero))):
        assert not np.any(h.mg.coarse_pc(0, 0, op, p, **kw)[0]), op
    worst1 = 0.0
    for nrhs in ((8, 24) if h.n == 48 else (8,)):
        B = h.blocks[nrhs]
        Xs = B[::-1]   # the solved parity of another column order: x and b are unrelated
        xh = np.ascontiguousarray(Xs[:, p * h.Vh:(p + 1) * h.Vh])
        wants = [schur_reference(h, p, Xs[k], B[k]) for k in range(nrhs)]
        for j, (op, kw) in enumerate((("M", dict(x=xh)), ("prepare", dict(b=B)), ("reconstruct", dict(x=xh, b=B)))):
            got, leaked = h.mg.coarse_pc(0, 1, op, p, **kw)
            assert leaked == 0, (op, nrhs, leaked)
            if op != "reconstruct":
                assert not np.any(got[:, q * h.Vh:(q + 1) * h.Vh]), (op, nrhs)
            for k in range(nrhs):
                worst1 = max(worst1, check(got[k], wants[k][j], (op, nrhs, k), tol))
    print("matpc %d: complex64 numpy deviation %.2e -> tolerance %.2e; device worst rel: DiracCoarsePC %.2e, block fields %.2e" % (p, dev, tol, worst0, worst1))


# ---------------------------------------------------------------------------------------------------------------------------------------------
# the fp16 mirror of the links and of the preconditioned links
# ---------------------------------------------------------------------------------------------------------------------------------------------
def test_fp16_mirror(hier):
    """coarse_apply_kernel<64, true>: after set_half_storage(True) the mirrors are the fp32 matrices rounded through fp16 bit for bit (and the
    rounded preconditioned links are finite), Dslash, CloverInv and M of DiracCoarsePC follow the reference evaluated with the ROUNDED matrices
    to 2e-5 and differ from the fp32 results; afterwards the fp32 results are back bit for bit."""
    h = hier
    p = 0
    src = cr.half(h.v[0], 1)

    def run():
        return (h.mg.coarse_apply(0, "hat", cr.HOPS, src, parity=p), h.mg.coarse_apply(0, "hat", cr.LOCAL, cr.half(h.v[0], p), parity=p),
                h.mg.coarse_pc(0, 0, "M", p, x=cr.half(h.v[0], p))[0])

    fp32 = run()
    h.mg.set_half_storage(True)
    try:
        L16, H16 = h.mg.coarse_site_links(0, "links16"), h.mg.coarse_site_links(0, "hat16")
        got = run()
    finally:
        h.mg.set_half_storage(False)
    for m16, m32 in ((L16, h.L), (H16, h.H)):
        assert np.array_equal(m16.real, m32.real.astype(np.float16).astype(np.float32)) and np.array_equal(m16.imag, m32.imag.astype(np.float16).astype(np.float32))
    assert np.all(np.isfinite(H16.real)) and np.all(np.isfinite(H16.imag))
    H16r = cr.round16(h.H)
    assert np.array_equal(H16r, H16.astype(np.complex128))
    xp = cr.embed(cr.half(h.v[0], p), p, h.Xc)
    want = (cr.half(cr.apply(H16r, cr.embed(src, 1, h.Xc), h.Xc, cr.HOPS, p), p), cr.half(cr.apply(H16r, xp, h.Xc, cr.LOCAL, p), p),
            cr.matpc(h.L, xp, h.Xc, p, hatlinks=H16r))
    for name, g, w, f in zip(("Dslash", "CloverInv", "M"), got, want, fp32):
        r = check(g, w, name)
        print("fp16 mirror %s: rel %.2e against the rounded matrices, %.2e away from the fp32 result" % (name, r, rel(g, f)))
        assert not np.array_equal(g, f), name
    for g, f in zip(run(), fp32):
        assert np.array_equal(g, f)
