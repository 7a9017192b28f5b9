"""Self-test of tests/fine_stencil_ref.py (no GPU; the oracle only).  On the 8 x 4 x 6 x 10 lattice, whose four extents differ:

  * the reference's own hop sum reproduces oracle.wil_dslash, so the term sums stand on pinned neighbours, daggers and projectors;
  * one launch per parity reproduces the full operators oracle.tm_mat (s0 = 1, a0 = 2 kappa mu, k1 = -kappa, a1 = 0) and, with the direct
    site matrices on `same`, oracle.tmc_mat, to 1e-13; the two-launch Schur compositions of the multi-source smoother
    (csrc/block_fine_smoother.cpp BlockFineSmoother::matpc) reproduce oracle.tmc_matpc and oracle.tm_matpc to 1e-12;
  * the bound constants: the oracle's fp32 variants (qo_wil_dslash_f, qo_apply_clover_f) and float32 numpy stand in for the device on every
    coefficient case and kind of links of tests/test_fine_stencil_gpu.py; twice the worst |err| / (2^-24 T), rounded up, must not exceed
    K_PLAIN / K_SITE, and those must not exceed the caps 24 / 40.  The ratios are printed (pytest -s);
  * every planted error is rejected by the checker at those constants: the antiperiodic sign dropped on one slice, a0 and a1 swapped, the sign
    of a1 flipped on the lower chirality only, the site matrix transposed, the site matrix or the links of the other parity, one backward
    hop's link not daggered, two right-hand sides exchanged, y and z exchanged in the index of one face of the ghost zone, and one element
    off by a few roundings more than allowed."""
import math

import numpy as np
import pytest

import blas_ref as R
import block_ref as B
import fine_stencil_ref as F
from synth import smooth_gauge

X = (8, 4, 6, 10)
VH = int(np.prod(X)) // 2
KAPPA, MU = F.KAPPA, 0.05
NRHS, ZERO_COL = 8, 2
LINKS = {"recon 18 periodic": (18, False), "recon 18 antiperiodic": (18, True), "recon 12 antiperiodic": (12, True)}
f32 = np.float32


@pytest.fixture(scope="module")
def env(oracle):
    """per kind of links: the links as an fp32 device field holds them, the clover term of those links rounded to fp32 (what a device field
    of fp32 holds), the fp64 site matrices of both parities, operands, and the reference of every case and parity; never modified"""
    oracle.set_threads(8)
    try:
        rng = np.random.default_rng(50)
        cols = {(k, p): B.operand(rng, VH, 12, NRHS, k=2 * k + p, zero_col=ZERO_COL) for k in (0, 1) for p in (0, 1)}      # k 0: same, 1: other
        out = {"oracle": oracle, "cols": cols}
        smooth = smooth_gauge(X, 0.35)
        for name, (recon, anti) in LINKS.items():
            links = F.device_links(F.fold_antiperiodic(smooth, X) if anti else smooth, X, recon, anti)
            clover = oracle.clover_compute(links, F.CSW_COEFF, list(X)).astype(f32).astype(np.float64)
            e = {"links": links, "clover": clover, "ref": {}}
            e["mats"] = {(p, inv): F.dense_matrices(oracle, clover, X, p, F.A_SITE, inv) for p in (0, 1) for inv in (False, True)}
            for p in (0, 1):
                hop, hop_t = F.hop_sum(oracle, links, X, p, cols[1, 1 - p])
                same = F.to_complex(cols[0, p], VH)
                for c, (cname, s0, a0, k1, a1, tmode, inv) in enumerate(F.CASES):
                    e["ref"][c, p] = F.combine(same if s0 else None, hop, hop_t, s0, a0, k1, a1, tmode, e["mats"][p, inv] if tmode else None)
            out[name] = e
        return out
    finally:
        oracle.set_threads(1)


# ---- the stand-in for the device: fp32 oracle for the hop sum and A, float32 numpy for the rest ----
def _dagger(block):
    """[x][3][3][2] -> its Hermitian conjugate"""
    d = block.transpose(0, 2, 1, 3).copy()
    d[..., 1] *= -1
    return d


def stand_in(env, name, c, p, bug=None):
    """what fine_block_kernel computes for case c on parity p, in fp32: [rhs][Vh * 24] float64 of float32 values"""
    oracle, e = env["oracle"], env[name]
    cname, s0, a0, k1, a1, tmode, inv = F.CASES[c]
    if bug == "a0 and a1 swapped":
        a0, a1 = a1, a0
    g = e["links"].astype(f32).reshape(4, 2, VH, 3, 3, 2).copy()
    last = VH - VH // X[3]
    if bug == "sign dropped on one slice":      # the forward t hops out of the last time slice
        g[3, p, last:] *= -1
    if bug == "links of the other parity":
        g = g[:, ::-1].copy()
    if bug == "backward link not daggered":     # the -y hops read the links of the other parity
        g[1, 1 - p] = _dagger(g[1, 1 - p])
    other = env["cols"][1, 1 - p].astype(f32)
    same = env["cols"][0, p].astype(f32)
    lat = [int(v) for v in X]

    def hops(links, field):
        links = np.ascontiguousarray(links.reshape(4, -1))
        return np.stack([oracle.wil_dslash(links, np.ascontiguousarray(col), lat, p, 0) for col in field])

    if bug == "y and z exchanged in the t face":
        # the +t hops of the last slice read the ghost zone by the face index (z Y + y) Xh + xh, which on the t face is the checkerboard index
        # within the first slice; with (y Z + z) Xh + xh they get another site's panel
        x, y, z, t = F.coordinates(X, p)
        face = np.nonzero(t == X[3] - 1)[0]
        xh = x[face] // 2
        right, wrong = (z[face] * X[1] + y[face]) * (X[0] // 2) + xh, (y[face] * X[2] + z[face]) * (X[0] // 2) + xh
        assert np.array_equal(right, F.neighbours(X, p)[6][face]) and np.any(right != wrong) and sorted(wrong) == sorted(right)
        rest, only = g.copy(), np.zeros_like(g)
        only[3, p, last:] = g[3, p, last:]
        rest[3, p, last:] = 0
        moved = other.reshape(NRHS, VH, 24).copy()
        moved[:, right] = other.reshape(NRHS, VH, 24)[:, wrong]
        hop = hops(rest, other) + hops(only, moved.reshape(NRHS, -1))
    else:
        hop = hops(g, other)
    assert hop.dtype == f32
    hop, same5 = hop.reshape(NRHS, VH, 4, 3, 2), same.reshape(NRHS, VH, 4, 3, 2)
    g5 = np.array([1, 1, -1, -1], dtype=f32)[None, None, :, None]

    def twist(v, a, sign=g5):
        a5 = f32(a) * sign
        return np.stack([v[..., 0] - a5 * v[..., 1], v[..., 1] + a5 * v[..., 0]], axis=-1)

    mats = e["mats"][(1 - p) if bug == "site matrix of the other parity" else p, inv] if tmode else None
    if tmode == 1:
        m = mats.astype(np.complex64)
        if bug == "site matrix transposed":
            m = m.transpose(0, 1, 3, 2)
        h = np.ascontiguousarray(hop).view(np.complex64).reshape(NRHS, VH, 2, 6)
        res = np.einsum("xcij,nxcj->nxci", m, h)
        out = f32(k1) * np.ascontiguousarray(res).view(f32).reshape(hop.shape)
    else:
        out = f32(k1) * twist(hop, a1, np.ones_like(g5) if bug == "a1 with one sign for both chiralities" else g5)
    if s0 != 0.0:
        if tmode == 2:
            par = (1 - p) if bug == "site matrix of the other parity" else p
            cl = e["clover"].astype(f32)
            a_same = np.stack([oracle.apply_clover(cl, np.ascontiguousarray(col), lat, par) for col in same]).reshape(same5.shape)
            a5 = f32(F.A_SITE) * g5
            res = np.stack([a_same[..., 0] - a5 * same5[..., 1], a_same[..., 1] + a5 * same5[..., 0]], axis=-1)
            out = out + f32(s0) * res
        else:
            out = out + f32(s0) * twist(same5, a0)
    assert out.dtype == f32
    out = out.reshape(NRHS, -1).astype(np.float64)
    if bug == "two right-hand sides exchanged":
        out[[0, 1]] = out[[1, 0]]
    return out


def k_of(c):
    return F.K_SITE if F.CASES[c][5] else F.K_PLAIN


# ---- the reference against the oracle's operators ----
def test_own_hop_sum_is_the_oracles(env):
    e, oracle = env["recon 12 antiperiodic"], env["oracle"]
    for p in (0, 1):
        other = env["cols"][1, 1 - p]
        want, _ = F.hop_sum(oracle, e["links"], X, p, other)
        got = F.hop_terms(e["links"], X, p, F.to_complex(other, VH))
        assert np.max(np.abs(got - want)) <= 1e-13 * np.max(np.abs(want))
        t = F.hop_terms(e["links"], X, p, F.to_complex(other, VH), absolute=True)
        assert np.all(t.real >= np.abs(want.real) * (1 - 1e-12)) and np.all(t.imag >= np.abs(want.imag) * (1 - 1e-12))
        assert not np.any(F.to_real(t)[ZERO_COL])


def test_neighbour_table_is_the_oracles(oracle):
    for p in (0, 1):
        nb = F.neighbours(X, p)
        for i in (0, 3, 17, 475, VH - 1):
            for d in range(8):
                dx = [0, 0, 0, 0]
                dx[3 - d // 2] = 1 if d % 2 == 0 else -1
                assert nb[d][i] == oracle.neighbor_index(list(X), i, p, *dx), (p, i, d)


@pytest.fixture(scope="module")
def full(oracle):
    rng = np.random.default_rng(51)
    gauge = F.fold_antiperiodic(smooth_gauge(X, 0.35), X)
    clover = oracle.clover_compute(gauge, F.CSW_COEFF, list(X))
    return gauge, clover, rng.standard_normal(2 * VH * 24)


@pytest.mark.parametrize("flavor", [+1, -1])
def test_two_launches_are_the_full_operators(oracle, full, flavor):
    gauge, clover, v = full
    a = 2 * KAPPA * MU * flavor
    half = [v[:VH * 24][None], v[VH * 24:][None]]
    for name, want in (("tm", oracle.tm_mat(gauge, v.copy(), list(X), KAPPA, MU, flavor, 0)), ("tmc", oracle.tmc_mat(gauge, clover, v.copy(), list(X), KAPPA, MU, flavor, 0))):
        for p in (0, 1):
            if name == "tm":
                got, _ = F.parity_launch(oracle, gauge, X, p, half[p], half[1 - p], 1.0, a, -KAPPA, 0.0)
            else:
                got, _ = F.parity_launch(oracle, gauge, X, p, half[p], half[1 - p], 1.0, 0.0, -KAPPA, 0.0, 2, F.dense_matrices(oracle, clover, X, p, a, False))
            err = np.max(np.abs(got[0] - want[p * VH * 24:(p + 1) * VH * 24])) / np.max(np.abs(want))
            print("FINE-REF %s flavor %+d parity %d: %.2e of the largest element" % (name, flavor, p, err))
            assert err <= 1e-13, (name, p, err)


@pytest.mark.parametrize("matpc,p", [("ee", 0), ("oo", 1)])
def test_schur_compositions_are_the_preconditioned_operators(oracle, full, matpc, p):
    """the two launches of BlockFineSmoother::matpc: out = in - kappa^2 M_p H M_q H in with M = (A + i a g5)^-1 as site matrices (mode 1),
    resp. M = (1 + i a g5)^-1 = binv (1 - i a g5) through k1 = binv, a1 = -a"""
    gauge, clover, v = full
    q, a = 1 - p, 2 * KAPPA * MU
    inp = v[:VH * 24][None]
    m = {r: F.dense_matrices(oracle, clover, X, r, a, True) for r in (0, 1)}
    tmp, _ = F.parity_launch(oracle, gauge, X, q, None, inp, 0.0, 0.0, 1.0, 0.0, 1, m[q])
    got, _ = F.parity_launch(oracle, gauge, X, p, inp, tmp, 1.0, 0.0, -KAPPA * KAPPA, 0.0, 1, m[p])
    cinv = oracle.clover_twisted_inverse(clover, 4 * KAPPA * KAPPA * MU * MU)
    want = oracle.tmc_matpc(gauge, inp[0].copy(), clover, cinv, list(X), KAPPA, MU, +1, matpc, 0)
    err = np.max(np.abs(got[0] - want)) / np.max(np.abs(want))
    print("FINE-REF tmc_matpc %s: %.2e" % (matpc, err))
    assert err <= 1e-12
    binv = 1.0 / (1.0 + a * a)
    tmp, _ = F.parity_launch(oracle, gauge, X, q, None, inp, 0.0, 0.0, binv, -a)
    got, _ = F.parity_launch(oracle, gauge, X, p, inp, tmp, 1.0, 0.0, -KAPPA * KAPPA * binv, -a)
    want = oracle.tm_matpc(gauge, inp[0].copy(), list(X), KAPPA, MU, +1, matpc, 0)
    err = np.max(np.abs(got[0] - want)) / np.max(np.abs(want))
    print("FINE-REF tm_matpc %s: %.2e" % (matpc, err))
    assert err <= 1e-12


def test_dense_reference_is_the_oracles_clover_term(oracle, full):
    """M v with the direct matrices is apply_clover v + i a g5 v on a random field, and the inverse times the direct matrix is 1"""
    gauge, clover, v = full
    for p in (0, 1):
        m, mi = (F.dense_matrices(oracle, clover, X, p, 0.3, inv) for inv in (False, True))
        assert np.max(np.abs(np.einsum("xcij,xcjk->xcik", m, mi) - np.eye(6))) < 1e-13
        assert np.max(np.abs(m[:, 0] - m[:, 0].conj().transpose(0, 2, 1) - 0.6j * np.eye(6))) == 0.0        # A Hermitian, + i a on the upper chirality
        assert np.max(np.abs(m[:, 1] - m[:, 1].conj().transpose(0, 2, 1) + 0.6j * np.eye(6))) == 0.0
        col = v[p * VH * 24:(p + 1) * VH * 24]
        want = F.to_complex(oracle.apply_clover(clover, col.copy(), list(X), p)[None], VH) + 0.3j * F.G5[None, None, :, None] * F.to_complex(col[None], VH)
        got = F._site(m, F.to_complex(col[None], VH), False)
        assert np.max(np.abs(got - want)) <= 1e-14 * np.max(np.abs(want))


# ---- the bound constants ----
def test_bound_constants_hold_twice_the_fp32_stand_in(env):
    worst = {False: 0.0, True: 0.0}
    for name in LINKS:
        for c, case in enumerate(F.CASES):
            for p in (0, 1):
                want, t = env[name]["ref"][c, p]
                got = stand_in(env, name, c, p)
                assert np.any(got[0]) and not np.any(got[ZERO_COL])
                rec = F.check_launch("%s | %s | parity %d" % (name, case[0], p), got, want, t, k_of(c))
                print("FINE-REF fp32 stand-in | %-60s | worst error %.3e = %.3f x 2^-24 T" % (rec[0], rec[1], rec[3]))
                worst[bool(case[5])] = max(worst[bool(case[5])], rec[3])
    print("FINE-REF worst ratio without site matrices %.3f (K_PLAIN %d), with site matrices %.3f (K_SITE %d)" % (worst[False], F.K_PLAIN, worst[True], F.K_SITE))
    assert math.ceil(2 * worst[False]) <= F.K_PLAIN <= F.K_CAP_PLAIN == 24
    assert math.ceil(2 * worst[True]) <= F.K_SITE <= F.K_CAP_SITE == 40


# ---- planted errors ----
PLANTED = [("sign dropped on one slice", 1, "recon 18 antiperiodic"), ("sign dropped on one slice", 3, "recon 12 antiperiodic"),
           ("a0 and a1 swapped", 1, "recon 18 periodic"), ("a1 with one sign for both chiralities", 1, "recon 18 periodic"),
           ("a1 with one sign for both chiralities", 5, "recon 18 periodic"),
           ("site matrix transposed", 3, "recon 18 periodic"), ("site matrix transposed", 4, "recon 12 antiperiodic"),
           ("site matrix of the other parity", 3, "recon 18 periodic"), ("site matrix of the other parity", 4, "recon 18 periodic"),
           ("site matrix of the other parity", 5, "recon 18 periodic"),
           ("links of the other parity", 0, "recon 18 periodic"), ("links of the other parity", 4, "recon 12 antiperiodic"),
           ("backward link not daggered", 0, "recon 18 periodic"), ("backward link not daggered", 1, "recon 12 antiperiodic"),
           ("two right-hand sides exchanged", 1, "recon 18 periodic"), ("two right-hand sides exchanged", 3, "recon 18 periodic"),
           ("y and z exchanged in the t face", 0, "recon 18 periodic"), ("y and z exchanged in the t face", 1, "recon 12 antiperiodic"),
           ("y and z exchanged in the t face", 4, "recon 18 antiperiodic")]


@pytest.mark.parametrize("p", [0, 1])
@pytest.mark.parametrize("bug,c,name", PLANTED, ids=lambda v: str(v))
def test_planted_errors_are_rejected(env, bug, c, name, p):
    want, t = env[name]["ref"][c, p]
    F.check_launch("unharmed", stand_in(env, name, c, p), want, t, k_of(c))
    with pytest.raises(R.Mismatch):
        F.check_launch(bug, stand_in(env, name, c, p, bug), want, t, k_of(c))


@pytest.mark.parametrize("c", range(len(F.CASES)))
def test_one_element_off_by_more_than_the_bound_is_rejected(env, c):
    want, t = env["recon 18 periodic"]["ref"][c, 1]
    got = stand_in(env, "recon 18 periodic", c, 1)
    i = 5 * VH * 24 + 77 * 24 + 13
    assert t[5, 77 * 24 + 13] > 0
    got.reshape(-1)[i] = want.reshape(-1)[i] + (k_of(c) + 0.5) * F.EPS32 * t.reshape(-1)[i]
    with pytest.raises(R.Mismatch):
        F.check_launch("one element", got, want, t, k_of(c))
    got[ZERO_COL, 40] = 1e-30
    with pytest.raises(R.Mismatch):
        F.check_launch("zero column", got, want, t, 1e9)


def test_dense_checker(env, oracle):
    e = env["recon 18 periodic"]
    for inv in (False, True):
        want = e["mats"][0, inv]
        got = want.astype(np.complex64)
        F.check_dense("dense", got, want, inv)
        bad = got.copy()
        bad[5, 1, 2, 3] = np.nextafter(bad[5, 1, 2, 3].real, f32(9)) + 1j * bad[5, 1, 2, 3].imag
        if not inv:
            with pytest.raises(R.Mismatch):
                F.check_dense("dense, one ulp", bad, want, inv)
        bad[5, 1, 2, 3] *= f32(1 + 3e-7)
        with pytest.raises(R.Mismatch):
            F.check_dense("dense, five ulps", bad, want, inv)
        with pytest.raises(R.Mismatch):
            F.check_dense("dense, transposed", np.ascontiguousarray(got.transpose(0, 1, 3, 2)), want, inv)
        with pytest.raises(R.Mismatch):
            F.check_dense("dense, other chirality's sign", np.ascontiguousarray(got[:, ::-1]), want, inv)
