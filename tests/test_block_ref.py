"""Self-test of tests/block_ref.py (no GPU, no library): the checker must accept a correct fp32 evaluation of every operation of namespace
blockblas, of the minimal-residual updates and of the epilogue sums, in both layouts, and must reject "kernel outputs" with the errors the
lockstep solvers forgive: a flipped imaginary sign of ONE column's coefficient, the coefficient of column i + 1 used for column i, the two
halves of a pair-major word given to two right-hand sides, rho from the residual before the update, bicgstabFused with p built from the old
r, a1 of the paired MR step with (w2, r) not conjugated, an update that writes r although no residual was asked for, an epilogue sum that
includes a tail site, one element off by 100 roundings.  The evaluations here work on the DEVICE image with numpy's complex64, independently
of the term-by-term code of the reference; the paired MR step is evaluated the way mr2_update_kernel does it, by the expansion in the sums."""
import numpy as np
import pytest

import blas_ref as R
import block_ref as B

SHAPES = [(16, 16, 8), (10, 12, 8), (10, 12, 4)]       # (sites, components, right-hand sides): rhs-fastest, pair-major, pair-major
OMEGA = 0.85


def fields(seed, op_names, shape, zero_col=2):
    rng = np.random.default_rng(seed)
    return {n: B.operand(rng, *shape, k=k, zero_col=zero_col) for k, n in enumerate(op_names)}


def coeffs(op, nrhs):
    return [B.coefficients(nrhs, k, converged=1) for k in range(B.NCOEFF.get(op, 0))]


def word_rhs(shape):
    """right-hand side of every complex number of the device image, in image order"""
    ns, nc, nr = shape
    owner = np.empty(ns * nc * nr, dtype=np.int64)
    owner[B.device_index(ns, nc, nr)] = np.arange(nr)[:, None]
    return owner


def simulate(op, co, f, shape, bug=None):
    """blockblas::<op> in complex64 on the device images; returns (after as [rhs][reals], sums [sum][rhs])"""
    ns, nc, nr = shape
    owner = word_rhs(shape)
    if bug == "split word":        # the pair-major word treated as rhs-fastest: its halves go to right-hand sides 2 pr, 2 pr + 1
        q = np.arange(owner.size) // 2
        owner = 2 * (q % (nr // 2)) + np.arange(owner.size) % 2
    img = {n: B.to_device(f[n], *shape).view(np.complex64).copy() for n in f}

    def coef(c):
        c = np.array(c, dtype=np.complex64)
        if bug == "imag sign":
            c[3] = np.conj(c[3])
        if bug == "neighbour":
            c = np.roll(c, -1)
        return c[owner]

    def norm(v):
        w = v.view(np.float32).astype(np.float64)
        return [float(np.sum((w * w).reshape(-1, 2)[owner == i])) for i in range(nr)]

    def cdot(p, q):
        d = np.conj(p.astype(np.complex128)) * q.astype(np.complex128)
        return [[float(np.sum(d[owner == i].real)) for i in range(nr)], [float(np.sum(d[owner == i].imag)) for i in range(nr)]]

    g = img
    sums = []
    if op == "norm2":
        sums = [norm(g["x"])]
    elif op == "cDot":
        sums = cdot(g["x"], g["y"])
    elif op == "caxpy":
        g["y"] += coef(co[0]) * g["x"]
    elif op == "cDotNormA":
        sums = cdot(g["t"], g["r"]) + [norm(g["t"])]
    elif op == "bicgstabUpdate":
        a, w = coef(co[0]), coef(co[1])
        old = g["r"].copy()
        g["x"] += a * g["p"] + w * g["r"]
        g["r"] -= w * g["t"]
        sums = cdot(g["r0"], old if bug == "old rho" else g["r"]) + [norm(g["r"])]
    elif op == "cxpaypbz":
        g["p"][:] = g["r"] + coef(co[0]) * g["v"] + coef(co[1]) * g["p"]
    elif op == "bicgstabDots":
        sums = cdot(g["t"], g["s"]) + [norm(g["t"])] + cdot(g["r0"], g["s"]) + cdot(g["r0"], g["t"])
    elif op == "bicgstabFused":
        a, w, b = coef(co[0]), coef(co[1]), coef(co[2])
        old = g["r"].copy()
        g["x"] += a * g["p"] + w * g["r"]
        g["r"] -= w * g["t"]
        g["p"][:] = (old if bug == "old r" else g["r"]) + b * (g["p"] - w * g["v"])
        sums = [norm(g["r"])]
    elif op == "xmy":
        g["y"][:] = g["x"] - g["y"]
    elif op == "negate":
        g["x"][:] = -g["x"]
    elif op == "copy":
        g["dst"][:] = g["src"]
    elif op == "zero":
        g["x"][:] = 0
    else:
        raise ValueError(op)
    return {n: B.from_device(g[n].view(np.float32), *shape) for n in g}, np.array(sums).reshape(-1, nr)


@pytest.mark.parametrize("shape", SHAPES)
def test_layout_maps_are_permutations_and_inverse(shape):
    ns, nc, nr = shape
    idx = B.device_index(*shape)
    assert sorted(idx.reshape(-1)) == list(range(ns * nc * nr))
    v = fields(1, "x", shape)["x"]
    assert np.array_equal(B.from_device(B.to_device(v, *shape), *shape), v)
    if nc == 12:       # the 16-byte word (x 6 + k) nrhs + i holds components 2k, 2k + 1 of right-hand side i
        assert idx[3, 7 * 12 + 2 * 4] == ((7 * 6 + 4) * nr + 3) * 2 and idx[3, 7 * 12 + 2 * 4 + 1] == ((7 * 6 + 4) * nr + 3) * 2 + 1
    else:
        assert idx[3, 7 * nc + 5] == (7 * nc + 5) * nr + 3


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("op", sorted(B.OPERANDS))
def test_correct_evaluations_are_accepted(op, shape):
    f = fields(5, B.OPERANDS[op], shape)
    co = coeffs(op, shape[2])
    after, sums = simulate(op, co, f, shape)
    for rec in B.check(op, co, f, after, sums):
        print("%-44s error %.3e bound %.3e ratio %.3f" % rec)


PLANTED = [("caxpy", "imag sign"), ("bicgstabUpdate", "imag sign"), ("cxpaypbz", "imag sign"), ("bicgstabFused", "imag sign"),
           ("caxpy", "neighbour"), ("bicgstabUpdate", "neighbour"), ("cxpaypbz", "neighbour"), ("bicgstabFused", "neighbour"),
           ("bicgstabUpdate", "old rho"), ("bicgstabFused", "old r")]


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("op,bug", PLANTED)
def test_planted_errors_are_rejected(op, bug, shape):
    f = fields(6, B.OPERANDS[op], shape)
    co = coeffs(op, shape[2])
    after, sums = simulate(op, co, f, shape, bug)
    with pytest.raises(R.Mismatch):
        B.check(op, co, f, after, sums)


@pytest.mark.parametrize("shape", SHAPES[1:])
@pytest.mark.parametrize("op", ["caxpy", "cDot", "norm2", "bicgstabFused"])
def test_pair_major_word_split_between_two_right_hand_sides_is_rejected(op, shape):
    f = fields(7, B.OPERANDS[op], shape)
    co = coeffs(op, shape[2])
    after, sums = simulate(op, co, f, shape, "split word")
    with pytest.raises(R.Mismatch):
        B.check(op, co, f, after, sums)


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("op", ["caxpy", "bicgstabUpdate", "cxpaypbz", "bicgstabFused", "xmy"])
def test_one_element_off_by_a_hundred_roundings_is_rejected(op, shape):
    f = fields(8, B.OPERANDS[op], shape)
    co = coeffs(op, shape[2])
    after, sums = simulate(op, co, f, shape)
    ref = B.reference(op, co, f)
    name = sorted(ref.written)[0]
    i = 5 * 2 * shape[1] + 3
    after[name][3, i] += 100 * 2.0 ** -24 * float(ref.written[name][1][3, i])
    with pytest.raises(R.Mismatch):
        B.check(op, co, f, after, sums)


def test_changed_read_only_operand_is_rejected():
    shape = SHAPES[1]
    f = fields(9, B.OPERANDS["bicgstabDots"], shape)
    after, sums = simulate("bicgstabDots", [], f, shape)
    after["r0"][1, 40] = np.nextafter(after["r0"][1, 40], 1.0)
    with pytest.raises(R.Mismatch):
        B.check("bicgstabDots", [], f, after, sums)


# ---- minimal residual ----
def mr_fields(seed, shape, steps):
    return B.mr_operands(np.random.default_rng(seed), shape, steps)


def simulate_mr(steps, omega, fresh, need_r, f, s3, s7, bug=None):
    """the update kernels in numpy: coefficients in fp64 from the SUMS (mr2: by the expansion), cast to fp32, then complex64 arithmetic"""
    c64 = lambda v: v.astype(np.float32).view(np.complex64)
    x, rin, w1 = c64(f["x"]), c64(f["rin"]), c64(f["w1"])
    w2 = c64(f["w2"]) if steps == 2 else None
    x = np.zeros_like(x) if fresh else x.copy()
    r = c64(f["r"]).copy()
    for i in range(rin.shape[0]):
        c, n1 = complex(s3[0, i], s3[1, i]), s3[2, i]
        if steps == 1:
            al = np.complex64(np.float32(omega) * c / n1) if n1 > 0 else np.complex64(0)
            x[i] += al * rin[i]
            if need_r or bug == "writes r":
                r[i] = rin[i] - al * w1[i]
            continue
        d, n2, e = complex(s7[0, i], s7[1, i]), s7[2, i], complex(s7[5, i], s7[6, i])
        a0 = omega * c / n1 if n1 > 0 else 0j
        w2r = e if bug == "not conjugated" else np.conj(e)
        num = c - a0 * n1 - np.conj(a0) * w2r + abs(a0) ** 2 * d
        den = n1 - 2.0 * (np.conj(a0) * d).real + abs(a0) ** 2 * n2
        a1 = omega * num / den if den > 0 else 0j
        cs, cp = np.complex64(a0 + a1), np.complex64(a0 * a1)
        x[i] += cs * rin[i] - cp * w1[i]
        if need_r or bug == "writes r":
            r[i] = rin[i] - cs * w1[i] + cp * w2[i]
    after = dict(f)
    after["x"], after["r"] = x.view(np.float32).astype(np.float64), r.view(np.float32).astype(np.float64)
    return after


@pytest.mark.parametrize("shape", SHAPES[1:])
@pytest.mark.parametrize("need_r", [0, 1])
@pytest.mark.parametrize("fresh", [0, 1])
@pytest.mark.parametrize("steps", [1, 2])
def test_mr_updates_are_accepted_and_well_conditioned(steps, fresh, need_r, shape):
    f = mr_fields(20, shape, steps)
    s3, s7 = B.mr_sums(f["rin"], f["w1"], f.get("w2"))
    assert not np.any(s3[:, 2]) and np.all(s3[2, [0, 1, 3]] > 0)          # the zero column has zero sums
    if steps == 2:
        for kn, kd in B.mr_condition(OMEGA, s3, s7):
            assert kn < B.MR_KAPPA_LIMIT and kd < B.MR_KAPPA_LIMIT, (kn, kd)
            assert kn < 1e3 and kd < 1e3, (kn, kd)      # in fact by many orders of magnitude
    after = simulate_mr(steps, OMEGA, fresh, need_r, f, s3, s7)
    for rec in B.check_mr(steps, OMEGA, fresh, need_r, f, after):
        print("%-44s error %.3e bound %.3e ratio %.3f" % rec)


@pytest.mark.parametrize("shape", SHAPES[1:])
@pytest.mark.parametrize("fresh", [0, 1])
def test_a1_with_w2_r_not_conjugated_is_rejected(fresh, shape):
    f = mr_fields(21, shape, 2)
    s3, s7 = B.mr_sums(f["rin"], f["w1"], f["w2"])
    after = simulate_mr(2, OMEGA, fresh, 1, f, s3, s7, "not conjugated")
    with pytest.raises(R.Mismatch):
        B.check_mr(2, OMEGA, fresh, 1, f, after)


@pytest.mark.parametrize("shape", SHAPES[1:])
@pytest.mark.parametrize("steps", [1, 2])
def test_update_that_writes_r_without_being_asked_is_rejected(steps, shape):
    f = mr_fields(22, shape, steps)
    s3, s7 = B.mr_sums(f["rin"], f["w1"], f.get("w2"))
    after = simulate_mr(steps, OMEGA, 0, 0, f, s3, s7, "writes r")
    with pytest.raises(R.Mismatch):
        B.check_mr(steps, OMEGA, 0, 0, f, after)


def test_mr_condition_sees_a_cancellation():
    """w1 nearly orthogonal to r: the numerator of a0 is small but that of a1 is formed from O(1) terms"""
    s3 = np.array([[1e-9], [0.0], [1.0]])
    s7 = np.array([[0.5], [0.0], [1.0], [1e-9], [0.0], [1.0], [0.0]])
    (kn, kd), = B.mr_condition(1.0, s3, s7)
    assert kn > 1.5 and kd >= 1.0
    s3[0, 0] = 1.0
    s7[5, 0] = 1.0                     # a0 = 1: (A r1, r1) = 1 - 1 - 1 + 0.5 with terms of size 3.5
    (kn, kd), = B.mr_condition(1.0, s3, s7)
    assert abs(kn - 7.0) < 1e-12


# ---- epilogue sums ----
def epilogue_sums(mode, vals, extra_site=None):
    """the kernel's way: 24 products of a site added in fp32, the site sums in fp64; extra_site: that site is counted once more (a tail site
    that the reduction should have left out)"""
    out = []
    nrhs = vals["out"].shape[0]
    for kind in B.EPILOGUE_SUMS[mode]:
        row = []
        for i in range(nrhs):
            terms = np.asarray(R.summands(kind, {n: vals[n][i] for n in kind[1:]}), dtype=np.float64)
            per_site = terms.reshape(2, -1, 12).transpose(1, 0, 2).reshape(-1, 24) if kind[0] != "norm" else terms.reshape(-1, 24)
            site = np.zeros(per_site.shape[0], dtype=np.float32)
            for k in range(24):
                site = (site + per_site[:, k].astype(np.float32)).astype(np.float32)
            tot = float(np.sum(site.astype(np.float64)))
            if extra_site is not None:
                tot += float(site[extra_site])
            row.append(tot)
        out.append(row)
    return np.array(out)


@pytest.mark.parametrize("mode", [1, 2, 3])
def test_epilogue_sums_accepted_and_tail_site_rejected(mode):
    shape = (24, 12, 8)
    rng = np.random.default_rng(30 + mode)
    vals = {n: B.operand(rng, *shape, k=k, zero_col=5) for k, n in enumerate(["out", "same", "a"])}
    vals["out"] = (0.9 * vals["same"] + 0.02 * vals["out"]).astype(np.float32).astype(np.float64)     # out = s0 same + hops: (out, same) does not cancel
    vals["a"] = (0.7 * vals["same"] + 0.05 * vals["a"]).astype(np.float32).astype(np.float64)
    for rec in B.check_epilogue_sums(mode, epilogue_sums(mode, vals), vals):
        print("%-44s error %.3e bound %.3e ratio %.3f" % rec)
    with pytest.raises(R.Mismatch):
        B.check_epilogue_sums(mode, epilogue_sums(mode, vals, extra_site=23), vals)
    with pytest.raises(R.Mismatch):      # sums handed out under the neighbouring right-hand side
        B.check_epilogue_sums(mode, np.roll(epilogue_sums(mode, vals), 1, axis=1), vals)
