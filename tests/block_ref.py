"""High-precision numpy references of the multi-right-hand-side ("block") path: namespace blockblas (include/block.h, csrc/block.hip), the
minimal-residual updates mrUpdateDev / mr2UpdateDev, the layout of a block field and the inner products the fine stencil takes in its
epilogue (include/dslash.h FineBlockDots).  A plain module: no GPU, no library.  Built on the term machinery of tests/blas_ref.py.

A field is a float64 array [rhs][reals of that right-hand side]: site-major, ncomp (re, im) pairs per site — the values READ BACK from the
device through from_device(), so the rounding of the storage format cancels.  device_index() restates the two formulas of block.h:
    rhs-fastest                 float2 index  (x * ncomp + j) * nrhs + i
    pair-major (ncomp == 12)    float2 index  ((x * 6 + j / 2) * nrhs + i) * 2 + j % 2
so a kernel that hands a word to another right-hand side than the header says fails the element checks.

Bounds — from the formulas and the number formats, never from what a kernel returns:
  * elements: |got - want| <= 8 * 2^-24 * T (blas_ref.ROUNDINGS), T the sum of the absolute values of the FULLY EXPANDED terms; nesting
    _cplx / _add produces it.  The deepest chain is p of bicgstabFused, p = r + beta (p - omega v) with r = s - omega t: rounding of omega,
    product, the sum inside omega v, subtraction from p, rounding of beta, product, sum of the two beta products, addition of r: eight.
  * minimal-residual updates: the coefficient is formed in fp64 from the sums and cast to fp32, which counts as its coefficient rounding.
    mrUpdateDev: omega is passed as fp32 (1), alpha cast (1), product (1), the sum inside the complex product (1), the addition (1): five.
    mr2UpdateDev: cast of a0 + a1 resp. a0 a1 (1), product (1), inner sum (1), two additions (2): five; its a1 comes from an expansion in the
    sums that cancels: with kappa = sum |terms| / |result| of its numerator and denominator and at most eight fp64 operations each, a1 is off
    by 8 kappa 2^-53 relative.  mr_condition() returns kappa and the tests assert kappa 2^-53 < 2^-26 for their inputs, so this is below
    2^-23 = two more roundings: seven.  The reference takes the other route — two explicit steps on the vectors — so T holds |a1 a0 w1| etc.
  * sums of blockblas: 1e-13 of the sum of the absolute values of the summands (blas_ref.SUM_REL), the summands from the values the fields
    hold after the kernel: fp32 x fp32 products are exact in fp64 and the accumulation is fp64 (at most ~100 additions deep).
  * epilogue sums of fine_block_kernel: (25 * 2^-24 + 1e-13) of the sum of the absolute values of the summands — the bound of a kernel that
    adds the 24 products of a site in fp32 and only then goes to fp64 (24 sequential fp32 operations per site sum and one for the conversion),
    which is what the kernel did when the bound was set.  It now takes the site sums in fp64 and is far inside it; the check that needs that,
    the MR update fed with these sums against the update fed with longdouble sums, holds it to the element bound."""
import numpy as np

import blas_ref as R

HP = R.HP
EPS32 = R.EPS[4]
EPILOGUE_REL = 25 * EPS32 + R.SUM_REL
MR_KAPPA_LIMIT = 2.0 ** -26 / 2.0 ** -53


# ---- layout ----
def device_index(nsites, ncomp, nrhs):
    """float2 index in the device image of (rhs i, site x, component j), shape (nrhs, nsites * ncomp): the formulas of include/block.h"""
    i = np.arange(nrhs)[:, None, None]
    x = np.arange(nsites)[None, :, None]
    j = np.arange(ncomp)[None, None, :]
    if ncomp == 12:
        idx = ((x * 6 + j // 2) * nrhs + i) * 2 + j % 2
    else:
        idx = (x * ncomp + j) * nrhs + i
    return idx.reshape(nrhs, nsites * ncomp)


def to_device(cols, nsites, ncomp, nrhs, nghost=0):
    """[rhs][reals] -> the float32 device image (ghost panels zero)"""
    img = np.zeros(((nsites + nghost) * ncomp * nrhs, 2), dtype=np.float32)
    img[device_index(nsites, ncomp, nrhs)] = np.asarray(cols).reshape(nrhs, nsites * ncomp, 2)
    return img.reshape(-1)


def from_device(img, nsites, ncomp, nrhs):
    """the float32 device image -> [rhs][reals] in float64"""
    return np.asarray(img).reshape(-1, 2)[device_index(nsites, ncomp, nrhs)].reshape(nrhs, -1).astype(np.float64)


# ---- operands and coefficients of the tests ----
def operand(rng, nsites, ncomp, nrhs, k=0, zero_col=None):
    """normal reals times 10^u per (site, right-hand side), u uniform in [-3, 3]; one zero site per column, a different one in each column and
    for each k; column zero_col identically zero.  Rounded to fp32."""
    v = rng.standard_normal((nrhs, nsites, 2 * ncomp)) * 10.0 ** rng.uniform(-3, 3, (nrhs, nsites, 1))
    for i in range(nrhs):
        v[i, (3 + 5 * i + 11 * k) % nsites] = 0.0
    if zero_col is not None:
        v[zero_col] = 0.0
    return v.reshape(nrhs, -1).astype(np.float32).astype(np.float64)


def coefficients(nrhs, k=0, converged=None):
    """one complex coefficient per column with two nonzero, unequal parts that differ from column to column; column `converged`: zero"""
    c = [complex(0.37 + 0.043 * i + 0.11 * k, -0.61 + 0.029 * i - 0.07 * k) * (-1) ** (i + k) for i in range(nrhs)]
    if converged is not None:
        c[converged] = 0j
    return c


def mr_operands(rng, shape, steps, zero_col=2):
    """x, r, rin, w1 (, w2) of a minimal-residual update as the smoother meets them: w1 = A rin, w2 = A w1 for an A = 0.9 + small, so that no
    coefficient comes from a cancellation; column zero_col is zero in every field (the padding column of block_coarse_cycle.cpp)"""
    f = {n: operand(rng, *shape, k=k, zero_col=zero_col) for k, n in enumerate(["x", "rin", "r"])}
    prev = f["rin"]
    for k, n in enumerate(["w1", "w2"][:steps]):
        pert = np.roll(prev, 2 * (k + 1), axis=1) * np.array([0.21, -0.13] * (prev.shape[1] // 2))
        f[n] = ((0.9 - 0.05 * k) * prev + pert).astype(np.float32).astype(np.float64)
        prev = f[n]
    return f


# ---- terms with one coefficient per right-hand side ----
def _cols(a, t):
    v, T = t
    out = [R._cplx(a[i], (v[i], T[i])) for i in range(len(a))]
    return np.stack([o[0] for o in out]), np.stack([o[1] for o in out])


OPERANDS = {"norm2": ["x"], "cDot": ["x", "y"], "caxpy": ["x", "y"], "cDotNormA": ["t", "r"], "bicgstabUpdate": ["p", "r", "x", "t", "r0"],
            "cxpaypbz": ["r", "v", "p"], "bicgstabDots": ["t", "s", "r0"], "bicgstabFused": ["p", "r", "x", "t", "v"], "xmy": ["x", "y"],
            "negate": ["x"], "copy": ["src", "dst"], "zero": ["x"]}
NCOEFF = {"caxpy": 1, "bicgstabUpdate": 2, "cxpaypbz": 2, "bicgstabFused": 3}


def reference(op, co, f):
    """exact results of blockblas::<op> (operands named as in block.h) with the coefficient lists co = (a, b, c) on the fields f"""
    t = {n: R._id(f[n]) for n in OPERANDS[op]}
    a, b, c = (list(co) + [None] * 3)[:3]
    if op == "norm2":
        return R.Ref({}, [("norm", "x")])
    if op == "cDot":
        return R.Ref({}, [("cre", "x", "y"), ("cim", "x", "y")])
    if op == "caxpy":
        return R.Ref({"y": R._add(t["y"], _cols(a, t["x"]))})
    if op == "cDotNormA":
        return R.Ref({}, [("cre", "t", "r"), ("cim", "t", "r"), ("norm", "t")])
    if op == "bicgstabUpdate":      # x += a p + w r ; r -= w t ; rho = (r0, r), r2 = |r|^2 of the NEW r
        return R.Ref({"x": R._add(t["x"], _cols(a, t["p"]), _cols(b, t["r"])), "r": R._add(t["r"], R._neg(_cols(b, t["t"])))},
                     [("cre", "r0", "r"), ("cim", "r0", "r"), ("norm", "r")])
    if op == "cxpaypbz":
        return R.Ref({"p": R._add(t["r"], _cols(a, t["v"]), _cols(b, t["p"]))})
    if op == "bicgstabDots":
        return R.Ref({}, [("cre", "t", "s"), ("cim", "t", "s"), ("norm", "t"), ("cre", "r0", "s"), ("cim", "r0", "s"), ("cre", "r0", "t"), ("cim", "r0", "t")])
    if op == "bicgstabFused":       # x += a p + w s ; r = s - w t ; p = r + b (p - w v) ; |r|^2 of the new r
        rn = R._add(t["r"], R._neg(_cols(b, t["t"])))
        return R.Ref({"x": R._add(t["x"], _cols(a, t["p"]), _cols(b, t["r"])), "r": rn,
                      "p": R._add(rn, _cols(c, R._add(t["p"], R._neg(_cols(b, t["v"])))))}, [("norm", "r")])
    if op == "xmy":
        return R.Ref({"y": R._add(t["x"], R._neg(t["y"]))})
    if op == "negate":
        return R.Ref({"x": R._neg(t["x"])})
    if op == "copy":
        return R.Ref({"dst": t["src"]})
    if op == "zero":
        return R.Ref({"x": (np.zeros_like(t["x"][0]), np.zeros_like(t["x"][0]))})
    raise ValueError("no reference for %s" % op)


def _flat(label, got, want, T):
    return R.check_elements(label, 4, np.asarray(got).reshape(-1), want.reshape(-1), T.reshape(-1))


def check(op, co, before, after, sums):
    """Compare what a kernel made of blockblas::<op> with the reference.  before / after: operand name -> [rhs][reals] read back before / after
    the call; sums: [sum][rhs] as it returned them.  Returns the list of (label, error, bound, error / bound); raises R.Mismatch."""
    ref = reference(op, co, before)
    out = []
    for n in OPERANDS[op]:
        if n in ref.written:
            out.append(_flat("%s %s" % (op, n), after[n], *ref.written[n]))
        elif not np.array_equal(after[n], before[n]):
            raise R.Mismatch("%s: read-only operand %s changed in %d elements" % (op, n, int(np.sum(after[n] != before[n]))))
    sums = np.asarray(sums)
    nrhs = next(iter(before.values())).shape[0]
    if sums.size != len(ref.sums) * nrhs:
        raise R.Mismatch("%s: %d sums returned, %d x %d expected" % (op, sums.size, len(ref.sums), nrhs))
    sums = sums.reshape(len(ref.sums), nrhs)
    for k, kind in enumerate(ref.sums):
        worst = None
        for i in range(nrhs):
            label = "%s sum %s(%s) rhs %d" % (op, kind[0], ",".join(kind[1:]), i)
            rec = R.check_sum(label, sums[k, i], R.summands(kind, {n: after[n][i] for n in kind[1:]}))
            worst = rec if worst is None or rec[3] > worst[3] else worst
        out.append(worst)
    return out


# ---- minimal residual: two explicit steps on the vectors ----
def _cdot(f, g):
    """(f, g) = sum conj(f) g of interleaved longdouble arrays, as (re, im)"""
    fr, fi, gr, gi = f[0::2], f[1::2], g[0::2], g[1::2]
    return np.sum(fr * gr + fi * gi), np.sum(fr * gi - fi * gr)


def _coef(omega, dot, nrm):
    return complex(float(HP(omega) * dot[0] / nrm), float(HP(omega) * dot[1] / nrm)) if nrm > 0 else 0j


def mr_sums(r, w1, w2=None):
    """the sums the stencil epilogues hand to the updates, in longdouble from the vectors, rounded to fp64: s3[3][rhs] = Re, Im (w1, r), |w1|^2
    and s7[7][rhs] = Re, Im (w2, w1), |w2|^2, Re, Im (r, w1), Re, Im (r, w2) (None without w2)"""
    nrhs = r.shape[0]
    s3, s7 = np.zeros((3, nrhs)), (np.zeros((7, nrhs)) if w2 is not None else None)
    for i in range(nrhs):
        rr, a = np.asarray(r[i], dtype=HP), np.asarray(w1[i], dtype=HP)
        s3[0, i], s3[1, i] = _cdot(a, rr)
        s3[2, i] = np.sum(a * a)
        if w2 is not None:
            b = np.asarray(w2[i], dtype=HP)
            s7[0, i], s7[1, i] = _cdot(b, a)
            s7[2, i] = np.sum(b * b)
            s7[3, i], s7[4, i] = _cdot(rr, a)
            s7[5, i], s7[6, i] = _cdot(rr, b)
    return s3, s7


def mr_reference(steps, omega, fresh, f):
    """x and r after one or two minimal-residual steps, every coefficient from the VECTORS: a0 = omega (w1, r) / |w1|^2; r1 = r - a0 w1,
    A r1 := w1 - a0 w2, a1 = omega (A r1, r1) / |A r1|^2; x [+]= a0 r + a1 r1, r = r1 - a1 A r1.  f: x, rin, w1 (, w2) as [rhs][reals].
    Returns {"x": (want, T), "r": (want, T)} and the coefficients [(a0, a1)] per right-hand side"""
    nrhs = f["rin"].shape[0]
    xs, rs, coefs = [], [], []
    for i in range(nrhs):
        r, w1 = R._id(f["rin"][i]), R._id(f["w1"][i])
        a0 = _coef(omega, _cdot(w1[0], r[0]), np.sum(w1[0] * w1[0]))
        r1 = R._add(r, R._neg(R._cplx(a0, w1)))
        xt = [] if fresh else [R._id(f["x"][i])]
        if steps == 1:
            xs.append(R._add(*(xt + [R._cplx(a0, r)])))
            rs.append(r1)
            coefs.append((a0, 0j))
            continue
        w2 = R._id(f["w2"][i])
        ar1 = R._add(w1, R._neg(R._cplx(a0, w2)))
        a1 = _coef(omega, _cdot(ar1[0], r1[0]), np.sum(ar1[0] * ar1[0]))
        xs.append(R._add(*(xt + [R._cplx(a0, r), R._cplx(a1, r1)])))
        rs.append(R._add(r1, R._neg(R._cplx(a1, ar1))))
        coefs.append((a0, a1))
    stack = lambda ts: (np.stack([t[0] for t in ts]), np.stack([t[1] for t in ts]))
    return {"x": stack(xs), "r": stack(rs)}, coefs


def mr_coefficients(omega, s3, s7=None):
    """[(a0, a1)] per right-hand side formed from the SUMS in fp64 the way the update kernels do it (a1 by the expansion; 0 without s7) — for
    diagnostics: how far two sets of sums move the coefficients.  The checks never use it."""
    out = []
    for i in range(s3.shape[1]):
        c, n1 = complex(s3[0, i], s3[1, i]), s3[2, i]
        a0 = omega * c / n1 if n1 > 0 else 0j
        a1 = 0j
        if s7 is not None:
            d, n2, e = complex(s7[0, i], s7[1, i]), s7[2, i], complex(s7[5, i], s7[6, i])
            num = c - a0 * n1 - np.conj(a0) * np.conj(e) + abs(a0) ** 2 * d
            den = n1 - 2.0 * (np.conj(a0) * d).real + abs(a0) ** 2 * n2
            a1 = omega * num / den if den > 0 else 0j
        out.append((complex(a0), complex(a1)))
    return out


def mr_condition(omega, s3, s7):
    """kappa = sum |terms| / |result| of the numerator and of the denominator of a1 in the expansion mr2_update_kernel uses, per right-hand side
    (0 where the result is exactly 0 because every term is): [(kappa_num, kappa_den)]"""
    out = []
    for i in range(s3.shape[1]):
        c, n1 = complex(s3[0, i], s3[1, i]), s3[2, i]
        d, n2, e = complex(s7[0, i], s7[1, i]), s7[2, i], complex(s7[5, i], s7[6, i])
        a0 = omega * c / n1 if n1 > 0 else 0j
        num = [c, -a0 * n1, -np.conj(a0) * np.conj(e), abs(a0) ** 2 * d]
        den = [n1, -2.0 * (np.conj(a0) * d).real, abs(a0) ** 2 * n2]
        k = []
        for terms in (num, den):
            tot, mag = abs(sum(terms)), sum(abs(t) for t in terms)
            k.append(0.0 if mag == 0 else (float("inf") if tot == 0 else mag / tot))
        out.append(tuple(k))
    return out


def check_mr(steps, omega, fresh, need_r, before, after):
    """mrUpdateDev / mr2UpdateDev against mr_reference.  before / after: x, r, rin, w1 (, w2) as [rhs][reals].  x (and r if need_r) element-wise;
    without need_r r must be untouched; rin, w1, w2 bit-identical; in a column whose rin, w1 and w2 are zero x is unchanged (zero when fresh) and r = rin"""
    what = "mr%s fresh %d needR %d" % ("2" if steps == 2 else "", fresh, need_r)
    ref, coefs = mr_reference(steps, omega, fresh, before)
    out = [_flat(what + " x", after["x"], *ref["x"])]
    if need_r:
        out.append(_flat(what + " r", after["r"], *ref["r"]))
    elif not np.array_equal(after["r"], before["r"]):
        raise R.Mismatch("%s: r written although no residual was asked for (%d elements)" % (what, int(np.sum(after["r"] != before["r"]))))
    for n in ("rin", "w1", "w2"):
        if n in before and not np.array_equal(after[n], before[n]):
            raise R.Mismatch("%s: read-only operand %s changed" % (what, n))
    for i in range(before["rin"].shape[0]):
        if any(np.any(before[n][i]) for n in ("rin", "w1", "w2") if n in before):
            continue
        if not np.array_equal(after["x"][i], np.zeros_like(before["x"][i]) if fresh else before["x"][i]):
            raise R.Mismatch("%s: x of the zero column %d changed" % (what, i))
        if need_r and np.any(after["r"][i]):
            raise R.Mismatch("%s: r of the zero column %d is not rin" % (what, i))
    return out


# ---- epilogue sums of the fine stencil ----
EPILOGUE_SUMS = {1: [("cre", "a", "out"), ("cim", "a", "out")],
                 2: [("cre", "out", "same"), ("cim", "out", "same"), ("norm", "out"), ("cre", "a", "same"), ("cim", "a", "same"), ("cre", "a", "out"),
                     ("cim", "a", "out")],
                 3: [("cre", "out", "same"), ("cim", "out", "same"), ("norm", "out")]}


def check_epilogue_sums(mode, sums, vals):
    """sums[k][rhs] of FineBlockDots mode 1, 2, 3 against the longdouble sums over the read-back fields vals = {"out", "same", "a"} ([rhs][reals]),
    to EPILOGUE_REL of the sum of the absolute values of the summands"""
    kinds = EPILOGUE_SUMS[mode]
    sums = np.asarray(sums)
    nrhs = vals["out"].shape[0]
    if sums.shape != (len(kinds), nrhs):
        raise R.Mismatch("mode %d: sums of shape %s, expected %s" % (mode, sums.shape, (len(kinds), nrhs)))
    out = []
    for k, kind in enumerate(kinds):
        worst = None
        for i in range(nrhs):
            got = sums[k, i]
            label = "epilogue mode %d %s(%s) rhs %d" % (mode, kind[0], ",".join(kind[1:]), i)
            if not np.isfinite(got):
                raise R.Mismatch("%s: %r" % (label, got))
            terms = R.summands(kind, {n: vals[n][i] for n in kind[1:]})
            rec = R._record(label, abs(HP(got) - np.sum(terms)), EPILOGUE_REL * np.sum(np.abs(terms)))
            worst = rec if worst is None or rec[3] > worst[3] else worst
        out.append(worst)
    return out
