"""High-precision numpy references of the fused BLAS functions of namespace blas (include/blas.h; the CPU twins in the reference's
lib/blas_cpu.cpp define the semantics) and the checker that compares a kernel's output with them.  A plain module: no GPU, no library.

Fields are float64 arrays of interleaved (re, im) pairs, site-major with 24 reals per site — the operand values READ BACK from the device, so
the rounding of the storage format cancels.  The arithmetic is numpy's longdouble (a 64-bit mantissa on x86: 2^-11 of the tightest bound
below), so the reference counts as exact.  For every written field reference() returns the exact result and T, the sum of the absolute
values of the terms that form each real element (for y = a x + y with complex a: |ar xr| + |ai xi| + |yr| for the real part).

Bounds — derived from those terms and the number formats, never from what a kernel returns:
  * elements of fp64 / fp32 fields: |got - want| <= 8 eps T, eps = 2^-53 / 2^-24: the rounding of each coefficient to the field's precision
    and of each product are one eps of their term, the additions one eps of a partial sum <= T each; the functors have at most five terms
    per element, so eight roundings cover them with or without FMA contraction;
  * elements of 16-bit fields: 1e-4 of the SITE's largest expected element (the storage quantum is 2^-15 = 3.1e-5 of it);
  * sums over fp64 / fp32 fields and sums that read 16-bit fields without updating them: 1e-13 of the sum of the absolute values of the
    summands, the summands taken from the values the fields hold after the kernel (accumulation in fp64 in a fixed order);
  * sums of the functors that update a 16-bit field and sum over it in the same sweep (xmyNorm, axpyNorm, caxpyNorm, caxpyXmazNormX,
    cabxpyAxNorm, caxpyDotzy): the kernel sums its fp32 REGISTERS, not the values the store rounds them to, so the sum is compared with the
    exact update v of the read-back operands: a register differs from v_i by at most d_i = 8 * 2^-24 T_i, hence sum_i (2 |v_i| d_i + d_i^2)
    for a norm and sum_i |z_i| d_i for a dot with a read-only z (real part: |zr| d_r + |zi| d_i per complex element, imaginary part
    |zr| d_i + |zi| d_r)."""
import numpy as np

HP = np.longdouble
EPS = {8: 2.0 ** -53, 4: 2.0 ** -24}
ROUNDINGS = 8            # roundings allowed per element
HALF_ELEMENT = 1e-4      # 16-bit fields: of the site's largest expected element
SUM_REL = 1e-13          # sums: of the sum of the absolute values of the summands
SITE = 24                # reals per site of a fine-grid spinor


class Mismatch(AssertionError):
    pass


# ---- terms: (value, T) pairs of longdouble arrays ----
def _id(x):
    x = np.asarray(x, dtype=HP)
    return x, np.abs(x)


def _real(a, t):
    """real coefficient times a term"""
    a = HP(a)
    return a * t[0], np.abs(a) * t[1]


def _cplx(a, t):
    """complex coefficient times a term of interleaved (re, im) pairs"""
    a = complex(a)
    ar, ai = HP(a.real), HP(a.imag)
    v, T = t
    out, To = np.empty_like(v), np.empty_like(T)
    out[0::2] = ar * v[0::2] - ai * v[1::2]
    out[1::2] = ar * v[1::2] + ai * v[0::2]
    To[0::2] = np.abs(ar) * T[0::2] + np.abs(ai) * T[1::2]
    To[1::2] = np.abs(ar) * T[1::2] + np.abs(ai) * T[0::2]
    return out, To


def _add(*terms):
    v, T = terms[0][0].copy(), terms[0][1].copy()
    for t in terms[1:]:
        v = v + t[0]
        T = T + t[1]
    return v, T


def _neg(t):
    return -t[0], t[1]


# ---- summands of the sums, from field values ----
def summands(kind, vals):
    """the summands of one sum: kind = ("norm", f) | ("re", f, g) | ("cre", f, g) | ("cim", f, g) with (f, g) = sum conj(f) g"""
    what = kind[0]
    f = np.asarray(vals[kind[1]], dtype=HP)
    if what == "norm":
        return f * f
    g = np.asarray(vals[kind[2]], dtype=HP)
    if what == "re":
        return f * g
    fr, fi, gr, gi = f[0::2], f[1::2], g[0::2], g[1::2]
    if what == "cre":
        return np.concatenate([fr * gr, fi * gi])
    if what == "cim":
        return np.concatenate([fr * gi, -(fi * gr)])
    raise ValueError(kind)


def _register_allowance(kind, vals, written):
    """16-bit update-and-sum: how far the sum over fp32 registers may be from the sum over the exact update (module docstring)"""
    d = {n: ROUNDINGS * EPS[4] * T for n, (v, T) in written.items()}
    what = kind[0]
    if what == "norm":
        v = np.abs(np.asarray(vals[kind[1]], dtype=HP))
        return np.sum(2 * v * d[kind[1]] + d[kind[1]] ** 2)
    z = np.abs(np.asarray(vals[kind[1]], dtype=HP))
    dg = d[kind[2]]
    if what == "re":
        return np.sum(z * dg)
    if what == "cre":
        return np.sum(z[0::2] * dg[0::2] + z[1::2] * dg[1::2])
    if what == "cim":
        return np.sum(z[0::2] * dg[1::2] + z[1::2] * dg[0::2])
    raise ValueError(kind)


class Ref:
    def __init__(self, written, sums=()):
        self.written = written      # name -> (want, T)
        self.sums = list(sums)      # kinds, in the order the function returns them


# coefficient layout of qudaAmdBlasApply: complex a = (c0, c1), complex b = (c2, c3); real a, b = c0, c1
def _ca(c):
    return complex(c[0], c[1])


def _cb(c):
    return complex(c[2], c[3])


def reference(op, c, f):
    """exact results of blas::<op> with coefficients c (four reals) on the operands f = {"x": ..., "y": ..., ...}"""
    c = list(c) + [0.0] * (4 - len(c))
    x, y, z, w = (_id(f[n]) if n in f else None for n in "xyzw")
    if op == "norm2":
        return Ref({}, [("norm", "x")])
    if op == "reDotProduct":
        return Ref({}, [("re", "x", "y")])
    if op == "cDotProduct":
        return Ref({}, [("cre", "x", "y"), ("cim", "x", "y")])
    if op == "cDotProductNormA":
        return Ref({}, [("cre", "x", "y"), ("cim", "x", "y"), ("norm", "x")])
    if op == "cDotProductNormB":
        return Ref({}, [("cre", "x", "y"), ("cim", "x", "y"), ("norm", "y")])
    if op == "ax":
        return Ref({"x": _real(c[0], x)})
    if op == "axpy":
        return Ref({"y": _add(_real(c[0], x), y)})
    if op == "xpy":
        return Ref({"y": _add(x, y)})
    if op == "xpay":
        return Ref({"y": _add(x, _real(c[0], y))})
    if op == "mxpy":
        return Ref({"y": _add(y, _neg(x))})
    if op == "axpby":
        return Ref({"y": _add(_real(c[0], x), _real(c[1], y))})
    if op == "xmyNorm":
        return Ref({"y": _add(x, _neg(y))}, [("norm", "y")])
    if op == "axpyNorm":
        return Ref({"y": _add(_real(c[0], x), y)}, [("norm", "y")])
    if op == "caxpy":
        return Ref({"y": _add(_cplx(_ca(c), x), y)})
    if op == "caxpby":
        return Ref({"y": _add(_cplx(_ca(c), x), _cplx(_cb(c), y))})
    if op == "xmyz":
        return Ref({"z": _add(x, _neg(y))})
    if op == "cxpaypbz":
        return Ref({"z": _add(x, _cplx(_ca(c), y), _cplx(_cb(c), z))})
    if op == "caxpyNorm":
        return Ref({"y": _add(_cplx(_ca(c), x), y)}, [("norm", "y")])
    if op in ("caxpyXmaz", "caxpyXmazNormX"):
        a = _ca(c)
        return Ref({"y": _add(y, _cplx(a, x)), "x": _add(x, _neg(_cplx(a, z)))}, [("norm", "x")] if op == "caxpyXmazNormX" else [])
    if op == "caxXmaz":
        a = _ca(c)
        return Ref({"y": _cplx(a, x), "x": _add(x, _neg(_cplx(a, z)))})
    if op == "caxInit":
        a = _ca(c)
        return Ref({"y": _cplx(a, x), "w": _add(x, _neg(_cplx(a, z)))})
    if op in ("cabxpyAx", "cabxpyAxNorm"):
        xn = _real(c[0], x)
        return Ref({"x": xn, "y": _add(y, _cplx(_cb(c), xn))}, [("norm", "y")] if op == "cabxpyAxNorm" else [])
    if op == "caxpyDotzy":
        return Ref({"y": _add(y, _cplx(_ca(c), x))}, [("cre", "z", "y"), ("cim", "z", "y")])
    if op == "caxpbypzYmbw":
        a, b = _ca(c), _cb(c)
        return Ref({"z": _add(z, _cplx(a, x), _cplx(b, y)), "y": _add(y, _neg(_cplx(b, w)))})
    raise ValueError("no reference for %s" % op)


OPERANDS = {"norm2": "x", "reDotProduct": "xy", "cDotProduct": "xy", "cDotProductNormA": "xy", "cDotProductNormB": "xy", "ax": "x", "axpy": "xy",
            "xpy": "xy", "xpay": "xy", "mxpy": "xy", "axpby": "xy", "xmyNorm": "xy", "axpyNorm": "xy", "caxpy": "xy", "caxpby": "xy", "xmyz": "xyz",
            "cxpaypbz": "xyz", "caxpyNorm": "xy", "caxpyXmaz": "xyz", "caxpyXmazNormX": "xyz", "caxXmaz": "xyz", "caxInit": "xyzw", "cabxpyAx": "xy",
            "cabxpyAxNorm": "xy", "caxpyDotzy": "xyz", "caxpbypzYmbw": "xyzw"}


# ---- the multi-field kernels and the heavy-quark residual ----
def multi_caxpy_reference(c, fs, scale, y, a=None, r=None):
    """y <- scale (y + sum_i c_i f_i) ; r <- r - a y (if r is given): {"y": (want, T), "r": (want, T)}.  T of r carries the terms of y"""
    t = _add(_id(y), *[_cplx(ci, _id(fi)) for ci, fi in zip(c, fs)]) if len(fs) else _id(y)
    t = _real(scale, t)
    out = {"y": t}
    if r is not None:
        out["r"] = _add(_id(r), _neg(_cplx(a, t)))
    return out


def heavy_quark_summands(x, r):
    """the summands of the three components: |x|^2, |r|^2 per real and r2 / x2 per site, a site with x2 = 0 counting 1"""
    x, r = np.asarray(x, dtype=HP), np.asarray(r, dtype=HP)
    x2, r2 = np.sum((x * x).reshape(-1, SITE), axis=1), np.sum((r * r).reshape(-1, SITE), axis=1)
    ratio = np.ones_like(x2)
    np.divide(r2, x2, out=ratio, where=x2 > 0)
    return x * x, r * r, ratio


# ---- checks: each returns (label, error, bound, error / bound) and raises Mismatch ----
def _record(label, err, bound):
    ratio = 0.0 if err == 0 else (float("inf") if bound == 0 else float(err / bound))
    if not err <= bound:
        raise Mismatch("%s: error %.3e exceeds bound %.3e" % (label, float(err), float(bound)))
    return label, float(err), float(bound), ratio


def element_bound(prec, want, T, extra=None):
    if prec == 2:
        site = np.max(np.abs(want).reshape(-1, SITE), axis=1)
        b = np.repeat(HALF_ELEMENT * site, SITE)
    else:
        b = ROUNDINGS * EPS[prec] * T
    return b if extra is None else b + extra


def check_elements(label, prec, got, want, T, extra=None):
    """element-wise comparison; reports the element with the largest error over bound"""
    got = np.asarray(got)
    if got.shape != want.shape:
        raise Mismatch("%s: shape %s, expected %s" % (label, got.shape, want.shape))
    if not np.all(np.isfinite(got)):
        raise Mismatch("%s: non-finite elements" % label)
    err = np.abs(got.astype(HP) - want)
    b = element_bound(prec, want, T, extra)
    bad = err > b
    if np.any(bad):
        i = int(np.argmax(np.where(b > 0, err / np.where(b > 0, b, 1), np.where(err > 0, np.inf, 0))))
        raise Mismatch("%s: %d elements out of bound, worst at %d (site %d): got %.17g, expected %.17g, error %.3e, bound %.3e"
                       % (label, int(np.sum(bad)), i, i // SITE, float(got[i]), float(want[i]), float(err[i]), float(b[i])))
    ratio = np.where(b > 0, err / np.where(b > 0, b, 1), 0)
    i = int(np.argmax(ratio))
    return label, float(err[i]), float(b[i]), float(ratio[i])


def check_sum(label, got, terms):
    """a sum against its summands: 1e-13 of the sum of their absolute values"""
    if not np.isfinite(got):
        raise Mismatch("%s: %r" % (label, got))
    want, scale = np.sum(terms), np.sum(np.abs(terms))
    return _record(label, abs(HP(got) - want), SUM_REL * scale)


def check_register_sum(label, got, want, allowance):
    if not np.isfinite(got):
        raise Mismatch("%s: %r" % (label, got))
    return _record(label, abs(HP(got) - want), allowance)


def check(op, prec, c, before, after, sums, aliases=(), extra=None):
    """Compare what a kernel made of blas::<op> with the reference.  before / after: operand name -> values read back before / after the
    call; sums: what it returned; aliases: groups of operand names that are one field, e.g. ("yz",); extra: name -> additional element-wise
    allowance.  Returns the list of (label, error, bound, error / bound); raises Mismatch at the first failure."""
    ref = reference(op, c, before)
    out = []
    written = set(ref.written)
    for g in aliases:
        if written & set(g):
            written |= set(g)
    for n in before:
        if n in ref.written:
            want, T = ref.written[n]
            out.append(check_elements("%s %s" % (op, n), prec, after[n], want, T, None if extra is None else extra.get(n)))
        elif n not in written and not np.array_equal(after[n], before[n]):
            raise Mismatch("%s: read-only operand %s changed in %d elements" % (op, n, int(np.sum(after[n] != before[n]))))
    if len(sums) != len(ref.sums):
        raise Mismatch("%s: %d sums returned, %d expected" % (op, len(sums), len(ref.sums)))
    exact = dict(before)
    exact.update({n: v for n, (v, T) in ref.written.items()})
    for got, kind in zip(sums, ref.sums):
        label = "%s sum %s" % (op, "".join(kind[:1]) + "(" + ",".join(kind[1:]) + ")")
        if prec == 2 and set(kind[1:]) & set(ref.written):
            out.append(check_register_sum(label + " over registers", got, np.sum(summands(kind, exact)), _register_allowance(kind, exact, ref.written)))
        else:
            out.append(check_sum(label, got, summands(kind, after)))
    return out
