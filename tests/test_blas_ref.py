"""Self-test of tests/blas_ref.py (no GPU, no library): the checker must accept a correct evaluation of every operation in fp64 and in
fp32 numpy arithmetic at the respective bounds, and must reject "kernel outputs" with the errors a fused BLAS kernel can plausibly have —
a flipped imaginary sign, conjugation on the wrong operand, an update read in the wrong order, a norm of the old field, NormA / NormB
swapped, one untouched element in the second parity segment, one element off by 100 fp32 roundings, a 16-bit scale applied at the wrong
site.  The evaluations here are written with numpy's complex types, independently of the term-by-term code of the reference."""
import numpy as np
import pytest

import blas_ref as R

NSITE = 2 * 36                      # a "full field": two parity segments of 36 sites
A, B = 0.37 - 0.61j, -0.83 + 0.29j
COEFF = {"ax": (0.7,), "axpy": (-0.37,), "xpay": (0.61,), "axpby": (0.61, -0.83), "axpyNorm": (0.45,),
         "cabxpyAx": (0.7, 0.0, B.real, B.imag), "cabxpyAxNorm": (0.7, 0.0, B.real, B.imag)}


def coeff(op):
    return COEFF.get(op, (A.real, A.imag, B.real, B.imag))


def fields(seed, names, dtype=np.float64):
    """operands as the GPU tests make them: normal times 10^u per site, one zero site in the second segment, rounded to the field's type"""
    rng = np.random.default_rng(seed)
    out = {}
    for j, n in enumerate(names):
        v = rng.standard_normal((NSITE, 24)) * 10.0 ** rng.uniform(-3, 3, (NSITE, 1))
        v[NSITE // 2 + 3 + j] = 0.0
        out[n] = v.reshape(-1).astype(dtype).astype(np.float64)
    return out


def simulate(op, c, f, dtype, bug=None):
    """blas::<op> in numpy arithmetic of the given real type; returns (after, sums).  bug plants one of the errors"""
    ctype = np.complex64 if dtype == np.float32 else np.complex128
    c = list(c) + [0.0] * (4 - len(c))
    a, b = ctype(complex(c[0], c[1])), ctype(complex(c[2], c[3]))
    if bug == "imag sign":
        a, b = np.conj(a), np.conj(b)
    ra, rb = dtype(c[0]), dtype(c[1])
    v = {n: f[n].astype(dtype).view(ctype).copy() for n in f}
    x, y, z, w = (v.get(n) for n in "xyzw")
    old = {n: v[n].copy() for n in v}

    def norm(q):
        q = q.view(dtype).astype(np.float64)
        return float(np.sum(q * q))

    def cdot(p, q):
        p, q = p.astype(np.complex128), q.astype(np.complex128)
        d = np.sum(p * np.conj(q)) if bug == "conjugate" else np.sum(np.conj(p) * q)
        return [float(d.real), float(d.imag)]

    sums = []
    if op == "norm2":
        sums = [norm(x)]
    elif op == "reDotProduct":
        sums = [float(np.sum(x.view(dtype).astype(np.float64) * y.view(dtype).astype(np.float64)))]
    elif op == "cDotProduct":
        sums = cdot(x, y)
    elif op == "cDotProductNormA":
        sums = cdot(x, y) + [norm(y if bug == "swap norms" else x)]
    elif op == "cDotProductNormB":
        sums = cdot(x, y) + [norm(x if bug == "swap norms" else y)]
    elif op == "ax":
        x *= ra
    elif op in ("axpy", "axpyNorm"):
        y[:] = ra * x + y
    elif op == "xpy":
        y[:] = x + y
    elif op == "xpay":
        y[:] = x + ra * y
    elif op == "mxpy":
        y[:] = y - x
    elif op == "axpby":
        y[:] = ra * x + rb * y
    elif op == "xmyNorm":
        y[:] = x - y
    elif op in ("caxpy", "caxpyNorm"):
        y[:] = a * x + y
    elif op == "caxpby":
        y[:] = a * x + b * y
    elif op == "xmyz":
        z[:] = x - y
    elif op == "cxpaypbz":
        z[:] = x + a * y + b * z
    elif op in ("caxpyXmaz", "caxpyXmazNormX"):
        if bug == "order":
            x[:] = x - a * z
            y[:] = y + a * x
        else:
            y[:] = y + a * x
            x[:] = x - a * z
    elif op == "caxXmaz":
        y[:] = a * x
        x[:] = x - a * z
    elif op == "caxInit":
        y[:] = a * x
        w[:] = x - a * z
    elif op in ("cabxpyAx", "cabxpyAxNorm"):
        if bug == "order":
            y[:] = y + b * x
            x *= ra
        else:
            x *= ra
            y[:] = y + b * x
    elif op == "caxpyDotzy":
        y[:] = y + a * x
    elif op == "caxpbypzYmbw":
        z[:] = z + a * x + b * y
        y[:] = y - b * w
    else:
        raise ValueError(op)
    if op in ("xmyNorm", "axpyNorm", "caxpyNorm", "cabxpyAxNorm"):
        sums = [norm(old["y"] if bug == "old norm" else y)]
    if op == "caxpyXmazNormX":
        sums = [norm(old["x"] if bug == "old norm" else x)]
    if op == "caxpyDotzy":
        sums = cdot(z, y)
    after = {n: v[n].view(dtype).astype(np.float64) for n in v}
    return after, sums


@pytest.mark.parametrize("dtype,prec", [(np.float64, 8), (np.float32, 4)])
@pytest.mark.parametrize("op", sorted(R.OPERANDS))
def test_correct_evaluations_are_accepted(op, dtype, prec):
    f = fields(5, R.OPERANDS[op], dtype)
    after, sums = simulate(op, coeff(op), f, dtype)
    for rec in R.check(op, prec, coeff(op), f, after, sums):
        print("%-40s error %.3e bound %.3e ratio %.3f" % rec)


PLANTED = [("caxpy", "imag sign"), ("caxpbypzYmbw", "imag sign"), ("cxpaypbz", "imag sign"), ("caxInit", "imag sign"), ("caxXmaz", "imag sign"),
           ("cDotProduct", "conjugate"), ("cDotProductNormA", "conjugate"), ("caxpyDotzy", "conjugate"),
           ("caxpyXmaz", "order"), ("caxpyXmazNormX", "order"), ("cabxpyAx", "order"), ("cabxpyAxNorm", "order"),
           ("xmyNorm", "old norm"), ("axpyNorm", "old norm"), ("caxpyNorm", "old norm"), ("caxpyXmazNormX", "old norm"), ("cabxpyAxNorm", "old norm"),
           ("cDotProductNormA", "swap norms"), ("cDotProductNormB", "swap norms")]


@pytest.mark.parametrize("dtype,prec", [(np.float64, 8), (np.float32, 4)])
@pytest.mark.parametrize("op,bug", PLANTED)
def test_planted_errors_are_rejected(op, bug, dtype, prec):
    f = fields(6, R.OPERANDS[op], dtype)
    after, sums = simulate(op, coeff(op), f, dtype, bug)
    with pytest.raises(R.Mismatch):
        R.check(op, prec, coeff(op), f, after, sums)


WRITERS = ["ax", "axpby", "caxpby", "xmyz", "cxpaypbz", "caxpyXmaz", "caxInit", "cabxpyAx", "caxpbypzYmbw"]


@pytest.mark.parametrize("dtype,prec", [(np.float64, 8), (np.float32, 4)])
@pytest.mark.parametrize("op", WRITERS)
def test_untouched_element_in_the_second_segment_is_rejected(op, dtype, prec):
    f = fields(7, R.OPERANDS[op], dtype)
    after, sums = simulate(op, coeff(op), f, dtype)
    name = sorted(R.reference(op, coeff(op), f).written)[-1]
    i = (NSITE // 2 + 11) * 24 + 5
    assert after[name][i] != f[name][i]
    after[name][i] = f[name][i]
    with pytest.raises(R.Mismatch):
        R.check(op, prec, coeff(op), f, after, sums)


@pytest.mark.parametrize("op", WRITERS)
def test_one_element_off_by_a_hundred_roundings_is_rejected(op):
    """fp32: an error of 100 x 2^-24 of the element's terms is 12 times the bound; the same evaluation without it passes (above)"""
    f = fields(8, R.OPERANDS[op], np.float32)
    after, sums = simulate(op, coeff(op), f, np.float32)
    ref = R.reference(op, coeff(op), f)
    name = sorted(ref.written)[0]
    i = (NSITE // 2 + 17) * 24 + 2
    after[name][i] += 100 * 2.0 ** -24 * float(ref.written[name][1][i])
    with pytest.raises(R.Mismatch):
        R.check(op, 4, coeff(op), f, after, sums)


def test_changed_read_only_operand_is_rejected():
    f = fields(9, "xyz", np.float64)
    after, sums = simulate("caxpyDotzy", coeff("caxpyDotzy"), f, np.float64)
    after["z"][100] = np.nextafter(after["z"][100], 1.0)
    with pytest.raises(R.Mismatch):
        R.check("caxpyDotzy", 8, coeff("caxpyDotzy"), f, after, sums)


def test_aliased_operands():
    """xmyz with z being y and caxpy(a, x, x): the aliased read operand may change, the results are checked against the values before"""
    f = fields(10, "xy", np.float64)
    f["z"] = f["y"]
    after, _ = simulate("xmyz", (), f, np.float64)
    after["y"] = after["z"]
    R.check("xmyz", 8, (), f, after, [], aliases=("yz",))
    with pytest.raises(R.Mismatch):
        R.check("xmyz", 8, (), f, after, [])
    g = {"x": f["x"], "y": f["x"]}
    after, _ = simulate("caxpy", coeff("caxpy"), g, np.float64)
    after["x"] = after["y"]
    R.check("caxpy", 8, coeff("caxpy"), g, after, [], aliases=("xy",))


# ---- 16-bit fields: a numpy model of the per-site scaled int16 store ----
def store16(v):
    v = v.astype(np.float32).reshape(-1, 24)
    m = np.max(np.abs(v), axis=1, keepdims=True)
    s = np.where(m > 0, np.float32(32767) / np.where(m > 0, m, 1), 0).astype(np.float32)
    q = np.rint(v * s)
    return (q * (m / np.float32(32767))).astype(np.float32).astype(np.float64).reshape(-1)


UPDATE_AND_SUM = ["xmyNorm", "axpyNorm", "caxpyNorm", "caxpyXmazNormX", "cabxpyAxNorm", "caxpyDotzy"]


def simulate16(op, f, shift_scale=False, stored_sums=False):
    after, sums = simulate(op, coeff(op), f, np.float32)     # sums: over the fp32 registers
    ref = R.reference(op, coeff(op), f)
    for n in ref.written:
        after[n] = store16(after[n])
        if shift_scale:      # every site stored with its neighbour's scale
            sc = np.max(np.abs(after[n]).reshape(-1, 24), axis=1)
            sc = np.where(sc > 0, np.roll(sc, 1) / np.where(sc > 0, sc, 1), 0)
            after[n] = (after[n].reshape(-1, 24) * sc[:, None]).reshape(-1)
    return after, sums


@pytest.mark.parametrize("op", UPDATE_AND_SUM + ["caxpbypzYmbw", "caxInit"])
def test_sixteen_bit_model_is_accepted(op):
    f = {n: store16(v) for n, v in fields(11, R.OPERANDS[op]).items()}
    after, sums = simulate16(op, f)
    for rec in R.check(op, 2, coeff(op), f, after, sums):
        print("%-40s error %.3e bound %.3e ratio %.3f" % rec)


@pytest.mark.parametrize("op", UPDATE_AND_SUM + ["caxpbypzYmbw", "caxInit"])
def test_sixteen_bit_scale_of_the_wrong_site_is_rejected(op):
    f = {n: store16(v) for n, v in fields(11, R.OPERANDS[op]).items()}
    after, sums = simulate16(op, f, shift_scale=True)
    with pytest.raises(R.Mismatch):
        R.check(op, 2, coeff(op), f, after, sums)


@pytest.mark.parametrize("op", ["xmyNorm", "caxpyNorm", "caxpyXmazNormX"])
def test_sixteen_bit_norm_of_the_old_field_is_rejected(op):
    f = {n: store16(v) for n, v in fields(12, R.OPERANDS[op]).items()}
    after, _ = simulate16(op, f)
    _, sums = simulate(op, coeff(op), f, np.float32, "old norm")
    with pytest.raises(R.Mismatch):
        R.check(op, 2, coeff(op), f, after, sums)


# ---- multi-field reference and heavy-quark summands ----
def test_multi_caxpy_reference_matches_sequential_caxpys():
    rng = np.random.default_rng(13)
    f = fields(14, "abcde")
    fs = [f[n] for n in "abc"]
    c = [complex(*rng.standard_normal(2)) for _ in fs]
    y = f["d"].view(np.complex128).copy()
    for ci, fi in zip(c, fs):
        y += ci * fi.view(np.complex128)
    y *= 0.77
    a = 0.3 - 0.9j
    r = f["e"].view(np.complex128) - a * y
    ref = R.multi_caxpy_reference(c, fs, 0.77, f["d"], a, f["e"])
    R.check_elements("y", 8, y.view(np.float64), *ref["y"])
    R.check_elements("r", 8, r.view(np.float64), *ref["r"])
    with pytest.raises(R.Mismatch):      # the residual update with the conjugate coefficient
        R.check_elements("r", 8, (f["e"].view(np.complex128) - np.conj(a) * y).view(np.float64), *ref["r"])
    k0 = R.multi_caxpy_reference([], [], 1.0, f["d"])
    assert np.array_equal(k0["y"][0], f["d"])


def test_heavy_quark_summands():
    f = fields(15, "xr")
    sx, sr, ratio = R.heavy_quark_summands(f["x"], f["r"])
    zero = NSITE // 2 + 3
    assert ratio[zero] == 1.0 and ratio.shape == (NSITE,)
    i = 5
    assert abs(float(ratio[i]) - np.sum(f["r"][24 * i:24 * i + 24] ** 2) / np.sum(f["x"][24 * i:24 * i + 24] ** 2)) <= 1e-14 * float(ratio[i])
    R.check_sum("third", float(np.sum(ratio)), ratio)
    with pytest.raises(R.Mismatch):      # the zero site counted 0 instead of 1 in a sum that it dominates
        small = np.minimum(ratio, 1.0)
        R.check_sum("third", float(np.sum(small)) - 1.0, small)
