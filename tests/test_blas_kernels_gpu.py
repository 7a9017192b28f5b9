"""Every kernel-launching function of namespace blas (include/blas.h, csrc/blas.hip) on fine-grid fields, through the test hooks
(qudaAmdBlasApply, qudaAmdBlasDevUpdate, qudaAmdBlasMulti*, qudaAmdBlasHeavyQuarkResidualNorm), against the longdouble numpy references
of tests/blas_ref.py, whose docstring derives the bounds.  In short: elements of fp64 / fp32 fields to 8 roundings of the sum of the absolute
values of their terms, elements of 16-bit fields to 1e-4 of the site's largest expected element, sums to 1e-13 of the sum of the absolute
values of their summands, taken from the values the fields hold after the kernel.

16-bit fields, sums over registers: xmyNorm, axpyNorm, caxpyNorm, caxpyXmazNormX, cabxpyAxNorm and caxpyDotzy update a field and sum over it
in one sweep and have no site() form, so on a 16-bit field they sum the fp32 REGISTERS, not the values the store then rounds to int16 times
the site's scale (the four CG functors, tests/test_cg_kernels_gpu.py, sum the stored values).  These sums are therefore compared with the
exact update of the read-back operands, to sum_i (2 |v_i| d_i + d_i^2) for a norm and sum_i |z_i| d_i for a dot, d_i = 8 * 2^-24 T_i.

Operands: 24 normal reals per site times 10^u, u uniform in [-3, 3] per site and field, and one identically zero site per field (in the
second parity segment of a full field; a different site in every field) — a 16-bit scale or norm index taken from the wrong site shows as
an error of orders of magnitude.  Complex coefficients have two nonzero, unequal parts.

Geometries (from a resident gauge field):
  4x4x4x4 parity      3072 reals: ONE partial work-group of 128 sites in 16 bits
  6x6x4x2 full        Vh = 144: 1728 / 864 / 144 chunks per parity segment in fp64 / fp32 / 16 bits, none a multiple of 256: the switch between
                      the segments falls inside a work-group in every precision
  16x16x16x16 full    fp64 only, the six functors with the most operands: 786432 chunks are two trips of the 4-way unrolled loop at the default
                      cap of 512 work-groups, the second with dead u = 2, 3 lanes
The capped loops (QUDA_AMD_BLAS_BLOCKS = 1, 2: several trips, a partly live group, a group across the segment switch, one and two blocks in
the completion-counter reduction) need a fresh process each: test_capped_grids starts tools/blas_capped_check.py twice.

Function -> test:
  norm2, reDotProduct, cDotProduct, cDotProductNormA, cDotProductNormB, ax, axpy, xpy, xpay, mxpy, axpby, xmyNorm, axpyNorm, caxpy, caxpby,
  xmyz, cxpaypbz, caxpyNorm, caxpyXmaz (caxpyXmazMR is the same call), caxpyXmazNormX, caxXmaz, caxInit, cabxpyAx, cabxpyAxNorm, caxpyDotzy,
  caxpbypzYmbw                                          test_single_field (all), test_large_field (six of them), test_capped_grids
  xmyz with z = y, caxpy(a, x, x), cDotProduct(x, x)    test_aliased_operands
  cDotProductNormADev + caxpyXmazDev / caxXmazDev / caxInitDev     test_device_scalars, test_device_scalars_breakdown
  multiSupported, multiDot, multiCaxpyResidual, multiCaxpy         test_multi_supported, test_multi_dot, test_multi_caxpy_residual, test_multi_caxpy
  HeavyQuarkResidualNorm                                test_heavy_quark_residual_norm, test_capped_grids
  axpyCGNorm, axpyZpbx, tripleCGReduction, axpyReDot, multiShiftUpdate     tests/test_cg_kernels_gpu.py
  zero, copy, caxpy / cDotProduct over vectors of fields: loops over the above, not tested here"""
import importlib
import os
import subprocess
import sys

import numpy as np
import pytest

import blas_ref as R
from synth import smooth_gauge

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LATTICES = {"4x4x4x4-parity": ((4, 4, 4, 4), 1), "6x6x4x2-full": ((6, 6, 4, 2), 2), "16x16x16x16-full": ((16, 16, 16, 16), 2)}   # name -> (X, site subset)
SMALL = ["4x4x4x4-parity", "6x6x4x2-full"]
PRECS = [8, 4, 2]
A, B = 0.37 - 0.61j, -0.83 + 0.29j
COEFF = {"ax": (0.7,), "axpy": (-0.37,), "xpay": (0.61,), "axpby": (0.61, -0.83), "axpyNorm": (0.45,),
         "cabxpyAx": (0.7, 0.0, B.real, B.imag), "cabxpyAxNorm": (0.7, 0.0, B.real, B.imag)}
SINGLE_OPS = sorted(R.OPERANDS)
LARGE_OPS = ["caxpbypzYmbw", "cxpaypbz", "caxpyXmazNormX", "caxpyDotzy", "caxInit", "cDotProductNormB"]
MULTI_K = [0, 1, 3, 4, 5, 12, 13, 20]
OMEGA = 0.85


def coeff(op):
    return COEFF.get(op, (A.real, A.imag, B.real, B.imag))


@pytest.fixture(scope="module")
def qa():
    mod = importlib.import_module("quda-qkxtm-multigrid_amd")
    mod.init(0)
    yield mod
    mod.end()


_resident = {}


def _gauge(X):
    if int(np.prod(X)) > 4096:      # unit links: the BLAS kernels only take the geometry from the gauge field
        return np.tile(np.eye(3)[:, :, None] * np.array([1.0, 0.0]), (4, int(np.prod(X)), 1, 1, 1)).reshape(4, -1)
    return smooth_gauge(X, 0.35)


def _geometry(qa, name):
    """the spinor handles take their geometry from the resident gauge field: one load per lattice"""
    X, subset = LATTICES[name]
    if _resident.get("name") != name:
        qa.load_gauge(_gauge(X), qa.gauge_param(X, cuda_prec=8, t_boundary=qa.QUDA_PERIODIC_T))
        _resident["name"] = name
    n = int(np.prod(X)) * 24 // (2 if subset == 1 else 1)
    ip = qa.invert_param(qa.QUDA_TWISTED_MASS_DSLASH, 0.124, 0.005, +1, "ee", 0, cuda_prec=8)
    return X, subset, n, ip


class Fields:
    """device fields of one precision and geometry, made from site-scaled host fields with one zero site each"""

    def __init__(self, qa, name, prec, seed):
        self.qa, self.name, self.prec = qa, name, prec
        self.X, self.subset, self.n, self.ip = _geometry(qa, name)
        self.rng = np.random.default_rng(seed)
        self.live, self.made = [], 0

    def host(self, zero=False):
        ns = self.n // R.SITE
        if zero:
            return np.zeros(self.n)
        v = self.rng.standard_normal((ns, R.SITE)) * 10.0 ** self.rng.uniform(-3, 3, (ns, 1))
        vh = ns // self.subset
        v[(ns - vh) + (5 + 7 * self.made) % vh] = 0.0     # in the second parity segment of a full field, another site in every field
        self.made += 1
        return v.reshape(-1)

    def new(self, host=None, zero=False):
        f = self.qa.Spinor(self.prec, self.subset)
        self.live.append(f)
        f.host = self.host(zero) if host is None else host
        return f.load(f.host, self.ip)

    def reload(self, f):
        f.load(f.host, self.ip)

    def read(self, f):
        return f.save(self.ip, np.empty(self.n))

    def free(self):
        for f in self.live:
            f.free()
        self.live = []


def report(recs, what, F):
    """one line per check of a call (pytest -s shows them; DESIGN.md quotes the worst ratio per operation and precision); returns the worst"""
    for label, err, bound, ratio in recs:
        print("BLAS %s | %s | prec %d | %s | error %.3e bound %.3e ratio %.4f" % (what, F.name, F.prec, label, err, bound, ratio))
    return max(recs, key=lambda r: r[3]) if recs else (what, 0.0, 0.0, 0.0)


# ---- the checks: each makes its fields, runs the kernel, compares, frees; shared with tools/blas_capped_check.py ----
def check_single(qa, F, op, alias=None):
    """blas::<op> through qudaAmdBlasApply: written fields element-wise, read-only operands bit-identical, sums to their bounds and
    bit-identical when the call is repeated on the same inputs.  alias = "yz": operand z is the field y"""
    try:
        names = R.OPERANDS[op]
        f = {}
        for n in names:
            f[n] = f[alias[0]] if alias and n == alias[1] else F.new()
        before = {n: F.read(f[n]) for n in names}
        for n in names:      # what the device holds is the host field rounded to the storage format: the zero site survives
            assert not np.any(before[n].reshape(-1, R.SITE)[np.all(f[n].host.reshape(-1, R.SITE) == 0, axis=1)])
        sums = qa.blas_apply(op, coeff(op), **f)
        after = {n: F.read(f[n]) for n in names}
        recs = R.check(op, F.prec, coeff(op), before, after, sums, aliases=(alias,) if alias else ())
        if sums:
            for n in set(names):
                F.reload(f[n])
            again = qa.blas_apply(op, coeff(op), **f)
            if again != sums:
                raise R.Mismatch("%s: sums %r, then %r from the same inputs" % (op, sums, again))
        return report(recs, op + (" " + alias[1] + "=" + alias[0] if alias else ""), F)
    finally:
        F.free()


def check_self_dot(qa, F):
    """cDotProduct(x, x): imaginary part exactly 0, real part the bits of norm2"""
    try:
        x = F.new()
        re, im = qa.blas_apply("cDotProduct", (), x=x, y=x)
        n2, = qa.blas_apply("norm2", (), x=x)
        if im != 0.0 or re != n2 or n2 != x.norm2():
            raise R.Mismatch("cDotProduct(x, x) = (%r, %r), norm2 %r" % (re, im, n2))
        v = F.read(x)
        return report([R.check_sum("cDotProduct(x,x)", re, R.summands(("norm", "x"), {"x": v}))], "cDotProduct x=x", F)
    finally:
        F.free()


DEV_OPS = {"caxpyXmaz": "xyz", "caxXmaz": "xyz", "caxInit": "xyzw"}
DEV_SOURCE = {"caxpyXmaz": {"y": "x", "x": "z"}, "caxXmaz": {"y": "x", "x": "z"}, "caxInit": {"y": "x", "w": "z"}}   # written field -> operand alpha multiplies


def check_dev(qa, F, op, breakdown=False):
    """cDotProductNormADev(p, q) + <op>Dev(omega, ...) in one call.  As in MR, p = z (the operator applied to the residual) and q = x (the
    residual); alpha = omega (p, q) / |p|^2 is recomputed here from the sums cDotProductNormA returns for the same operands, and the element
    bound grows by 1e-13 |alpha| |operand| for the last bit of the quotient.  breakdown: p identically zero, so alpha = 0: caxpyXmazDev must
    leave x and y as they were, bit for bit; caxXmazDev / caxInitDev leave y identically zero and x / w equal to the source x — bit for bit in
    fp64 / fp32; a 16-bit x / w is a field written anew with its scale derived anew and is held to the element-wise bound of written fields"""
    try:
        names = DEV_OPS[op]
        f = {n: F.new() for n in names}
        p, q = (F.new(zero=True), f["x"]) if breakdown else (f["z"], f["x"])
        before = {n: F.read(f[n]) for n in names}
        re, im, nrm = qa.blas_apply("cDotProductNormA", (), x=p, y=q)
        alpha = OMEGA * complex(re, im) / nrm if nrm > 0 else 0j
        if breakdown and (re, im, nrm) != (0.0, 0.0, 0.0):
            raise R.Mismatch("sums of a zero field: %r" % ((re, im, nrm),))
        qa.blas_dev_update(op + "Dev", OMEGA, p, q, f["x"], f["y"], f["z"], f.get("w"))
        after = {n: F.read(f[n]) for n in names}
        extra = {}
        for wn, src in DEV_SOURCE[op].items():
            s = np.abs(before[src])
            extra[wn] = 1e-13 * abs(alpha) * np.repeat(s[0::2] + s[1::2], 2)
        recs = R.check(op, F.prec, (alpha.real, alpha.imag), before, after, [], extra=extra)
        if breakdown:
            if op == "caxpyXmaz":
                same = [n for n in "xy" if not np.array_equal(after[n], before[n])]
                if same:
                    raise R.Mismatch("caxpyXmazDev with alpha = 0 changed %s (%d elements)" % (same, sum(int(np.sum(after[n] != before[n])) for n in same)))
            else:
                out = "x" if op == "caxXmaz" else "w"
                if np.any(after["y"] != 0):
                    raise R.Mismatch("%sDev with alpha = 0: y is not zero" % op)
                if F.prec != 2 and not np.array_equal(after[out], before["x"]):
                    raise R.Mismatch("%sDev with alpha = 0: %s is not the source" % (op, out))
        return report(recs, op + "Dev" + (" breakdown" if breakdown else ""), F)
    finally:
        F.free()


def _multi_coefficients(k):
    return [complex(0.3 + 0.07 * i, -0.5 + 0.11 * i) * (-1) ** i for i in range(k)]


def check_multi_dot(qa, F, k):
    try:
        fs, y, r = [F.new() for _ in range(k)], F.new(), F.new()
        vals = {"y": F.read(y), "r": F.read(r)}
        vals.update({"f%d" % i: F.read(g) for i, g in enumerate(fs)})
        beta, yr, yn = qa.multi_dot(fs, y, r)
        recs = []
        for i in range(k):
            recs.append(R.check_sum("multiDot k=%d re beta_%d" % (k, i), beta[i].real, R.summands(("cre", "f%d" % i, "y"), vals)))
            recs.append(R.check_sum("multiDot k=%d im beta_%d" % (k, i), beta[i].imag, R.summands(("cim", "f%d" % i, "y"), vals)))
        recs.append(R.check_sum("multiDot k=%d re (y,r)" % k, yr.real, R.summands(("cre", "y", "r"), vals)))
        recs.append(R.check_sum("multiDot k=%d im (y,r)" % k, yr.imag, R.summands(("cim", "y", "r"), vals)))
        recs.append(R.check_sum("multiDot k=%d |y|^2" % k, yn, R.summands(("norm", "y"), vals)))
        if (beta, yr, yn) != qa.multi_dot(fs, y, r):
            raise R.Mismatch("multiDot k=%d: two calls on the same inputs differ" % k)
        for n, g in [("y", y), ("r", r)] + [("f%d" % i, g) for i, g in enumerate(fs)]:
            if not np.array_equal(F.read(g), vals[n]):
                raise R.Mismatch("multiDot k=%d changed %s" % (k, n))
        return report(recs, "multiDot k=%d" % k, F)
    finally:
        F.free()


def check_multi_caxpy(qa, F, k, residual):
    """multiCaxpyResidual (scale != 1, complex a) or multiCaxpy; with k = 0 multiCaxpy must return y bit-identical"""
    try:
        fs, y = [F.new() for _ in range(k)], F.new()
        r = F.new() if residual else None
        c, scale, a = _multi_coefficients(k), (0.77 if residual else 1.0), 0.41 - 0.23j
        fv, yv = [F.read(g) for g in fs], F.read(y)
        rv = F.read(r) if residual else None
        what = "%s k=%d" % ("multiCaxpyResidual" if residual else "multiCaxpy", k)
        if residual:
            r2, y2 = qa.multi_caxpy_residual(c, fs, scale, y, a, r)
        else:
            qa.multi_caxpy(c, fs, y)
        ref = R.multi_caxpy_reference(c, fv, scale, yv, a, rv)
        ya = F.read(y)
        recs = [R.check_elements(what + " y", F.prec, ya, *ref["y"])]
        if residual:
            ra = F.read(r)
            recs.append(R.check_elements(what + " r", F.prec, ra, *ref["r"]))
            recs.append(R.check_sum(what + " |r|^2", r2, R.summands(("norm", "r"), {"r": ra})))
            recs.append(R.check_sum(what + " |y|^2", y2, R.summands(("norm", "y"), {"y": ya})))
            F.reload(y)
            F.reload(r)
            if (r2, y2) != qa.multi_caxpy_residual(c, fs, scale, y, a, r):
                raise R.Mismatch(what + ": two calls on the same inputs differ")
        elif k == 0 and not np.array_equal(ya, yv):
            raise R.Mismatch("multiCaxpy k=0 changed y")
        for i, g in enumerate(fs):
            if not np.array_equal(F.read(g), fv[i]):
                raise R.Mismatch(what + " changed f_%d" % i)
        return report(recs, what, F)
    finally:
        F.free()


def check_multi_supported(qa, F):
    try:
        x = F.new()
        want = F.prec != 2
        got = [qa.multi_supported(x, k) for k in (0, 1, 20, 21, -1)]
        if got != [want, want, want, False, False]:
            raise R.Mismatch("multiSupported prec %d: %r for k = 0, 1, 20, 21, -1" % (F.prec, got))
    finally:
        F.free()


def check_heavy_quark(qa, F):
    """(|x|^2, |r|^2, mean over sites of r2 / x2 with a zero x site counting 1), bit-identical when the call is repeated on the same inputs"""
    try:
        x, r = F.new(), F.new()
        xv, rv = F.read(x), F.read(r)
        got = qa.heavy_quark_residual_norm(x, r)
        again = qa.heavy_quark_residual_norm(x, r)
        if tuple(again) != tuple(got):
            raise R.Mismatch("HeavyQuarkResidualNorm: sums %r, then %r from the same inputs" % (tuple(got), tuple(again)))
        sx, sr, ratio = R.heavy_quark_summands(xv, rv)
        assert np.sum(ratio == 1.0) >= 1
        recs = [R.check_sum("HeavyQuarkResidualNorm |x|^2", got[0], sx), R.check_sum("HeavyQuarkResidualNorm |r|^2", got[1], sr),
                R.check_sum("HeavyQuarkResidualNorm mean r2/x2", got[2], ratio / ratio.size)]
        for g, v in ((x, xv), (r, rv)):
            if not np.array_equal(F.read(g), v):
                raise R.Mismatch("HeavyQuarkResidualNorm changed an operand")
        return report(recs, "HeavyQuarkResidualNorm", F)
    finally:
        F.free()


# ---- the tests ----
@pytest.mark.parametrize("op", SINGLE_OPS)
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("name", SMALL)
def test_single_field(qa, name, prec, op):
    check_single(qa, Fields(qa, name, prec, 31), op)


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("name", SMALL)
def test_aliased_operands(qa, name, prec):
    """the aliasing the solvers use: xmyz with z being y, caxpy(a, x, x), cDotProduct(x, x)"""
    check_single(qa, Fields(qa, name, prec, 32), "xmyz", alias="yz")
    check_single(qa, Fields(qa, name, prec, 33), "caxpy", alias="xy")
    check_self_dot(qa, Fields(qa, name, prec, 34))


@pytest.mark.parametrize("op", sorted(DEV_OPS))
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("name", SMALL)
def test_device_scalars(qa, name, prec, op):
    check_dev(qa, Fields(qa, name, prec, 35), op)


@pytest.mark.parametrize("op", sorted(DEV_OPS))
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("name", SMALL)
def test_device_scalars_breakdown(qa, name, prec, op):
    check_dev(qa, Fields(qa, name, prec, 36), op, breakdown=True)


@pytest.mark.parametrize("prec", PRECS)
def test_multi_supported(qa, prec):
    check_multi_supported(qa, Fields(qa, SMALL[1], prec, 37))


@pytest.mark.parametrize("k", MULTI_K)
@pytest.mark.parametrize("prec", [8, 4])
@pytest.mark.parametrize("name", SMALL)
def test_multi_dot(qa, name, prec, k):
    check_multi_dot(qa, Fields(qa, name, prec, 40 + k), k)


@pytest.mark.parametrize("k", MULTI_K)
@pytest.mark.parametrize("prec", [8, 4])
@pytest.mark.parametrize("name", SMALL)
def test_multi_caxpy_residual(qa, name, prec, k):
    check_multi_caxpy(qa, Fields(qa, name, prec, 70 + k), k, True)


@pytest.mark.parametrize("k", MULTI_K)
@pytest.mark.parametrize("prec", [8, 4])
@pytest.mark.parametrize("name", SMALL)
def test_multi_caxpy(qa, name, prec, k):
    check_multi_caxpy(qa, Fields(qa, name, prec, 100 + k), k, False)


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("name", SMALL)
def test_heavy_quark_residual_norm(qa, name, prec):
    check_heavy_quark(qa, Fields(qa, name, prec, 130))


@pytest.mark.parametrize("op", LARGE_OPS)
def test_large_field(qa, op):
    """two trips of the unrolled loop at the default grid cap, the second with dead lanes"""
    check_single(qa, Fields(qa, "16x16x16x16-full", 8, 140), op)


def test_capped_grids():
    """tools/blas_capped_check.py in a fresh process per grid cap (the cap is read once per process): every single-field, device-scalar,
    multi-field and heavy-quark check on 6x6x4x2 full in all three precisions with one and with two work-groups.  The second run only starts if the first passed"""
    tool = os.path.join(ROOT, "tools", "blas_capped_check.py")
    for cap in (1, 2):
        env = dict(os.environ, QUDA_AMD_BLAS_BLOCKS=str(cap))
        r = subprocess.run([sys.executable, tool], env=env, capture_output=True, text=True, timeout=240)
        lines = [ln for ln in r.stdout.splitlines() if ln.startswith("OK ")]
        print("QUDA_AMD_BLAS_BLOCKS=%d: exit %d, %d OK lines" % (cap, r.returncode, len(lines)))
        print("\n".join(lines))
        assert r.returncode == 0, (cap, r.stdout[-3000:], r.stderr[-3000:])
        assert ("cap %d" % cap) in r.stdout
        ops = {ln.split()[1] for ln in lines}
        missing = [op for op in SINGLE_OPS + [o + "Dev" for o in DEV_OPS] + ["multiDot", "multiCaxpyResidual", "multiCaxpy", "multiSupported", "HeavyQuarkResidualNorm"] if op not in ops]
        assert not missing, missing
        for p in PRECS:
            assert sum(1 for ln in lines if ln.split()[2] == str(p)) >= len(SINGLE_OPS), p
