"""High-precision numpy reference of the momentum projection that the two-point, loop and three-point contractions share
(momentumProject, csrc/momproj.hip; the contract is stated in csrc/qkxtm_internal.h), the per-element error bound the device result is
held to, a float64 restatement of the kernel's summation order for the CPU tests, and the table of cases that the CPU and the GPU
tests share.  A plain module: no GPU, no library.

    acc[k][t0 + tl][m][e] += sum_s exp(-2 pi i sum_d n_d (x_d(s) + gx[d]) / L[d]) cs[k][tl * Vs + s][e]

project() takes that sum over ALL sites of a slice in numpy's longdouble (a 64-bit mantissa on x86, 2^-11 of an fp64 rounding).  The
phase argument is reduced exactly, in integers, over the common denominator D = L0 L1 L2: q = sum_d n_d (x_d + gx_d) (D / L_d) mod D,
and only then multiplied by 2 pi / D in longdouble, so the reference counts as exact next to the bound below.

The bound — derived from the order of operations and the number formats, never from what a kernel returns.  u = 2^-53.  For one output
element (block, slice, momentum, entry) let A = sum_s |cs[s][e]| over the slice (complex moduli).  The modulus of the error of the
complex element, and with it the error of its real and of its imaginary part, is at most

    K u A  +  u (|acc_old| + A),            K = K_TERM + K_SUM.

  per term, K_TERM = 3 (ANGLE + SINCOS) + 3 PRODUCT, rounded up to a whole number = 119:
    * ANGLE = 8 pi.  A table entry is sincos(2.0 * M_PI * (double)kk / L) with an exact integer 0 <= kk < L.  The argument carries the
      rounding of pi to M_PI and three operations (the doubling, which happens to be exact, the product with kk and the quotient by
      L): four relative errors of at most u on a value below 2 pi, 4 * 2 pi u.  An absolute error d of the angle moves e^{i angle}
      by at most d.
    * SINCOS = 8 sqrt 2.  fp64 sincos: no accuracy figure is installed with the ROCm device libraries (the
      library ships as bitcode, lib/llvm/lib/clang/*/lib/amdgcn/bitcode/ocml.bc, without its documentation, and neither
      __clang_hip_math.h nor the HIP headers state one; opencl-c.h quotes ulps for the half_ functions only), so the OpenCL
      full-profile requirement is used: 4 ulp for each of sin and cos.  One ulp of a value of magnitude <= 1 is at most 2^-52 = 2 u,
      so each component is off by <= 8 u and the complex entry by <= 8 sqrt 2 u.
    * three table entries (x, y, z) of modulus 1 enter a term, each off by (ANGLE + SINCOS) u.
    * PRODUCT = 3.  A complex product in fp64, with or without FMA contraction, has a relative error below sqrt 5 u < 3 u (each
      component: two products and one sum, at most 2 u of |a||b| by component, 2 sqrt 2 u in modulus).  There are two for the phase,
      (a b) d, and one for the term c * phase.
    3 (25.14 + 11.32) + 9 = 118.4; the second-order terms are 1e-14 of that and disappear in the rounding up to 119.
  summation, K_SUM = ceil(share / 16) + 15 + 63 with share = ceil(Vs / 64), the largest share: a term passes through at most
    ceil(share / 16) additions in its site lane, 15 when the lanes are added, 63 when the shares are added; each addition rounds a
    partial sum whose modulus is at most A (1 + small) by a relative u (component by component, hence in modulus too).
  the last addition, acc_old + sum, rounds a value of modulus at most |acc_old| + A once.

K is 199 on 12 x 10 x 14 (shares of 27 sites) and 217 on 64 x 32 x 10.  A float64 emulation on a CPU stays near 3.5 u A; the smallest
mutant effect (one dropped site of the smallest magnitude, 1e-3 among up to 1e3) is about 1e-8 A.

emulate() restates the kernel's order in float64: per-direction phase tables from the reduced integer kk, the phase (a b) d, 16 site
lanes per share striding by 16, the lanes added in order, the 64 shares added in order, the old value last.  It exists for the CPU
tests: it shows that the bound holds for that order on every case, and its mutants show that the cases discriminate."""
import functools
import math

import numpy as np

HP = np.longdouble
CHP = np.clongdouble
U = 2.0 ** -53
NPART, NLANE = 64, 16
PI_HP = 4 * np.arctan(HP(1))

SINCOS_ULP = 4      # OpenCL full profile; see the docstring
ANGLE = 4 * 2 * math.pi
SINCOS = SINCOS_ULP * 2 * math.sqrt(2)
PRODUCT = 3
K_TERM = math.ceil(3 * (ANGLE + SINCOS) + 3 * PRODUCT)

MUTANTS = ("lane_stride_8", "share_end_minus_1", "yz_swapped", "gx_ignored", "phase_sign", "L_taken_as_X", "acc_overwritten", "slice_tl")


def k_sum(Vs):
    share = -(-Vs // NPART)
    return -(-share // NLANE) + (NLANE - 1) + (NPART - 1)


def K(Vs):
    return K_TERM + k_sum(Vs)


def _coords(X):
    s = np.arange(X[0] * X[1] * X[2])
    return s % X[0], (s // X[0]) % X[1], s // (X[0] * X[1])


def project(cs, X, gx, L, moms):
    """cs (nblk, nt * Vs, 16) complex -> (nblk, nt, Nm, 16) clongdouble: the sum over all sites of each slice"""
    X, gx, L = [int(v) for v in X], [int(v) for v in gx], [int(v) for v in L]
    Vs = X[0] * X[1] * X[2]
    D = L[0] * L[1] * L[2]
    c = np.asarray(cs)
    nblk, nt = c.shape[0], c.shape[1] // Vs
    c = c.reshape(nblk, nt, Vs, 16)
    cr, ci = c.real.astype(HP), c.imag.astype(HP)
    xyz = _coords(X)
    out = np.empty((nblk, nt, len(moms), 16), dtype=CHP)
    for m, n in enumerate(np.asarray(moms).reshape(-1, 3)):
        q = np.zeros(Vs, dtype=np.int64)
        for d in range(3):
            q += ((int(n[d]) * (xyz[d] + gx[d])) % L[d]) * (D // L[d])     # exact: every factor is an integer below 2^31
        ang = (2 * PI_HP) * (q % D).astype(HP) / HP(D)
        pr, pi = np.cos(ang), -np.sin(ang)
        re = np.einsum("s,ktse->kte", pr, cr) - np.einsum("s,ktse->kte", pi, ci)
        im = np.einsum("s,ktse->kte", pr, ci) + np.einsum("s,ktse->kte", pi, cr)
        out[:, :, m, :] = re + 1j * im
    return out


def bound(cs, acc_old, Vs):
    """per element of acc_old's slices that cs covers: cs (nblk, nt * Vs, 16), acc_old (nblk, nt, Nm, 16) -> (nblk, nt, Nm, 16) float64"""
    c = np.asarray(cs)
    nblk, nt = c.shape[0], c.shape[1] // Vs
    A = np.abs(c.reshape(nblk, nt, Vs, 16)).astype(HP).sum(axis=2)[:, :, None, :]
    return np.asarray(K(Vs) * U * A + U * (np.abs(np.asarray(acc_old)).astype(HP) + A), dtype=np.float64)


def sum_abs(cs, Vs):
    """A of the docstring, (nblk, nt, 1, 16)"""
    c = np.asarray(cs)
    nblk, nt = c.shape[0], c.shape[1] // Vs
    return np.asarray(np.abs(c.reshape(nblk, nt, Vs, 16)).astype(HP).sum(axis=2)[:, :, None, :], dtype=np.float64)


def _table(n, ext, g, L, sign):
    """one direction's phase table [m][c] as the kernel fills it"""
    kk = (n[:, None].astype(np.int64) * (np.arange(ext)[None, :] + g)) % L      # numpy's % is non-negative for L > 0
    ang = 2.0 * math.pi * kk.astype(np.float64) / L
    return np.cos(ang) + sign * 1j * np.sin(ang)


def emulate(acc, cs, t0, X, gx, L, moms, mutant=None):
    """float64, in the kernel's order; acc (nblk, Lt, Nm, 16) complex128 is not modified.  mutant: one of MUTANTS or None"""
    assert mutant is None or mutant in MUTANTS, mutant
    X, gx, L = [int(v) for v in X], [int(v) for v in gx], [int(v) for v in L]
    if mutant == "gx_ignored":
        gx = [0, 0, 0]
    if mutant == "L_taken_as_X":
        L = list(X)
    moms = np.asarray(moms).reshape(-1, 3)
    Vs = X[0] * X[1] * X[2]
    out = np.array(acc, dtype=np.complex128)
    c = np.asarray(cs, dtype=np.complex128)
    nblk, nt = c.shape[0], c.shape[1] // Vs
    c = c.reshape(nblk, nt, Vs, 16)
    sign = +1 if mutant == "phase_sign" else -1
    ex, ey, ez = [_table(moms[:, d], X[d], gx[d], L[d], sign) for d in range(3)]
    s = np.arange(Vs)
    x = s % X[0]
    if mutant == "yz_swapped":      # the slice decoded as if z ran before y
        z, y = (s // X[0]) % X[2], s // (X[0] * X[2])
    else:
        y, z = (s // X[0]) % X[1], s // (X[0] * X[1])
    ph = (ex[:, x] * ey[:, y]) * ez[:, z]                      # (Nm, Vs): (a b) d
    p = np.arange(NPART)
    s0, s1 = Vs * p // NPART, Vs * (p + 1) // NPART
    if mutant == "share_end_minus_1":
        s1 = s1 - 1
    stride = 8 if mutant == "lane_stride_8" else NLANE
    first = s0[:, None] + np.arange(NLANE)[None, :]           # (64, 16)
    phT = np.ascontiguousarray(ph.T)
    for k in range(nblk):
        for tl in range(nt):
            lanes = np.zeros((NPART, NLANE, len(moms), 16), dtype=np.complex128)
            j = 0
            while True:
                site = first + stride * j
                live = site < s1[:, None]
                if not live.any():
                    break
                sc = np.where(live, site, 0)
                term = c[k, tl][sc][:, :, None, :] * phT[sc][:, :, :, None]       # (64, 16, Nm, 16)
                lanes = np.where(live[:, :, None, None], lanes + term, lanes)
                j += 1
            share = lanes[:, 0]
            for q in range(1, NLANE):
                share = share + lanes[:, q]
            tot = np.zeros_like(share[0])
            for q in range(NPART):
                tot = tot + share[q]
            t = tl if mutant == "slice_tl" else t0 + tl
            out[k, t] = tot if mutant == "acc_overwritten" else out[k, t] + tot
    return out


# ---- the cases that the CPU and the GPU tests share ----
SHAPES = {  # id: (local X, [gx, ...], global L or None for X)
    "A": ((6, 4, 2), [(-5, -1, -1)], None),
    "B": ((12, 10, 14), [(0, 0, 0)], None),
    "C": ((16, 12, 18), [(0, 0, 0)], None),
    "D": ((12, 10, 14), [(12, 0, 28), (-7, -3, -30)], (24, 10, 42)),
    "E": ((64, 32, 10), [(0, 0, 0)], None),
    "F": ((64, 32, 12), [(0, 0, 0)], None),
}
SLICES_B = [(1, 1, 0, 1), (3, 5, 0, 5), (3, 5, 2, 3), (18, 5, 4, 1), (2, 5, 1, 3)]      # (nblk, Lt, t0, nt)
ONE_SLICE = (1, 2, 1, 1)


def momenta(count, L):
    """a deterministic list of `count` distinct momentum triples on global extents L.  From 8 entries on it holds 0, +-1, mixed signs, a
    component beyond +-L/2, an alias pair (n and n +- L of the same momentum) and one component near 10^4; longer lists add further
    aliases.  A single momentum is the mixed-sign (1, -1, 1)."""
    L0, L1, L2 = [int(v) for v in L]
    head = [(0, 0, 0), (1, 0, 0), (0, -1, 0), (1, -1, 1), (1 + L0, -1, 1 - L2), (L0 // 2 + 1, -(L1 // 2 + 2), 2), (10007, -3, 2), (-2, 3, -1)]
    if count == 1:
        return np.array([head[3]], dtype=np.int32)
    more = [(-2 - L0, 3 + L1, -1), (-1, 0, 0), (0, 0, 1), (10007 - L0, -3, 2 + L2), (0, 1, -1), (2, 0, -3), (-1, -1, -1), (3, 2, 1)]
    out = head + more
    n = 0
    while len(out) < count:      # distinct fillers, mixed signs, some beyond L/2
        cand = (((7 * n + 2) % 11) - 5, ((5 * n + 1) % 9) - 4, ((3 * n) % 13) - 6)
        if cand not in out:
            out.append(cand)
        n += 1
    return np.array(out[:count], dtype=np.int32)


def alias_pairs(moms, L):
    """index pairs (i, j), i < j, of momenta that are equal modulo L in every component"""
    r = np.asarray(moms) % np.asarray(L)
    return [(i, j) for i in range(len(r)) for j in range(i + 1, len(r)) if np.array_equal(r[i], r[j])]


def _case_list():
    out = []
    for shape, g, slices, nm in [("A", 0, ONE_SLICE, 36)] + [("B", 0, sl, nm) for sl, nm in zip(SLICES_B, (1, 36, 9, 8, 37))] + \
                                [("B", 0, SLICES_B[0], 8), ("B", 0, SLICES_B[2], 36), ("C", 0, ONE_SLICE, 36), ("D", 0, ONE_SLICE, 36), ("D", 1, ONE_SLICE, 9),
                                 ("E", 0, ONE_SLICE, 36), ("F", 0, ONE_SLICE, 9), ("F", 0, ONE_SLICE, 36)]:
        out.append("%s%d-b%d.Lt%d.t%d.n%d-m%d" % ((shape, g) + slices + (nm,)))
    return out


CASES = _case_list()


class Case:
    """the inputs of one case, its exact projection and its bound; made once per id and left unchanged"""

    def __init__(self, cid):
        geom, sl, nm = cid.split("-")
        X, gxs, L = SHAPES[geom[0]]
        self.id, self.shape = cid, geom[0]
        self.X, self.gx, self.L = X, gxs[int(geom[1:])], L if L is not None else X
        self.nblk, self.Lt, self.t0, self.nt = [int(v.lstrip("bLtn")) for v in sl.split(".")]
        self.Vs = X[0] * X[1] * X[2]
        self.moms = momenta(int(nm[1:]), self.L)
        rng = np.random.default_rng(sum(ord(ch) * (i + 1) for i, ch in enumerate(cid)))
        n = self.nblk * self.nt * self.Vs
        cs = (rng.standard_normal((n, 16)) + 1j * rng.standard_normal((n, 16))) * 10.0 ** rng.uniform(-3, 3, size=(n, 1))
        cs = cs.reshape(self.nblk, self.nt, self.Vs, 16)
        zero = rng.integers(0, self.Vs, size=(self.nblk, self.nt))          # one site per slice is identically zero
        for k in range(self.nblk):
            for t in range(self.nt):
                cs[k, t, zero[k, t]] = 0
        self.cs = cs.reshape(self.nblk, self.nt * self.Vs, 16)
        self.acc = rng.standard_normal((self.nblk, self.Lt, len(self.moms), 16)) + 1j * rng.standard_normal((self.nblk, self.Lt, len(self.moms), 16))
        for i, j in alias_pairs(self.moms, self.L):      # aliases start from the same value, so that they must end on the same bits
            self.acc[:, :, j] = self.acc[:, :, i]
        self.touched = slice(self.t0, self.t0 + self.nt)
        self.want = self.acc[:, self.touched].astype(CHP) + project(self.cs, self.X, self.gx, self.L, self.moms)
        self.bound = bound(self.cs, self.acc[:, self.touched], self.Vs)
        self.sum_abs = sum_abs(self.cs, self.Vs)
        for a in (self.cs, self.acc, self.want, self.bound, self.sum_abs):
            a.setflags(write=False)

    def excess(self, got):
        """max over the touched slices of |got - want| / bound, of the real and of the imaginary parts; <= 1 passes"""
        d = np.asarray(got)[:, self.touched].astype(CHP) - self.want
        return float(max(np.max(np.abs(d.real) / self.bound), np.max(np.abs(d.imag) / self.bound)))

    def units(self, got):
        """the largest error in units of 2^-53 sum_s |cs|, for the record"""
        d = np.asarray(got)[:, self.touched].astype(CHP) - self.want
        return float(np.max(np.maximum(np.abs(d.real), np.abs(d.imag)) / (U * self.sum_abs)))

    def untouched_equal(self, got):
        mask = np.ones(self.Lt, dtype=bool)
        mask[self.touched] = False
        g, a = np.asarray(got)[:, mask], self.acc[:, mask]
        return np.array_equal(g.view(np.uint64), np.ascontiguousarray(a).view(np.uint64))


@functools.lru_cache(maxsize=None)
def case(cid):
    return Case(cid)
