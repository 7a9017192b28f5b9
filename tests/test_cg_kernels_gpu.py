"""The fused sweeps of CG and multi-shift CG (csrc/blas.hip: AxpyCGNormF, AxpyZpbxF, TripleCGF, AxpyReDotF, multi_shift_update_kernel) and
the shifted DiracMdagM functor, through their test hooks, against numpy.

Fields: a 4^4 parity field (3072 reals: twelve 256-thread blocks of fp64 chunks with a grid-stride loop of one trip, three blocks of fp32
chunks, ONE partial block of 128 sites in 16 bits) and a full 6x4x2x8 field (2 x 4608 reals: the chunk index crosses the boundary between
the two parity segments inside a block, and the last block is partial in every precision).

The reference is numpy on the operand values READ BACK from the device fields, so the rounding of the storage format cancels:
  * element-wise results: 1e-14 (fp64), 5e-7 (fp32: a few 2^-24 of one multiply-add each) of the result field's largest element,
    1e-4 of the SITE's largest element for 16-bit fields (the quantum of the per-site scale is 2^-15 = 3.1e-5 of it);
  * sums: 1e-13 of the sum of the absolute values of the summands in every precision — they are accumulated in fp64 from the values the
    fields hold (for a 16-bit field that is updated and summed in one sweep: the values it holds AFTER the update), in a fixed order."""
import importlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from synth import smooth_gauge  # noqa: E402

LATTICES = {"4x4x4x4-parity": ((4, 4, 4, 4), 1), "6x4x2x8-full": ((6, 4, 2, 8), 2)}   # name -> (X, site subset)
PRECS = [8, 4, 2]


@pytest.fixture(scope="module")
def qa():
    mod = importlib.import_module("quda-qkxtm-multigrid_amd")
    mod.init(0)
    yield mod
    mod.end()


_resident = {}


def _geometry(qa, name):
    """the spinor handles take their geometry from the resident gauge field: one load per lattice"""
    X, subset = LATTICES[name]
    if _resident.get("name") != name:
        qa.load_gauge(smooth_gauge(X, 0.35), qa.gauge_param(X, cuda_prec=8, t_boundary=qa.QUDA_PERIODIC_T))
        _resident["name"] = name
    n = int(np.prod(X)) * 24 // (2 if subset == 1 else 1)
    ip = qa.invert_param(qa.QUDA_TWISTED_MASS_DSLASH, 0.124, 0.005, +1, "ee", 0, cuda_prec=8)
    return X, subset, n, ip


class Fields:
    """device fields of one precision and geometry with their read-back values"""

    def __init__(self, qa, name, prec, seed):
        self.qa = qa
        self.X, self.subset, self.n, self.ip = _geometry(qa, name)
        self.prec = prec
        self.rng = np.random.default_rng(seed)
        self.live = []

    def new(self, scale=1.0):
        f = self.qa.Spinor(self.prec, self.subset).load(scale * self.rng.standard_normal(self.n), self.ip)
        self.live.append(f)
        return f

    def read(self, f):
        return f.save(self.ip, np.empty(self.n))

    def free(self):
        for f in self.live:
            f.free()

    def check_elements(self, got, want, what):
        if self.prec == 8:
            err, bound = np.max(np.abs(got - want)), 1e-14 * np.max(np.abs(want))
        elif self.prec == 4:
            err, bound = np.max(np.abs(got - want)), 5e-7 * np.max(np.abs(want))
        else:
            site = np.max(np.abs(want.reshape(-1, 24)), axis=1)
            ratio = np.max(np.abs(got - want).reshape(-1, 24) / site[:, None])
            err, bound = ratio, 1e-4
        print("%s prec %d: error %.3e, bound %.3e" % (what, self.prec, err, bound))
        assert err <= bound, (what, self.prec, err, bound)


def _check_sum(got, summands, what):
    want, scale = float(np.sum(summands)), float(np.sum(np.abs(summands)))
    print("%s: %.15e, numpy %.15e, |difference| / sum|summands| = %.3e" % (what, got, want, abs(got - want) / scale))
    assert abs(got - want) <= 1e-13 * scale, (what, got, want)


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("name", list(LATTICES))
def test_axpy_cg_norm(qa, name, prec):
    F = Fields(qa, name, prec, 11)
    try:
        x, y = F.new(), F.new()
        xo, yo = F.read(x), F.read(y)
        a = -0.37
        n2, sigma = y.axpy_cg_norm(a, x)
        yn = F.read(y)
        assert np.array_equal(F.read(x), xo)
        F.check_elements(yn, yo + a * xo, "axpyCGNorm y")
        _check_sum(n2, yn * yn, "axpyCGNorm |y|^2")
        _check_sum(sigma, yn * (yn - yo), "axpyCGNorm (y_new, y_new - y_old)")
    finally:
        F.free()


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("name", list(LATTICES))
def test_axpy_zpbx(qa, name, prec):
    F = Fields(qa, name, prec, 12)
    try:
        x, y, z = F.new(), F.new(), F.new()
        xo, yo, zo = F.read(x), F.read(y), F.read(z)
        a, b = 0.61, 0.83
        y.axpy_zpbx(a, x, z, b)
        assert np.array_equal(F.read(z), zo)
        F.check_elements(F.read(y), yo + a * xo, "axpyZpbx y")
        F.check_elements(F.read(x), zo + b * xo, "axpyZpbx x")
    finally:
        F.free()


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("name", list(LATTICES))
def test_triple_cg_reduction(qa, name, prec):
    F = Fields(qa, name, prec, 13)
    try:
        x, y, z = F.new(), F.new(), F.new()
        xo, yo, zo = F.read(x), F.read(y), F.read(z)
        x2, y2, yz = x.triple_cg_reduction(y, z)
        _check_sum(x2, xo * xo, "tripleCGReduction |x|^2")
        _check_sum(y2, yo * yo, "tripleCGReduction |y|^2")
        _check_sum(yz, yo * zo, "tripleCGReduction (y, z)")
        assert (x2, y2, yz) == x.triple_cg_reduction(y, z)      # fixed summation order
        for f, o in ((x, xo), (y, yo), (z, zo)):
            assert np.array_equal(F.read(f), o)
    finally:
        F.free()


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("name", list(LATTICES))
def test_axpy_re_dot(qa, name, prec):
    F = Fields(qa, name, prec, 14)
    try:
        x, y = F.new(), F.new()
        xo, yo = F.read(x), F.read(y)
        a = 0.05
        dot = y.axpy_re_dot(a, x)
        yn = F.read(y)
        assert np.array_equal(F.read(x), xo)
        F.check_elements(yn, yo + a * xo, "axpyReDot y")
        _check_sum(dot, xo * yn, "axpyReDot (x, y)")
    finally:
        F.free()


@pytest.mark.parametrize("kcase", ["1", "3", "KB", "KB+1"])
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("name", list(LATTICES))
def test_multi_shift_update(qa, name, prec, kcase):
    """x_i += alpha_i p_i ; p_i = zeta_i r + beta_i p_i with distinct coefficients per shift (one beta zero): a whole chunk, less than a
    chunk, and one shift more than a chunk (two sweeps); r untouched"""
    KB = qa.multi_shift_chunk()
    k = {"1": 1, "3": 3, "KB": KB, "KB+1": KB + 1}[kcase]
    F = Fields(qa, name, prec, 15 + k)
    try:
        r = F.new()
        x = [F.new(0.5 + 0.1 * i) for i in range(k)]
        p = [F.new(1.0 + 0.05 * i) for i in range(k)]
        ro, xo, po = F.read(r), [F.read(f) for f in x], [F.read(f) for f in p]
        alpha = [0.3 + 0.07 * i for i in range(k)]
        beta = [0.0 if i == k // 2 else 0.9 - 0.06 * i for i in range(k)]
        zeta = [1.0 / (1.0 + 0.4 * i) for i in range(k)]
        qa.multi_shift_update(x, p, r, alpha, beta, zeta)
        assert np.array_equal(F.read(r), ro)
        for i in range(k):
            F.check_elements(F.read(x[i]), xo[i] + alpha[i] * po[i], "multiShiftUpdate k = %d x_%d" % (k, i))
            F.check_elements(F.read(p[i]), zeta[i] * ro + beta[i] * po[i], "multiShiftUpdate k = %d p_%d" % (k, i))
    finally:
        F.free()


@pytest.mark.parametrize("name,pc", [("4x4x4x4-parity", True), ("6x4x2x8-full", False)])
def test_mdagm_shift(qa, name, pc):
    """the DiracMdagM functor with a shift: M^dag M in + shift in to 1e-13 of the largest element; shift = 0 launches nothing extra and
    gives the bits of Dirac::MdagM"""
    F = Fields(qa, name, 8, 21)
    d = qa.Dirac(F.ip, pc=pc)
    try:
        inp, out, ref = F.new(), F.new(), F.new()
        src = F.read(inp)
        d.MdagM(ref, inp)
        plain = F.read(ref)
        d.MdagM_shift(out, inp, 0.0)
        assert np.array_equal(F.read(out), plain)
        shift = 0.37
        d.MdagM_shift(out, inp, shift)
        want = plain + shift * src
        err = np.max(np.abs(F.read(out) - want)) / np.max(np.abs(want))
        print("MdagM + shift, %s: error %.3e" % (name, err))
        assert err <= 1e-13
        assert np.array_equal(F.read(inp), src)
    finally:
        d.free()
        F.free()
