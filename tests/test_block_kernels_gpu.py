"""The multi-right-hand-side ("block") path below the solvers: every function of namespace blockblas (include/block.h, csrc/block.hip), the
four pack functions and the inner products fine_block_kernel takes in its epilogue (csrc/fine_block.hip), through the qudaAmdBlock* test
hooks, against the longdouble numpy references of tests/block_ref.py, whose docstring derives the bounds.  In short: written elements to
8 roundings (2^-24) of the sum of the absolute values of their fully expanded terms; sums of blockblas to 1e-13 of the sum of the absolute
values of their summands; epilogue sums to 25 * 2^-24 + 1e-13 of it (the bound of fp32 site sums; the kernel now takes them in fp64); pack images
bit for bit.  The device images are permuted here by the two formulas of block.h, so a word given to the wrong right-hand side fails.

Operands: normal fp32 reals times 10^u per (site, right-hand side), u uniform in [-3, 3]; right-hand side 2 identically zero in every field
(for MR the padding column of block_coarse_cycle.cpp); one zero site per column, another one in each column and field; per-column complex
coefficients with two nonzero, unequal parts that differ from column to column; column 1 converged (all its coefficients zero).

BLAS shapes (sites, components, right-hand sides), free of any lattice; n4 = 16-byte words, work-groups of 192:
  16 x 16 x 8      rhs-fastest, half = 4    n4 1024     5 1/3 work-groups: partial last work-group
  16 x 64 x 32     rhs-fastest, half = 16   n4 16384    85 1/3: partial last work-group
  50 x 48 x 24     rhs-fastest, half = 12   n4 28800    150: a panel is exactly three work-groups, so pr walks every pair
  1040 x 48 x 32   rhs-fastest, half = 16   n4 798720   4160 > the cap of 4096: a second trip of the grid-stride loop with 64 live work-groups
  650 x 12 x 8     pair-major, half = 8     n4 31200    162 1/2: partial last work-group
  650 x 12 x 32    pair-major, half = 32    the wider pair-major case
  650 x 12 x 4 / 8 pair-major: the MR updates (and the parity pack) only run at 4 and 8; mr_update_kernel runs 31 work-groups with dead
                   u = 3 lanes.  NOT covered: the outer loop of the MR kernels beyond their grid caps (fields of 67 MB and more).
Lattices of the pack and epilogue tests: 4^4 (Vh = 128: no tail) and 6^4 (Vh = 648 = 10 * 64 + 8 = 20 * 32 + 8: the last work-group of
block_fine_pack_kernel and of fine_block_kernel holds 8 sites, the smallest tail an even lattice produces).  The parity pack kernel is
launched at 4 and 8 right-hand sides only: its LDS request passes 64 KiB beyond 10 and finePtrs rejects that (read, not run; as are odd
counts and 10 right-hand sides in blockblas::run).

Function -> test:
  norm2, cDot, caxpy, cDotNormA, bicgstabUpdate, cxpaypbz, bicgstabDots, bicgstabFused, xmy, negate, copy, zero
        (block_blas_kernel<OP, NSUM> OP 0-9, block_blas_finish)                  test_block_blas (every shape), test_cdot_of_a_field_with_itself
  mrUpdateDev (mr_update_kernel), mr2UpdateDev (mr2_update_kernel)               test_mr_updates, test_epilogue_sums_feed_the_mr_update
  blockPackParity, blockUnpackParity (block_fine_pack_kernel modes 0, 1, 2)      test_parity_pack
  blockPack, blockUnpack (block_pack_kernel<*, 4>, pair-major branch)            test_full_field_pack
  FineBlockDots modes 1, 2, 3, fine_block_dots_reduce / _finish, fineBlockDotsFinish / FinishDev      test_epilogue_sums
  applyFineBlockParity: `out` of fine_block_kernel<4..32, 0 / 1 / 2> element-wise (general form, site-matrix modes 1 and 2, 12-real links,
        tail work-group, plane-tiled order, ghost faces), cloverTwistDense (clover_twist_dense_kernel)
                                                                                 tests/test_fine_stencil_gpu.py (reference: tests/fine_stencil_ref.py)
  block_pack_kernel<*, 2> (coarse levels), blockExchangeGhost, applyCoarseBlock: pinned through the operator tests against the oracle
  (tests/test_mg_gpu.py); the recurrences of blockBiCGstabNull: through the solver tests.  Not covered here, by decision."""
import importlib

import numpy as np
import pytest

import blas_ref as R
import block_ref as B
from synth import smooth_gauge

pytestmark = pytest.mark.gpu

BLAS_SHAPES = [(16, 16, 8), (16, 64, 32), (50, 48, 24), (1040, 48, 32), (650, 12, 8), (650, 12, 32)]
MR_SHAPES = [(650, 12, 4), (650, 12, 8)]
OPS = sorted(B.OPERANDS)
OMEGA = 0.85
ZERO_COL, CONVERGED = 2, 1


@pytest.fixture(scope="module")
def qa():
    mod = importlib.import_module("quda-qkxtm-multigrid_amd")
    mod.init(0)
    yield mod
    mod.lib().qudaAmdSetPartitionMask(0)
    mod.end()


def report(recs, what, shape):
    """one line per check (pytest -s shows them; DESIGN.md quotes the worst ratio per operation and layout); returns the worst"""
    for label, err, bound, ratio in recs:
        print("BLOCK %s | %s | %s | error %.3e bound %.3e ratio %.4f" % (what, "x".join(str(s) for s in shape), label, err, bound, ratio))
    return max(recs, key=lambda r: r[3]) if recs else (what, 0.0, 0.0, 0.0)


class Blocks:
    """block fields of one shape, loaded from / read back as [rhs][reals] through the layout maps of block_ref"""

    def __init__(self, qa, shape):
        self.qa, self.shape, self.live = qa, shape, []

    def new(self, cols, nghost=0):
        f = self.qa.BlockField(*self.shape, nghost)
        self.live.append(f)
        f.image = B.to_device(cols, *self.shape, nghost)
        return f.load(f.image)

    def reload(self, f):
        f.load(f.image)

    def read(self, f):
        return B.from_device(f.save(), *self.shape)

    def free(self):
        for f in self.live:
            f.free()
        self.live = []


# ---- namespace blockblas ----
@pytest.mark.parametrize("op", OPS)
@pytest.mark.parametrize("shape", BLAS_SHAPES, ids=lambda s: "x".join(str(v) for v in s))
def test_block_blas(qa, shape, op):
    """written fields element-wise, read-only operands bit-identical, sums per right-hand side, and sums and written fields bit-identical
    when the call is repeated on reloaded inputs"""
    F = Blocks(qa, shape)
    try:
        rng = np.random.default_rng(1000 + 17 * OPS.index(op) + shape[0])
        names = B.OPERANDS[op]
        f = {n: F.new(B.operand(rng, *shape, k=k, zero_col=ZERO_COL)) for k, n in enumerate(names)}
        co = [B.coefficients(shape[2], k, converged=CONVERGED) for k in range(B.NCOEFF.get(op, 0))]
        before = {n: F.read(f[n]) for n in names}
        for n in names:
            assert not np.any(before[n][ZERO_COL]) and np.any(before[n][0])
        sums = qa.block_blas_apply(op, *co, **f)
        after = {n: F.read(f[n]) for n in names}
        recs = B.check(op, co, before, after, sums)
        for n in names:
            F.reload(f[n])
        again = qa.block_blas_apply(op, *co, **f)
        if not np.array_equal(again, sums):
            raise R.Mismatch("%s: sums differ between two calls on the same inputs" % op)
        for n in names:
            if not np.array_equal(F.read(f[n]), after[n]):
                raise R.Mismatch("%s: %s differs between two calls on the same inputs" % (op, n))
        if sums.size:
            assert not np.any(sums[:, ZERO_COL])
        report(recs, op, shape)
    finally:
        F.free()


@pytest.mark.parametrize("shape", [(16, 16, 8), (650, 12, 8)], ids=["rhs-fastest", "pair-major"])
def test_cdot_of_a_field_with_itself(qa, shape):
    """cDot(x, x): the imaginary part is exactly 0, the real part is the norm"""
    F = Blocks(qa, shape)
    try:
        x = F.new(B.operand(np.random.default_rng(7), *shape, zero_col=ZERO_COL))
        v = F.read(x)
        sums = qa.block_blas_apply("cDot", x=x, y=x)
        assert sums.shape == (2, shape[2])
        if np.any(sums[1] != 0.0):
            raise R.Mismatch("cDot(x, x): imaginary parts %r" % (sums[1],))
        report([R.check_sum("cDot(x,x) rhs %d" % i, sums[0, i], R.summands(("norm", "x"), {"x": v[i]})) for i in range(shape[2])], "cDot x=x", shape)
    finally:
        F.free()


# ---- minimal-residual updates with the sums as inputs ----
@pytest.mark.parametrize("need_r", [0, 1])
@pytest.mark.parametrize("fresh", [0, 1])
@pytest.mark.parametrize("steps", [1, 2])
@pytest.mark.parametrize("shape", MR_SHAPES, ids=lambda s: "x".join(str(v) for v in s))
def test_mr_updates(qa, shape, steps, fresh, need_r):
    """mrUpdateDev / mr2UpdateDev with longdouble sums of the read-back vectors as inputs, against two explicit steps on the vectors; without
    need_r r is untouched; in the zero column x is unchanged (zero when fresh) and r = rin; bit-identical on repetition"""
    F = Blocks(qa, shape)
    try:
        host = B.mr_operands(np.random.default_rng(2000 + shape[2] + steps), shape, steps, zero_col=ZERO_COL)
        f = {n: F.new(v) for n, v in host.items()}
        before = {n: F.read(f[n]) for n in f}
        s3, s7 = B.mr_sums(before["rin"], before["w1"], before.get("w2"))
        if steps == 2:
            for kn, kd in B.mr_condition(OMEGA, s3, s7):
                assert kn < B.MR_KAPPA_LIMIT and kd < B.MR_KAPPA_LIMIT, (kn, kd)
        qa.block_mr_update(steps, OMEGA, fresh, need_r, s3, s7, f["x"], f["r"], f["rin"], f["w1"], f.get("w2"))
        after = {n: F.read(f[n]) for n in f}
        recs = B.check_mr(steps, OMEGA, fresh, need_r, before, after)
        for n in f:
            F.reload(f[n])
        qa.block_mr_update(steps, OMEGA, fresh, need_r, s3, s7, f["x"], f["r"], f["rin"], f["w1"], f.get("w2"))
        for n in ("x", "r"):
            if not np.array_equal(F.read(f[n]), after[n]):
                raise R.Mismatch("mr update: %s differs between two calls on the same inputs" % n)
        report(recs, "mr%d" % steps, shape)
    finally:
        F.free()


# ---- lattices ----
LATTICES = {"4^4": (4, 4, 4, 4), "6^4": (6, 6, 6, 6)}
_resident = {}


def _lattice(qa, name, recon=18, mask=0):
    """fp32 links of the lattice resident (one load per configuration): recon 18 with periodic, recon 12 with antiperiodic t"""
    X = LATTICES[name]
    key = (name, recon, mask)
    if _resident.get("key") != key:
        qa.lib().qudaAmdSetPartitionMask(mask)
        gp = qa.gauge_param(X, cuda_prec=4, recon=qa.QUDA_RECONSTRUCT_12 if recon == 12 else qa.QUDA_RECONSTRUCT_NO,
                            t_boundary=qa.QUDA_ANTI_PERIODIC_T if recon == 12 else qa.QUDA_PERIODIC_T)
        qa.load_gauge(smooth_gauge(X, 0.35), gp)
        _resident["key"] = key
    ip = qa.invert_param(qa.QUDA_TWISTED_MASS_DSLASH, 0.124, 0.005, +1, "ee", 0, cuda_prec=4)
    return X, int(np.prod(X)) // 2, ip


def _words(f):
    """raw device image of an fp32 spinor as 16-byte words [word][4] (uint32 view of it), its stride and the word offset of the odd half"""
    i = f.raw_info()
    assert i["precision"] == 4 and i["N"] == 4
    return f.qa.raw_device_copy(i["v"], i["bytes"]).view(np.uint32).reshape(-1, 4), i["stride"], i["odd_offset"] // 16


class Spinors:
    def __init__(self, qa, ip, subset, n_real, seed):
        self.qa, self.ip, self.subset, self.n, self.rng, self.live = qa, ip, subset, n_real, np.random.default_rng(seed), []

    def new(self):
        f = self.qa.Spinor(4, self.subset)
        f.qa = self.qa
        self.live.append(f)
        return f.load(self.rng.standard_normal(self.n) * 10.0 ** self.rng.uniform(-3, 3), self.ip)

    def free(self):
        for f in self.live:
            f.free()
        self.live = []


def _parity_block_image(spinors, vh, nrhs, base=None):
    """block image [word (x 6 + k) nrhs + i][4] (uint32) that block.h prescribes for the single-parity spinors (None: zeros, or base's column)"""
    img = np.zeros((vh, 6, nrhs, 4), dtype=np.uint32) if base is None else base.reshape(vh, 6, nrhs, 4).copy()
    for i, f in enumerate(spinors):
        if f is None:
            continue
        w, stride, _ = _words(f)
        for k in range(6):
            img[:, k, i, :] = w[k * stride:k * stride + vh]
    return img.reshape(-1, 4)


@pytest.mark.parametrize("nrhs", [4, 8])
@pytest.mark.parametrize("name", sorted(LATTICES))
def test_parity_pack(qa, name, nrhs):
    """block_fine_pack_kernel: pack with n = nrhs - 1 and a null column in the middle (zeros, also in the columns past n), accumulate onto a
    loaded block (exactly one fp32 addition, the null column unchanged), unpack (null column skipped); every image bit for bit"""
    X, vh, ip = _lattice(qa, name)
    S, F = Spinors(qa, ip, qa.QUDA_PARITY_SITE_SUBSET, vh * 24, 3000 + nrhs), Blocks(qa, (vh, 12, nrhs))
    try:
        n = nrhs - 1
        sp = [S.new() for _ in range(n)]
        sp[1] = None
        rng = np.random.default_rng(3100 + nrhs)
        blk = F.new(rng.standard_normal((nrhs, vh * 24)))
        prev = blk.save()
        qa.block_pack_parity(blk, sp)
        got = blk.save().view(np.uint32).reshape(-1, 4)
        want = _parity_block_image(sp, vh, nrhs)
        assert np.array_equal(got, want), "pack: %d words differ" % int(np.sum(np.any(got != want, axis=1)))
        # accumulate onto the block as it was loaded
        blk.load(prev)
        qa.block_pack_parity(blk, sp, accumulate=True)
        got = blk.save()
        want = (prev + _parity_block_image(sp, vh, nrhs).view(np.float32).reshape(-1)).astype(np.float32)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), "accumulate: %d reals differ" % int(np.sum(got.view(np.uint32) != want.view(np.uint32)))
        assert np.array_equal(got.reshape(vh, 6, nrhs, 4)[:, :, [1, nrhs - 1]], prev.reshape(vh, 6, nrhs, 4)[:, :, [1, nrhs - 1]])
        # unpack into fresh fields; the field of the null column is not handed over and stays as it is
        blk.load(prev)
        dst = [S.new() for _ in range(n)]
        untouched, keep = dst[1], _words(dst[1])[0].copy()
        before = [_words(d)[0].copy() for d in dst]
        qa.block_unpack_parity(blk, [d if i != 1 else None for i, d in enumerate(dst)])
        assert np.array_equal(_words(untouched)[0], keep)
        pw = prev.view(np.uint32).reshape(vh, 6, nrhs, 4)
        for i, d in enumerate(dst):
            if i == 1:
                continue
            w, stride, _ = _words(d)
            want = before[i].copy()
            for k in range(6):
                want[k * stride:k * stride + vh] = pw[:, k, i]
            assert np.array_equal(w, want), "unpack column %d" % i
        assert np.array_equal(blk.save(), prev)
    finally:
        F.free()
        S.free()


@pytest.mark.parametrize("parity", [-1, 0, 1])
@pytest.mark.parametrize("nrhs", [4, 8])
@pytest.mark.parametrize("name", sorted(LATTICES))
def test_full_field_pack(qa, name, nrhs, parity):
    """blockPack / blockUnpack of full fp32 fields (block_pack_kernel<*, 4>, pair-major branch): both halves (block of V sites, site
    parity * Vh + x) or one half (block of Vh sites), bit for bit against the raw spinor images; the other half is left alone on unpack"""
    X, vh, ip = _lattice(qa, name)
    ns = 2 * vh if parity < 0 else vh
    S, F = Spinors(qa, ip, qa.QUDA_FULL_SITE_SUBSET, 2 * vh * 24, 3200 + nrhs), Blocks(qa, (ns, 12, nrhs))
    try:
        sp = [S.new() for _ in range(nrhs)]
        blk = F.new(np.random.default_rng(3300).standard_normal((nrhs, ns * 24)))
        halves = [0, 1] if parity < 0 else [parity]

        def image(fields):
            img = np.zeros((ns, 6, nrhs, 4), dtype=np.uint32)
            for i, f in enumerate(fields):
                w, stride, odd = _words(f)
                for h, par in enumerate(halves):
                    for k in range(6):
                        img[h * vh:(h + 1) * vh, k, i, :] = w[par * odd + k * stride:par * odd + k * stride + vh]
            return img.reshape(-1, 4)

        qa.block_pack(blk, sp, parity)
        got = blk.save().view(np.uint32).reshape(-1, 4)
        want = image(sp)
        assert np.array_equal(got, want), "pack: %d words differ" % int(np.sum(np.any(got != want, axis=1)))
        dst = [S.new() for _ in range(nrhs)]
        before = [_words(d)[0].copy() for d in dst]
        qa.block_unpack(blk, dst, parity)
        assert np.array_equal(image(dst), want)
        for i, d in enumerate(dst):      # nothing else of the field was written
            w, stride, odd = _words(d)
            expect = before[i].copy()
            for par in halves:
                for k in range(6):
                    expect[par * odd + k * stride:par * odd + k * stride + vh] = want.reshape(ns, 6, nrhs, 4)[halves.index(par) * vh:(halves.index(par) + 1) * vh, k, i]
            assert np.array_equal(w, expect), "unpack field %d" % i
    finally:
        F.free()
        S.free()


# ---- epilogue sums of the fine stencil ----
S0, A0, K1, A1 = 0.9, 0.3, -0.021, -0.17
EPILOGUE_CONFIGS = [("6^4", 18, 0), ("6^4", 12, 0), ("4^4", 18, 0), ("6^4", 18, 15), ("6^4", 12, 15)]
EPILOGUE_CASES = [(8, 1), (8, 2), (8, 3), (4, 3)]


def _epilogue_case(qa, F, name, recon, mask, nrhs, mode):
    """the launches of one case with the checks (a), (b), (c) on each; returns what the MR update of (d) needs"""
    X, vh, ip = _lattice(qa, name, recon, mask)
    shape = (vh, 12, nrhs)
    assert F.shape == shape
    nghost = qa.block_ghost_panels(True)
    assert (nghost > 0) == (mask != 0)
    rng = np.random.default_rng(4000 + 10 * nrhs + mode)
    r = F.new(B.operand(rng, *shape, k=0, zero_col=ZERO_COL))                       # the same-parity input of the first launch
    other = [F.new(B.operand(rng, *shape, k=1 + j, zero_col=ZERO_COL), nghost) for j in range(2)]
    a = F.new(B.operand(rng, *shape, k=3, zero_col=ZERO_COL))
    plain, w1, w2 = (F.new(np.zeros((nrhs, vh * 24))) for _ in range(3))
    what = "epilogue %s recon %d mask %d mode %d" % (name, recon, mask, mode)

    def launch(out, same, oth, m, dev=False):
        return qa.block_fine_apply(out, same, oth, 1, S0, A0, K1, A1, mode=m, dot_a=a if m in (1, 2) else None, device_sums=dev)

    def checked(out, same, oth, m):
        launch(plain, same, oth, 0)
        sums = launch(out, same, oth, m)
        vals = {"out": F.read(out), "same": F.read(same), "a": F.read(a)}
        if not np.array_equal(vals["out"], F.read(plain)):
            raise R.Mismatch("%s: out differs from the launch without sums" % what)
        assert np.any(vals["out"][0]) and not np.any(vals["out"][ZERO_COL])
        recs = B.check_epilogue_sums(m, sums, vals)
        for dev in (False, True):
            again = launch(out, same, oth, m, dev)
            if not np.array_equal(again, sums):
                raise R.Mismatch("%s: sums differ on repetition (device sums %d)" % (what, dev))
        report(recs, what + " launch mode %d" % m, shape)
        return sums, vals

    if mode == 1:
        checked(w1, r, other[0], 1)
        return None
    s3, v1 = checked(w1, r, other[0], 3)
    steps, s7 = 1, None
    vecs = {"x": F.read(other[0]), "r": F.read(other[1]), "rin": v1["same"], "w1": v1["out"]}
    if mode == 2:      # the second launch of a paired step: same = w1, a = r
        a.load(r.image)
        s7, v2 = checked(w2, w1, other[1], 2)
        steps, vecs["w2"] = 2, v2["out"]
    return dict(what=what, shape=shape, steps=steps, s3=s3, s7=s7, vecs=vecs, rin=r, w1=w1, w2=w2 if steps == 2 else None)


@pytest.mark.parametrize("nrhs,mode", EPILOGUE_CASES)
@pytest.mark.parametrize("name,recon,mask", EPILOGUE_CONFIGS, ids=lambda v: str(v))
def test_epilogue_sums(qa, name, recon, mask, nrhs, mode):
    """FineBlockDots modes 1, 2, 3 of one parity launch out = s0 (1 + i a0 g5) same + k1 (1 + i a1 g5) hops(other), s0 != 0:
    (a) out is bit-identical to the launch without sums; (b) every sum against the longdouble sum over the read-back out, same and a;
    (c) sums bit-identical on repetition and between fineBlockDotsFinish and fineBlockDotsFinishDev.  Mode 2 is the second launch of a
    paired MR step (same = w1 of a mode-3 launch, a = r).  Mask 15: every hop across a face goes through the ghost zone, and the sums
    are global sums"""
    F = Blocks(qa, (int(np.prod(LATTICES[name])) // 2, 12, nrhs))
    try:
        _epilogue_case(qa, F, name, recon, mask, nrhs, mode)
    finally:
        F.free()


@pytest.mark.parametrize("nrhs,mode", [c for c in EPILOGUE_CASES if c[1] != 1])
@pytest.mark.parametrize("name,recon,mask", EPILOGUE_CONFIGS, ids=lambda v: str(v))
def test_epilogue_sums_feed_the_mr_update(qa, name, recon, mask, nrhs, mode):
    """(d) mrUpdateDev (mode 3) / mr2UpdateDev (mode 3 + mode 2) fed with the epilogue's sums give the x and r they give with the longdouble
    sums of the same vectors, within the element bound 8 * 2^-24 T.

    This is the check that made fine_block_kernel take its site sums in fp64.  With the 24 products of a site added in fp32 the sums were
    within 0.04 of their own bound and moved alpha by 1e-9 to 5e-8 of |alpha| — in BOTH its parts, while the element bound is componentwise
    (T of Re(alpha r) is |Re alpha Re r| + |Im alpha Im r|): with alpha = 0.86 + 0.001..0.04 i an element with |Re r| << |Im r| saw that
    amplified by |alpha| / |Im alpha|, 20 to 700, and a1 of the paired step, whose numerator (A r1, r1) is a difference of O(1) terms formed
    from the sums, was off by up to 1e-6 of |a1|.  Measured error over bound then: one step 0.70 at 4 right-hand sides, 1.5 to 2.4 at 8;
    paired step 6.2 to 14.5.  The differences of the coefficients are printed (pytest -s)."""
    F = Blocks(qa, (int(np.prod(LATTICES[name])) // 2, 12, nrhs))
    try:
        c = _epilogue_case(qa, F, name, recon, mask, nrhs, mode)
        steps, vecs, what = c["steps"], c["vecs"], c["what"]
        exact = B.mr_sums(vecs["rin"], vecs["w1"], vecs.get("w2"))
        if steps == 2:
            for kn, kd in B.mr_condition(OMEGA, *exact):
                assert kn < B.MR_KAPPA_LIMIT and kd < B.MR_KAPPA_LIMIT, (kn, kd)
        x, rout = F.new(vecs["x"]), F.new(vecs["r"])
        ref, _ = B.mr_reference(steps, OMEGA, 0, vecs)
        runs = []
        for s3, s7 in ((c["s3"], c["s7"]), exact):
            F.reload(x)
            F.reload(rout)
            qa.block_mr_update(steps, OMEGA, 0, 1, s3, s7, x, rout, c["rin"], c["w1"], c["w2"])
            runs.append({"x": F.read(x), "r": F.read(rout)})
        after = dict(vecs)
        after.update(runs[1])
        report(B.check_mr(steps, OMEGA, 0, 1, vecs, after), what + " longdouble sums", c["shape"])
        ce, cx = B.mr_coefficients(OMEGA, c["s3"], c["s7"]), B.mr_coefficients(OMEGA, *exact)
        for i, (e, v) in enumerate(zip(ce, cx)):
            if abs(v[0]) > 0:
                print("BLOCK %s | rhs %d | a0 %.6f%+.6fi off by %.2e of |a0|, a1 %.6f%+.6fi off by %.2e of |a1|"
                      % (what, i, v[0].real, v[0].imag, abs(e[0] - v[0]) / abs(v[0]), v[1].real, v[1].imag, abs(e[1] - v[1]) / abs(v[1]) if abs(v[1]) > 0 else 0.0))
        recs = []
        for n in ("x", "r"):      # the run on the epilogue's sums against the run on the longdouble sums, T from the reference
            label = "%s mr%d %s, epilogue sums against longdouble sums" % (what, steps, n)
            err = np.abs(runs[0][n] - runs[1][n]).reshape(-1)
            b = np.asarray(R.ROUNDINGS * B.EPS32 * ref[n][1], dtype=np.float64).reshape(-1)
            print("BLOCK %s | %s | worst error over bound %.3f" % (what, label, float(np.max(np.where(b > 0, err / np.where(b > 0, b, 1), 0)))))
            recs.append(B._flat(label, runs[0][n], runs[1][n].astype(B.HP), ref[n][1]))
        report(recs, what, c["shape"])
    finally:
        F.free()
