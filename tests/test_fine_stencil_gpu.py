"""One parity launch of the multi-right-hand-side fine stencil (csrc/fine_block.hip fine_block_kernel through applyFineBlockParity) and the
dense clover-twist site matrices it applies (clover_twist_dense_kernel), through the hooks qudaAmdBlockFineApplySite and
qudaAmdCloverTwistDense, element by element against the fp64 reference of tests/fine_stencil_ref.py, whose docstring derives the bound
K 2^-24 T and whose self-test (tests/test_fine_stencil_ref.py) measures K and shows that the checker rejects a dropped boundary sign, swapped or
mis-signed twists, a transposed or misplaced site matrix, the wrong links, a missing dagger, exchanged right-hand sides and a y/z mix-up in a
ghost face.

Inputs go through host spinors: Spinor.load, then block_pack_parity at 4 and 8 right-hand sides and, because that kernel packs at most 10, block_pack
of one half of full spinors at 16, 24 and 32 (both pinned bit for bit in tests/test_block_kernels_gpu.py); the reference reads what Spinor.save
returns after the load.  Outputs come back through block_unpack_parity resp. block_unpack and save.  Operands as block_ref.operand: 10^u per
(site, right-hand side), u in [-3, 3], column 2 identically zero, one zero site per column.  On EVERY launch: every element within the bound;
the zero column exactly zero; the inputs bit-identical afterwards; the sentinel panels behind the Vh sites of `out` bit-identical (the tail
work-group writes nothing past the end); a second launch bit-identical.

Lattices — the smallest that reach each path, asserted through the hook's flag in test_case_reaches_what_it_is_for:
  6^4         Vh = 648, linear work-group order; the last work-group holds 8 sites at 4, 8 and 16 right-hand sides
  8x4x6x10    all four extents differ (a y/z mix-up in a ghost-face index moves panels); linear order at every width
  16x8x4x4    the XCD plane-tiled BlockOrder at 4, 8, 16, 24 and 32 right-hand sides
Links: fp32 18 reals with periodic and with antiperiodic t, fp32 12 reals with antiperiodic t (third row rebuilt, tsign_fwd / tsign_bwd); the
clover term is built on the device from the resident links at cuda_prec = 4 and read back, so the reference holds the device's own A.
Partition masks: 0 everywhere, 15 and 5 (the process its own neighbour: hops across those faces go through the ghost zone) on 8x4x6x10 and 6^4.
Coefficient cases: fine_stencil_ref.CASES.  The worst error in units of 2^-24 T is printed per case (pytest -s)."""
import importlib

import numpy as np
import pytest

import blas_ref as R
import block_ref as B
import fine_stencil_ref as F
from synth import smooth_gauge

pytestmark = pytest.mark.gpu

LATTICES = {"6^4": (6, 6, 6, 6), "8x4x6x10": (8, 4, 6, 10), "16x8x4x4": (16, 8, 4, 4)}
TILED = {"6^4": False, "8x4x6x10": False, "16x8x4x4": True}
LINKS = {"recon18-periodic": (18, False), "recon18-antiperiodic": (18, True), "recon12-antiperiodic": (12, True)}
CONFIGS = [(lat, links, 0) for lat in LATTICES for links in LINKS] + [(lat, links, mask) for lat in ("8x4x6x10", "6^4") for mask in (15, 5) for links in LINKS]
WIDTHS = (4, 8, 16, 24, 32)
NMAX, ZERO_COL, SENTINEL_PANELS = 32, 2, 5
_resident, _inputs = {}, {}


@pytest.fixture(scope="module")
def qa():
    mod = importlib.import_module("quda-qkxtm-multigrid_amd")
    mod.init(0)
    yield mod
    mod.lib().qudaAmdSetPartitionMask(0)
    mod.end()


def sites_per_group(nrhs):
    return 8 if nrhs == 24 else 256 // nrhs


def _lattice(qa, lat, links, mask):
    """fp32 links and the device-built fp32 clover term resident (one load per configuration); returns X, Vh, the parameter set of the host
    spinors and the clover term read back from the device (host packed order)"""
    X = LATTICES[lat]
    vh = int(np.prod(X)) // 2
    key = (lat, links, mask)
    if _resident.get("key") != key:
        _resident.clear()
        recon, anti = LINKS[links]
        qa.lib().qudaAmdSetPartitionMask(mask)
        host = smooth_gauge(X, 0.35)
        gp = qa.gauge_param(X, cuda_prec=4, recon=qa.QUDA_RECONSTRUCT_12 if recon == 12 else qa.QUDA_RECONSTRUCT_NO,
                            t_boundary=qa.QUDA_ANTI_PERIODIC_T if anti else qa.QUDA_PERIODIC_T)
        qa.load_gauge(F.fold_antiperiodic(host, X) if anti else host, gp)
        ipc = qa.invert_param(qa.QUDA_TWISTED_CLOVER_DSLASH, F.KAPPA, 0.05, +1, "ee", 0, cuda_prec=4)
        ipc.clover_coeff = F.CSW_COEFF
        ipc.compute_clover, ipc.return_clover = 1, 1
        clover = np.zeros(2 * vh * 72)
        qa.load_clover(clover, None, ipc)
        assert np.any(clover) and np.array_equal(clover, clover.astype(np.float32).astype(np.float64))
        _resident.update(key=key, clover=clover)
    ip = qa.invert_param(qa.QUDA_TWISTED_MASS_DSLASH, F.KAPPA, 0.05, +1, "ee", 0, cuda_prec=4)
    return X, vh, ip, _resident["clover"]


def _host_operands(lat):
    """same[p], other[p]: NMAX columns each, living on parity p; one draw per lattice"""
    vh = int(np.prod(LATTICES[lat])) // 2
    rng = np.random.default_rng(6000 + vh)
    return {(k, p): B.operand(rng, vh, 12, NMAX, k=2 * k + p, zero_col=ZERO_COL) for k in (0, 1) for p in (0, 1)}


def _reference(oracle, lat, links, loaded):
    """hop sums and their term sums of both parities for the NMAX columns: once per (lattice, links), never modified.  `loaded`: the operands
    as Spinor.save returned them after the load; they must be the same on every visit"""
    key = (lat, links)
    if key not in _inputs:
        X = LATTICES[lat]
        recon, anti = LINKS[links]
        host = smooth_gauge(X, 0.35)
        dev = F.device_links(F.fold_antiperiodic(host, X) if anti else host, X, recon, anti)
        oracle.set_threads(8)
        try:
            hops = {p: F.hop_sum(oracle, dev, X, p, loaded[1, 1 - p]) for p in (0, 1)}
        finally:
            oracle.set_threads(1)
        _inputs[key] = dict(loaded={k: v.copy() for k, v in loaded.items()}, hops=hops)
    ref = _inputs[key]
    for k in loaded:
        assert np.array_equal(loaded[k], ref["loaded"][k]), "the loaded operands differ from those the reference was computed for"
    return ref["hops"]


class Fields:
    """host spinors on the device and block fields, freed together.  A field of the tests is a FULL spinor [even | odd]: blockPack / blockUnpack
    with a parity argument move one half of it at any width; at 4 and 8 right-hand sides the test goes through single-parity spinors and
    blockPackParity / blockUnpackParity instead, which cannot pack more than 10 (tests/test_block_kernels_gpu.py pins all four bit for bit)"""

    def __init__(self, qa, ip, vh):
        self.qa, self.ip, self.vh, self.spinors, self.blocks = qa, ip, vh, [], []

    def spinor(self, host):
        f = self.qa.Spinor(4, self.qa.QUDA_PARITY_SITE_SUBSET if host.size == self.vh * 24 else self.qa.QUDA_FULL_SITE_SUBSET)
        self.spinors.append(f)
        return f.load(host, self.ip)

    def saved(self, f, full=False):
        return f.save(self.ip, np.empty((2 if full else 1) * self.vh * 24))

    def block(self, nrhs, nghost, image=None):
        b = self.qa.BlockField(self.vh, 12, nrhs, nghost)
        self.blocks.append(b)
        return b.load(np.zeros(b.nreal, dtype=np.float32) if image is None else image)

    def free(self):
        for f in self.blocks + self.spinors:
            f.free()
        self.blocks, self.spinors = [], []


PARITY_PACK_MAX = 8


def _bits(a):
    return np.asarray(a, dtype=np.float32).view(np.uint32)


def _sentinel(nreal):
    return ((np.arange(nreal) % 251) + 1000.0).astype(np.float32)


@pytest.mark.parametrize("lat", sorted(LATTICES))
def test_case_reaches_what_it_is_for(qa, lat):
    """the work-group order the launcher chose (the hook's flag, from makeBlockOrder itself), the size of the last work-group and the ghost zone"""
    X, vh, ip, _ = _lattice(qa, lat, "recon18-periodic", 0)
    assert qa.block_ghost_panels(True) == 0
    fl = Fields(qa, ip, vh)
    try:
        for w in WIDTHS:
            out, other = fl.block(w, 0), fl.block(w, 0)
            flags = qa.block_fine_apply_site(out, None, other, 0, 0.0, 0.0, 1.0, 0.0)
            assert bool(flags & 1) == TILED[lat], (lat, w, flags)
            assert not np.any(out.save())
        tails = {w: vh % sites_per_group(w) for w in WIDTHS}
        if lat == "6^4":
            assert vh == 648 and tails == {4: 8, 8: 8, 16: 8, 24: 0, 32: 0}
        else:
            assert not any(tails.values())
        if lat == "8x4x6x10":
            assert len(set(X)) == 4
    finally:
        fl.free()
    if lat != "16x8x4x4":
        for mask in (15, 5):
            _lattice(qa, lat, "recon18-periodic", mask)
            assert qa.block_ghost_panels(True) > 0
        qa.lib().qudaAmdSetPartitionMask(0)
        _resident.clear()


@pytest.mark.parametrize("lat,links,mask", CONFIGS, ids=lambda v: str(v))
def test_parity_launch_against_the_reference(qa, oracle, lat, links, mask):
    X, vh, ip, clover = _lattice(qa, lat, links, mask)
    nghost = qa.block_ghost_panels(True)
    assert (nghost > 0) == (mask != 0)
    fl = Fields(qa, ip, vh)
    try:
        host = _host_operands(lat)
        n = vh * 24
        full = {k: [fl.spinor(np.concatenate([host[k, 0][i], host[k, 1][i]])) for i in range(NMAX)] for k in (0, 1)}
        half = {(k, p): [fl.spinor(host[k, p][i]) for i in range(PARITY_PACK_MAX)] for k in (0, 1) for p in (0, 1)}
        back = {k: np.stack([fl.saved(f, full=True) for f in full[k]]) for k in (0, 1)}
        loaded = {(k, p): np.ascontiguousarray(back[k][:, p * n:(p + 1) * n]) for k in (0, 1) for p in (0, 1)}
        for kp, fields in half.items():
            assert np.array_equal(np.stack([fl.saved(f) for f in fields]), loaded[kp][:PARITY_PACK_MAX])
        for k in host:
            assert not np.any(loaded[k][ZERO_COL]) and np.any(loaded[k][0])
        hops = _reference(oracle, lat, links, loaded)
        mats = {(p, inv): F.dense_matrices(oracle, clover, X, p, F.A_SITE, inv) for p in (0, 1) for inv in (False, True)}
        same_c = {p: F.to_complex(loaded[0, p], vh) for p in (0, 1)}
        want = {}
        for c, (name, s0, a0, k1, a1, tmode, inv) in enumerate(F.CASES):
            for p in (0, 1):
                want[c, p] = F.combine(same_c[p] if s0 else None, hops[p][0], hops[p][1], s0, a0, k1, a1, tmode, mats[p, inv] if tmode else None)
        out_full = [fl.spinor(np.zeros(2 * n)) for _ in range(NMAX)]
        out_half = [fl.spinor(np.zeros(n)) for _ in range(PARITY_PACK_MAX)]
        worst = {}
        for w in WIDTHS:
            blk = {}
            for k, p in loaded:
                blk[k, p] = fl.block(w, nghost if k == 1 else 0)
                if w <= PARITY_PACK_MAX:
                    qa.block_pack_parity(blk[k, p], half[k, p][:w])
                else:
                    qa.block_pack(blk[k, p], full[k][:w], p)
            before = {k: b.save() for k, b in blk.items()}
            local = vh * 12 * w * 2
            sentinel = _sentinel(2 * (vh + SENTINEL_PANELS) * 12 * w)
            out, again = fl.block(w, SENTINEL_PANELS, sentinel), fl.block(w, SENTINEL_PANELS, sentinel)
            for c, (name, s0, a0, k1, a1, tmode, inv) in enumerate(F.CASES):
                for p in (0, 1):
                    what = "%s %s mask %d | %d rhs | %s | parity %d" % (lat, links, mask, w, name, p)
                    same, other = (blk[0, p] if s0 else None), blk[1, 1 - p]
                    out.load(sentinel)
                    again.load(sentinel)
                    flags = qa.block_fine_apply_site(out, same, other, p, s0, a0, k1, a1, tmode, F.A_SITE, inv)
                    assert bool(flags & 1) == TILED[lat], what
                    raw = out.save()
                    if not np.array_equal(_bits(raw[local:]), _bits(sentinel[local:])):
                        raise R.Mismatch("%s: the panels behind the last site were written" % what)
                    if not np.array_equal(_bits(blk[1, 1 - p].save()[:local]), _bits(before[1, 1 - p][:local])):
                        raise R.Mismatch("%s: in_other changed" % what)
                    if same is not None and not np.array_equal(_bits(same.save()), _bits(before[0, p])):
                        raise R.Mismatch("%s: in_same changed" % what)
                    qa.block_fine_apply_site(again, same, other, p, s0, a0, k1, a1, tmode, F.A_SITE, inv)
                    if not np.array_equal(_bits(again.save()), _bits(raw)):
                        raise R.Mismatch("%s: a second launch differs" % what)
                    if w <= PARITY_PACK_MAX:
                        qa.block_unpack_parity(out, out_half[:w])
                        got = np.stack([fl.saved(f) for f in out_half[:w]])
                    else:
                        qa.block_unpack(out, out_full[:w], p)
                        got = np.stack([fl.saved(f, full=True)[p * n:(p + 1) * n] for f in out_full[:w]])
                    if np.any(got[ZERO_COL] != 0.0):
                        raise R.Mismatch("%s: the zero column is not zero" % what)
                    assert np.any(got[0]) and np.any(got[w - 1]), what
                    rec = F.check_launch(what, got, want[c, p][0][:w], want[c, p][1][:w], F.K_SITE if tmode else F.K_PLAIN)
                    worst[c] = max(worst.get(c, 0.0), rec[3])
            for b in list(blk.values()) + [out, again]:
                b.free()
        for c, case in enumerate(F.CASES):
            print("FINE %s %s mask %d | %-46s | worst error %.3f x 2^-24 T, allowed %d" % (lat, links, mask, case[0], worst[c], F.K_SITE if case[5] else F.K_PLAIN))
    finally:
        fl.free()


@pytest.mark.parametrize("lat,links,mask", [("8x4x6x10", "recon18-periodic", 0), ("6^4", "recon12-antiperiodic", 15), ("16x8x4x4", "recon18-antiperiodic", 0)],
                         ids=lambda v: str(v))
def test_dense_site_matrices(qa, oracle, lat, links, mask):
    """clover_twist_dense_kernel on the resident fp32 clover term: direct matrices bit-identical to the fp32 entries of A + i a s, inverses
    within one fp32 rounding of numpy's fp64 inverse; both parities, a of both signs and a = 0"""
    X, vh, ip, clover = _lattice(qa, lat, links, mask)
    for p in (0, 1):
        for a in (F.A_SITE, -0.31, 0.0):
            for inv in (False, True):
                want = F.dense_matrices(oracle, clover, X, p, a, inv)
                got = qa.clover_twist_dense(p, a, inv, vh)
                rec = F.check_dense("dense %s %s mask %d | parity %d a %+.2f %s" % (lat, links, mask, p, a, "inverse" if inv else "direct"), got, want, inv)
                print("FINE %-72s | worst error over bound %.3f" % (rec[0], rec[3]))
