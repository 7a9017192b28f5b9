"""The 16-bit kernels and the 12- and 8-real link reconstructions on the device's OWN stored operands: every image is read back raw
(qudaAmdRawDeviceCopy at the addresses of Spinor.raw_info, gauge_raw_info, clover_raw_info), decoded to float64 by tests/stored_ref.py, and the
reference of a launch is evaluated on the decoded links, input, A / Ainv and xpay operand.  What is left between kernel and reference is the
kernel's fp32 arithmetic and ONE rounding of the output, both bounded per element (tests/stored_ref.py; constants measured in
tests/test_stored_ref.py, which also shows that every planted decoder error is caught by the checks used here).

  a  link storage: all 16 blocks of the nine (precision, reconstruct) formats, periodic and antiperiodic, against the host links with the
     neighbour of the backward blocks from coordinate arithmetic here; the sloppy and preconditioner copies; the forced-halo load in a child
  b  one launch at a time through Dirac.dslash / dslash_xpay / M on resident Spinors (stored_ref.launches): 16-bit with 18, 12, 8 reals, and fp32
     with 12 and 8 reals; the two launches of the preconditioned operators with the intermediate field read back raw
  c  clover_invert_kernel: decoded Ainv against the fp64 inverse of the decoded A, block by block, and the trlog sums
  d  one partitioned 16-bit case (the process its own neighbour in all four dimensions)
Lattices: 2^4 (every neighbour wraps, one partial work-group) and 12 x 6 x 10 x 4 (Vh = 1440, Xh = 6).  Inputs: stored_ref.operands, 10^u per
site with u in [-2, 2] and one zero site per parity, the xpay operand with a scale profile of its own.  pytest -s prints the worst ratio of
error to bound per case."""
import importlib
import os
import subprocess
import sys

import numpy as np
import pytest

import stored_ref as S

pytestmark = pytest.mark.gpu

FORMATS = [(p, r) for p in (8, 4, 2) for r in (18, 12, 8)]
_fields = {}


@pytest.fixture(scope="module")
def qa():
    mod = importlib.import_module("quda-qkxtm-multigrid_amd")
    mod.init(0)
    yield mod
    mod.lib().qudaAmdSetPartitionMask(0)
    mod.end()


def host_fields(oracle, lat, anti):
    """the seeded host links and clover term of a lattice, and the 16 blocks the links ask for; made once, never modified"""
    key = (lat, anti)
    if key not in _fields:
        X = S.LATTICES[lat]
        gauge, _, clover = oracle.make_fields(list(X), seed=S.SEEDS[lat], antiperiodic_t=anti, clover=True)
        Wh = expected_blocks(gauge, X)
        for a in (gauge, clover, Wh):
            a.setflags(write=False)
        _fields[key] = (X, gauge, clover, Wh)
    return _fields[key]


def expected_blocks(gauge, X):
    """block 2 mu of site x = U_mu(x), block 2 mu + 1 = U_mu(x - mu)^dagger, the neighbour from the coordinates: checkerboard index
    ((t Z + z) Y + y) Xh + xh with x = 2 xh + ((y + z + t + parity) & 1)"""
    X = [int(v) for v in X]
    vh = int(np.prod(X)) // 2
    u = S.to_matrix(np.asarray(gauge).reshape(4, 2, vh, 18))
    W = np.empty((2, 8, vh, 3, 3), dtype=np.complex128)
    idx = np.arange(vh)
    xh, y, z, t = idx % (X[0] // 2), idx // (X[0] // 2) % X[1], idx // (X[0] // 2 * X[1]) % X[2], idx // (X[0] // 2 * X[1] * X[2])
    for p in range(2):
        c = [2 * xh + ((y + z + t + p) & 1), y, z, t]
        for mu in range(4):
            n = list(c)
            n[mu] = (c[mu] - 1) % X[mu]
            assert np.all((n[0] + n[1] + n[2] + n[3]) % 2 == 1 - p)
            nb = (((n[3] * X[2] + n[2]) * X[1] + n[1]) * X[0] + n[0]) // 2
            W[p, 2 * mu] = u[mu, p]
            W[p, 2 * mu + 1] = u[mu, 1 - p][nb].conj().transpose(0, 2, 1)
    return W


def load_links(qa, X, gauge, prec, recon, anti, **kw):
    qa.load_gauge(gauge, qa.gauge_param(X, cuda_prec=prec, recon=recon, t_boundary=qa.QUDA_ANTI_PERIODIC_T if anti else qa.QUDA_PERIODIC_T, **kw))


def link_image(qa, which, X, anti):
    i = qa.gauge_raw_info(which)
    vh = int(np.prod(X)) // 2
    assert i["Vh"] == vh and i["stride"] >= vh and i["bytes"] == 16 * i["link_bytes"] and i["link_bytes"] >= i["stride"] * i["reconstruct"] * i["precision"]
    assert i["data"] % 256 == 0
    raw = qa.raw_device_copy(i["data"], i["bytes"])
    return (raw, i) + S.decode_links(raw, i, X, anti)


def spinor_image(qa, f, parity=0):
    i = f.raw_info()
    raw = qa.raw_device_copy(i["v"], i["bytes"])
    nraw = qa.raw_device_copy(i["norm"], i["norm_bytes"]) if i["precision"] == 2 else None
    return S.decode_spinor(raw, nraw, i, parity)


def clover_images(qa, which=0, as_loaded=False):
    i = qa.clover_raw_info(which)
    out = []
    for data, norm in (("A", "norm"), ("Ainv", "invNorm")):
        raw = qa.raw_device_copy(i[data], 2 * i["parity_bytes"])
        nraw = qa.raw_device_copy(i[norm], 4 * i["stride"] * 4) if i["precision"] == 2 else None
        out.append(S.decode_clover(raw, nraw, i, as_loaded=as_loaded))
    return i, out[0], out[1]


# ---------------------------------------------------------------------------------------------------------------------------------------------
# a. link storage
# ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("anti", [False, True], ids=["periodic", "antiperiodic"])
@pytest.mark.parametrize("prec,recon", FORMATS)
def test_link_storage(qa, oracle, prec, recon, anti):
    """all 16 blocks of the precise field on both lattices (stored_ref.check_links states and derives the bounds): stored reals bit-identical
    (fp64, fp32 to astype(float32)) or within the half step (16-bit); rebuilt rows and 8-real links within the rounding of the stored reals pushed
    through the decode, which for 8 reals carries 1 / rs"""
    for lat in sorted(S.LATTICES):
        X, gauge, _, Wh = host_fields(oracle, lat, anti)
        load_links(qa, X, gauge, prec, recon, anti)
        raw, i, W, stored, rs = link_image(qa, 0, X, anti)
        assert (i["precision"], i["reconstruct"]) == (prec, recon)
        res = S.check_links("%s %d/%d" % (lat, prec, recon), W, stored, rs, Wh, X, prec, recon, anti)
        print("%s prec %d recon %d %s: rebuilt entries worst error / bound %.3f%s" % (lat, prec, recon, "antiperiodic" if anti else "periodic", res[1],
                                                                                       "; fp64 8-real error / (2^-53 / rs) = %.1f" % res[2] if (prec, recon) == (8, 8) else ""))
        if recon != 18 and anti:      # the folded sign is where the format puts it: the boundary links themselves are negated host links
            t = S.time_slice(X, W.shape[2])
            assert np.max(np.abs(W[:, 6][:, t == X[3] - 1] - Wh[:, 6][:, t == X[3] - 1])) < 1e-3


def test_sloppy_and_preconditioner_copies(qa, oracle):
    """one mixed load: fp64 18-real precise, fp32 8-real sloppy, 16-bit 12-real preconditioner links, each image checked like the precise one"""
    X, gauge, _, Wh = host_fields(oracle, "12x6x10x4", True)
    load_links(qa, X, gauge, 8, 18, True, prec_sloppy=4, recon_sloppy=8, prec_precondition=2, recon_precondition=12)
    for which, (prec, recon) in enumerate([(8, 18), (4, 8), (2, 12)]):
        raw, i, W, stored, rs = link_image(qa, which, X, True)
        assert (i["precision"], i["reconstruct"]) == (prec, recon), (which, i)
        print(S.check_links("copy %d: %d/%d" % (which, prec, recon), W, stored, rs, Wh, X, prec, recon, True))


def test_forced_halo_load_is_bit_identical():
    """QUDA_AMD_FORCE_GAUGE_HALO=1 with partition mask 15 takes the backward links of the x_d = 0 faces from the packed ghost slices: the images
    (fp32 12-real, 16-bit 8-real) must be those of the unpartitioned load.  The variable is read once per process: a fresh child"""
    env = dict(os.environ, QUDA_AMD_FORCE_GAUGE_HALO="1")
    r = subprocess.run([sys.executable, os.path.join(os.path.dirname(os.path.abspath(__file__)), "stored_halo_child.py")], env=env, capture_output=True, text=True, timeout=120)
    out = r.stdout + r.stderr
    assert r.returncode == 0, out[-2000:]
    assert out.count("IDENTICAL") == 2, out[-2000:]


# ---------------------------------------------------------------------------------------------------------------------------------------------
# b. one launch at a time
# ---------------------------------------------------------------------------------------------------------------------------------------------
class Resident:
    """links, clover term and operands of one configuration on the device, with what the device stores of them decoded"""

    def __init__(self, qa, oracle, lat, prec, recon, anti, mask=0):
        self.qa, self.prec, self.recon, self.mask = qa, prec, recon, mask
        self.X, gauge, clover, _ = host_fields(oracle, lat, anti)
        self.vh = int(np.prod(self.X)) // 2
        qa.lib().qudaAmdSetPartitionMask(mask)
        load_links(qa, self.X, gauge, prec, recon, anti)
        _, _, self.W, _, self.rs = link_image(qa, 0, self.X, anti)
        self.ipc = self.ip(dict(op="tmc", flavor=+1, dagger=0, matpc="ee", pc=True))
        qa.load_clover(clover, None, self.ipc)
        ci, (A, _), (Ainv, _) = clover_images(qa, 0)
        assert ci["twisted"] == 1 and ci["precision"] == prec
        self.A, self.Ainv = S.clover_matrices(A), S.clover_matrices(Ainv)
        self.delta = S.E8 * S.EPS32 / self.rs if recon == 8 else None
        self.spinors = []
        host = [S.operands(self.X, w) for w in (0, 1)]
        ip = self.ip(dict(op="tm", flavor=+1, dagger=0, matpc="ee", pc=True))
        self.inp = [self.spinor().load(host[0][p].reshape(-1), ip) for p in (0, 1)]
        self.xop = [self.spinor().load(host[1][p].reshape(-1), ip) for p in (0, 1)]
        ipf = self.ip(dict(op="tm", flavor=+1, dagger=0, matpc="ee", pc=False))
        self.full = self.spinor(True).load(host[0].reshape(-1), ipf)
        self.out, self.tmp, self.fout = self.spinor(), self.spinor(), self.spinor(True)
        self.inp_dec = [spinor_image(qa, f) for f in self.inp]
        self.xop_dec = [spinor_image(qa, f) for f in self.xop]
        self.full_dec = [spinor_image(qa, self.full, p) for p in (0, 1)]
        for p in (0, 1):      # the zero site decodes to zero, with scale 0 in 16-bit; both parities of the full field hold what the parity fields hold
            zero = ~np.any(host[0][p], axis=1)
            assert np.sum(zero) == 1 and not np.any(self.inp_dec[p][0][zero])
            assert prec != 2 or not np.any(self.inp_dec[p][1][zero])
            assert np.array_equal(self.full_dec[p][0], self.inp_dec[p][0])

    def spinor(self, full=False):
        f = self.qa.Spinor(self.prec, self.qa.QUDA_FULL_SITE_SUBSET if full else self.qa.QUDA_PARITY_SITE_SUBSET)
        self.spinors.append(f)
        return f

    def ip(self, c):
        qa = self.qa
        kind = {"wilson": qa.QUDA_WILSON_DSLASH, "tm": qa.QUDA_TWISTED_MASS_DSLASH, "tmc": qa.QUDA_TWISTED_CLOVER_DSLASH}[c["op"]]
        return qa.invert_param(kind, S.KAPPA, S.MU, c["flavor"] or +1, c["matpc"], c["dagger"], cuda_prec=self.prec,
                               solution_type=qa.QUDA_MATPC_SOLUTION if c["pc"] else qa.QUDA_MAT_SOLUTION)

    def set_flavor(self, c):
        for f in self.spinors:
            self.qa.lib().qudaAmdSpinorSetTwist(f.h, self.qa.QUDA_TWIST_MINUS if c["flavor"] == -1 else self.qa.QUDA_TWIST_PLUS)

    def check(self, label, f, parity, inp, arg, x=None, field_parity=0):
        """the output field f of a launch onto `parity` against the reference on the decoded operands; returns the worst ratios"""
        ghost = S.ghost_error(self.X, parity, inp, self.mask, arg["mode"], arg["a"], arg["dagger"]) if self.mask else None
        want, T, extra = S.launch(self.W, self.X, parity, inp, arg["mode"], arg["a"], arg["b"], arg["k"], x=x, dagger=arg["dagger"],
                                  A=self.A[parity], Ainv=self.Ainv[parity], delta=None if self.delta is None else self.delta[parity], ghost=ghost)
        k = S.K16_SITE if S.uses_site_matrices(arg["mode"]) else S.K16_PLAIN
        dec, scale = spinor_image(self.qa, f, field_parity)
        if self.prec == 2:
            return S.check_stored16(label, dec, scale, want, T, extra, k)[1:]
        return (S.check_stored32(label, dec, want, T, extra, k)[1], 0.0)

    def run(self, c):
        """every launch of case c (both parities); returns the worst (value, scale) ratios"""
        qa, arg = self.qa, S.kernel_args(c)
        self.set_flavor(c)
        d = qa.Dirac(self.ip(c), pc=c["pc"])
        worst = [0.0, 0.0]
        try:
            if c["call"] == "M":
                d.M(self.fout, self.full)
                for parity in (0, 1):
                    r = self.check("%s parity %d" % (S.launch_name(c), parity), self.fout, parity, self.full_dec[1 - parity][0], arg, x=self.full_dec[parity][0], field_parity=parity)
                    worst = [max(a, b) for a, b in zip(worst, r)]
                return worst
            for parity in (0, 1):
                if c["call"] == "dslash":
                    d.dslash(self.out, self.inp[1 - parity], parity)
                else:
                    d.dslash_xpay(self.out, self.inp[1 - parity], parity, self.xop[parity], S.KX)
                r = self.check("%s parity %d" % (S.launch_name(c), parity), self.out, parity, self.inp_dec[1 - parity][0], arg, x=self.xop_dec[parity][0] if arg["xpay"] else None)
                worst = [max(a, b) for a, b in zip(worst, r)]
            return worst
        finally:
            d.free()

    def free(self):
        for f in self.spinors:
            f.free()
        self.qa.lib().freeCloverQuda()
        self.qa.lib().qudaAmdSetPartitionMask(0)


CONFIGS = ([("12x6x10x4", 2, r, a) for r in (18, 12, 8) for a in (False, True)] + [("2^4", 2, r, True) for r in (18, 12, 8)]
           + [("12x6x10x4", 4, r, a) for r in (12, 8) for a in (False, True)])


@pytest.mark.parametrize("lat,prec,recon,anti", CONFIGS, ids=lambda v: str(v))
def test_single_launches(qa, oracle, lat, prec, recon, anti):
    """every launch of stored_ref.launches(): Wilson, twisted mass (both flavours, dagger 0 / 1, both parities, ee and eeasym) and twisted clover,
    Dirac.dslash, Dirac.dslash_xpay and the two xpay launches of the full operator's M.  Per output real k of site x with the device's scale n_x
        |dec(out) - ref| <= 0.5 n_x / 32767 (1 + 2^-10) + K 2^-24 T  (+ E8 2^-24 / rs over the eight links of the site for 8 reals)
        |n_x - max_k |ref|| <= K 2^-24 max_k T                        (+ the same)
    fp32 fields: the same without the output-rounding term"""
    res = Resident(qa, oracle, lat, prec, recon, anti)
    try:
        worst = {}
        for c in S.launches():
            r = res.run(c)
            key = (c["op"], c["call"])
            worst[key] = [max(a, b) for a, b in zip(worst.get(key, [0.0, 0.0]), r)]
        for key in sorted(worst):
            print("%s prec %d recon %d %s  %-6s %-6s worst error / bound %.3f, scale error / bound %.3f"
                  % (lat, prec, recon, "antiperiodic" if anti else "periodic", key[0], key[1], worst[key][0], worst[key][1]))
    finally:
        res.free()


@pytest.mark.parametrize("op", ["tm", "tmc"])
@pytest.mark.parametrize("recon", [18, 12, 8])
def test_two_step_operators(qa, oracle, op, recon):
    """the even-odd preconditioned operator as its two launches, out = in - kappa^2 (A^-1 D)(A^-1 D) in: the intermediate field is read back
    raw, so the reference of the second launch starts from what the device stored"""
    res = Resident(qa, oracle, "12x6x10x4", 2, recon, True)
    try:
        c = dict(op=op, flavor=+1, dagger=0, matpc="ee", pc=True, call="dslash")
        res.set_flavor(c)
        d = res.qa.Dirac(res.ip(c), pc=True)
        try:
            d.dslash(res.tmp, res.inp[0], 1)
            first = res.check("%s first launch" % op, res.tmp, 1, res.inp_dec[0][0], S.kernel_args(c))
            mid = spinor_image(res.qa, res.tmp)[0]
            d.dslash_xpay(res.out, res.tmp, 0, res.inp[0], -S.KAPPA ** 2)
            second = res.check("%s second launch" % op, res.out, 0, mid, S.kernel_args(dict(c, call="xpay"), kx=-S.KAPPA ** 2), x=res.inp_dec[0][0])
            print("%s recon %d: first launch %.3f / %.3f, second %.3f / %.3f of the bounds" % ((op, recon) + tuple(first) + tuple(second)))
        finally:
            d.free()
    finally:
        res.free()


# ---------------------------------------------------------------------------------------------------------------------------------------------
# c. the clover inverse
# ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", [8, 4, 2])
def test_clover_inverse(qa, oracle, prec):
    """clover_invert_kernel computes in fp64 whatever the storage (csrc/clover.hip): decoded Ainv against numpy's fp64 inverse of M = A^2 + mu2
    built from the A the kernel loaded (16-bit: the fp32 products of Planar<short>::load restated bit for bit), block by block, within
        C_INV n eps64 (|Ainv| (|A| |A| + mu2) |Ainv|)  +  one rounding to the storage type: 0 (fp64), 2^-24 |Ainv| (fp32), 0.5 n / 32767 + 3 2^-24 |Ainv|
    with n the device's scale of the (site, chiral block), itself within the first term (+ 2^-24) of max |Ainv|; trlog against numpy"""
    for lat in sorted(S.LATTICES):
        X, gauge, clover, _ = host_fields(oracle, lat, True)
        load_links(qa, X, gauge, prec, 18, True)
        ip = qa.invert_param(qa.QUDA_TWISTED_CLOVER_DSLASH, S.KAPPA, S.MU, +1, "ee", 0, cuda_prec=prec)
        ip.compute_clover_trlog = 1
        qa.load_clover(clover, None, ip)
        try:
            i, (A, _), (Ainv, scales) = clover_images(qa, 0, as_loaded=True)
            assert i["twisted"] == 1
            mu2 = (2 * S.KAPPA * S.MU) ** 2
            Am = S.clover_matrices(A)
            M = S.inverted_matrix(Am, mu2, True)
            want = np.linalg.inv(M)
            eb = S.pack_bound(S.C_INV * S.inverse_bound(Am, want, mu2, True))       # the elimination's bound of every packed real
            wp = S.pack_clover(want)
            if prec == 2:
                _, (_, _), (Ainv, scales) = clover_images(qa, 0)
                sc = scales.transpose(0, 2, 1)
                top = np.max(np.abs(wp), axis=-1)
                assert np.all(np.abs(sc - top) <= np.max(eb, axis=-1) + S.EPS32 * top), "scales of Ainv"
                bound = eb + S.half_step_bound(wp, sc[..., None])
            else:
                bound = eb + (S.EPS32 * np.abs(wp) if prec == 4 else 0.0)
            err = np.abs(Ainv - wp)
            ratio = float(np.max(err / bound))
            print("%s prec %d: Ainv worst error / bound %.3f (elimination part alone: worst error / it %.3g)" % (lat, prec, ratio, float(np.max(err / eb))))
            assert ratio <= 1.0, (lat, prec, ratio, np.argwhere(err > bound)[:4])
            logdet = np.sum(np.linalg.slogdet(M)[1], axis=(1, 2))
            got = np.array([ip.trlogA[0], ip.trlogA[1]])
            print("%s prec %d: trlog %s, numpy %s" % (lat, prec, got, logdet))
            assert np.all(np.abs(got - logdet) <= 1e-12 * np.sum(np.abs(np.linalg.slogdet(M)[1]), axis=(1, 2)))
        finally:
            qa.lib().freeCloverQuda()


# ---------------------------------------------------------------------------------------------------------------------------------------------
# d. partitioned
# ---------------------------------------------------------------------------------------------------------------------------------------------
def test_partitioned_16_bit(qa, oracle):
    """mask 15 on 12 x 6 x 10 x 4 with 18-real links: hops across a face read ghost half spinors that were quantised once more with a scale of
    their own: + 2.5 * 0.5 g / 32767 per partitioned hop (stored_ref.ghost_error); interior sites keep the bound of the unpartitioned launch"""
    res = Resident(qa, oracle, "12x6x10x4", 2, 18, True, mask=15)
    try:
        for c in (dict(op="wilson", flavor=0, dagger=0, matpc="ee", pc=True, call="dslash"), dict(op="tm", flavor=+1, dagger=0, matpc="ee", pc=True, call="xpay"),
                  dict(op="tm", flavor=-1, dagger=1, matpc="ee", pc=True, call="dslash"), dict(op="tmc", flavor=+1, dagger=0, matpc="ee", pc=True, call="dslash")):
            r = res.run(c)
            print("partitioned %s: worst error / bound %.3f, scale error / bound %.3f" % ((S.launch_name(c),) + tuple(r)))
        interior = np.all(S.ghost_error(res.X, 0, res.inp_dec[1][0], 15) == 0, axis=0)
        assert 0 < np.sum(interior) < res.vh
    finally:
        res.free()
