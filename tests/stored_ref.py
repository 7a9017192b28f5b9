"""The device's stored operands decoded to float64, and the fp64 reference of ONE stencil launch on them.  A plain module: numpy only, no GPU
and no library of the project.  The bytes come from qudaAmdRawDeviceCopy with the addresses of Spinor.raw_info, gauge_raw_info and
clover_raw_info; the matching encoders restate the loaders in numpy for the CPU tests (tests/test_stored_ref.py).

Layouts (csrc/device_io.h Planar<T, NR>): a block of NR reals per site is planes of N reals per site, N = 2 (fp64), 4 (fp32), 8 (16-bit);
    real k of site x:  element (k / N) stride N + x N + k % N                       for k < F = (NR / N) N
                       element F stride + x (NR - F) + (k - F)                      the narrower tail plane (fp32 18; 16-bit 18, 12, 36)
  spinor   24 reals (spin, colour, re / im); 16-bit: int16 * norm[x] / 32767 with one fp32 scale per site; the odd half of a full field at
           odd_offset bytes, its scales at odd_norm_offset bytes
  links    16 blocks [parity][2 mu + backward] of link_bytes each: block 2 mu of site x holds U_mu(x), block 2 mu + 1 U_mu(x - mu)^dagger, both
           as 18 reals (row-major), the 12 of rows 0 and 1, or the 8 of su3_reconstruct8; 16-bit: int16 / 32767, no scale array
           12 reals: row 2 = conj(row 0 x row 1) * sign
            8 reals: [arg U00, arg U20, U01, U02, U10] (16-bit: the two phases in units of pi), M = u0 V with u0 = sign:
                     rs = |U01|^2 + |U02|^2, |U00| = sqrt(max(1 - rs, 0)), |U20| = sqrt(max(1 - |U00|^2 - |U10|^2, 0)),
                     U11 = -(u0 conj(U20 U02) + A U01) / rs, U12 = (u0 conj(U20 U01) - A U02) / rs,        A = conj(U00) U10
                     U21 = (u0 conj(U10 U02) - B U01) / rs,  U22 = -(u0 conj(U10 U01) + B U02) / rs,       B = conj(U00) U20
           sign (csrc/dslash_arg.h fillDslashFields): -1 on the forward t block of the slice t = T - 1 and on the backward t block of t = 0 when the
           field is antiperiodic AND reconstructed; 18-real links store the folded sign themselves
  clover   [parity][chiral block][36 reals] of parity_bytes per parity, block chi at chi 36 sizeof(T) stride bytes; the 36 reals are the
           packed Hermitian 6 x 6 (6 real diagonal entries, 15 complex strictly-lower ones column by column); 16-bit: one fp32 scale per
           (site, block) at norm[parity 2 stride + chi stride + x].  Ainv (csrc/clover.hip clover_invert_kernel, fp64 Gauss-Jordan, then ONE
           rounding to the storage type) holds (A^2 + mu2)^-1 where clover_raw_info says `twisted`, else A^-1

Quantisation (Planar<short>::store, q16): int16 = rint(clamp(fl(v) * s)), s = fl(32767 / scale), all in fp32, round to nearest even.  Against
the fp64 value v the decoded int16 * scale / 32767 is off by at most
    0.5 scale / 32767 + 3 * 2^-24 |v|               (the rounding to int16, then fl(v), the division s and the product fl(v) s, 2^-24 each)
and links (fixed scale 1, s = 32767 exactly) by at most 0.5 / 32767 + 2^-23 |v|.

One launch (csrc/dslash.hip dslash_epilogue), H = the hop sum of the eight stored matrices of the site on the projected neighbours:
    plain              H                                   [xpay: x + k H]
    twist_inv          b (1 + i a g5) H                    [xpay: x + b (...)]
    twist_inv_dslash   b H((1 + i a g5) in)                [xpay: x + b (...)]
    twist_xpay         k H + (1 + i a g5) x
    clover_twist_inv   Ainv (A + i a g5) H                 [xpay: x + k (...)]
    clover_twist_xpay  k H + (A + i a g5) x
with the TERM SUM T of every element as tests/fine_stencil_ref.py defines it.  Bound of a 16-bit output real k of site x with the device's scale n_x:
    |dec(out) - ref| <= 0.5 n_x / 32767 (1 + 2^-10) + K 2^-24 T  [+ E8 2^-24 sum_d |.| / rs_d for 8-real links]
    |n_x - max_k |ref|| <= K 2^-24 max_k T                      [+ the largest of the site's 8-real (or ghost) terms: the scale is the largest output
                                                                  real of the kernel's own links, so it moves with them as the values do]
K16_PLAIN / K16_SITE are measured in tests/test_stored_ref.py as fine_stencil_ref measures K_PLAIN."""
import numpy as np

import fine_stencil_ref as F

N_OF = {8: 2, 4: 4, 2: 8}
DTYPE = {8: np.float64, 4: np.float32, 2: np.int16}
SHORT_MAX = 32767.0
EPS32 = 2.0 ** -24
K16_PLAIN, K16_SITE = 10, 9         # measured: tests/test_stored_ref.py test_stencil_constants
E8 = 128.0                          # measured: tests/test_stored_ref.py test_reconstruct8_in_fp32
RS_MIN = 0.02                       # condition on the test fields' 8-real links
C8_FP64 = 12.0                      # fp64 8-real decode against the host matrix, in units of 2^-53 cond8 (measured: tests/test_stored_ref.py)
C12_FP64 = 2.0 ** -47                # fp64 third row against the host matrix: the host fields are special-unitary to 3.4e-15 (measured likewise)
PHASE_ERR = {8: 2.0 ** -50, 4: 2.0 ** -21}    # atan2 of the loader against numpy's on the fp64 host entries, radians (fp32: 8 ulp of pi)
PLANTS = ("no_boundary_sign", "sign_on_forward_t0", "backward_not_daggered", "backward_from_forward_neighbour", "tail_full_stride",
          "phase_in_radians", "spinor_scale_next_site", "clover_scale_other_block")


def align(n, a=1024):
    return (int(n) + a - 1) // a * a


# ---- quantisation model ----
def quantise(v, scale):
    """q16 of v at `scale` (the largest representable magnitude; broadcast against v): fp32 arithmetic, round to nearest even, clamped; a zero
    scale gives zeros"""
    v32 = np.asarray(v, dtype=np.float64).astype(np.float32)
    sc = np.broadcast_to(np.asarray(scale, dtype=np.float32), v32.shape)
    with np.errstate(divide="ignore", invalid="ignore"):
        s = np.where(sc > 0, np.float32(SHORT_MAX) / np.where(sc > 0, sc, np.float32(1)), np.float32(0)).astype(np.float32)
    return np.rint(np.clip(v32 * s, -SHORT_MAX, SHORT_MAX)).astype(np.int16)


def half_step_bound(v, scale):
    """bound of |decode(quantise(v)) - v| at a per-site scale (docstring)"""
    return 0.5 * np.asarray(scale, dtype=np.float64) / SHORT_MAX + 3.0 * EPS32 * np.abs(v)


def link_step_bound(v):
    return 0.5 / SHORT_MAX + 2.0 * EPS32 * np.abs(v)


# ---- planar blocks ----
def plane_index(nr, n, stride, x, tail_full_stride=False):
    """element index [len(x)][nr] of the reals of sites x in a planar block"""
    k = np.arange(nr)[None, :]
    x = np.asarray(x)[:, None]
    full = (nr // n) * n
    tail = full * stride + x * (n if tail_full_stride else nr - full) + (k - full)
    return np.where(k < full, (k // n) * (stride * n) + x * n + k % n, tail)


def block_bytes(nr, prec, stride):
    return nr * prec * stride


def _gather(raw, byte0, nr, prec, stride, vh, **kw):
    raw = np.asarray(raw, dtype=np.uint8)
    img = raw[byte0: byte0 + (raw.size - byte0) // prec * prec].view(DTYPE[prec])      # to the end of the buffer: a wrong index reads another block, not nothing
    return np.take(img, plane_index(nr, N_OF[prec], stride, np.arange(vh), **kw), mode="clip")


def _scatter(values, prec, stride):
    """[Vh][nr] numbers of type DTYPE[prec] -> the bytes of one planar block"""
    vh, nr = values.shape
    img = np.zeros(nr * stride, dtype=DTYPE[prec])
    img[plane_index(nr, N_OF[prec], stride, np.arange(vh))] = values
    return img.view(np.uint8)


# ---- spinors ----
def decode_spinor(raw, norm_raw, info, parity=0, plant=None):
    """(values float64 [Vh][24], scales float64 [Vh] or None) of one parity; raw, norm_raw: the bytes at info["v"] and info["norm"]"""
    prec, stride, vh = info["precision"], info["stride"], info["volumeCB"]
    got = _gather(raw, parity * info["odd_offset"], 24, prec, stride, vh)
    if prec != 2:
        return got.astype(np.float64), None
    nrm = np.asarray(norm_raw, dtype=np.uint8)[parity * info["odd_norm_offset"]:].view(np.float32)[:stride].astype(np.float64)
    site = np.arange(vh)
    if plant == "spinor_scale_next_site":
        site = (site + 1) % vh
    elif plant is not None:
        raise ValueError(plant)
    return got.astype(np.float64) * nrm[site, None] / SHORT_MAX, nrm[:vh]


def spinor_info(prec, vh, full=False):
    half, half_norm = align(vh * 24 * prec), align(vh * 4) if prec == 2 else 0
    return dict(precision=prec, stride=vh, volumeCB=vh, bytes=(2 if full else 1) * half, norm_bytes=(2 if full else 1) * half_norm,
                odd_offset=half if full else 0, odd_norm_offset=half_norm if full else 0)


def encode_spinor(values, prec, full=False):
    """host values [Vh * 24] (or both parities [2 Vh * 24]) -> (raw, norm_raw, info) as Spinor.load stores them"""
    v = np.asarray(values, dtype=np.float64).reshape(2 if full else 1, -1, 24)
    vh = v.shape[1]
    info = spinor_info(prec, vh, full)
    raw, nraw = np.zeros(info["bytes"], dtype=np.uint8), np.zeros(info["norm_bytes"], dtype=np.uint8)
    for p in range(v.shape[0]):
        if prec == 2:
            m = np.max(np.abs(v[p].astype(np.float32)), axis=1)
            img = _scatter(quantise(v[p], m[:, None]), 2, vh)
            nraw[p * info["odd_norm_offset"]: p * info["odd_norm_offset"] + 4 * vh] = m.view(np.uint8)
        else:
            img = _scatter(v[p].astype(DTYPE[prec]), prec, vh)
        raw[p * info["odd_offset"]: p * info["odd_offset"] + img.size] = img
    return raw, nraw, info


# ---- links ----
def to_matrix(r18):
    r = np.asarray(r18, dtype=np.float64).reshape(r18.shape[:-1] + (3, 3, 2))
    return r[..., 0] + 1j * r[..., 1]


def to_reals(m):
    return np.stack([m.real, m.imag], axis=-1).reshape(m.shape[:-2] + (18,))


def third_row(rows, sign):
    """rows [..][2][3] complex -> [..][3][3] with row 2 = conj(row 0 x row 1) * sign"""
    a, b = rows[..., 0, :], rows[..., 1, :]
    c = np.conj(np.cross(a, b)) * np.asarray(sign)[..., None]
    return np.concatenate([rows, c[..., None, :]], axis=-2)


def reconstruct8(s, u0, unit, dtype=np.float64, ds=0.0, dc=0.0):
    """the 18 reals of M = u0 V from the 8 stored ones s [..][8] (docstring; su3_reconstruct8), evaluated in `dtype`; ds, dc: an absolute
    perturbation of every sine / cosine (the hardware's v_sin_f32 / v_cos_f32 are good to about 1e-6).  Returns (matrix complex [..][3][3], rs)"""
    t = dtype
    s = np.asarray(s).astype(t)
    u0 = np.asarray(u0).astype(t)
    one, zero = t(1), t(0)
    a2, a3, b1 = s[..., 2] + 1j * s[..., 3], s[..., 4] + 1j * s[..., 5], s[..., 6] + 1j * s[..., 7]
    ct = np.complex64 if t is np.float32 else np.complex128
    a2, a3, b1 = a2.astype(ct), a3.astype(ct), b1.astype(ct)
    rs = (s[..., 2] * s[..., 2] + s[..., 3] * s[..., 3] + s[..., 4] * s[..., 4] + s[..., 5] * s[..., 5]).astype(t)
    d0 = np.maximum(one - rs, zero)
    m0 = np.sqrt(d0).astype(t)
    ph0, ph1 = (s[..., 0] * t(unit)).astype(np.float64), (s[..., 1] * t(unit)).astype(np.float64)
    sin0, cos0, sin1, cos1 = ((f(p) + e).astype(t) for f, p, e in ((np.sin, ph0, ds), (np.cos, ph0, dc), (np.sin, ph1, ds), (np.cos, ph1, dc)))
    a1 = (m0 * cos0 + 1j * (m0 * sin0)).astype(ct)
    d1 = np.maximum(one - d0 - s[..., 6] * s[..., 6] - s[..., 7] * s[..., 7], zero).astype(t)
    m1 = np.sqrt(d1).astype(t)
    c1 = (m1 * cos1 + 1j * (m1 * sin1)).astype(ct)
    with np.errstate(divide="ignore", invalid="ignore"):
        ri = (one / rs).astype(t)
    A, B = np.conj(a1) * b1, np.conj(a1) * c1
    u11 = -(u0 * np.conj(c1 * a3) + A * a2) * ri
    u12 = (u0 * np.conj(c1 * a2) - A * a3) * ri
    u21 = (u0 * np.conj(b1 * a3) - B * a2) * ri
    u22 = -(u0 * np.conj(b1 * a2) + B * a3) * ri
    m = np.stack([np.stack([a1, a2, a3], axis=-1), np.stack([b1, u11, u12], axis=-1), np.stack([c1, u21, u22], axis=-1)], axis=-2)
    return m.astype(np.complex128), rs.astype(np.float64)


def pack8(m, unit, dtype):
    """the 8 stored reals of M [..][3][3] (su3_pack8), the phases divided by `unit`, evaluated in `dtype`"""
    r = to_reals(m).astype(dtype)
    inv = dtype(1.0 / unit)
    return np.stack([np.arctan2(r[..., 1], r[..., 0]).astype(dtype) * inv, np.arctan2(r[..., 13], r[..., 12]).astype(dtype) * inv]
                    + [r[..., i] for i in range(2, 8)], axis=-1).astype(dtype)


def time_slice(X, vh):
    """t of every checkerboard index (t is the slowest coordinate)"""
    return np.arange(vh) // (vh // int(X[3]))


def boundary_sign(X, recon, antiperiodic, plant=None):
    """sign [8][Vh] of the reconstruction per block 2 mu + backward (the same for both parities)"""
    vh = int(np.prod(X)) // 2
    sign = np.ones((8, vh))
    if recon != 18 and antiperiodic and plant != "no_boundary_sign":
        t = time_slice(X, vh)
        sign[6, t == (0 if plant == "sign_on_forward_t0" else int(X[3]) - 1)] = -1.0
        sign[7, t == 0] = -1.0
    return sign


def decode_links(raw, info, X, antiperiodic, plant=None):
    """(W complex [2][8][Vh][3][3], stored float64 [2][8][Vh][R], rs float64 [2][8][Vh] or None) from the bytes at info["data"]"""
    prec, recon, stride, vh, lb = info["precision"], info["reconstruct"], info["stride"], info["Vh"], info["link_bytes"]
    if plant not in (None, "no_boundary_sign", "sign_on_forward_t0", "tail_full_stride", "phase_in_radians"):
        raise ValueError(plant)
    stored = np.empty((2, 8, vh, recon))
    for p in range(2):
        for d in range(8):
            got = _gather(raw, (p * 8 + d) * lb, recon, prec, stride, vh, tail_full_stride=plant == "tail_full_stride").astype(np.float64)
            stored[p, d] = got / SHORT_MAX if prec == 2 else got
    sign = boundary_sign(X, recon, antiperiodic, plant)[None]
    if recon == 18:
        return to_matrix(stored), stored, None
    if recon == 12:
        rows = stored.reshape(2, 8, vh, 2, 3, 2)
        return third_row(rows[..., 0] + 1j * rows[..., 1], np.broadcast_to(sign, (2, 8, vh))), stored, None
    unit = np.pi if prec == 2 and plant != "phase_in_radians" else 1.0
    W, rs = reconstruct8(stored, np.broadcast_to(sign, (2, 8, vh)), unit)
    return W, stored, rs


def link_info(prec, recon, vh):
    lb = align(vh * recon * prec)
    return dict(precision=prec, reconstruct=recon, stride=vh, Vh=vh, link_bytes=lb, bytes=16 * lb)


def host_blocks(gauge, X, plant=None):
    """the 16 blocks of host QDP links (4, V * 18): complex [2][8][Vh][3][3], block 2 mu = U_mu(x), 2 mu + 1 = U_mu(x - mu)^dagger"""
    vh = int(np.prod(X)) // 2
    u = to_matrix(np.asarray(gauge, dtype=np.float64).reshape(4, 2, vh, 18))
    W = np.empty((2, 8, vh, 3, 3), dtype=np.complex128)
    for p in range(2):
        nb = F.neighbours(X, p)
        for mu in range(4):
            W[p, 2 * mu] = u[mu, p]
            back = u[mu, 1 - p][nb[2 * mu if plant == "backward_from_forward_neighbour" else 2 * mu + 1]]
            W[p, 2 * mu + 1] = back if plant == "backward_not_daggered" else back.conj().transpose(0, 2, 1)
    return W


def encode_links(gauge, X, prec, recon):
    """(raw, info) as gauge_load_kernel stores host QDP links (the folded antiperiodic sign is in the host field)"""
    vh = int(np.prod(X)) // 2
    info = link_info(prec, recon, vh)
    real = np.float64 if prec == 8 else np.float32
    W = host_blocks(gauge, X)
    r = to_reals(W).astype(real)
    if recon == 8:
        r = pack8(to_matrix(r.astype(np.float64)).astype(np.complex128 if prec == 8 else np.complex64), np.pi if prec == 2 else 1.0, real)
    else:
        r = r[..., :recon]
    raw = np.zeros(info["bytes"], dtype=np.uint8)
    for p in range(2):
        for d in range(8):
            v = quantise(r[p, d], np.float32(1)) if prec == 2 else r[p, d].astype(DTYPE[prec])
            img = _scatter(v, prec, vh)
            raw[(p * 8 + d) * info["link_bytes"]: (p * 8 + d) * info["link_bytes"] + img.size] = img
    return raw, info


def stored_error(prec, v):
    """bound of |stored real - v| for a link real of fp64 value v (not a phase)"""
    if prec == 8:
        return np.zeros_like(v)
    return EPS32 * np.abs(v) if prec == 4 else link_step_bound(v)


def _cabs_err(e):
    return np.sqrt(2.0) * e       # both parts of a complex entry off by e


def cond8(W):
    """(1 + 1 / |U00| + 1 / |U20|) / rs of the matrices W [..][3][3]: the amplification of the 8-real reconstruction"""
    rs = np.abs(W[..., 0, 1]) ** 2 + np.abs(W[..., 0, 2]) ** 2
    with np.errstate(divide="ignore"):
        return (1.0 + 1.0 / np.abs(W[..., 0, 0]) + 1.0 / np.abs(W[..., 2, 0])) / rs


def check_links(label, W, stored, rs, Wh, X, prec, recon, antiperiodic):
    """the decoded image (decode_links) against the blocks Wh the host field asks for (complex [2][8][Vh][3][3]).
    Stored reals: fp64 bit-identical, fp32 bit-identical to astype(float32), 16-bit within 0.5 / 32767 + 2^-23 |v| (link_step_bound); the two
    phases of the 8-real format within PHASE_ERR of numpy's atan2 (16-bit: plus pi times the step bound), compared modulo 2 pi.
    Rebuilt entries against the host matrix: the rounding e of the stored reals pushed through the decode.
      12 reals: row 2 is sign conj(a x b), every entry a difference of two products a_j b_k of stored entries, so with |da|, |db| <= sqrt(2) e
                |d(a_j b_k)| <= |da_j| |b_k| + |a_j| |db_k| + |da_j| |db_k|,        summed over the two products
      8 reals:  every entry is a smooth function of the 8 stored reals wherever rs > 0, 1 - rs > 0 and |U20| > 0, with first derivatives that
                carry the 1 / rs of the reconstruction: sum_i |dM / ds_i| e_i, the derivatives by central differences of the fp64 decode,
                doubled for the second-order terms
    plus, in both, the fp64 evaluation and what the host matrix itself is off from special-unitary at fp64: C12_FP64 for 12 reals,
    C8_FP64 2^-53 cond8 for 8 (measured on the host fields' own exact reals, tests/test_stored_ref.py), cond8 = (1 + 1 / |U00| + 1 / |U20|) / rs:
    next to rs -> 0 the two square roots make |U00| -> 0 and |U20| -> 0 singular too (d sqrt(d) = dd / (2 sqrt(d))).  Returns (label, worst ratio of the rebuilt entries to their bound, worst
    |dec - host| rs / 2^-53 for fp64 8-real links); raises blas_ref.Mismatch naming the block"""
    import blas_ref as R
    vh = int(np.prod(X)) // 2
    sign = np.broadcast_to(boundary_sign(X, recon, antiperiodic)[None], (2, 8, vh))
    hr = to_reals(Wh)
    unit = np.pi if prec == 2 else 1.0
    if recon == 8:
        want = np.concatenate([np.angle(Wh[..., 0, 0])[..., None] / unit, np.angle(Wh[..., 2, 0])[..., None] / unit, hr[..., 2:8]], axis=-1)
    else:
        want = hr[..., :recon]
    first = 2 if recon == 8 else 0

    def fail(what, bad):
        p, d = np.argwhere(np.any(bad.reshape(2, 8, -1), axis=2))[0]
        sites = np.nonzero(np.any(bad[p, d].reshape(vh, -1), axis=1))[0]
        ts = np.unique(time_slice(X, vh)[sites])
        raise R.Mismatch("%s: %s differ in block [parity %d][%d] (%s mu = %d) at %d of %d sites (first %d, time slices %s), %d blocks in all"
                         % (label, what, p, d, "backward" if d % 2 else "forward", d // 2, sites.size, vh, sites[0], ts[:6], int(np.sum(np.any(bad.reshape(16, -1), axis=1)))))

    got, ref = stored[..., first:], want[..., first:]
    if prec == 8:
        bad = got != ref
    elif prec == 4:
        bad = got != ref.astype(np.float32).astype(np.float64)
    else:
        bad = ~(np.abs(got - ref) <= link_step_bound(ref))
    if np.any(bad):
        fail("stored reals", bad)
    e = stored_error(prec, want)
    if recon == 8:
        dphi = np.angle(np.exp(1j * unit * (stored[..., :2] - want[..., :2])))
        ephi = PHASE_ERR[4 if prec == 2 else prec] + (np.pi * link_step_bound(want[..., :2]) if prec == 2 else 0.0)
        bad = ~(np.abs(dphi) <= ephi)
        if np.any(bad):
            fail("stored phases", bad)
        e[..., :2] = ephi / unit
    if recon == 18:
        bound = np.broadcast_to(_cabs_err(np.max(e, axis=-1))[..., None, None], W.shape)
        fp64_ratio = 0.0
    elif recon == 12:
        a, b = np.abs(Wh[..., 0, :]), np.abs(Wh[..., 1, :])
        ea = _cabs_err(np.max(e, axis=-1))                      # [2][8][Vh]: the largest rounding of the link's stored entries, as a modulus
        push = np.stack([(ea * b[..., k] + a[..., j] * ea + ea ** 2) + (ea * b[..., j] + a[..., k] * ea + ea ** 2) for j, k in ((1, 2), (2, 0), (0, 1))], axis=-1)
        bound = np.zeros(W.shape)
        bound[..., 2, :] = push + C12_FP64
        bound[..., :2, :] = ea[..., None, None]
        fp64_ratio = 0.0
    else:
        h = 1e-6
        push = np.zeros(W.shape)
        for i in range(8):
            sp, sm = want.copy(), want.copy()
            sp[..., i] += h
            sm[..., i] -= h
            dM = (reconstruct8(sp, sign, unit)[0] - reconstruct8(sm, sign, unit)[0]) / (2 * h)
            push += np.abs(dM) * e[..., i, None, None]
        bound = 2.0 * push + C8_FP64 * 2.0 ** -53 * cond8(Wh)[..., None, None]
        fp64_ratio = float(np.max(np.abs(W - Wh) * rs[..., None, None]) / 2.0 ** -53) if prec == 8 else 0.0
    err = np.abs(W - Wh)
    bad = ~(err <= bound)
    if np.any(bad):
        fail("rebuilt entries (worst error / bound %.3g)" % float(np.max(err / np.where(bound > 0, bound, 1e-300))), bad)
    return label, float(np.max(err / np.where(bound > 0, bound, 1.0))), fp64_ratio


def blocks_to_qdp(W):
    """the forward blocks as host QDP links (4, V * 18): what an oracle call can take (it rebuilds the backward links itself)"""
    return np.ascontiguousarray(np.stack([to_reals(np.stack([W[0, 2 * mu], W[1, 2 * mu]])).reshape(-1) for mu in range(4)]))


# ---- clover ----
def decode_clover(raw, norm_raw, info, plant=None, as_loaded=False):
    """(packed float64 [2][Vh][2][36], scales float64 [2][2][Vh] or None) of A or Ainv; raw: 2 parity_bytes from info["A"] or info["Ainv"],
    norm_raw: the scale array from info["norm"] or info["invNorm"]; as_loaded: the 16-bit values bit for bit as Planar<short>::load hands them
    to a kernel, fl(int16 * fl(scale * fl(1 / 32767))) in fp32, instead of the exact int16 * scale / 32767"""
    prec, stride, vh, pb = info["precision"], info["stride"], info["Vh"], info["parity_bytes"]
    out = np.empty((2, vh, 2, 36))
    scales = np.empty((2, 2, vh)) if prec == 2 else None
    if plant not in (None, "clover_scale_other_block"):
        raise ValueError(plant)
    for p in range(2):
        for chi in range(2):
            got = _gather(raw, p * pb + chi * 36 * prec * stride, 36, prec, stride, vh).astype(np.float64)
            if prec == 2:
                nrm = np.asarray(norm_raw, dtype=np.uint8).view(np.float32).astype(np.float64)
                scales[p, chi] = nrm[p * 2 * stride + chi * stride: p * 2 * stride + chi * stride + vh]
                src = 1 - chi if plant == "clover_scale_other_block" else chi
                sc = nrm[p * 2 * stride + src * stride: p * 2 * stride + src * stride + vh, None]
                if as_loaded:
                    got = (got.astype(np.float32) * (sc.astype(np.float32) * (np.float32(1) / np.float32(SHORT_MAX)))).astype(np.float64)
                else:
                    got = got * sc / SHORT_MAX
            out[p, :, chi] = got
    return out, scales


def clover_info(prec, vh):
    return dict(precision=prec, stride=vh, Vh=vh, parity_bytes=align(vh * 72 * prec), parity_norm_bytes=2 * vh * 4 if prec == 2 else 0)


def encode_clover(packed, prec):
    """host packed clover [2 Vh * 72] -> (raw, norm_raw, info) as clover_load_kernel stores it"""
    h = np.asarray(packed, dtype=np.float64).reshape(2, -1, 2, 36)
    vh = h.shape[1]
    info = clover_info(prec, vh)
    raw = np.zeros(2 * info["parity_bytes"], dtype=np.uint8)
    nrm = np.zeros(4 * vh, dtype=np.float32)
    for p in range(2):
        for chi in range(2):
            v = h[p, :, chi]
            if prec == 2:
                m = np.max(np.abs(v.astype(np.float32)), axis=1)
                nrm[p * 2 * vh + chi * vh: p * 2 * vh + (chi + 1) * vh] = m
                v = quantise(v, m[:, None])
            img = _scatter(v.astype(DTYPE[prec]), prec, vh)
            base = p * info["parity_bytes"] + chi * 36 * prec * vh
            raw[base: base + img.size] = img
    return raw, nrm.view(np.uint8), info


_LOWER = [(r, c) for c in range(6) for r in range(c + 1, 6)]      # strictly-lower entries column by column: k = 15 - (6 - c)(5 - c) / 2 + r - c - 1


def clover_matrices(packed):
    """packed [..][36] -> Hermitian complex [..][6][6] (clover_block_mv)"""
    packed = np.asarray(packed, dtype=np.float64)
    m = np.zeros(packed.shape[:-1] + (6, 6), dtype=np.complex128)
    for i in range(6):
        m[..., i, i] = packed[..., i]
    for k, (r, c) in enumerate(_LOWER):
        m[..., r, c] = packed[..., 6 + 2 * k] + 1j * packed[..., 7 + 2 * k]
        m[..., c, r] = packed[..., 6 + 2 * k] - 1j * packed[..., 7 + 2 * k]
    return m


def pack_clover(m):
    """the inverse of clover_matrices, symmetrised as clover_invert_kernel does"""
    out = np.empty(m.shape[:-2] + (36,))
    for i in range(6):
        out[..., i] = m[..., i, i].real
    for k, (r, c) in enumerate(_LOWER):
        out[..., 6 + 2 * k] = 0.5 * (m[..., r, c].real + m[..., c, r].real)
        out[..., 7 + 2 * k] = 0.5 * (m[..., r, c].imag - m[..., c, r].imag)
    return out


def pack_bound(b):
    """bounds b [..][6][6] of the entries of a matrix -> bounds of its 36 packed reals (pack_clover averages the two triangles)"""
    out = np.empty(b.shape[:-2] + (36,))
    for i in range(6):
        out[..., i] = b[..., i, i]
    for k, (r, c) in enumerate(_LOWER):
        out[..., 6 + 2 * k] = out[..., 7 + 2 * k] = 0.5 * (b[..., r, c] + b[..., c, r])
    return out


def inverted_matrix(A, mu2, twisted):
    """the matrix clover_invert_kernel inverts: A^2 + mu2 where `twisted`, else A; A complex [..][6][6]"""
    if not twisted:
        return A
    return A @ A + mu2 * np.eye(6)


def gauss_jordan(m, dtype=np.complex128):
    """(inverse, sum of log |pivot|) of the matrices m [n][6][6] by the elimination of clover_invert_kernel (partial pivoting by rows), evaluated
    in `dtype`"""
    n = m.shape[0]
    s = np.concatenate([m.astype(dtype), np.broadcast_to(np.eye(6, dtype=dtype), (n, 6, 6))], axis=2).copy()
    tl = np.zeros(n)
    rows = np.arange(n)
    for p in range(6):
        best = p + np.argmax(np.abs(s[:, p:, p]), axis=1)
        tmp = s[rows, p].copy()
        s[rows, p] = s[rows, best]
        s[rows, best] = tmp
        piv = s[:, p, p].copy()
        tl += np.log(np.abs(piv.astype(np.complex128)))
        s[:, p] = (s[:, p] / piv[:, None]).astype(dtype)
        for r in range(6):
            if r != p:
                s[:, r] = (s[:, r] - s[:, r, p, None] * s[:, p]).astype(dtype)
    return s[:, :, 6:], tl


def inverse_bound(A, inv, mu2, twisted):
    """n eps (|inv| |M| |inv|) of an elimination in fp64 (n = 6, eps = 2^-53), per entry [..][6][6]; where `twisted`, |M| is taken as
    |A| |A| + mu2, which also covers the rounding of the product A A the kernel forms first"""
    a = np.abs(A)
    m = a @ a + mu2 * np.eye(6) if twisted else a
    return 6 * 2.0 ** -53 * (np.abs(inv) @ m @ np.abs(inv))


C_INV = 2.1                         # four times the worst ratio of a numpy fp64 elimination to inverse_bound (0.515, tests/test_stored_ref.py)


# ---- one launch ----
MODES = ("plain", "twist_inv", "twist_inv_dslash", "twist_xpay", "clover_twist_inv", "clover_twist_xpay")


def launch(W, X, parity, inp, mode, a=0.0, b=1.0, k=0.0, x=None, dagger=False, A=None, Ainv=None, delta=None, ghost=None):
    """(want, T, extra) float64 [Vh][24] of one launch onto `parity`: W decoded blocks [2][8][Vh][3][3]; inp [Vh][24] the decoded input (other
    parity); x the decoded xpay operand or None; a, b, k as the launcher hands them to the kernel (a with the dagger's flip applied); A, Ainv
    complex [Vh][2][6][6] of `parity`; delta [8][Vh]: an absolute deviation of every real of the site's eight matrices (8-real links), whose
    worst effect on the output is returned as `extra` (zeros without it); ghost [8][Vh]: an absolute error of every real that hop d adds to the
    site (the second quantisation of a ghost half spinor), pushed through the epilogue into `extra` as well"""
    vh = int(np.prod(X)) // 2
    psi = F.to_complex(np.asarray(inp).reshape(1, -1), vh)
    psi_t = F._abs(psi)
    if mode == "twist_inv_dslash":
        psi, psi_t = F._twist(psi, a, False), F._twist(psi_t, a, True)
    hop = F.hop_terms(None, X, parity, psi, blocks=W, dagger=dagger)
    parts = [F.hop_terms(None, X, parity, psi_t, absolute=True, blocks=W, dagger=dagger)]
    if delta is not None:
        D = np.zeros((2, 8, vh, 3, 3), dtype=np.complex128)
        D[parity] = (np.asarray(delta)[:, :, None, None] * (1.0 + 1.0j))
        parts.append(F.hop_terms(None, X, parity, psi_t, absolute=True, blocks=D, dagger=dagger))
    if ghost is not None:
        parts.append(np.broadcast_to((np.sum(np.asarray(ghost), axis=0) * (1.0 + 1.0j))[None, :, None, None], hop.shape))
    xc = None if x is None else F.to_complex(np.asarray(x).reshape(1, -1), vh)

    def site(m, v, absolute):
        return F._site(m, v, absolute)

    def epilogue(h, absolute, with_x):
        f = abs if absolute else (lambda v: v)
        xs = None if xc is None else (F._abs(xc) if absolute else xc)
        if mode == "plain":
            out = h if x is None else f(k) * h
        elif mode in ("twist_inv", "twist_inv_dslash"):
            out = f(b) * (F._twist(h, a, absolute) if mode == "twist_inv" else h)
        elif mode == "twist_xpay":
            out = f(k) * h
            return out + F._twist(xs, a, absolute) if with_x else out
        elif mode == "clover_twist_inv":
            out = site(Ainv, site(A, h, absolute) + (F._twist(h, a, absolute) - h), absolute)
            if x is not None:
                out = f(k) * out
        elif mode == "clover_twist_xpay":
            out = f(k) * h
            return out + site(A, xs, absolute) + (F._twist(xs, a, absolute) - xs) if with_x else out
        else:
            raise ValueError(mode)
        return out + xs if (with_x and xs is not None) else out

    want, T = epilogue(hop, False, True), epilogue(parts[0], True, True)
    extra = sum((epilogue(q, True, False) for q in parts[1:]), np.zeros_like(T))
    return tuple(F.to_real(v).reshape(vh, 24) for v in (want, T, extra))


def ghost_error(X, parity, inp, mask, mode="plain", a=0.0, dagger=False):
    """[8][Vh]: 2.5 * 0.5 g / 32767 for every hop that crosses a partitioned face (bit mu of mask), 0 elsewhere; g the largest |real| of the
    projected neighbour half spinor (the two independent spin rows of (1 -+ gamma_mu) psi), which travels as 16-bit with a scale of its own.
    The three link entries of a row have 1-norm at most sqrt(3) and multiply complex errors of modulus at most sqrt(2) half steps: 2.45 < 2.5"""
    vh = int(np.prod(X)) // 2
    psi = F.to_complex(np.asarray(inp).reshape(1, -1), vh)
    if mode == "twist_inv_dslash":
        psi = F._twist(psi, a, False)
    nb = F.neighbours(X, parity)
    c = F.coordinates(X, parity)
    out = np.zeros((8, vh))
    for d in range(8):
        mu = d // 2
        if not (mask >> mu) & 1:
            continue
        crossing = c[mu] == (int(X[mu]) - 1 if d % 2 == 0 else 0)
        h = np.einsum("st,xtb->xsb", F.PROJECTORS[d ^ 1] if dagger else F.PROJECTORS[d], psi[0][nb[d]])[:, :2]
        g = np.max(np.maximum(np.abs(h.real), np.abs(h.imag)), axis=(1, 2))
        out[d] = np.where(crossing, 2.5 * 0.5 * g / SHORT_MAX, 0.0)
    return out


def check_stored16(label, dec, scale, want, T, extra, k):
    """the two bounds of a 16-bit output (docstring); returns (label, worst value ratio, worst scale ratio), both against their bounds; raises
    blas_ref.Mismatch"""
    import blas_ref as R
    dec, want, T, extra = (np.asarray(v, dtype=np.float64).reshape(-1, 24) for v in (dec, want, T, extra))
    scale = np.asarray(scale, dtype=np.float64)
    if not (np.all(np.isfinite(dec)) and np.all(np.isfinite(scale))):
        raise R.Mismatch("%s: non-finite elements" % label)
    bound = 0.5 * scale[:, None] / SHORT_MAX * (1.0 + 2.0 ** -10) + k * EPS32 * T + extra
    err = np.abs(dec - want)
    ratio = np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err > 0, np.inf, 0.0))
    nb = k * EPS32 * np.max(T, axis=1) + np.max(extra, axis=1)
    ne = np.abs(scale - np.max(np.abs(want), axis=1))
    nratio = np.where(nb > 0, ne / np.where(nb > 0, nb, 1.0), np.where(ne > 0, np.inf, 0.0))
    i = int(np.argmax(ratio))
    if ratio.reshape(-1)[i] > 1.0:
        raise R.Mismatch("%s: %d reals out of bound, worst at site %d, real %d: got %.9g, expected %.9g, error %.3e, allowed %.3e (scale %.6g, T %.6g)"
                         % (label, int(np.sum(ratio > 1.0)), i // 24, i % 24, dec.reshape(-1)[i], want.reshape(-1)[i], err.reshape(-1)[i],
                            bound.reshape(-1)[i], scale[i // 24], T.reshape(-1)[i]))
    j = int(np.argmax(nratio))
    if nratio[j] > 1.0:
        raise R.Mismatch("%s: %d scales out of bound, worst at site %d: scale %.9g, max |ref| %.9g, allowed %.3e"
                         % (label, int(np.sum(nratio > 1.0)), j, scale[j], np.max(np.abs(want[j])), nb[j]))
    return label, float(ratio.reshape(-1)[i]), float(nratio[j])


def check_stored32(label, got, want, T, extra, k):
    """an fp32 (or fp64) output: |got - want| <= k 2^-24 T + extra; returns (label, worst ratio)"""
    import blas_ref as R
    got, want, T, extra = (np.asarray(v, dtype=np.float64).reshape(-1) for v in (got, want, T, extra))
    if not np.all(np.isfinite(got)):
        raise R.Mismatch("%s: non-finite elements" % label)
    bound = k * EPS32 * T + extra
    err = np.abs(got - want)
    ratio = np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err > 0, np.inf, 0.0))
    i = int(np.argmax(ratio))
    if ratio[i] > 1.0:
        raise R.Mismatch("%s: %d reals out of bound, worst at site %d, real %d: got %.9g, expected %.9g, error %.3e, allowed %.3e"
                         % (label, int(np.sum(ratio > 1.0)), i // 24, i % 24, got[i], want[i], err[i], bound[i]))
    return label, float(ratio[i])


# ---- the lattices, fields and launches of tests/test_stored_gpu.py; the self-test measures K on the same ones ----
LATTICES = {"2^4": (2, 2, 2, 2), "12x6x10x4": (12, 6, 10, 4)}
SEEDS = {"2^4": 8, "12x6x10x4": 37}          # oracle.make_fields seeds whose links have rs >= RS_MIN on all 16 blocks (asserted on the CPU)
KAPPA, MU, KX = 0.124, 0.3, -0.37             # a = 2 kappa mu = 0.0744: a dropped or mis-signed twist is 7 % of an element


def operands(X, which):
    """host spinor of both parities [2][Vh][24]: uniform (-0.5, 0.5) times 10^u per site, u uniform in [-2, 2]; one site of each parity
    identically zero.  which: 0 the input, 1 the xpay operand (its own draws, so another scale profile)"""
    vh = int(np.prod(X)) // 2
    rng = np.random.default_rng(9100 + 10 * vh + which)
    v = (rng.random((2, vh, 24)) - 0.5) * 10.0 ** rng.uniform(-2.0, 2.0, (2, vh, 1))
    v[0, (3 + which) % vh] = 0.0
    v[1, (vh - 2 - which) % vh] = 0.0
    return v


def launches():
    """every single launch the resident API reaches: dicts(op, flavor, dagger, matpc, pc, call) with call = dslash / xpay (Dirac.dslash /
    Dirac.dslash_xpay of the preconditioned operator on parity fields) or M (Dirac.M of the full operator: one xpay launch per parity)"""
    out = []
    for dagger in (0, 1):
        for call in ("dslash", "xpay"):
            out.append(dict(op="wilson", flavor=0, dagger=dagger, matpc="ee", pc=True, call=call))
    for op in ("tm", "tmc"):
        for flavor in (+1, -1):
            for dagger in (0, 1):
                for matpc in ("ee", "eeasym"):
                    for call in ("dslash", "xpay"):
                        if op == "tmc" and flavor == -1 and matpc == "eeasym":
                            continue          # twisted clover: one flavour through the asymmetric form (the launch differs in the sign of a only)
                        out.append(dict(op=op, flavor=flavor, dagger=dagger, matpc=matpc, pc=True, call=call))
                out.append(dict(op=op, flavor=flavor, dagger=dagger, matpc="ee", pc=False, call="M"))
    return out


def launch_name(c):
    return "%s f%+d dag%d %s %s" % (c["op"], c["flavor"], c["dagger"], c["matpc"], c["call"])


def kernel_args(c, kappa=KAPPA, mu=MU, kx=KX):
    """dict(mode, a, b, k, dagger, xpay) of the launch the library makes for case c (csrc/dirac.cpp), kx the k of dslash_xpay"""
    dag, asym, xpay = bool(c["dagger"]), c["matpc"].endswith("asym"), c["call"] != "dslash"
    flip = -1.0 if dag else 1.0
    if c["op"] == "wilson":
        return dict(mode="plain", a=0.0, b=1.0, k=kx, dagger=dag, xpay=xpay)
    if c["call"] == "M":
        return dict(mode="twist_xpay" if c["op"] == "tm" else "clover_twist_xpay", a=flip * 2.0 * kappa * c["flavor"] * mu, b=-kappa, k=-kappa, dagger=dag, xpay=True)
    a = -2.0 * kappa * c["flavor"] * mu
    if c["op"] == "tm":
        b = (kx if xpay else 1.0) / (1.0 + a * a)
        after = (not dag) if xpay else (not dag or asym)        # DiracTwistedMassPC::DslashXpay looks at dagger alone
        return dict(mode="twist_inv" if after else "twist_inv_dslash", a=flip * a, b=b, k=b, dagger=dag, xpay=xpay)
    after = (not dag) if xpay else (not dag or asym)
    return dict(mode="clover_twist_inv" if after else "plain", a=flip * a, b=kx if xpay else 1.0, k=kx, dagger=dag, xpay=xpay)


def uses_site_matrices(mode):
    return mode.startswith("clover")
