"""fp64 reference of ONE parity launch of the multi-right-hand-side fine stencil (csrc/fine_block.hip fine_block_kernel through
applyFineBlockParity) and of the dense clover-twist site matrices it applies (clover_twist_dense_kernel).  A plain module: no GPU, no
library of the project; the pieces come from the oracle (tests/oracle_api.py): wil_dslash for the bare hop sum of one parity, apply_clover for
A, gamma5 = diag(+, +, -, -) of the host DeGrand-Rossi basis (qo_twist_gamma5).

    out = s0 (1 + i a0 g5) same + k1 (1 + i a1 g5) H other            H other = sum of the 8 hops U P other(x + mu) onto one parity
    tmode 1:  a dense site matrix M of the OUTPUT parity replaces (1 + i a1 g5) on the hop sum      (M = (A + i a g5)^-1: the Schur form)
    tmode 2:  it replaces (1 + i a0 g5) on `same`                                                  (M = A + i a g5: the full operator)

A field is a float64 array [rhs][Vh * 24]: the host order of a single-parity spinor (site, spin, colour, re / im), the values the device
holds read back, so the rounding of the load cancels.  Links are the (4, V * 18) host QDP arrays AS THE DEVICE HOLDS THEM (device_links):
rounded to fp32, for 12-real storage the third row rebuilt from the two stored ones in fp32, the antiperiodic sign folded into the forward t
links of the last time slice.  Dense matrices: apply_clover on the 12 unit vectors (nothing assumed about the packing), + i a on the upper,
- i a on the lower chirality, numpy.linalg.inv in fp64.

Besides the value every function returns the TERM SUM T of each element: the same expression on absolute values — |Re|, |Im| of every link,
spinor component, projector and matrix entry and |coefficient|, a complex product (a b)_re counted as |a_re||b_re| + |a_im||b_im|.  It needs
the hop sum term by term, so the module carries its own numpy hop sum (hop_terms; projectors restated from the reference's table); signed,
it must reproduce oracle.wil_dslash (tests/test_fine_stencil_ref.py), which pins the neighbour tables, the daggers and the projectors T uses.

Bound: |got - want| <= K 2^-24 T per element, K_PLAIN without site matrices, K_SITE with them.  The longest rounding chain of an element
counts about 22 fp32 operations — 8 hops accumulated, each behind a projection (1), an SU(3) row of three complex products (5) and the
reconstruction, then the twist (2), the two scales (2), the final sum (1) and the casts of the coefficients — and the dense 6 x 6 complex row
adds about 12 (11 additions and the rounding of the matrix entry to fp32).  Roundings do not all push one way, so the constants are not the
counts but MEASURED: tests/test_fine_stencil_ref.py evaluates every coefficient case of the GPU test with the oracle's fp32 variants
(qo_*_f) standing in for the device, on the 8 x 4 x 6 x 10 lattice with fp32 18-real periodic, 18-real antiperiodic and 12-real antiperiodic
links, and asserts twice its worst |err| / (2^-24 T), rounded up, <= K <= the caps 24 (plain) and 40 (site matrices):
    worst measured ratio   without site matrices 4.43 (hop only)   with site matrices 4.31 (site matrix on same)   ->   K_PLAIN = K_SITE = 9
(per case 3.5 to 4.4 whatever the links: the hop sum dominates, the dense row shows in no worst element.  The stand-in rounds as a sequential C
loop does; the kernel contracts to fused multiply-adds, which only removes roundings).
Dense matrices: direct ones bit-identical to the fp32 entries; inverses within 2^-24 |want| + 1e-12 max|want| per site matrix — an fp64
elimination, then one rounding to fp32."""
import numpy as np

import blas_ref as R
from gauge_obs_ref import fp32_recon12

EPS32 = 2.0 ** -24
K_PLAIN, K_SITE = 9, 9
K_CAP_PLAIN, K_CAP_SITE = 24, 40
G5 = np.array([1.0, 1.0, -1.0, -1.0])

# 1 -+ gamma_mu of the host basis, index 2 mu + (0: forward hop, 1: backward hop) without dagger (tests/wilson_dslash_reference.cpp:28-69)
_P = [[[1, 0, 0, -1j], [0, 1, -1j, 0], [0, 1j, 1, 0], [1j, 0, 0, 1]],
      [[1, 0, 0, 1j], [0, 1, 1j, 0], [0, -1j, 1, 0], [-1j, 0, 0, 1]],
      [[1, 0, 0, 1], [0, 1, -1, 0], [0, -1, 1, 0], [1, 0, 0, 1]],
      [[1, 0, 0, -1], [0, 1, 1, 0], [0, 1, 1, 0], [-1, 0, 0, 1]],
      [[1, 0, -1j, 0], [0, 1, 0, 1j], [1j, 0, 1, 0], [0, -1j, 0, 1]],
      [[1, 0, 1j, 0], [0, 1, 0, -1j], [-1j, 0, 1, 0], [0, 1j, 0, 1]],
      [[1, 0, -1, 0], [0, 1, 0, -1], [-1, 0, 1, 0], [0, -1, 0, 1]],
      [[1, 0, 1, 0], [0, 1, 0, 1], [1, 0, 1, 0], [0, 1, 0, 1]]]
PROJECTORS = np.array(_P, dtype=np.complex128)


# ---- layouts ----
def to_complex(v, vh):
    """[rhs][Vh * 24] reals -> complex [rhs][Vh][4][3]"""
    v = np.asarray(v, dtype=np.float64).reshape(-1, vh, 4, 3, 2)
    return v[..., 0] + 1j * v[..., 1]


def to_real(c):
    """complex [rhs][Vh][4][3] -> [rhs][Vh * 24] reals"""
    return np.stack([c.real, c.imag], axis=-1).reshape(c.shape[0], -1)


def _abs(c):
    """|Re| + i |Im|: the container of a term sum"""
    return np.abs(c.real) + 1j * np.abs(c.imag)


def _mul(spec, a, b, absolute):
    """einsum of two complex operands; absolute: on containers of term sums, (a b)_re = a_re b_re + a_im b_im, (a b)_im = a_re b_im + a_im b_re"""
    if not absolute:
        return np.einsum(spec, a, b)
    return np.einsum(spec, a.real, b.real) + np.einsum(spec, a.imag, b.imag) + 1j * (np.einsum(spec, a.real, b.imag) + np.einsum(spec, a.imag, b.real))


# ---- geometry: checkerboard index ((t Z + z) Y + y) Xh + xh, x = 2 xh + ((y + z + t + parity) & 1) ----
def coordinates(X, parity):
    X = [int(v) for v in X]
    xh_n = X[0] // 2
    idx = np.arange(xh_n * X[1] * X[2] * X[3])
    xh, y, z, t = idx % xh_n, (idx // xh_n) % X[1], (idx // (xh_n * X[1])) % X[2], idx // (xh_n * X[1] * X[2])
    return 2 * xh + ((y + z + t + parity) & 1), y, z, t


def cb_index(X, x, y, z, t):
    return (((t * X[2] + z) * X[1] + y) * X[0] + x) // 2


def neighbours(X, parity):
    """nb[dir][x]: checkerboard index (on the other parity) of the site that hop dir = 2 mu + (0 forward, 1 backward) reads"""
    c = coordinates(X, parity)
    nb = np.empty((8, c[0].size), dtype=np.int64)
    for d in range(8):
        s = [np.array(v) for v in c]
        s[d // 2] = (s[d // 2] + (1 if d % 2 == 0 else -1)) % int(X[d // 2])
        nb[d] = cb_index(X, *s)
    return nb


# ---- links as the device holds them ----
def device_links(gauge, X, recon, antiperiodic):
    """host QDP links (4, V * 18), the antiperiodic sign already folded into the t links of the last time slice if `antiperiodic`, as an fp32
    device field of 18 or 12 reals holds them; same shape, float64"""
    X = [int(v) for v in X]
    g = np.asarray(gauge, dtype=np.float64).astype(np.float32).astype(np.float64)
    if recon == 18:
        return g
    if recon != 12:
        raise ValueError("fp32 links of 18 or 12 reals")
    vh = int(np.prod(X)) // 2
    u = g.reshape(4, 2, X[3], vh // X[3], 3, 3, 2)         # t is the slowest coordinate of the checkerboard index
    u = (u[..., 0] + 1j * u[..., 1]).transpose(0, 2, 1, 3, 4, 5)
    u = fp32_recon12(u, antiperiodic).transpose(0, 2, 1, 3, 4, 5)
    return np.ascontiguousarray(np.stack([u.real, u.imag], axis=-1).reshape(4, -1))


def fold_antiperiodic(gauge, X):
    """the links with the t links of the last time slice negated (both parities)"""
    X = [int(v) for v in X]
    out = np.array(gauge, dtype=np.float64)
    vh = int(np.prod(X)) // 2
    out[3].reshape(2, vh, 18)[:, vh - vh // X[3]:, :] *= -1.0
    return out


# ---- the hop sum ----
def hop_terms(links, X, parity, psi, absolute=False, blocks=None, dagger=False):
    """sum of the 8 hops onto `parity` of psi[rhs][Vh][4][3] (complex, other parity) in numpy; absolute: its term sum (container |Re| + i |Im|).
    blocks: complex [2][8][Vh][3][3], the eight matrices of every site as the device stores them (block 2 mu + 1 already the daggered link of
    x - mu, tests/stored_ref.py) instead of `links`; dagger: the hops of D^dagger = g5 D g5 (the projectors 1 -+ gamma_mu exchanged)"""
    vh = int(np.prod(X)) // 2
    if blocks is None:
        u = np.asarray(links, dtype=np.float64).reshape(4, 2, vh, 3, 3, 2)
        u = u[..., 0] + 1j * u[..., 1]
    nb = neighbours(X, parity)
    if absolute:
        psi = _abs(psi)
    out = np.zeros(psi.shape, dtype=np.complex128)
    for d in range(8):
        if blocks is not None:
            m = blocks[parity][d]
        else:
            m = u[d // 2, parity] if d % 2 == 0 else u[d // 2, 1 - parity][nb[d]].conj().transpose(0, 2, 1)
        p = PROJECTORS[d ^ 1] if dagger else PROJECTORS[d]
        if absolute:
            m, p = _abs(m), _abs(p)
        out += _mul("xab,nxsb->nxsa", m, _mul("st,nxtb->nxsb", p, psi[:, nb[d]], absolute), absolute)
    return out


def hop_sum(oracle, links, X, parity, other):
    """(H other, its term sum) on `parity`: the value from oracle.wil_dslash column by column, the term sum from hop_terms; complex [rhs][Vh][4][3]"""
    vh = int(np.prod(X)) // 2
    links = np.ascontiguousarray(links, dtype=np.float64)
    other = np.asarray(other, dtype=np.float64)
    val = np.stack([oracle.wil_dslash(links, np.ascontiguousarray(col), [int(v) for v in X], parity, 0) for col in other])
    return to_complex(val, vh), hop_terms(links, X, parity, to_complex(other, vh), absolute=True)


# ---- site terms ----
def dense_matrices(oracle, clover, X, parity, a, inverse):
    """A + i a s per site of `parity` and chirality (s = +1 upper, -1 lower), or its inverse: complex [Vh][2][6][6]; clover: the packed host
    field of both parities.  A from apply_clover on the 12 unit vectors"""
    X = [int(v) for v in X]
    vh = int(np.prod(X)) // 2
    clover = np.ascontiguousarray(clover, dtype=np.float64)
    full = np.empty((vh, 12, 12), dtype=np.complex128)
    for j in range(12):
        e = np.zeros((vh, 12, 2))
        e[:, j, 0] = 1.0
        col = oracle.apply_clover(clover, e.reshape(-1), X, parity).reshape(vh, 12, 2)
        full[:, :, j] = col[..., 0] + 1j * col[..., 1]
    if np.any(full[:, :6, 6:]) or np.any(full[:, 6:, :6]):
        raise ValueError("the clover term mixes the chiralities")
    m = np.stack([full[:, :6, :6], full[:, 6:, 6:]], axis=1)
    m[:, 0] += 1j * a * np.eye(6)
    m[:, 1] -= 1j * a * np.eye(6)
    return np.linalg.inv(m) if inverse else m


def _twist(v, a, absolute):
    """(1 + i a g5) v on [rhs][Vh][4][3]"""
    if absolute:
        return v + abs(a) * (v.imag + 1j * v.real)
    return v * (1.0 + 1j * a * G5)[None, None, :, None]


def _site(m, v, absolute):
    n, vh = v.shape[:2]
    if absolute:
        m = _abs(m)
    return _mul("xcij,nxcj->nxci", m, v.reshape(n, vh, 2, 6), absolute).reshape(v.shape)


def combine(same, hop, hop_t, s0, a0, k1, a1, tmode=0, mats=None):
    """(want, T) of out = s0 (1 + i a0 g5) same + k1 (1 + i a1 g5) hop with the site matrices of tmode; same: complex [rhs][Vh][4][3] or None
    with s0 = 0; hop, hop_t from hop_sum; returns reals [rhs][Vh * 24]"""
    if tmode not in (0, 1, 2) or (tmode != 0) != (mats is not None):
        raise ValueError("site-matrix mode %r with%s matrices" % (tmode, "" if mats is not None else "out"))
    if tmode == 1:
        want, t = k1 * _site(mats, hop, False), abs(k1) * _site(mats, hop_t, True)
    else:
        want, t = k1 * _twist(hop, a1, False), abs(k1) * _twist(hop_t, a1, True)
    if s0 != 0.0:
        if tmode == 2:
            want, t = want + s0 * _site(mats, same, False), t + abs(s0) * _site(mats, _abs(same), True)
        else:
            want, t = want + s0 * _twist(same, a0, False), t + abs(s0) * _twist(_abs(same), a0, True)
    elif tmode == 2:
        raise ValueError("site matrix on the same-parity input, but that input is switched off")
    return to_real(want), to_real(t)


def parity_launch(oracle, links, X, parity, same, other, s0, a0, k1, a1, tmode=0, mats=None):
    """(want, T) of one launch on `parity`; same (None with s0 = 0), other: [rhs][Vh * 24] reals; mats: dense_matrices of `parity`"""
    vh = int(np.prod(X)) // 2
    hop, hop_t = hop_sum(oracle, links, X, parity, other)
    return combine(None if same is None else to_complex(same, vh), hop, hop_t, s0, a0, k1, a1, tmode, mats)


# ---- the checks ----
def check_launch(label, got, want, T, k):
    """every element of got within k 2^-24 T of want (an element whose T is 0 must be exactly 0); returns (label, error, bound, ratio) of the
    worst element, the ratio taken against 2^-24 T (so it compares with k directly); raises blas_ref.Mismatch"""
    got, want, T = (np.asarray(v, dtype=np.float64).reshape(-1) for v in (got, want, T))
    if not (got.shape == want.shape == T.shape):
        raise R.Mismatch("%s: shapes %s, %s, %s" % (label, got.shape, want.shape, T.shape))
    if not np.all(np.isfinite(got)):
        raise R.Mismatch("%s: non-finite elements" % label)
    err, unit = np.abs(got - want), EPS32 * T
    ratio = np.where(unit > 0, err / np.where(unit > 0, unit, 1.0), np.where(err > 0, np.inf, 0.0))
    i = int(np.argmax(ratio))
    if ratio[i] > k:
        raise R.Mismatch("%s: %d elements out of bound, worst at %d (site %d, component %d): got %.9g, expected %.9g, error %.3e = %.2f x 2^-24 T, allowed %g"
                         % (label, int(np.sum(ratio > k)), i, (i // 24), i % 24, got[i], want[i], err[i], ratio[i], k))
    return label, float(err[i]), float(k * unit[i]), float(ratio[i])


def check_dense(label, got, want, inverse):
    """dense site matrices complex64 [Vh][2][6][6] against dense_matrices: direct bit-identical to the fp32 entries, inverse within
    2^-24 |want| + 1e-12 max|want| of its site matrix, per real part"""
    got = np.asarray(got)
    if got.shape != want.shape or got.dtype != np.complex64:
        raise R.Mismatch("%s: %s %s, expected complex64 %s" % (label, got.dtype, got.shape, want.shape))
    if not inverse:
        bad = got.view(np.float32) != want.astype(np.complex64).view(np.float32)     # by value: -0 and +0 are the same entry, a NaN never passes
        if np.any(bad):
            raise R.Mismatch("%s: %d reals differ from the fp32 entries" % (label, int(np.sum(bad))))
        return label, 0.0, 0.0, 0.0
    worst = 0.0
    top = np.max(np.abs(want), axis=(2, 3), keepdims=True)
    for part in ("real", "imag"):
        g, w = getattr(got, part).astype(np.float64), getattr(want, part)
        err, bound = np.abs(g - w), EPS32 * np.abs(w) + 1e-12 * top
        if not np.all(np.isfinite(g)) or np.any(err > bound):
            raise R.Mismatch("%s: %d %s parts out of bound, worst error / bound %.3f" % (label, int(np.sum(~(err <= bound))), part, float(np.max(err / bound))))
        worst = max(worst, float(np.max(err / bound)))
    return label, worst, 1.0, worst


# ---- the coefficient cases of tests/test_fine_stencil_gpu.py; the self-test measures K on the same ones ----
KAPPA, CSW_COEFF, A_SITE = 0.124, 0.124 * 1.57551, 0.23
# (name, s0, a0, k1, a1, tmode, inverse): in_same is not handed over when s0 = 0; the site matrices are those of a = A_SITE
CASES = [("hop only", 0.0, 0.0, 1.0, 0.0, 0, False),
         ("general", 0.9, 0.3, -0.021, -0.17, 0, False),
         ("plain same, twisted hops", 1.0, 0.0, -KAPPA, 0.41, 0, False),
         ("inverse site matrix on the hops", 0.0, 0.0, 1.0, 0.0, 1, True),
         ("inverse site matrix on the hops, twisted same", 1.0, 0.3, -KAPPA * KAPPA, 0.0, 1, True),
         ("site matrix on same, twisted hops", 1.0, 0.0, -KAPPA, -0.17, 2, False)]
