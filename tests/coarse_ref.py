"""Plain numpy (complex128) reference of the coarse operator and of its even-odd preconditioned form, working from the nine matrices every
coarse site multiplies with (include/coarse.h: m = 2 mu forward hop, 2 mu + 1 backward hop, 8 local; qudaAmdMultigridGetCoarseSiteLinks):

    out(A) = sum_m  L[A][m] in(neighbour_m(A))

Fields are (sites, n) or (sites, spin 2, colour) complex arrays over the full coarse lattice, site A = parity * Vh + x_cb with coordinates
c = (2 xh + ((y + z + t + parity) & 1), y, z, t), x_cb = ((t X2 + z) X1 + y) Xh + xh.  A parity field is the half [parity * Vh, (parity + 1) * Vh);
embed() / half() move between the two.  The Schur pieces follow the formulas of the reference's DiracCoarsePC (lib/dirac_coarse.cpp:296-372:
M = 1 - A^-1 D_pq A^-1 D_qp, prepare src_p = A_pp^-1 (b_p - D_pq A_qq^-1 b_q), reconstruct x_q = A_qq^-1 (b_q - D_qp x_p)), A = the local
matrices, D = the eight hops.  tests/test_coarse_ref.py ties this file to the oracle and to a dense solve."""
import numpy as np

HOPS, LOCAL, ALL = 0xff, 1 << 8, 0x1ff
EPS32 = 2.0 ** -24
# Worst |error| / (n 2^-24 |Xinv| |X| |Xinv|) that gauss_jordan_c64 (below) shows against the complex128 inverse on the matrices of
# tests/test_coarse_pc_gpu.py.  MEASURED: synthetic row-swap batches n = 4 / 16 / 48 / 64: 0.63 / 1.49 / 0.12 / 0.03 (test_coarse_ref.py
# re-measures these); the X of its three hierarchies (n = 16 / 48 / 64): 0.39 / 0.21 / 0.14 (test_hat_links there re-measures those).  The
# device's elimination has the same arithmetic in another order: it is allowed C_HAT = 4 times the worst of them.
GJ_C64_WORST = 1.49
C_HAT = 4 * GJ_C64_WORST


def volume(Xc):
    return int(np.prod(Xc))


def coords(Xc):
    """(sites, 4) coordinates of every site in the order parity * Vh + x_cb"""
    Vh = volume(Xc) // 2
    Xh = Xc[0] // 2
    out = np.zeros((2 * Vh, 4), dtype=np.int64)
    for par in (0, 1):
        l = np.arange(Vh)
        xh = l % Xh
        l = l // Xh
        y = l % Xc[1]
        l = l // Xc[1]
        z, t = l % Xc[2], l // Xc[2]
        out[par * Vh:(par + 1) * Vh] = np.stack([2 * xh + ((y + z + t + par) & 1), y, z, t], axis=1)
    return out


def site_index(c, Xc):
    c = np.asarray(c)
    par = c.sum(axis=-1) & 1
    lex = ((c[..., 3] * Xc[2] + c[..., 2]) * Xc[1] + c[..., 1]) * Xc[0] + c[..., 0]
    return par * (volume(Xc) // 2) + lex // 2


def neighbour(Xc, m, _swap_dirs=False):
    """index of the site matrix m of every site multiplies: its forward (m = 2 mu) or backward (2 mu + 1) periodic neighbour, itself for m = 8.
    _swap_dirs plants the error of a forward / backward mix-up (tests/test_coarse_ref.py)."""
    c = coords(Xc)
    if m == 8:
        return site_index(c, Xc)
    mu, back = m >> 1, bool(m & 1) != bool(_swap_dirs)
    c[:, mu] = (c[:, mu] + (-1 if back else 1)) % Xc[mu]
    return site_index(c, Xc)


def parity_of_sites(Xc):
    Vh = volume(Xc) // 2
    return np.repeat([0, 1], Vh)


def embed(half_field, parity, Xc):
    h = np.asarray(half_field)
    out = np.zeros((2 * h.shape[0],) + h.shape[1:], dtype=h.dtype)
    out[parity * h.shape[0]:(parity + 1) * h.shape[0]] = h
    return out


def half(field, parity):
    Vh = field.shape[0] // 2
    return field[parity * Vh:(parity + 1) * Vh]


def apply(links, vec, Xc, mmask=ALL, out_parity=-1, _swap_dirs=False, dtype=np.complex128):
    """out = sum over the matrices in mmask of L[A][m] vec(neighbour_m(A)) on every site, or (out_parity 0 / 1) on the sites of one parity with
    zeros on the other; dtype: the arithmetic (complex64 to see what single precision alone does to a composition)"""
    L = np.asarray(links)
    v = np.asarray(vec).astype(dtype)
    shape = v.shape
    v = v.reshape(L.shape[0], -1)
    out = np.zeros_like(v)
    for m in range(9):
        if (mmask >> m) & 1:
            out += np.einsum("arc,ac->ar", L[:, m].astype(dtype), v[neighbour(Xc, m, _swap_dirs)])
    if out_parity >= 0:
        out[parity_of_sites(Xc) != out_parity] = 0
    return out.reshape(shape)


def hat(links):
    """the preconditioned links: slot 8 = X^-1 (np.linalg.inv per site), slots 0..7 = X^-1 H_d"""
    L = np.asarray(links).astype(np.complex128)
    Xinv = np.linalg.inv(L[:, 8])
    out = np.einsum("aik,amkj->amij", Xinv, L)
    out[:, 8] = Xinv
    return out


def round16(links):
    """a link set rounded through fp16 the way the device's mirror is made (each real through np.float16)"""
    L = np.asarray(links)
    return L.real.astype(np.float16).astype(np.float64) + 1j * L.imag.astype(np.float16).astype(np.float64)


def matpc(links, v, Xc, p, hatlinks=None, _xinv_wrong_parity=False, dtype=np.complex128):
    """Mhat v = v - A_pp^-1 D_pq A_qq^-1 D_qp v for a full field v whose parity 1 - p is zero; hatlinks: the preconditioned links to use
    (default: hat(links)).  _xinv_wrong_parity plants the error of A^-1 applied on the other parity's sites (taken from the forward x neighbour)."""
    H = hat(links) if hatlinks is None else hatlinks
    if _xinv_wrong_parity:
        H = np.array(H, dtype=np.complex128)
        H[:, :8] = np.einsum("aik,amkj->amij", H[neighbour(Xc, 0), 8], np.asarray(links).astype(np.complex128)[:, :8])
    v = np.asarray(v).astype(dtype)
    t = apply(H, v, Xc, HOPS, 1 - p, dtype=dtype)
    return v - apply(H, t, Xc, HOPS, p, dtype=dtype)


def prepare(links, b, Xc, p, hatlinks=None, dtype=np.complex128):
    """the source of the preconditioned system of M x = b (MAT solution): A_pp^-1 (b_p - D_pq A_qq^-1 b_q) on parity p, zero on the other"""
    H = hat(links) if hatlinks is None else hatlinks
    b = np.asarray(b).astype(dtype)
    s = apply(H, b, Xc, LOCAL, 1 - p, dtype=dtype)
    t = apply(links, s, Xc, HOPS, p, dtype=dtype)
    par = parity_of_sites(Xc).reshape((-1,) + (1,) * (b.ndim - 1))
    return apply(H, np.where(par == p, b - t, 0).astype(dtype), Xc, LOCAL, p, dtype=dtype)


def reconstruct(links, x, b, Xc, p, hatlinks=None, dtype=np.complex128):
    """the full solution from its parity p: x_q = A_qq^-1 (b_q - D_qp x_p); the parity 1 - p of the x passed in is ignored"""
    H = hat(links) if hatlinks is None else hatlinks
    b = np.asarray(b).astype(dtype)
    par = parity_of_sites(Xc).reshape((-1,) + (1,) * (b.ndim - 1))
    xp = np.where(par == p, np.asarray(x).astype(dtype), 0).astype(dtype)
    t = apply(links, xp, Xc, HOPS, 1 - p, dtype=dtype)
    return xp + apply(H, np.where(par == p, 0, b - t).astype(dtype), Xc, LOCAL, 1 - p, dtype=dtype)


def to_oracle(links, Xc):
    """(Y[8][sites][n][n], X[sites][n][n]) in the index convention of the oracle's mg_coarse_apply with kappa = 1 (dims 0-3: the link applied
    daggered from the backward neighbour, 4-7 forward; the hopping sign folded out) from bidirectional links whose backward matrices are the
    daggered forward matrices of the neighbours"""
    L = np.asarray(links).astype(np.complex128)
    Y = np.zeros((8,) + L[:, 0].shape, dtype=np.complex128)
    for mu in range(4):
        Y[4 + mu] = -L[:, 2 * mu]
        Y[mu] = -np.conj(np.swapaxes(L[neighbour(Xc, 2 * mu), 2 * mu + 1], -1, -2))
    return Y, L[:, 8].copy()


def random_links(Xc, n, rng, hermitian_hops=True):
    """random bidirectional links; hermitian_hops: the backward matrix of a site is the daggered forward matrix of the neighbour behind it"""
    V = volume(Xc)
    L = rng.standard_normal((V, 9, n, n)) + 1j * rng.standard_normal((V, 9, n, n))
    L[:, 8] += 4 * np.sqrt(n) * np.eye(n)
    if hermitian_hops:
        for mu in range(4):
            L[neighbour(Xc, 2 * mu), 2 * mu + 1] = np.conj(np.swapaxes(L[:, 2 * mu], -1, -2))
    return L


# ---- fp32 elimination: its forward-error bounds and a complex64 restatement to calibrate their constant ----
def inverse_bound(X, Xinv):
    """element-wise forward-error bound of an fp32 elimination without its constant: n 2^-24 (|Xinv| |X| |Xinv|)"""
    n = X.shape[-1]
    return n * EPS32 * (np.abs(Xinv) @ np.abs(X) @ np.abs(Xinv))


def product_bound(X, Xinv, H):
    """the matching bound of the fp32 product Xinv H_d: the inverse's error carried through H plus the product's own rounding"""
    n = X.shape[-1]
    aH = np.abs(H)
    aXi = np.abs(Xinv)[:, None]
    return n * EPS32 * ((aXi @ np.abs(X)[:, None] @ aXi + aXi) @ aH)


def gauss_jordan_c64(X, count_swaps=False, _skip_swap=False):
    """batched Gauss-Jordan inverse with partial pivoting in complex64 arithmetic (numpy's order of operations, the device's arithmetic);
    count_swaps: also the number of columns per site at which the pivot search picked another row.  _skip_swap plants the error of a kernel
    that finds the pivot row and scales by it but leaves the rows where they are."""
    X = np.asarray(X).astype(np.complex64)
    S, n, _ = X.shape
    aug = np.concatenate([X, np.broadcast_to(np.eye(n, dtype=np.complex64), X.shape)], axis=2)
    rows = np.arange(S)
    swaps = np.zeros(S, dtype=np.int64)
    for p in range(n):
        piv = p + np.argmax(np.abs(aug[:, p:, p]), axis=1)
        swaps += piv != p
        pivot = aug[rows, piv, p]
        if not _skip_swap:
            tmp = aug[rows, p].copy()
            aug[rows, p] = aug[rows, piv]
            aug[rows, piv] = tmp
        aug[:, p] = aug[:, p] / pivot[:, None]
        f = aug[:, :, p].copy()
        f[:, p] = 0
        aug = aug - f[:, :, None] * aug[:, None, p, :]
    assert aug.dtype == np.complex64
    return (aug[:, :, n:], swaps) if count_swaps else aug[:, :, n:]


def worst_ratio(got, want, bound):
    """max over the elements of |got - want| / bound; an exact element counts as 0 whatever its bound (a zero bound allows nothing else)"""
    err = np.abs(np.asarray(got).astype(np.complex128) - want)
    with np.errstate(divide="ignore", invalid="ignore"):
        return float(np.max(np.where(err == 0, 0.0, err / bound)))


def synthetic_batches(n, rng, sites=8):
    """the batches of tests/test_coarse_pc_gpu.py: 'swap' P (D + 0.1 R), a random row permutation of a diagonal of moduli 10^uniform(-1, 1) with
    random phases plus a tenth of a complex normal matrix R (E |R_ij|^2 = 1), so that the pivot search has to pick another row in almost every
    column — a site is drawn again until its 2-norm condition number is at most 1e3; 'exact' the identity and diagonal matrices of powers of two
    with phases 1, i, -1, -i, whose elimination is exact in fp32"""
    swap = np.zeros((sites, n, n), dtype=np.complex128)
    for s in range(sites):
        while True:
            D = 10.0 ** rng.uniform(-1, 1, n) * np.exp(2j * np.pi * rng.uniform(0, 1, n))
            R = (rng.standard_normal((n, n)) + 1j * rng.standard_normal((n, n))) / np.sqrt(2)
            perm = rng.permutation(n)
            M = (np.diag(D) + 0.1 * R)[perm]
            if not np.any(perm == np.arange(n)) and np.linalg.cond(M.astype(np.complex64).astype(np.complex128)) <= 1e3:
                break
        swap[s] = M
    M = swap
    exact = np.zeros_like(M)
    exact[0] = np.eye(n)
    d = 2.0 ** rng.integers(-3, 4, (sites, n)) * (1j ** rng.integers(0, 4, (sites, n)))
    exact[1:, np.arange(n), np.arange(n)] = d[1:]
    return swap.astype(np.complex64), exact.astype(np.complex64)
