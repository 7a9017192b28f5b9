"""CPU self-test of tests/coarse_ref.py, the numpy reference that tests/test_coarse_pc_gpu.py holds the coarse kernels to.  It is tied to
things that do not depend on it: the oracle's coarse operator (oracle/qo_mg.c mg_coarse_apply) on a lattice with a different extent in every
dimension, and a dense solve of M x = b through the Schur pieces.  Planted errors — forward / backward neighbour swapped, Xinv taken from the
wrong site — must be caught by the same checks."""
import numpy as np
import pytest

import coarse_ref as cr


def rel(a, b):
    return float(np.max(np.abs(a - b)) / np.max(np.abs(b)))


def dense_operator(L, Xc):
    V, n = L.shape[0], L.shape[-1]
    M = np.zeros((V * n, V * n), dtype=np.complex128)
    for j in range(V * n):
        e = np.zeros((V, n), dtype=np.complex128)
        e.reshape(-1)[j] = 1
        M[:, j] = cr.apply(L, e, Xc).reshape(-1)
    return M


def test_site_order_is_a_bijection_with_the_stated_coordinates():
    Xc = (4, 2, 6, 2)
    c = cr.coords(Xc)
    assert np.array_equal(cr.site_index(c, Xc), np.arange(cr.volume(Xc)))
    assert np.array_equal(c.sum(axis=1) & 1, cr.parity_of_sites(Xc))
    for m in range(8):   # forward then backward along the same direction returns home; a hop changes the parity
        nb = cr.neighbour(Xc, m)
        assert np.array_equal(cr.neighbour(Xc, m ^ 1)[nb], np.arange(cr.volume(Xc)))
        assert np.all(cr.parity_of_sites(Xc)[nb] != cr.parity_of_sites(Xc))


@pytest.fixture(scope="module")
def anisotropic(oracle):
    Xc, nvec = (4, 2, 6, 2), 2
    rng = np.random.default_rng(5)
    L = cr.random_links(Xc, 2 * nvec, rng)
    v = rng.standard_normal((cr.volume(Xc), 2, nvec)) + 1j * rng.standard_normal((cr.volume(Xc), 2, nvec))
    Y, X = cr.to_oracle(L, Xc)
    want = oracle.mg_coarse_apply(v, Y, X, 1.0, list(Xc), nvec)
    return Xc, L, v, want


def test_apply_equals_the_oracle_on_a_lattice_with_four_different_extents(anisotropic):
    Xc, L, v, want = anisotropic
    r = rel(cr.apply(L, v, Xc, cr.ALL, -1), want)
    print("apply vs oracle: rel %.2e" % r)
    assert r < 1e-12
    # the masks and the single output parity partition the same sum
    parts = sum(cr.apply(L, v, Xc, 1 << m, -1) for m in range(9))
    assert rel(parts, want) < 1e-12
    assert rel(cr.apply(L, v, Xc, cr.ALL, 0) + cr.apply(L, v, Xc, cr.ALL, 1), want) < 1e-12
    assert not np.any(cr.half(cr.apply(L, v, Xc, cr.ALL, 0), 1))


def test_swapped_neighbour_direction_is_caught(anisotropic):
    Xc, L, v, want = anisotropic
    assert rel(cr.apply(L, v, Xc, cr.ALL, -1, _swap_dirs=True), want) > 1e-2
    for m in range(8):   # ... by every single hop in the dimensions longer than 2; at extent 2 both neighbours are the same site
        bad = rel(cr.apply(L, v, Xc, 1 << m, -1, _swap_dirs=True), cr.apply(L, v, Xc, 1 << m, -1))
        assert (bad > 1e-2) == (Xc[m >> 1] > 2), (m, bad)


@pytest.fixture(scope="module")
def dense():
    Xc, nvec = (2, 2, 2, 4), 2
    rng = np.random.default_rng(6)
    L = cr.random_links(Xc, 2 * nvec, rng, hermitian_hops=False)
    b = rng.standard_normal((cr.volume(Xc), 2 * nvec)) + 1j * rng.standard_normal((cr.volume(Xc), 2 * nvec))
    M = dense_operator(L, Xc)
    x = np.linalg.solve(M, b.reshape(-1)).reshape(b.shape)
    return Xc, L, b, x


def schur_solve(Xc, L, b, p, **planted):
    """x from prepare -> dense solve of the matpc system on parity p -> reconstruct"""
    V, n = b.shape
    src = cr.prepare(L, b, Xc, p)
    assert not np.any(cr.half(src, 1 - p))
    idx = np.flatnonzero(np.repeat(cr.parity_of_sites(Xc) == p, n))
    Mhat = np.zeros((idx.size, idx.size), dtype=np.complex128)
    for k, j in enumerate(idx):
        e = np.zeros((V, n), dtype=np.complex128)
        e.reshape(-1)[j] = 1
        col = cr.matpc(L, e, Xc, p, **planted)
        Mhat[:, k] = col.reshape(-1)[idx]
    xp = np.zeros((V, n), dtype=np.complex128)
    xp.reshape(-1)[idx] = np.linalg.solve(Mhat, src.reshape(-1)[idx])
    return cr.reconstruct(L, xp, b, Xc, p)


@pytest.mark.parametrize("p", [0, 1])
def test_schur_pieces_solve_the_full_system(dense, p):
    Xc, L, b, x = dense
    r = rel(schur_solve(Xc, L, b, p), x)
    print("matpc %d: Schur solve vs dense solve rel %.2e" % (p, r))
    assert r < 1e-10
    # matpc leaves the other parity alone
    v = np.where((cr.parity_of_sites(Xc) == p)[:, None], b, 0)
    assert not np.any(cr.half(cr.matpc(L, v, Xc, p), 1 - p))


@pytest.mark.parametrize("p", [0, 1])
def test_xinv_from_the_wrong_site_is_caught(dense, p):
    Xc, L, b, x = dense
    assert rel(schur_solve(Xc, L, b, p, _xinv_wrong_parity=True), x) > 1e-3


def test_hat_links_are_the_inverse_and_its_products():
    Xc = (2, 2, 2, 2)
    L = cr.random_links(Xc, 4, np.random.default_rng(7), hermitian_hops=False)
    H = cr.hat(L)
    assert np.allclose(H[:, 8] @ L[:, 8], np.eye(4), atol=1e-13)
    for d in range(8):
        assert np.allclose(L[:, 8] @ H[:, d], L[:, d], atol=1e-12)


@pytest.mark.parametrize("n", [4, 16, 48, 64])
def test_complex64_elimination_stays_inside_the_forward_error_bound(n):
    """the calibration behind C_HAT of tests/test_coarse_pc_gpu.py on the synthetic batches: a complex64 Gauss-Jordan with partial pivoting against
    the complex128 inverse, in units of n 2^-24 |Xinv| |X| |Xinv|"""
    swap, exact = cr.synthetic_batches(n, np.random.default_rng(100 + n))
    assert np.max(np.linalg.cond(swap.astype(np.complex128))) <= 1e3
    for name, X in (("swap", swap), ("exact", exact)):
        X128 = X.astype(np.complex128)
        want = np.linalg.inv(X128)
        got, swaps = cr.gauss_jordan_c64(X, count_swaps=True)
        assert np.all(swaps >= n // 2) if name == "swap" else not np.any(swaps)   # the batch is there for the row swap
        ratio = cr.worst_ratio(got, want, cr.inverse_bound(X128, want))
        print("n %d %s: complex64 Gauss-Jordan worst ratio %.3f, row swaps per site %s" % (n, name, ratio, swaps))
        assert ratio <= cr.GJ_C64_WORST
    assert np.array_equal(cr.gauss_jordan_c64(exact), np.linalg.inv(exact.astype(np.complex128)).astype(np.complex64))


@pytest.mark.parametrize("n", [4, 16, 48, 64])
def test_skipped_row_swap_is_caught_by_the_bound_on_the_row_swap_batch(n):
    """what test_synthetic_batches of tests/test_coarse_pc_gpu.py would see of a kernel that skips its row swap: far outside C_HAT (and nothing on
    the 'exact' batch or on a near-diagonal X, which never swap — the reason the batch exists)"""
    swap, exact = cr.synthetic_batches(n, np.random.default_rng(100 + n))
    want = np.linalg.inv(swap.astype(np.complex128))
    with np.errstate(all="ignore"):
        bad = cr.gauss_jordan_c64(swap, _skip_swap=True)
    ratio = cr.worst_ratio(np.nan_to_num(bad, nan=1e30, posinf=1e30, neginf=1e30), want, cr.inverse_bound(swap.astype(np.complex128), want))
    assert ratio > 100 * cr.C_HAT
    assert np.array_equal(cr.gauss_jordan_c64(exact, _skip_swap=True), cr.gauss_jordan_c64(exact))


def test_parity_field_on_the_wrong_half_is_caught(anisotropic):
    """hops read the other parity, the local term its own: the same half field embedded on the wrong side gives nothing at all"""
    Xc, L, v, _ = anisotropic
    for parity in (0, 1):
        for mmask, in_par in ((cr.HOPS, 1 - parity), (cr.LOCAL, parity)):
            src = cr.half(v, in_par)
            good = cr.apply(L, cr.embed(src, in_par, Xc), Xc, mmask, parity)
            assert np.any(cr.half(good, parity)) and not np.any(cr.half(good, 1 - parity))
            assert not np.any(cr.apply(L, cr.embed(src, 1 - in_par, Xc), Xc, mmask, parity))
            assert rel(cr.apply(L, cr.embed(cr.half(v, 1 - in_par), in_par, Xc), Xc, mmask, parity), good) > 1e-2   # the other half's data in its place


def test_round16_goes_through_numpy_float16():
    L = (np.arange(8).reshape(2, 1, 2, 2) * (0.1 + 0.3j)).astype(np.complex64)
    r = cr.round16(L)
    assert np.array_equal(r.real, L.real.astype(np.float16).astype(np.float64)) and np.array_equal(r.imag, L.imag.astype(np.float16).astype(np.float64))
    assert np.any(r != L)
