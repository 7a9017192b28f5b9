"""Host reference of the gauge observables (stout smearing, clover-leaf field strength, topological charge density, plaquette) in
plain numpy.  TEST INFRASTRUCTURE.

Links are complex arrays U[mu][t, z, y, x, 3, 3] (mu = 0..3 = x, y, z, t), periodic; a field with an anti-periodic time boundary
carries its sign on the last time slice, exactly as the host arrays handed to loadGaugeQuda do.  Neighbours come from np.roll.
exp(iQ) is evaluated through the eigen-decomposition (np.linalg.eigh), deliberately not by the Cayley-Hamilton form the device
kernel uses, so that the two share no arithmetic."""
import numpy as np


def from_qdp(oracle, gauge, X):
    """(4, V*18) host QDP arrays (even sites then odd) -> U[mu][t, z, y, x, 3, 3]"""
    X = [int(v) for v in X]
    out = np.empty((4, X[3], X[2], X[1], X[0], 3, 3), dtype=np.complex128)
    for mu in range(4):
        lex = oracle.eo_to_lex(np.ascontiguousarray(gauge[mu], dtype=np.float64), X, 18).reshape(X[3], X[2], X[1], X[0], 3, 3, 2)
        out[mu] = lex[..., 0] + 1j * lex[..., 1]
    return out


def to_qdp(oracle, U, X):
    """inverse of from_qdp"""
    X = [int(v) for v in X]
    out = np.empty((4, int(np.prod(X)) * 18))
    for mu in range(4):
        lex = np.stack([U[mu].real, U[mu].imag], axis=-1).reshape(-1)
        out[mu] = oracle.lex_to_eo(np.ascontiguousarray(lex), X, 18)
    return out


def flip_time_boundary(U):
    """the links with the time links of the last time slice negated: takes the anti-periodic sign off (or puts it on)"""
    out = np.array(U)
    out[3, -1] *= -1.0
    return out


def fp32_recon12(U, antiperiodic):
    """the links as a fp32 12-real device field holds them: rows 0 and 1 rounded to fp32, row 2 = conj(row 0 x row 1) in fp32, with
    the anti-periodic sign put back on the time links of the last time slice.  U[mu][t, ..., 3, 3]: any site axes behind t"""
    R = U.astype(np.complex64)
    R[..., 2, :] = np.conj(np.cross(R[..., 0, :], R[..., 1, :]))
    if antiperiodic:
        R[3, -1, ..., 2, :] *= -1
    return R.astype(np.complex128)


def _fwd(A, mu):
    """A(x + mu)"""
    return np.roll(A, -1, axis=3 - mu)


def _bwd(A, mu):
    """A(x - mu)"""
    return np.roll(A, 1, axis=3 - mu)


def _dag(A):
    return np.conj(np.swapaxes(A, -1, -2))


def exp_eigh(Q):
    """exp(iQ) of Hermitian matrices (..., 3, 3) through their eigen-decomposition"""
    Q = np.asarray(Q, dtype=np.complex128)
    w, V = np.linalg.eigh(Q)
    return (V * np.exp(1j * w)[..., None, :]) @ _dag(V)


def staple_sum(U, nu, dirs):
    """S_nu(x) = sum_{mu in dirs, mu != nu} [U_mu(x) U_nu(x+mu) U_mu(x+nu)^dag + U_mu(x-mu)^dag U_nu(x-mu) U_mu(x-mu+nu)]"""
    S = np.zeros_like(U[nu])
    for mu in dirs:
        if mu == nu:
            continue
        S += U[mu] @ _fwd(U[nu], mu) @ _dag(_fwd(U[mu], nu))
        S += _bwd(_dag(U[mu]) @ U[nu] @ _fwd(U[mu], nu), mu)
    return S


def stout(U, rho, n, ndir):
    """n stout steps (Morningstar and Peardon, hep-lat/0311018) of the directions 0..ndir-1, staples from those directions only;
    every direction of a step is smeared from the links of the previous step"""
    U = np.array(U, dtype=np.complex128)
    eye = np.eye(3)
    for _ in range(int(n)):
        new = U.copy()
        for nu in range(ndir):
            Om = rho * staple_sum(U, nu, range(ndir)) @ _dag(U[nu])
            A = _dag(Om) - Om
            A = A - np.trace(A, axis1=-2, axis2=-1)[..., None, None] * eye / 3.0
            new[nu] = exp_eigh(0.5j * A) @ U[nu]
        U = new
    return U


def fmunu(U):
    """the six F_mu_nu = (Q_mu_nu - Q_mu_nu^dag) / 8 (no trace removed), Q the sum of the four clover leaves at x; index
    mu (mu - 1) / 2 + nu for nu < mu: F10, F20, F21, F30, F31, F32"""
    F = []
    for mu in range(1, 4):
        for nu in range(mu):
            Um, Un = U[mu], U[nu]
            Q = Um @ _fwd(Un, mu) @ _dag(_fwd(Um, nu)) @ _dag(Un)
            Q = Q + Un @ _dag(_bwd(_fwd(Um, nu), mu)) @ _dag(_bwd(Un, mu)) @ _bwd(Um, mu)
            Q = Q + _dag(_bwd(Un, nu)) @ _bwd(Um, nu) @ _bwd(_fwd(Un, mu), nu) @ _dag(Um)
            Q = Q + _dag(_bwd(Um, mu)) @ _dag(_bwd(_bwd(Un, mu), nu)) @ _bwd(_bwd(Um, mu), nu) @ _bwd(Un, nu)
            F.append((Q - _dag(Q)) / 8.0)
    return F


def _retr(A, B):
    return np.einsum("...ij,...ji->...", A, B).real


def qdensity(U):
    """q(x) = [Re tr(F10 F32) + Re tr(F30 F21) - Re tr(F20 F31)] / (4 pi^2), shape [t, z, y, x]"""
    F = fmunu(U)
    return (_retr(F[0], F[5]) + _retr(F[3], F[2]) - _retr(F[1], F[4])) / (4.0 * np.pi ** 2)


def plaq(U):
    """(total, spatial, temporal) plaquette averages, Re tr / 3 per plaquette; total = mean of the other two"""
    V = U[0].size // 9
    s = [0.0, 0.0]
    for mu in range(3):
        for nu in range(mu + 1, 4):
            P = U[mu] @ _fwd(U[nu], mu) @ _dag(_fwd(U[mu], nu)) @ _dag(U[nu])
            s[0 if nu < 3 else 1] += np.trace(P, axis1=-2, axis2=-1).real.sum()
    sp, tm = s[0] / (9.0 * V), s[1] / (9.0 * V)
    return np.array([0.5 * (sp + tm), sp, tm])


def gauge_transform(U, g):
    """U_mu(x) -> g(x) U_mu(x) g(x + mu)^dag, g[t, z, y, x, 3, 3]"""
    return np.stack([g @ U[mu] @ _dag(_fwd(g, mu)) for mu in range(4)])


def random_su3(rng, shape):
    """Haar-ish SU(3) matrices of the given leading shape (QR of a complex Gaussian, determinant phase divided out)"""
    z = rng.standard_normal(tuple(shape) + (3, 3)) + 1j * rng.standard_normal(tuple(shape) + (3, 3))
    q, r = np.linalg.qr(z)
    d = np.diagonal(r, axis1=-2, axis2=-1)
    q = q * (d / np.abs(d))[..., None, :]
    return q / np.linalg.det(q)[..., None, None] ** (1.0 / 3.0)


def random_hermitian_traceless(rng, n, scale=1.0):
    a = rng.standard_normal((n, 3, 3)) + 1j * rng.standard_normal((n, 3, 3))
    h = 0.5 * (a + _dag(a))
    h = h - np.trace(h, axis1=-2, axis2=-1)[:, None, None] * np.eye(3) / 3.0
    return scale * h
