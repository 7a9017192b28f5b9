"""Host reference of Landau and Coulomb gauge fixing by overrelaxation in plain numpy.  TEST INFRASTRUCTURE.

Fields as in gauge_obs_ref.py: links U[mu][t, z, y, x, 3, 3], periodic, neighbours from np.roll; an anti-periodic time boundary sits
as a sign on the time links of the last time slice and is taken off before the first sweep and put back after the last.

D = 3 (Coulomb, spatial links) or 4 (Landau).  F = sum_x sum_{mu<D} Re tr U_mu(x) / (3 D V) is maximised;
theta = sum_x tr(Delta Delta^dag) / (3 V) with Delta = B - B^dag - tr(B - B^dag)/3, B = sum_{mu<D} [U_mu(x - mu) - U_mu(x)].
One iteration sweeps the even sites, then the odd ones; at a site the SU(2) subgroups (0,1), (1,2), (0,2) are hit in turn, every hit
applied to all eight links of the site before the next one is computed.  It shares no code with the device: whole-lattice arrays with
a parity mask, the projection by SVD (gauge_md_ref.project), not by the Newton iteration."""
import numpy as np

from gauge_md_ref import project
from gauge_obs_ref import _bwd, _dag, _fwd, flip_time_boundary

SUBGROUPS = ((0, 1), (1, 2), (0, 2))


def parity_mask(shape4):
    """(x + y + z + t) & 1 on [t, z, y, x]"""
    t, z, y, x = np.indices(shape4)
    return (t + z + y + x) & 1


def quality(U, D):
    """(F, theta)"""
    V = U[0].size // 9
    F = sum(np.trace(U[mu], axis1=-2, axis2=-1).real.sum() for mu in range(D)) / (3.0 * D * V)
    B = sum(_bwd(U[mu], mu) - U[mu] for mu in range(D))
    A = B - _dag(B)
    A = A - np.trace(A, axis1=-2, axis2=-1)[..., None, None] * np.eye(3) / 3.0
    theta = np.sum(np.abs(A) ** 2) / (3.0 * V)
    return float(F), float(theta)


def _hit(f, b, D, omega, p, q, active):
    """the overrelaxed SU(2) matrix of subgroup (p, q) embedded in SU(3): the unit matrix where active is False"""
    a = np.zeros((4,) + active.shape)
    for mu in range(D):
        L = b[mu]
        a[0] += (L[..., p, p] + L[..., q, q]).real
        a[1] += (L[..., p, q] + L[..., q, p]).imag
        a[2] += (L[..., p, q] - L[..., q, p]).real
        a[3] += (L[..., p, p] - L[..., q, q]).imag
        L = f[mu]
        a[0] += (L[..., p, p] + L[..., q, q]).real
        a[1] -= (L[..., p, q] + L[..., q, p]).imag
        a[2] -= (L[..., p, q] - L[..., q, p]).real
        a[3] -= (L[..., p, p] - L[..., q, q]).imag
    a0sq, asq = a[0] ** 2, a[1] ** 2 + a[2] ** 2 + a[3] ** 2
    xh = (omega * a0sq + asq) / (a0sq + asq)
    r = 1.0 / np.sqrt(a0sq + xh * xh * asq)
    a0 = a[0] * r
    a1, a2, a3 = a[1] * xh * r, a[2] * xh * r, a[3] * xh * r
    g = np.zeros(active.shape + (3, 3), dtype=np.complex128)
    g[...] = np.eye(3)
    g[..., p, p] = a0 + 1j * a3
    g[..., p, q] = a2 + 1j * a1
    g[..., q, p] = -a2 + 1j * a1
    g[..., q, q] = a0 - 1j * a3
    g[~active] = np.eye(3)
    return g


def sweep(U, D, omega, parity, G=None):
    """one sweep over the sites of one parity; returns the new links (and the new G where one is given)"""
    active = parity_mask(U[0].shape[:4]) == parity
    f = [np.array(U[mu]) for mu in range(4)]
    b = [_bwd(U[mu], mu) for mu in range(4)]
    for p, q in SUBGROUPS:
        g = _hit(f, b, D, omega, p, q, active)
        f = [g @ f[mu] for mu in range(4)]
        b = [b[mu] @ _dag(g) for mu in range(4)]
        if G is not None:
            G = g @ G
    # a site of the other parity: its forward link in mu is the backward link of x + mu, which is active
    m = active[..., None, None]
    out = np.stack([np.where(m, f[mu], _fwd(b[mu], mu)) for mu in range(4)])
    return out if G is None else (out, G)


def fix(U, D, omega, tol, nmax, reunit, stop_theta, transform=False, antiperiodic=False, history=None):
    """returns (links, G or None, (iterations, F, theta, last |dF|)); history (a list): gets (F, theta, |dF|) of every iteration"""
    if reunit <= 0:
        raise ValueError("reunit_interval = 0")
    U = np.array(U, dtype=np.complex128)
    if antiperiodic:
        U = flip_time_boundary(U)
    G = None
    if transform:
        G = np.zeros(U[0].shape, dtype=np.complex128)
        G[...] = np.eye(3)
    F, theta = quality(U, D)
    dF = 0.0
    it = 0
    while it < nmax:
        for parity in (0, 1):
            if transform:
                U, G = sweep(U, D, omega, parity, G)
            else:
                U = sweep(U, D, omega, parity)
        if it % reunit == reunit - 1:
            U = project(U)
        Fn, theta = quality(U, D)
        dF = abs(Fn - F)
        F = Fn
        it += 1
        if history is not None:
            history.append((F, theta, dF))
        if (theta < tol) if stop_theta else (dF < tol):
            break
    if it % reunit != 0:
        U = project(U)
    if antiperiodic:
        U = flip_time_boundary(U)
    return U, G, (it, F, theta, dF)
