"""Host reference of the twisted-clover fermion force and of the force of the clover determinant, in plain numpy.  TEST INFRASTRUCTURE.

Fields as in ferm_force_ref.py: links U[mu][t, z, y, x, 3, 3] (the anti-periodic sign on the time links of the last slice), spinors
psi[t, z, y, x, 4, 3] in the host DeGrand-Rossi basis, momenta as in gauge_md_ref.py.  A tensor field is T[f][t, z, y, x, 3, 3], six
general complex colour matrices per site, f = mu (mu - 1) / 2 + nu for nu < mu (F10, F20, F21, F30, F31, F32); on the host it is
[site (even, odd)][f][3][3][re, im].  The clover term is a dense 12 x 12 matrix per site, row and column index 3 spin + colour:
    A(U) = 1 + i c sum_f sigma_f (x) F_f(U),   sigma_mu_nu = (i / 2) [gamma_mu, gamma_nu],   F = gauge_obs_ref.fmunu
with explicit 4 x 4 sigma built from ferm_force_ref.GAMMA, inverses and determinants from np.linalg, neighbours from np.roll and the
plaquettes of the derivative walked link by link without any shared partial product: nothing of the device formulation is shared.

The derivative.  For a fixed tensor field T, L_T(U) = sum_x sum_f Re tr(T_f(x) F_f(x; U)) and G[T] is its force: sum_links
Re tr(Theta G) = d/d eps L_T(exp(eps Theta) U).  With K = (T - T^dag) / 8 (F is anti-Hermitian, so only that part of T counts) and
K_nu_mu = -K_mu_nu, L_T = sum over plaquettes and their four corners c of Re tr(K(c) P_c), P_c the plaquette read from corner c in the
orientation that belongs to K.  The link (x, mu) lies in the plaquette above and the one below it in each nu != mu; read from the link,
in the orientation in which the link is not daggered, each is U_mu(x) times three more links, and the derivative puts K between them at
the corner it passes:  G_mu(x) = TA(U_mu(x) sum_nu sum_(above, below) sum_(4 corners) [the three links with K(corner) inserted]).

sigma outer product  S_f[X, Y](x)_ba = sum_ss' (sigma_f)_ss' X(x)_s'b conj(Y(x)_sa),  so that  Y^dag dA X = i c sum_f tr(dF_f S_f);
sigma trace          (tr_sigma B)_f(x)_ba = sum_ss' (sigma_f)_ss' B(x)_(s'b)(sa)  of  B = A (A^2 + a^2)^-1,
so that d log det(A^2 + a^2) = 2 tr(B dA) = 2 i c sum_f tr(dF_f (tr_sigma B)_f).

Twisted clover: R_p = A_p + i a gamma5 on parity p, a = 2 kappa mu flavor; with w = Mh x in the kappa normalisation
    asymmetric  Mh = R - k^2 D R^-1 D        w^dag d_A Mh x = Y0^dag dA X0 + k^2 Y1^dag dA X1
    symmetric   Mh = 1 - k^2 R^-1 D R^-1 D    w^dag d_A Mh x = Y0^dag dA (X0 - w) + k^2 Y1^dag dA X1        (R0^-1 D R1^-1 D x = (x - w) / k^2)
X, Y the fields of ferm_force_ref.Op.force_fields (0: the operator's parity).  d(-|Mh x|^2) = -2 Re(w^dag dMh x), so the clover part of
the force is G[T] with T_f = -2 s^2 i c w_p S_f[X', Y], w_p = 1 on the operator's parity and k^2 on the other, s the normalisation factor."""
import numpy as np

import ferm_force_ref as ff
import gauge_md_ref as md
import gauge_obs_ref as ob
from oracle_api import TWIST_INVERSE

I = 1j
PLANES = [(mu, nu) for mu in range(1, 4) for nu in range(mu)]
SIGMA = np.array([0.5j * (ff.GAMMA[mu] @ ff.GAMMA[nu] - ff.GAMMA[nu] @ ff.GAMMA[mu]) for mu, nu in PLANES])


def plane(mu, nu):
    return mu * (mu - 1) // 2 + nu


# ---- layouts ----
def tensor_from_host(oracle, h, X):
    """host tensor field (V, 6, 3, 3, 2), even sites then odd -> T[f][t, z, y, x, 3, 3]"""
    X = [int(v) for v in X]
    lex = oracle.eo_to_lex(np.ascontiguousarray(h, dtype=np.float64).reshape(-1), X, 108).reshape(X[3], X[2], X[1], X[0], 6, 3, 3, 2)
    return np.moveaxis(lex[..., 0] + I * lex[..., 1], 4, 0)


def tensor_to_host(oracle, T, X):
    X = [int(v) for v in X]
    lex = np.moveaxis(np.asarray(T), 0, 4)
    lex = np.stack([lex.real, lex.imag], axis=-1).reshape(-1)
    return oracle.lex_to_eo(np.ascontiguousarray(lex), X, 108).reshape(-1, 6, 3, 3, 2)


def parity_mask(shape4):
    """[t, z, y, x] -> (x + y + z + t) & 1"""
    t, z, y, x = np.indices(shape4)
    return (t + z + y + x) & 1


def unpack_clover(oracle, packed, X):
    """host packed clover field (per site two chiral blocks of 6 diagonal reals and 15 lower complex entries column by column; block
    ch acts on spins 2 ch, 2 ch + 1) -> A[t, z, y, x, 12, 12]"""
    X = [int(v) for v in X]
    lex = oracle.eo_to_lex(np.ascontiguousarray(packed, dtype=np.float64), X, 72).reshape(X[3], X[2], X[1], X[0], 2, 36)
    A = np.zeros(lex.shape[:4] + (12, 12), dtype=np.complex128)
    for ch in range(2):
        k = 0
        for i in range(6):
            A[..., 6 * ch + i, 6 * ch + i] = lex[..., ch, i]
        for col in range(6):
            for row in range(col + 1, 6):
                v = lex[..., ch, 6 + 2 * k] + I * lex[..., ch, 7 + 2 * k]
                A[..., 6 * ch + row, 6 * ch + col] = v
                A[..., 6 * ch + col, 6 * ch + row] = np.conj(v)
                k += 1
    return A


# ---- the clover term and its site-local contractions ----
def clover_matrix(U, c):
    """A[t, z, y, x, 12, 12] = 1 + i c sum_f sigma_f (x) F_f"""
    F = ob.fmunu(U)
    A = np.zeros(U.shape[1:5] + (4, 3, 4, 3), dtype=np.complex128)
    for f in range(6):
        A += I * c * np.einsum("st,...ab->...satb", SIGMA[f], F[f])
    A = A.reshape(U.shape[1:5] + (12, 12))
    return A + np.eye(12)


def sigma_oprod(Xf, Yf):
    """S[f][t, z, y, x, b, a] = sum_ss' (sigma_f)_ss' X_s'b conj(Y_sa)"""
    return np.stack([np.einsum("st,...tb,...sa->...ba", SIGMA[f], Xf, np.conj(Yf)) for f in range(6)])


def b_matrix(A, a):
    """B = A (A^2 + a^2)^-1"""
    return A @ np.linalg.inv(A @ A + a * a * np.eye(12))


def sigma_trace(A, a, coeff=(1.0, 1.0)):
    """T[f][t, z, y, x, b, a] = coeff[parity] sum_ss' (sigma_f)_ss' B_(s'b)(sa)"""
    B = b_matrix(A, a).reshape(A.shape[:4] + (4, 3, 4, 3))
    w = np.where(parity_mask(A.shape[:4]) == 0, coeff[0], coeff[1])[..., None, None]
    return np.stack([w * np.einsum("st,...tbsa->...ba", SIGMA[f], B) for f in range(6)])


def logdet(U, c, a):
    """(L_even, L_odd), L_p = sum over the sites of parity p of log det(A^2 + a^2)"""
    A = clover_matrix(U, c)
    sign, ld = np.linalg.slogdet(A @ A + a * a * np.eye(12))
    par = parity_mask(ld.shape)
    return np.array([ld[par == 0].sum(), ld[par == 1].sum()])


# ---- the derivative ----
def l_t(U, T):
    """L_T(U) = sum_x sum_f Re tr(T_f F_f)"""
    F = ob.fmunu(U)
    return float(sum(np.einsum("...ij,...ji->...", T[f], F[f]).real.sum() for f in range(6)))


def _k_pair(K, mu, nu):
    return K[plane(mu, nu)] if mu > nu else -K[plane(nu, mu)]


def deriv_v(U, T):
    """V[mu]: G_mu = TA(U_mu V_mu)"""
    K = [(T[f] - ob._dag(T[f])) / 8.0 for f in range(6)]
    V = np.zeros(U.shape, dtype=np.complex128)
    for mu in range(4):
        for nu in range(4):
            if nu == mu:
                continue
            # the plaquette above: K_mu_nu, links nu, -mu, -nu from x + mu; below: K_nu_mu, links -nu, -mu, nu
            for Kp, steps in ((_k_pair(K, mu, nu), [nu, 7 - mu, 7 - nu]), (_k_pair(K, nu, mu), [7 - nu, 7 - mu, nu])):
                for ins in range(4):
                    off = [0, 0, 0, 0]
                    off[mu] = 1
                    P = np.eye(3)
                    for k, s in enumerate(steps):
                        if k == ins:
                            P = P @ md._shift(Kp, off)
                        if s < 4:
                            P = P @ md._shift(U[s], off)
                            off[s] += 1
                        else:
                            off[7 - s] -= 1
                            P = P @ ob._dag(md._shift(U[7 - s], off))
                    if ins == 3:
                        P = P @ md._shift(Kp, off)
                    V[mu] += P
    return V


def deriv_force(U, A, T, coeff):
    """A + coeff G[T]"""
    V = deriv_v(U, T)
    return np.stack([A[mu] + coeff * md.ta(U[mu] @ V[mu]) for mu in range(4)])


def logdet_force(U, A, c, a, dt, coeff):
    """A + dt (coeff[0] F[L_even] + coeff[1] F[L_odd])"""
    T = 2.0 * I * c * sigma_trace(clover_matrix(U, c), a, coeff)
    return deriv_force(U, A, T, dt)


# ---- the even-odd twisted-clover operator and its force ----
class Op(ff.Op):
    """kind 'tmc': twisted clover with the clover term rebuilt from the links, c = clover_coeff"""

    def __init__(self, kappa, mu, flavor, c, matpc="ee", norm="kappa"):
        ff.Op.__init__(self, "tmc", kappa, mu, flavor, matpc=matpc, norm=norm)
        self.c = c
        self.a = 2.0 * kappa * mu * flavor
        self._key = None

    def clover(self, oracle, gauge, X):
        key = hash(np.ascontiguousarray(gauge).tobytes())
        if self._key != key:
            cl = oracle.clover_compute(np.ascontiguousarray(gauge), self.c, list(X))
            self._cl, self._key = (cl, oracle.clover_twisted_inverse(cl, 4.0 * self.kappa * self.kappa * self.mu * self.mu)), key
        return self._cl

    def matpc_apply(self, oracle, gauge, v, X, dagger=0):
        cl, cinv = self.clover(oracle, gauge, X)
        return self.scale * oracle.tmc_matpc(gauge, np.ascontiguousarray(v), cl, cinv, list(X), self.kappa, self.mu, self.flavor, self.matpc, dagger)

    def rinv_parity(self, oracle, gauge, v, X, parity, dagger):
        cl, cinv = self.clover(oracle, gauge, X)
        return oracle.twist_clover_gamma5(np.ascontiguousarray(v), cl, cinv, list(X), self.kappa, self.mu, self.flavor, parity, dagger, TWIST_INVERSE)

    def force_fields(self, oracle, gauge, x, X):
        """(X, Y, X'): full fields psi[t, z, y, x, 4, 3]; X' is X with x - Mh x on the operator's parity (symmetric) or X itself"""
        p0, p1 = self.p0, 1 - self.p0
        x = np.ascontiguousarray(x, dtype=np.float64)
        xo = self.rinv_parity(oracle, gauge, oracle.wil_dslash(gauge, x, list(X), p1, 0), X, p1, 0)
        w = self.matpc_apply(oracle, gauge, x, X, 0) / self.scale
        y = w if self.asym else self.rinv_parity(oracle, gauge, w, X, p0, 1)
        yo = self.rinv_parity(oracle, gauge, oracle.wil_dslash(gauge, np.ascontiguousarray(y), list(X), p1, 1), X, p1, 1)
        full = lambda own, other: ff.lex_spinor(oracle, np.concatenate([own, other] if p0 == 0 else [other, own]), X)
        return full(x, xo), full(y, yo), full(x if self.asym else x - w, xo)

    def clover_tensor(self, oracle, gauge, x, X, fields=None):
        """T of the clover part of the force of -|Mh x|^2 per unit coefficient"""
        Xf, Yf, Xp = fields if fields is not None else self.force_fields(oracle, gauge, x, X)
        par = parity_mask(Xf.shape[:4])
        w = np.where(par == self.p0, 1.0, self.kappa * self.kappa)[..., None, None]
        return -2.0 * self.scale * self.scale * I * self.c * w * sigma_oprod(Xp, Yf)


def tmc_force(oracle, U, A, xs, coeff, dt, op, X):
    """A + dt sum_i coeff_i F[x_i]: the hop part through ferm_force_ref.oprod_force, the clover part through deriv_force"""
    gauge = ob.to_qdp(oracle, U, X)
    pairs, T = [], 0.0
    for x, c in zip(xs, coeff):
        Xf, Yf, Xp = op.force_fields(oracle, gauge, x, X)
        pairs.append((Xf, Yf))
        T = T + dt * c * op.clover_tensor(oracle, gauge, x, X, (Xf, Yf, Xp))
    A1 = ff.oprod_force(U, A, pairs, [-dt * c * op.force_coeff() for c in coeff])
    return deriv_force(U, A1, T, 1.0)


def minus_norm2_mx(oracle, U, x, op, X):
    return ff.minus_norm2_mx(oracle, U, x, op, X)


# ---- leapfrog of H = momentum action + Wilson gauge action + phi^dag (Mh^dag Mh)^-1 phi - sum_p cdet_p L_p ----
# (the determinant enters the action as -cdet_p log det: S = ... - sum_p cdet_p L_p is what the weight det(A^2 + a^2)^cdet_p gives)
def kick(oracle, U, A, phi, op, X, beta, h, tol, cdet):
    paths, coeff = md.wilson_paths()
    A = md.force(U, A, paths, coeff, h * beta / 3.0)
    A = tmc_force(oracle, U, A, [ff.solve(oracle, U, phi, op, X, tol)], [1.0], h, op, X)
    return logdet_force(U, A, op.c, op.a, h, [-cdet[0], -cdet[1]])


def leapfrog(oracle, U, A, phi, op, X, beta, dt, n, tol, cdet):
    A = kick(oracle, U, A, phi, op, X, beta, 0.5 * dt, tol, cdet)
    for step in range(n):
        U = md.update(U, A, dt)
        A = kick(oracle, U, A, phi, op, X, beta, dt if step < n - 1 else 0.5 * dt, tol, cdet)
    return U, A


def hamiltonian(oracle, U, A, phi, op, X, beta, tol, cdet):
    ld = logdet(U, op.c, op.a)
    return md.mom_action(A) + md.wilson_action(U, beta) + ff.pf_action(oracle, U, phi, op, X, tol) - cdet[0] * ld[0] - cdet[1] * ld[1]


# the inputs of the leapfrog tests (CPU: test_clover_force_ref.py, GPU: test_clover_force_gpu.py): ferm_force_ref.LEAPFROG with a clover
# coefficient and the determinant of both parities, as the symmetrically preconditioned two-flavour action has it (det M = det R_e
# det R_o det Mh; the asymmetric types keep the eliminated parity only)
LEAPFROG = dict(ff.LEAPFROG, c=0.12 * 1.57551, cdet=(1.0, 1.0))


def leapfrog_inputs(oracle):
    p = LEAPFROG
    U, A, phi, _ = ff.leapfrog_inputs(oracle)
    return U, A, phi, Op(p["kappa"], p["mu"], p["flavor"], p["c"], matpc=p["matpc"])
