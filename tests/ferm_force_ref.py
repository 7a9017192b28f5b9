"""Host reference of the fermion force of molecular dynamics (Wilson, degenerate twisted mass, non-degenerate doublet) in plain numpy.
TEST INFRASTRUCTURE.

Links U[mu][t, z, y, x, 3, 3] as gauge_obs_ref.from_qdp gives them (an anti-periodic time boundary sits as a sign on the time links of
the last time slice), spinors psi[t, z, y, x, 4, 3] in the host (DeGrand-Rossi) basis, momenta as in gauge_md_ref.py.  Neighbours come
from np.roll and the spin projectors 1 -+ gamma_mu are explicit 4x4 matrices contracted by einsum: no gather, no ghost zones and no
half spinors, so nothing of the device formulation is shared.

Outer product of two full fields (forward neighbours only, projectors as in the oracle's wil_dslash: forward hop (1 - g_mu) U psi(x+mu)):
    O_mu[X, Y](x) = tr_spin[(1 - g_mu) X(x + mu) Y^dag(x) + (1 + g_mu) Y(x + mu) X^dag(x)]      (a 3x3 colour matrix, summed over flavours)
and the kernel-level operation A_mu(x) <- TA(A_mu(x) - sum_i c_i U_mu(x) O_mu[X_i, Y_i](x)).

Pseudofermion force.  S = sum_i c_i phi^dag (Mh^dag Mh + s_i)^-1 phi, x_i = (Mh^dag Mh + s_i)^-1 phi on one parity p0 (p1 the other):
dS = -sum_i c_i d|Mh x_i|^2 at fixed x_i.  With R the site term (1: Wilson, 1 + i a g5: twisted mass, the flavour-mixing twist: doublet)
    asymmetric  Mh = R - k^2 D R^-1 D      X = (x, R^-1 D x),  y = Mh x,          Y = (y, R^-dag D^dag y)
    symmetric   Mh = 1 - k^2 R^-1 D R^-1 D  X = (x, R^-1 D x),  y = R^-dag Mh x,   Y = (y, R^-dag D^dag y)
(first entry on parity p0, second on p1) and F = 2 k^2 TA(U O[X, Y]) is what a force call adds to the momentum per unit dt:
sum_links Re tr(T F) = d/d eps S(exp(eps T) U).  X, Y are built from the oracle's wil_dslash / twist_gamma5, for the doublet from the
functions of tests/test_ndeg_golden.py.  The mass normalisations scale Mh by 1/(4 k^2) (mass) or 1/(2 k) (asymmetric mass), as the
solves and MatQuda do, and the force by the square of that."""
import numpy as np

import gauge_md_ref as md
import gauge_obs_ref as ob
import qa_cases as qc
import test_ndeg_golden as nd
from oracle_api import TWIST_INVERSE

I = 1j
# DeGrand-Rossi, the host basis of the oracle (and of the reference's tests/wilson_dslash_reference.cpp)
GAMMA = np.array([
    [[0, 0, 0, I], [0, 0, I, 0], [0, -I, 0, 0], [-I, 0, 0, 0]],
    [[0, 0, 0, -1], [0, 0, 1, 0], [0, 1, 0, 0], [-1, 0, 0, 0]],
    [[0, 0, I, 0], [0, 0, 0, -I], [-I, 0, 0, 0], [0, I, 0, 0]],
    [[0, 0, 1, 0], [0, 0, 0, 1], [1, 0, 0, 0], [0, 1, 0, 0]],
], dtype=np.complex128)
EYE4 = np.eye(4, dtype=np.complex128)


# ---- layouts ----
def lex_spinor(oracle, full, X):
    """full host spinor (V 24 reals, even sites then odd) -> psi[t, z, y, x, 4, 3]"""
    X = [int(v) for v in X]
    lex = oracle.eo_to_lex(np.ascontiguousarray(full, dtype=np.float64), X, 24).reshape(X[3], X[2], X[1], X[0], 4, 3, 2)
    return lex[..., 0] + I * lex[..., 1]


def host_spinor(oracle, psi, X):
    X = [int(v) for v in X]
    lex = np.stack([psi.real, psi.imag], axis=-1).reshape(-1)
    return oracle.lex_to_eo(np.ascontiguousarray(lex), X, 24)


def embed(v, p0):
    """a parity field as a full host field, zero on the other parity"""
    z = np.zeros_like(v)
    return np.concatenate([v, z] if p0 == 0 else [z, v])


def shift_fwd(psi, mu, antiperiodic=False):
    """psi(x + mu); antiperiodic: the fields change sign across the time boundary"""
    out = np.roll(psi, -1, axis=3 - mu)
    if antiperiodic and mu == 3:
        out = out.copy()
        out[-1] *= -1.0
    return out


# ---- the hop itself with these matrices: pins GAMMA and the projector placement to the oracle (test_ferm_force_ref.py) ----
def dslash(U, psi, dagger=False):
    """sum_mu (1 -+ g_mu) U_mu(x) psi(x + mu) + (1 +- g_mu) U_mu(x - mu)^dag psi(x - mu), all sites"""
    s = -1.0 if dagger else 1.0
    out = np.zeros_like(psi)
    for mu in range(4):
        f = np.einsum("...ab,...sb->...sa", U[mu], shift_fwd(psi, mu))
        out += np.einsum("st,...ta->...sa", EYE4 - s * GAMMA[mu], f)
        b = np.roll(np.einsum("...ba,...sb->...sa", np.conj(U[mu]), psi), 1, axis=3 - mu)
        out += np.einsum("st,...ta->...sa", EYE4 + s * GAMMA[mu], b)
    return out


# ---- outer product and the kernel-level operation ----
def oprod(U, Xf, Yf, antiperiodic=False):
    """O[mu][t, z, y, x, 3, 3] of the full fields Xf, Yf: arrays [t, z, y, x, 4, 3] or lists of them, one per flavour"""
    if isinstance(Xf, np.ndarray):
        Xf, Yf = [Xf], [Yf]
    O = np.zeros(U.shape, dtype=np.complex128)
    for mu in range(4):
        Pm, Pp = EYE4 - GAMMA[mu], EYE4 + GAMMA[mu]
        for Xa, Ya in zip(Xf, Yf):
            O[mu] += np.einsum("st,...ta,...sb->...ab", Pm, shift_fwd(Xa, mu, antiperiodic), np.conj(Ya))
            O[mu] += np.einsum("st,...ta,...sb->...ab", Pp, shift_fwd(Ya, mu, antiperiodic), np.conj(Xa))
    return O


def oprod_force(U, A, pairs, coeff, antiperiodic=False):
    """A_mu <- TA(A_mu - sum_i c_i U_mu O_mu[X_i, Y_i]); pairs = [(X_i, Y_i)]"""
    V = np.zeros(U.shape, dtype=np.complex128)
    for (Xf, Yf), c in zip(pairs, coeff):
        V += c * oprod(U, Xf, Yf, antiperiodic)
    return np.stack([md.ta(A[mu] - U[mu] @ V[mu]) for mu in range(4)])


# ---- the even-odd operators and the fields of their force ----
class Op:
    """kind 'wilson' | 'tm' | 'ndeg'; matpc 'ee' | 'oo' | 'eeasym' | 'ooasym'; norm 'kappa' | 'mass' | 'asym_mass'"""

    def __init__(self, kind, kappa, mu=0.0, flavor=+1, epsilon=0.0, matpc="ee", norm="kappa"):
        self.kind, self.kappa, self.mu, self.flavor, self.epsilon, self.matpc, self.norm = kind, kappa, mu, flavor, epsilon, matpc, norm
        self.p0 = qc.P0[matpc]
        self.asym = matpc.endswith("asym")
        self.nflavor = 2 if kind == "ndeg" else 1
        self.scale = {"kappa": 1.0, "mass": 0.25 / (kappa * kappa), "asym_mass": 0.5 / kappa}[norm]

    def matpc_apply(self, oracle, gauge, v, X, dagger=0):
        """Mh v from the oracle's own even-odd operators, in this normalisation"""
        if self.kind == "wilson":
            out = oracle.wil_matpc(gauge, np.ascontiguousarray(v), list(X), self.kappa, self.matpc, dagger)
        elif self.kind == "tm":
            out = oracle.tm_matpc(gauge, np.ascontiguousarray(v), list(X), self.kappa, self.mu, self.flavor, self.matpc, dagger)
        else:
            out = nd.ndeg_matpc(oracle, gauge, v, X, self.kappa, self.mu, self.epsilon, self.matpc, dagger)
        return self.scale * out

    def hop(self, oracle, gauge, v, X, parity, dagger):
        if self.kind == "ndeg":
            return nd._hop(oracle, gauge, v, X, parity, dagger)
        return oracle.wil_dslash(gauge, np.ascontiguousarray(v), list(X), parity, dagger)

    def rinv(self, oracle, v, dagger):
        if self.kind == "wilson":
            return v
        if self.kind == "tm":
            return oracle.twist_gamma5(np.ascontiguousarray(v), self.kappa, self.mu, self.flavor, dagger, TWIST_INVERSE)
        return nd.ndeg_twist(v, self.kappa, self.mu, self.epsilon, dagger, 1)

    def force_fields(self, oracle, gauge, x, X):
        """(X, Y): per flavour, the full fields psi[t, z, y, x, 4, 3] of the solution x (a parity field, or a parity doublet)"""
        p0, p1 = self.p0, 1 - self.p0
        x = np.ascontiguousarray(x, dtype=np.float64)
        xo = self.rinv(oracle, self.hop(oracle, gauge, x, X, p1, 0), 0)
        y = self.matpc_apply(oracle, gauge, x, X, 0) / self.scale
        if not self.asym:
            y = self.rinv(oracle, y, 1)
        yo = self.rinv(oracle, self.hop(oracle, gauge, y, X, p1, 1), 1)

        def full(own, other):
            out = []
            h = own.size // self.nflavor
            for f in range(self.nflavor):
                a, b = own[f * h:(f + 1) * h], other[f * h:(f + 1) * h]
                out.append(lex_spinor(oracle, np.concatenate([a, b] if p0 == 0 else [b, a]), X))
            return out

        return full(x, xo), full(y, yo)

    def force_coeff(self):
        """F = force_coeff() TA(U O[X, Y])"""
        return 2.0 * self.kappa * self.kappa * self.scale * self.scale


def tm_force(oracle, U, A, xs, coeff, dt, op, X):
    """A + dt sum_i coeff_i F[x_i] for the links U[mu][t, z, y, x, 3, 3] and the parity solutions xs"""
    gauge = ob.to_qdp(oracle, U, X)
    pairs = [op.force_fields(oracle, gauge, x, X) for x in xs]
    return oprod_force(U, A, pairs, [-dt * c * op.force_coeff() for c in coeff])


def minus_norm2_mx(oracle, U, x, op, X):
    """-|Mh(U) x|^2: the part of S that moves with the links at fixed x"""
    y = op.matpc_apply(oracle, ob.to_qdp(oracle, U, X), x, X, 0)
    return -float(np.dot(y, y))


# ---- pseudofermion action and the leapfrog of H = momentum action + Wilson gauge action + phi^dag (Mh^dag Mh)^-1 phi ----
def cg(apply, b, tol, maxiter=2000):
    """plain CG on a Hermitian positive operator over real arrays; stops at |r| <= tol |b|"""
    x = np.zeros_like(b)
    r = b.copy()
    p = r.copy()
    rr = float(np.dot(r, r))
    stop = tol * tol * rr
    for it in range(maxiter):
        if rr <= stop:
            return x, it
        Ap = apply(p)
        alpha = rr / float(np.dot(p, Ap))
        x += alpha * p
        r -= alpha * Ap
        new = float(np.dot(r, r))
        p = r + (new / rr) * p
        rr = new
    raise RuntimeError("CG did not converge")


def solve(oracle, U, phi, op, X, tol):
    gauge = ob.to_qdp(oracle, U, X)
    A = lambda v: op.matpc_apply(oracle, gauge, op.matpc_apply(oracle, gauge, v, X, 0), X, 1)
    return cg(A, np.ascontiguousarray(phi, dtype=np.float64), tol)[0]


def pf_action(oracle, U, phi, op, X, tol):
    return float(np.dot(phi, solve(oracle, U, phi, op, X, tol)))


def leapfrog(oracle, U, A, phi, op, X, beta, dt, n, tol):
    """n steps: half force, (update, force) ..., update, half force; the force is the Wilson gauge force plus the pseudofermion force"""
    paths, coeff = md.wilson_paths()

    def kick(U, A, h):
        A = md.force(U, A, paths, coeff, h * beta / 3.0)
        return tm_force(oracle, U, A, [solve(oracle, U, phi, op, X, tol)], [1.0], h, op, X)

    A = kick(U, A, 0.5 * dt)
    for step in range(n):
        U = md.update(U, A, dt)
        A = kick(U, A, dt if step < n - 1 else 0.5 * dt)
    return U, A


def hamiltonian(oracle, U, A, phi, op, X, beta, tol):
    return md.mom_action(A) + md.wilson_action(U, beta) + pf_action(oracle, U, phi, op, X, tol)


# the inputs of the leapfrog tests (CPU: test_ferm_force_ref.py, GPU: test_ferm_force_gpu.py), chosen so that the reference's own
# dH(dt) / dH(dt/2) lies in [3.7, 4.3]; the measured dH are in the docstring of test_ferm_force_ref.test_leapfrog_energy_violation_is_second_order
LEAPFROG = {"X": (4, 4, 4, 4), "eps": 0.35, "beta": 5.5, "kappa": 0.12, "mu": 0.2, "flavor": +1, "matpc": "ee", "seed": 11, "tau": 0.5,
            "dt": (0.05, 0.025), "tol": 1e-12}


def leapfrog_inputs(oracle):
    """links with the anti-periodic sign, momenta, pseudofermion field (a parity field of unit-variance Gaussians) and the operator"""
    from synth import smooth_gauge
    p = LEAPFROG
    U = ob.flip_time_boundary(ob.from_qdp(oracle, smooth_gauge(p["X"], p["eps"]), p["X"]))
    rng = np.random.default_rng(p["seed"])
    A = md.random_momentum(rng, U.shape[:-2])
    phi = rng.standard_normal(int(np.prod(p["X"])) // 2 * 24)
    return U, A, phi, Op("tm", p["kappa"], p["mu"], p["flavor"], matpc=p["matpc"])
