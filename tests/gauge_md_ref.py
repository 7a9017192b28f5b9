"""Host reference of the gauge sector of molecular dynamics (path-product force, link update, momentum action, SU(3) projection,
leapfrog) in plain numpy.  TEST INFRASTRUCTURE.

Fields as in gauge_obs_ref.py: links U[mu][t, z, y, x, 3, 3], momenta A[mu][t, z, y, x, 3, 3] (traceless anti-Hermitian), periodic;
an anti-periodic time boundary sits as a sign on the time links of the last time slice.  It shares no formulation with the device:
a path is walked by np.roll of whole fields by the accumulated displacement, exp by the eigen-decomposition (exp_eigh), the
projection by the singular value decomposition.

Conventions (restated from the reference library, lib/gauge_force.cu:51-142, lib/gauge_update_quda.cu:109-152, lib/momentum.cu:31-48,
include/gauge_field_order.h:424-456): steps 0..3 go forwards in x, y, z, t and 7 - d backwards in d; the walk for (x, mu) starts at
x + mu; a forward step multiplies with U_d(y), a backward step with U_d(y - d)^dag; A <- TA(A - eb3 U V)."""
import numpy as np

from gauge_obs_ref import _dag, exp_eigh, from_qdp
from synth import smooth_gauge

EYE = np.eye(3)


# ---- the ten-real momentum ----
def unpack(v):
    """(..., 10) reals -> (..., 3, 3) anti-Hermitian: {Re A01, Im A01, Re A02, Im A02, Re A12, Im A12, Im A00, Im A11, Im A22, 0}"""
    v = np.asarray(v, dtype=np.float64)
    A = np.zeros(v.shape[:-1] + (3, 3), dtype=np.complex128)
    for k, (i, j) in enumerate(((0, 1), (0, 2), (1, 2))):
        A[..., i, j] = v[..., 2 * k] + 1j * v[..., 2 * k + 1]
        A[..., j, i] = -np.conj(A[..., i, j])
    for i in range(3):
        A[..., i, i] = 1j * v[..., 6 + i]
    return A


def pack(A):
    A = np.asarray(A)
    v = np.zeros(A.shape[:-2] + (10,))
    for k, (i, j) in enumerate(((0, 1), (0, 2), (1, 2))):
        v[..., 2 * k] = A[..., i, j].real
        v[..., 2 * k + 1] = A[..., i, j].imag
    for i in range(3):
        v[..., 6 + i] = A[..., i, i].imag
    return v


def mom_from_host(oracle, mom, X):
    """host momentum (V, 4, 10), even sites then odd -> A[mu][t, z, y, x, 3, 3]"""
    X = [int(v) for v in X]
    mom = np.asarray(mom, dtype=np.float64).reshape(-1, 4, 10)
    out = np.empty((4, X[3], X[2], X[1], X[0], 3, 3), dtype=np.complex128)
    for mu in range(4):
        lex = oracle.eo_to_lex(np.ascontiguousarray(mom[:, mu, :]).reshape(-1), X, 10)
        out[mu] = unpack(lex.reshape(X[3], X[2], X[1], X[0], 10))
    return out


def mom_to_host(oracle, A, X):
    X = [int(v) for v in X]
    out = np.empty((int(np.prod(X)), 4, 10))
    for mu in range(4):
        out[:, mu, :] = oracle.lex_to_eo(np.ascontiguousarray(pack(A[mu]).reshape(-1)), X, 10).reshape(-1, 10)
    return out


def ta(M):
    """(M - M^dag)/2 - tr(M - M^dag)/6"""
    a = 0.5 * (M - _dag(M))
    return a - np.trace(a, axis1=-2, axis2=-1)[..., None, None] * EYE / 3.0


def random_momentum(rng, shape):
    """unit-variance Gaussian momenta: A = sum_a p_a T_a with p_a ~ N(0, 1) and tr(A^dag A)/2 = sum_a p_a^2 / 2, the heat bath of
    exp(-tr(A^dag A)/2); the mean of tr(A^dag A)/2 is 4 per link, which the momentum action subtracts"""
    a = rng.standard_normal(tuple(shape) + (3, 3)) + 1j * rng.standard_normal(tuple(shape) + (3, 3))
    return ta(a)


# ---- paths ----
def _shift(F, off):
    """F(x + off)"""
    for d in range(4):
        if off[d]:
            F = np.roll(F, -off[d], axis=3 - d)
    return F


def walk(U, steps, start=(0, 0, 0, 0)):
    """the ordered product of the links along steps, seen from x, for a walk that begins at x + start"""
    off = list(start)
    P = None
    for s in steps:
        if s < 4:
            L = _shift(U[s], off)
            off[s] += 1
        else:
            d = 7 - s
            off[d] -= 1
            L = _dag(_shift(U[d], off))
        P = L if P is None else P @ L
    return P


def _neg(s):
    return 7 - s


def plaquette_loop(a, b):
    return [a, b, _neg(a), _neg(b)]


def rectangle_loop(a, b):
    return [a, a, b, _neg(a), _neg(a), _neg(b)]


def staples(mu, loop_shape):
    """every distinct path that closes the link (x, mu) to a loop of the given shape: the loop in all its orientations, cut open at
    each of its forward steps in mu"""
    found = set()
    for a in range(8):
        for b in range(8):
            if a in (b, _neg(b)):
                continue
            loop = loop_shape(a, b)
            for lp in (loop, [_neg(s) for s in reversed(loop)]):
                for r, s in enumerate(lp):
                    if s == mu:
                        found.add(tuple(lp[r + 1:] + lp[:r]))
    return sorted(found)


def path_table(shapes_and_coeffs):
    """(paths[mu][i], coeff[i]) of an action sum_shapes c_shape sum_loops Re tr: the paths of every direction in one common order"""
    paths = [[] for _ in range(4)]
    coeff = []
    for shape, c in shapes_and_coeffs:
        n = None
        for mu in range(4):
            st = staples(mu, shape)
            paths[mu] += [list(p) for p in st]
            n = len(st) if n is None else n
            assert len(st) == n
        coeff += [float(c)] * n
    return paths, coeff


def wilson_paths():
    return path_table([(plaquette_loop, 1.0)])


def symanzik_paths(c1=-1.0 / 12.0):
    """tree-level Symanzik: plaquettes with c0 = 1 - 8 c1, 1x2 rectangles with c1"""
    return path_table([(plaquette_loop, 1.0 - 8.0 * c1), (rectangle_loop, c1)])


# ---- force, update, action ----
def force(U, A, paths, coeff, eb3):
    out = np.empty_like(A)
    for mu in range(4):
        start = [0, 0, 0, 0]
        start[mu] = 1
        V = np.zeros_like(U[mu])
        for p, c in zip(paths[mu], coeff):
            if c == 0 or len(p) == 0:
                continue
            V = V + c * walk(U, p, start)
        out[mu] = ta(A[mu] - eb3 * (U[mu] @ V))
    return out


def update(U, A, dt, conj=False, exact=True):
    A = A - np.trace(A, axis1=-2, axis2=-1)[..., None, None] * EYE / 3.0
    if conj:
        A = np.conj(A)
    if exact:
        return exp_eigh(-1j * dt * A) @ U
    R = U
    for r in range(8, 0, -1):
        R = (dt / r) * (A @ R) + U
    return R


def mom_action_terms(A):
    """per link: sum_{j<6} v_j^2 + (1/2) sum_{j=6..8} v_j^2 - 4 of the ten reals"""
    v = pack(A)
    return np.sum(v[..., :6] ** 2, axis=-1) + 0.5 * np.sum(v[..., 6:9] ** 2, axis=-1) - 4.0


def mom_action(A):
    return float(np.sum(mom_action_terms(A)))


def project(U):
    """the nearest unitary matrix (polar factor, through the SVD) with the phase of its determinant divided out"""
    u, _, vh = np.linalg.svd(U)
    W = u @ vh
    det = np.linalg.det(W)
    return W * np.exp(-1j * np.angle(det) / 3.0)[..., None, None]


def loop_action(U, beta, shapes_and_coeffs):
    """-(beta/3) sum_shapes c sum_loops Re tr, every unoriented loop once"""
    s = 0.0
    for shape, c in shapes_and_coeffs:
        pairs = [(a, b) for a in range(4) for b in range(4) if a != b]
        if shape is plaquette_loop:
            pairs = [(a, b) for a, b in pairs if a < b]
        for a, b in pairs:
            s += c * np.trace(walk(U, shape(a, b)), axis1=-2, axis2=-1).real.sum()
    return -(beta / 3.0) * s


def wilson_action(U, beta):
    return loop_action(U, beta, [(plaquette_loop, 1.0)])


def leapfrog(U, A, paths, coeff, beta, dt, n):
    """n steps: half force, (update, force) ..., update, half force"""
    eb3 = dt * beta / 3.0
    A = force(U, A, paths, coeff, 0.5 * eb3)
    for step in range(n):
        U = update(U, A, dt)
        A = force(U, A, paths, coeff, eb3 if step < n - 1 else 0.5 * eb3)
    return U, A


# the inputs of the leapfrog tests (CPU: test_gauge_md_ref.py, GPU: test_gauge_md_gpu.py): lattice, smooth_gauge width, beta, momentum
# seed, trajectory length, the two step sizes.  Kept because the reference's own dH(dt) / dH(dt/2) on them is 3.92 (dH = -4.986 and
# -1.271), inside [3.5, 4.5]; seeds 12 and 13 give 3.91 and 3.89
LEAPFROG = {"X": (4, 4, 4, 4), "eps": 0.35, "beta": 5.5, "seed": 11, "tau": 0.5, "dt": (0.05, 0.025)}


def leapfrog_inputs(oracle):
    p = LEAPFROG
    U = from_qdp(oracle, smooth_gauge(p["X"], p["eps"]), p["X"])
    A = random_momentum(np.random.default_rng(p["seed"]), U.shape[:-2])
    return U, A
