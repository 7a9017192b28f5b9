"""Nucleon three-point functions by the fixed-sink method (qudaAmdThreepSeqSource, qudaAmdContractThreep) against numpy restatements
written from the definitions in include/quda_amd_ext.h, and the lattice Ward identity of the conserved current on solved propagators.

The sequential source is the derivative of the projected nucleon two-point function with respect to one propagator.  That function
is linear in every propagator slot, so the derivative is the Wick sum of tests/test_twop_gpu.py with the slot left open: exact.
The contraction restates q, the nine 4 x 4 matrices with np.roll on the host links (boundary sign included), the operator and
current combinations, the '+' phase, the source-relative time and the wrap sign."""
import importlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from synth import smooth_gauge  # noqa: E402
from test_threep_tables import G, ONE, operators, projector  # noqa: E402
from test_twop_gpu import CC, EPS, _lex_gauge, _momenta, _to_tensor  # noqa: E402

LATTICES = [((4, 4, 4, 4), (1, 2, 3, 3), 2), ((6, 4, 2, 8), (5, 1, 1, 6), 3)]   # X, source, tsink: both sink slices wrap (tsink + t0 >= T)
MASKS = [0, 0b0110, 0b1010]


@pytest.fixture(scope="module")
def qa():
    mod = importlib.import_module("quda-qkxtm-multigrid_amd")
    mod.init(0)
    yield mod
    mod.end()


def _flavor_sign(particle, part):
    """+1: the operator sits on the up quark"""
    return +1 if (particle == 0) == (part == 1) else -1


# ---------------------------------------------------------------- sequential source

def _open_slot(A, B, Gtm, pi, Q, r):
    """the Wick sum of test_twop_gpu._wick, contracted with Gtm[n][k], with the propagator of sink slot r left out:
    -> sigma[x, nu (sink spin of the slot), nu' (its source spin), c, c']"""
    sink_s, src_s, sink_c, src_c = "ijk", "lmn", "abc", "def"
    specs = ["x" + sink_s[s] + src_s[pi[s]] + sink_c[s] + src_c[pi[s]] for s in range(3)]
    out = specs[r]
    rest = [specs[s] for s in range(3) if s != r]
    return np.einsum("abc,def,ij,ml,nk," + ",".join(rest) + "->" + out, EPS, EPS, A, B, Gtm, *[Q[s] for s in range(3) if s != r], optimize=True)


def numpy_seq_source(U3, D3, particle, part, pid):
    """U3, D3: smeared propagators on the sink slice, [x, mu, nu, a, b] -> the twelve columns g5 conj(sigma), [col = nu' * 3 + c', x, nu, c]"""
    Cg5 = CC @ G[5]
    Gtm = projector(pid, particle)
    Q = (U3, D3, U3) if particle == 0 else (D3, U3, D3)
    slots = (0, 2) if part == 1 else (1,)
    sigma = 0
    for r in slots:
        sigma = sigma + _open_slot(Cg5, Cg5.T, Gtm, (0, 1, 2), Q, r) - _open_slot(Cg5, Cg5.T, Gtm, (2, 1, 0), Q, r)
    src = np.roll(sigma.conj(), 2, axis=1)                       # g5 = [[0, 1], [1, 0]] in 2 x 2 blocks
    return src.transpose(2, 4, 0, 1, 3).reshape(12, -1, 4, 3)   # [nu', c', x, nu, c]


def _to_real(c):
    return np.ascontiguousarray(np.stack([c.real, c.imag], axis=-1).reshape(c.shape[0], -1))


@pytest.mark.parametrize("X,src,tsink", LATTICES)
@pytest.mark.parametrize("nsmear", [0, 2])
@pytest.mark.parametrize("mask", MASKS)
def test_seq_source_is_the_derivative_of_the_twop(qa, oracle, X, src, tsink, nsmear, mask):
    """random complex propagators, both particles, both parts, all five projectors; 1e-12 relative to the largest entry (the bound of
    the two-point tests for the same arithmetic).  Both sink slices have tsink + t0 >= T."""
    gauge, _, _ = oracle.make_fields(list(X), seed=5, antiperiodic_t=False, clover=False)
    qa.load_gauge(gauge, qa.gauge_param(X, t_boundary=qa.QUDA_PERIODIC_T))
    g_lex = _lex_gauge(oracle, gauge, X)
    V, T = int(np.prod(X)), X[3]
    Vs = V // T
    assert tsink + src[3] >= T
    tg = (tsink + src[3]) % T
    rng = np.random.default_rng(17 + nsmear + mask)
    up, dn = rng.standard_normal((12, V * 24)), rng.standard_normal((12, V * 24))
    alpha = 0.7
    smear = (lambda v: oracle.gauss_smear(np.ascontiguousarray(v), g_lex, list(X), alpha, nsmear)) if nsmear else (lambda v: v)
    U3 = _to_tensor(np.stack([smear(c) for c in up]), V)[tg * Vs:(tg + 1) * Vs]
    D3 = _to_tensor(np.stack([smear(c) for c in dn]), V)[tg * Vs:(tg + 1) * Vs]
    worst = 0.0
    qa.lib().qudaAmdSetPartitionMask(mask)
    try:
        for particle in (qa.PROTON, qa.NEUTRON):
            for part in (1, 2):
                for pid in range(5):
                    got = qa.threep_seq_source(up, dn, g_lex if nsmear else None, src, tsink, pid, particle, part, nsmear, alpha)
                    full = np.zeros((12, V, 4, 3), complex)
                    full[:, tg * Vs:(tg + 1) * Vs] = numpy_seq_source(U3, D3, particle, part, pid)
                    want = np.stack([smear(c) for c in _to_real(full.reshape(12, -1))])
                    assert np.max(np.abs(want)) > 0
                    err = np.max(np.abs(got - want)) / np.max(np.abs(want))
                    print("particle %d part %d projector %d: relative error %.3e" % (particle, part, pid, err))
                    worst = max(worst, err)
    finally:
        qa.lib().qudaAmdSetPartitionMask(0)
    assert worst < 1e-12, worst


# ---------------------------------------------------------------- contraction

def _cplx_links(g_lex, X):
    V = int(np.prod(X))
    g = np.asarray(g_lex).reshape(4, V, 3, 3, 2)
    return (g[..., 0] + 1j * g[..., 1]).reshape((4, X[3], X[2], X[1], X[0], 3, 3))


def _columns(v, X):
    """(12, V*24) -> [t, z, y, x, spin, colour, column]"""
    c = v.reshape(12, -1, 4, 3, 2)
    c = c[..., 0] + 1j * c[..., 1]
    return c.reshape(12, X[3], X[2], X[1], X[0], 4, 3).transpose(1, 2, 3, 4, 5, 6, 0)


def numpy_threep(seq, fwd, U, X, src, tsink, particle, part, moms):
    """the definitions, literally: returns local (T, Nm, 16), noether (T, Nm, 4), oneD (T, Nm, 4, 16)"""
    Fw = _columns(fwd, X)
    q = np.roll(_columns(seq, X), 2, axis=4).conj()             # q[x; kappa, a, (pi, b)] = conj((g5 y)[kappa, a])
    ax = [3, 2, 1, 0]                                           # array axis of direction mu
    S0 = np.einsum("...kac,...lac->...kl", q, Fw)
    AD, BC = [], []
    for mu in range(4):
        Um = U[mu]
        Ub = np.roll(Um, 1, axis=ax[mu])                        # U_mu(x - mu)
        A = np.einsum("...kac,...ab,...lbc->...kl", q, Um, np.roll(Fw, -1, axis=ax[mu]))
        B = np.einsum("...kac,...ba,...lbc->...kl", q, Ub.conj(), np.roll(Fw, 1, axis=ax[mu]))
        Cm = np.einsum("...kac,...ba,...lbc->...kl", np.roll(q, -1, axis=ax[mu]), Um.conj(), Fw)
        D = np.einsum("...kac,...ab,...lbc->...kl", np.roll(q, 1, axis=ax[mu]), Ub, Fw)
        AD.append(A + D)
        BC.append(B + Cm)
    O = operators(_flavor_sign(particle, part))
    local = np.stack([np.einsum("kl,...kl->...", o, S0) for o in O], axis=-1)
    oneD = np.stack([np.stack([0.25 * np.einsum("kl,...kl->...", o, AD[mu] - BC[mu]) for o in O], axis=-1) for mu in range(4)], axis=-2)
    noether = np.stack([0.25 * (np.einsum("kl,...kl->...", ONE + G[mu + 1], BC[mu]) - np.einsum("kl,...kl->...", ONE - G[mu + 1], AD[mu])) for mu in range(4)], axis=-1)
    T, Z, Y, Xx = X[3], X[2], X[1], X[0]
    z, y, x = np.meshgrid(np.arange(Z), np.arange(Y), np.arange(Xx), indexing="ij")
    ph = np.stack([np.exp(+2j * np.pi * (n[0] * (x - src[0]) / Xx + n[1] * (y - src[1]) / Y + n[2] * (z - src[2]) / Z)) for n in moms])
    ts = (np.arange(T) + src[3]) % T
    sign = -1.0 if tsink + src[3] >= T else 1.0
    return (sign * np.einsum("mzyx,tzyxi->tmi", ph, local)[ts], sign * np.einsum("mzyx,tzyxd->tmd", ph, noether)[ts],
            sign * np.einsum("mzyx,tzyxdi->tmdi", ph, oneD)[ts])


def _threep_err(got, want):
    """max over local, noether[mu], oneD[mu] of max |got - want| / max |want|"""
    errs = [np.max(np.abs(got[0] - want[0])) / np.max(np.abs(want[0]))]
    for mu in range(4):
        errs.append(np.max(np.abs(got[1][..., mu] - want[1][..., mu])) / np.max(np.abs(want[1][..., mu])))
        errs.append(np.max(np.abs(got[2][:, :, mu] - want[2][:, :, mu])) / np.max(np.abs(want[2][:, :, mu])))
    print("local, (noether, oneD) x 4 directions: " + " ".join("%.2e" % e for e in errs))
    return max(errs)


def _contract_case(qa, oracle, X, src, tsink, antiperiodic, recon, mask, given, Q, particle=0, part=1):
    gauge, _, _ = oracle.make_fields(list(X), seed=9, antiperiodic_t=antiperiodic, clover=False)
    qa.load_gauge(gauge, qa.gauge_param(X, recon=recon, t_boundary=qa.QUDA_ANTI_PERIODIC_T if antiperiodic else qa.QUDA_PERIODIC_T))
    g_lex = _lex_gauge(oracle, gauge, X)
    V = int(np.prod(X))
    rng = np.random.default_rng(23 + mask + Q)
    seq, fwd = rng.standard_normal((12, V * 24)), rng.standard_normal((12, V * 24))
    qa.lib().qudaAmdSetPartitionMask(mask)
    try:
        got = qa.contract_threep(seq, fwd, g_lex if given else None, src, Q, tsink, particle, part)
    finally:
        qa.lib().qudaAmdSetPartitionMask(0)
    moms = _momenta(Q)
    want = numpy_threep(seq, fwd, _cplx_links(g_lex, X), X, src, tsink, particle, part, moms)
    assert got[0].shape == (X[3], len(moms), 16) and got[1].shape == (X[3], len(moms), 4) and got[2].shape == (X[3], len(moms), 4, 16)
    return _threep_err(got, want)


@pytest.mark.parametrize("X,src,tsink", LATTICES)
@pytest.mark.parametrize("antiperiodic", [False, True])
@pytest.mark.parametrize("recon", [18, 12])
@pytest.mark.parametrize("mask", MASKS)
@pytest.mark.parametrize("given", [False, True])
def test_contraction_matches_numpy(qa, oracle, X, src, tsink, antiperiodic, recon, mask, given, Q=3):
    """random sequential and forward columns, random links; both time boundaries, 18- and 12-real resident links, the three partition
    masks, the links given by the caller (boundary applied) and NULL (the resident ones).  Q = 3: one projection pass.  1e-12
    relative to the largest entry of each of local / noether[mu] / oneD[mu].  The flavour assignment alternates with the case."""
    particle, part = (0, 1) if mask != 0b0110 else (1, 1)
    if antiperiodic:
        part = 2
    assert _contract_case(qa, oracle, X, src, tsink, antiperiodic, recon, mask, given, Q, particle, part) < 1e-12


@pytest.mark.parametrize("Q,nmoms", [(1, 7), (5, 57)])
def test_contraction_matches_numpy_momentum_chunks(qa, oracle, Q, nmoms):
    """the chunked branches of the shared projection on 6 x 4 x 2 x 8 (7 momenta: one chunk of 8; 57: eight chunks); a sink that does not wrap"""
    assert len(_momenta(Q)) == nmoms
    assert _contract_case(qa, oracle, (6, 4, 2, 8), (5, 1, 1, 2), 3, True, 18, 0, False, Q) < 1e-12


# ---------------------------------------------------------------- end to end: charge conservation

WARD_BOUND = 1.5e-11   # ten times the largest deviation measured on the MI355X (1.46e-12); the specification caps it at 1e-6


def _solve_lex(qa, oracle, ip, b_lex, X):
    """one solve of the public solver on a lexicographic UKQCD vector"""
    b = oracle.lex_to_eo(oracle.ukqcd_to_dr(np.ascontiguousarray(b_lex).reshape(-1, 24)).reshape(-1), list(X), 24)
    x = qa.invert(np.ascontiguousarray(b), ip)
    return oracle.dr_to_ukqcd(oracle.eo_to_lex(x, list(X), 24).reshape(-1, 24)).reshape(-1)


@pytest.mark.parametrize("t0", [1, 6])
@pytest.mark.parametrize("norm", ["kappa", "mass"])
def test_charge_conservation_on_solved_propagators(qa, oracle, t0, norm):
    """4 x 4 x 4 x 8, smooth gauge, antiperiodic t, twisted mass, plain GCR to 1e-12, two smearing steps; sources at t0 = 1 and t0 = 6
    (the sink slice wraps), tsink = 3, projector G4, proton and neutron, both parts.  calc_mg_propagators -> threep_seq_source ->
    twelve solves through invertQuda with the opposite twist -> contract_threep.  The lattice Ward identity of the conserved current:
    at zero momentum noether[3](it) is one constant a for 0 < it < 3, one constant b for 3 < it < 8, (a + b) / 2 at it = 0 and
    it = 3, and a - b = n_q C2 / (2 kappa) under kappa normalisation, n_q C2 under mass normalisation (n_q = 2 for part 1, 1 for
    part 2; C2 the G4-projected nucl_nucl two-point function of contract_twop at it = 3, p = 0).  A wrong sign, a missing term or a
    wrong boundary link gives O(1).

    The deviation depends on the solver only.  Measured on the MI355X over the sixteen (t0, normalisation, particle, part)
    combinations: |(a - b) - rhs| / |a| between 9.0e-13 and 1.46e-12, the plateaus and the two midpoints flat to 2.2e-13 of |a|;
    a / C2 = 7.43 (t0 = 1) and 7.56 (t0 = 6), b / C2 = -0.90 and -0.77 for part 1 under kappa normalisation, 1 / 2 kappa = 4.1667.
    The bound is ten times the largest measured deviation."""
    X, kappa, mu, tsink, ns, alpha = (4, 4, 4, 8), 0.12, 0.05, 3, 2, 0.5
    T = X[3]
    gauge = smooth_gauge(X, 0.35)
    gauge[3].reshape(2, -1, 18)[:, (X[0] // 2) * X[1] * X[2] * (T - 1):, :] *= -1.0   # anti-periodic in t, folded into the last time slice
    qa.load_gauge(gauge, qa.gauge_param(X, t_boundary=qa.QUDA_ANTI_PERIODIC_T))
    g_lex = _lex_gauge(oracle, gauge, X)
    V = int(np.prod(X))
    src = (1, 2, 3, t0)

    def make_ip(flavor, basis):
        ip = qa.invert_param(qa.QUDA_TWISTED_MASS_DSLASH, kappa, mu, flavor, "ee", 0, cuda_prec=8, solution_type=qa.QUDA_MAT_SOLUTION, gamma_basis=basis)
        ip.solve_type, ip.inv_type, ip.gcrNkrylov, ip.tol, ip.maxiter = qa.QUDA_DIRECT_PC_SOLVE, qa.QUDA_GCR_INVERTER, 20, 1e-12, 4000
        ip.inv_type_precondition = qa.QUDA_INVALID_ENUM
        ip.mass_normalization = qa.QUDA_MASS_NORMALIZATION if norm == "mass" else qa.QUDA_KAPPA_NORMALIZATION
        ip.verbosity = qa.QUDA_SILENT
        return ip

    up, dn = qa.calc_mg_propagators(g_lex, make_ip(+1, qa.QUDA_UKQCD_GAMMA_BASIS), src, ns, alpha, V)
    _, bar = qa.contract_twop(up, dn, g_lex, src, 0, ns, alpha)
    P4 = (ONE + G[4]) / 4
    worst = 0.0
    for particle in (qa.PROTON, qa.NEUTRON):
        C2 = np.einsum("hg,gh->", P4, bar[tsink, 0, particle, 0])       # sum_{g g'} P4[g'][g] nucl_nucl[g][g']
        for part in (1, 2):
            s = _flavor_sign(particle, part)
            seq_src = qa.threep_seq_source(up, dn, g_lex, src, tsink, qa.G4, particle, part, ns, alpha)
            ip = make_ip(-s, qa.QUDA_DEGRAND_ROSSI_GAMMA_BASIS)           # the twist opposite to the inserted flavour
            seq = np.stack([_solve_lex(qa, oracle, ip, b, X) for b in seq_src])
            _, noether, _ = qa.contract_threep(seq, up if s > 0 else dn, None, src, 0, tsink, particle, part)
            j4 = noether[:, 0, 3]
            a, b = j4[1], j4[tsink + 1]
            scale = abs(a)
            flat = max(np.max(np.abs(j4[1:tsink] - a)), np.max(np.abs(j4[tsink + 1:T] - b)), abs(j4[0] - (a + b) / 2), abs(j4[tsink] - (a + b) / 2)) / scale
            nq = 2 if part == 1 else 1
            rhs = nq * C2 / (2 * kappa) if norm == "kappa" else nq * C2
            dev = abs((a - b) - rhs) / scale
            print("t0 %d %s particle %d part %d: a/C2 = %.6f%+.6fi, b/C2 = %.6f%+.6fi, plateaus flat to %.3e, |(a - b) - rhs| / |a| = %.3e"
                  % (t0, norm, particle, part, (a / C2).real, (a / C2).imag, (b / C2).real, (b / C2).imag, flat, dev))
            worst = max(worst, flat, dev)
    assert worst < WARD_BOUND, worst
