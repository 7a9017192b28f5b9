"""One-end-trick loop contractions of one solution vector (qudaAmdContractLoop, reference oneEndTrick_w_One_Der,
lib/qudaQKXTM_Loops_Kepler.cpp:300-497) against a numpy restatement written from the formulas: the building block
C[u, v][4a + b] = sum_c conj(u[(a + 2) mod 4, c]) v[b, c] in the UKQCD basis, the covariant shifts on the host links as loaded
(time boundary included), phi = g5 D_W x with D_W from the oracle at mu = 0, explicit momentum phases with global coordinates.
Tolerance 1e-12 relative to the largest entry of each of the 18 blocks, as the two-point tests use for fp64 sums of this length."""
import importlib
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KAPPA = 0.13
QSQ = 3
LATTICES = [(4, 4, 4, 8), (8, 8, 8, 8)]


@pytest.fixture(scope="module")
def qa():
    mod = importlib.import_module("quda-qkxtm-multigrid_amd")
    mod.init(0)
    yield mod
    mod.end()


def _fields(oracle, X, antiperiodic, clover=False, seed=7):
    gauge, _, clv = oracle.make_fields(list(X), seed=seed, antiperiodic_t=antiperiodic, clover=clover)
    V = int(np.prod(X))
    x = np.random.default_rng(31 + seed + X[0]).standard_normal(V * 24)
    return gauge, clv, x


def _lex_links(oracle, gauge, X):
    V = int(np.prod(X))
    g = np.stack([oracle.eo_to_lex(np.ascontiguousarray(gauge[d]), list(X), 18) for d in range(4)]).reshape(4, V, 3, 3, 2)
    return (g[..., 0] + 1j * g[..., 1]).reshape((4, X[3], X[2], X[1], X[0], 3, 3))


def _cplx(v, X):
    c = v.reshape(-1, 4, 3, 2)
    return (c[..., 0] + 1j * c[..., 1]).reshape(X[3], X[2], X[1], X[0], 4, 3)


def _wilson(oracle, gauge, clover, x, X):
    """D_W x for a lexicographic UKQCD host vector: the oracle's full operator at mu = 0 (even-odd, DeGrand-Rossi)"""
    dr = oracle.ukqcd_to_dr(x.reshape(-1, 24)).reshape(-1)
    eo = oracle.lex_to_eo(dr, list(X), 24)
    if clover is None:
        out = oracle.tm_mat(gauge, eo, list(X), KAPPA, 0.0, +1, 0)
    else:
        out = oracle.tmc_mat(gauge, clover, eo, list(X), KAPPA, 0.0, +1, 0)
    return oracle.dr_to_ukqcd(oracle.eo_to_lex(out, list(X), 24).reshape(-1, 24)).reshape(-1)


def _C(u, v):
    return np.einsum("...ac,...bc->...ab", np.roll(u, -2, axis=-2).conj(), v)


def numpy_loops(x, Dx, U, X, moms):
    """x, Dx: (V*24,) lexicographic UKQCD; U: (4, T, Z, Y, X, 3, 3) host links as loaded.  Returns (18, T, Nmoms, 16)."""
    v = _cplx(x, X)
    phi = np.roll(_cplx(Dx, X), 2, axis=-2)      # g5 = [[0, 1], [1, 0]] in 2 x 2 blocks
    ax = [3, 2, 1, 0]                              # array axis of direction mu

    def F(f, mu):
        return np.einsum("...ab,...sb->...sa", U[mu], np.roll(f, -1, axis=ax[mu]))

    def B(f, mu):
        return np.roll(np.einsum("...ba,...sb->...sa", U[mu].conj(), f), 1, axis=ax[mu])

    blocks = [-_C(v, v), _C(v, phi)]
    std_d, std_c, gen_d, gen_c = [], [], [], []
    for mu in range(4):
        Fx, Bx, Fp, Bp = F(v, mu), B(v, mu), F(phi, mu), B(phi, mu)
        std_d.append(-(_C(v, Fx) + _C(Bx, v) - _C(Fx, v) - _C(v, Bx)))
        std_c.append(-(_C(v, Fx) + _C(Bx, v) + _C(Fx, v) + _C(v, Bx)))
        gen_d.append(_C(v, Fp) + _C(Bx, phi) - _C(Fx, phi) - _C(v, Bp))
        gen_c.append(_C(v, Fp) + _C(Bx, phi) + _C(Fx, phi) + _C(v, Bp))
    pos = np.stack(blocks + std_d + std_c + gen_d + gen_c).reshape(18, X[3], X[2], X[1], X[0], 16)
    z, y, xx = np.meshgrid(np.arange(X[2]), np.arange(X[1]), np.arange(X[0]), indexing="ij")
    ph = np.stack([np.exp(-2j * np.pi * (n[0] * xx / X[0] + n[1] * y / X[1] + n[2] * z / X[2])) for n in moms])
    return np.einsum("mzyx,ktzyxg->ktmg", ph, pos)


def _block_err(got, want):
    errs = [np.max(np.abs(got[k] - want[k])) / np.max(np.abs(want[k])) for k in range(18)]
    for k, e in enumerate(errs):
        print("block %2d: max |want| %.3e, relative error %.3e" % (k, np.max(np.abs(want[k])), e))
    return max(errs)


def _ip(qa, clover):
    ip = qa.invert_param(qa.QUDA_TWISTED_CLOVER_DSLASH if clover else qa.QUDA_TWISTED_MASS_DSLASH, KAPPA, 0.05, +1, "ee", 0, cuda_prec=8,
                         solution_type=qa.QUDA_MAT_SOLUTION, gamma_basis=qa.QUDA_UKQCD_GAMMA_BASIS)
    return ip


def _load(qa, gauge, X, antiperiodic, recon=18):
    qa.load_gauge(gauge, qa.gauge_param(X, recon=recon, t_boundary=qa.QUDA_ANTI_PERIODIC_T if antiperiodic else qa.QUDA_PERIODIC_T))


@pytest.mark.parametrize("X", LATTICES)
@pytest.mark.parametrize("antiperiodic", [False, True])
def test_twisted_mass_matches_numpy(qa, oracle, X, antiperiodic, qsq=QSQ):
    gauge, _, x = _fields(oracle, X, antiperiodic)
    _load(qa, gauge, X, antiperiodic)
    got = qa.contract_loop(x, _ip(qa, False), qsq, X[:3])
    moms = qa.loop_momenta(X[:3], qsq)
    assert got.shape == (18, X[3], len(moms), 16)
    want = numpy_loops(x, _wilson(oracle, gauge, None, x, X), _lex_links(oracle, gauge, X), X, moms)
    assert _block_err(got, want) < 1e-12


@pytest.mark.parametrize("qsq,nmoms", [(1, 7), (5, 42)])
def test_twisted_mass_matches_numpy_momentum_chunks(qa, oracle, qsq, nmoms):
    """QSQ = 3 (27 momenta on 4^3) takes the one-pass branch of the shared projection (up to 36 momenta); 7 momenta are one chunk of 8,
    42 are six chunks of 8, the last holding two.  Same restatement, same bound."""
    assert len(qa.loop_momenta(LATTICES[0][:3], qsq)) == nmoms
    test_twisted_mass_matches_numpy(qa, oracle, LATTICES[0], False, qsq)


@pytest.mark.parametrize("X", LATTICES)
@pytest.mark.parametrize("antiperiodic", [False, True])
def test_twisted_clover_matches_numpy(qa, oracle, X, antiperiodic):
    gauge, clover, x = _fields(oracle, X, antiperiodic, clover=True)
    _load(qa, gauge, X, antiperiodic)
    ip = _ip(qa, True)
    qa.load_clover(clover, None, ip)
    got = qa.contract_loop(x, ip, QSQ, X[:3])
    moms = qa.loop_momenta(X[:3], QSQ)
    want = numpy_loops(x, _wilson(oracle, gauge, clover, x, X), _lex_links(oracle, gauge, X), X, moms)
    assert _block_err(got, want) < 1e-12


def test_compressed_links_match_numpy(qa, oracle):
    """12-real links: the boundary sign is applied in the kernel, the stored links do not carry it"""
    X = LATTICES[0]
    gauge, _, x = _fields(oracle, X, True)
    _load(qa, gauge, X, True, recon=12)
    got = qa.contract_loop(x, _ip(qa, False), QSQ, X[:3])
    want = numpy_loops(x, _wilson(oracle, gauge, None, x, X), _lex_links(oracle, gauge, X), X, qa.loop_momenta(X[:3], QSQ))
    assert _block_err(got, want) < 1e-12


@pytest.mark.parametrize("mask", [0b0110, 0b1001])
def test_partitioned_directions_match_numpy(qa, oracle, mask):
    """single-process emulation of a grid-decomposed lattice: the neighbours across the faces come through the ghost exchange"""
    X = LATTICES[0]
    gauge, _, x = _fields(oracle, X, True)
    _load(qa, gauge, X, True)
    qa.lib().qudaAmdSetPartitionMask(mask)
    try:
        got = qa.contract_loop(x, _ip(qa, False), QSQ, X[:3])
    finally:
        qa.lib().qudaAmdSetPartitionMask(0)
    want = numpy_loops(x, _wilson(oracle, gauge, None, x, X), _lex_links(oracle, gauge, X), X, qa.loop_momenta(X[:3], QSQ))
    assert _block_err(got, want) < 1e-12


def _random_su3(rng, n):
    a = rng.standard_normal((n, 3, 3)) + 1j * rng.standard_normal((n, 3, 3))
    q, r = np.linalg.qr(a)
    d = np.diagonal(r, axis1=1, axis2=2)
    q = q * (d / np.abs(d))[:, None, :]
    return q / np.linalg.det(q)[:, None, None] ** (1.0 / 3.0)


@pytest.mark.parametrize("X", LATTICES)
def test_gauge_covariance(qa, oracle, X):
    """x -> g x, U_mu(x) -> g(x) U_mu(x) g(x + mu)^+ leaves all 18 colour-traced blocks unchanged"""
    gauge, _, x = _fields(oracle, X, True)
    _load(qa, gauge, X, True)
    ip = _ip(qa, False)
    before = qa.contract_loop(x, ip, QSQ, X[:3])
    V = int(np.prod(X))
    g = _random_su3(np.random.default_rng(5), V).reshape(X[3], X[2], X[1], X[0], 3, 3)
    U = _lex_links(oracle, gauge, X)
    ax = [3, 2, 1, 0]
    Ug = np.stack([np.einsum("...ab,...bc,...dc->...ad", g, U[mu], np.roll(g, -1, axis=ax[mu]).conj()) for mu in range(4)]).reshape(4, V, 9)
    gauge_g = np.stack([oracle.lex_to_eo(np.ascontiguousarray(np.stack([Ug[mu].real, Ug[mu].imag], axis=-1).reshape(-1)), list(X), 18) for mu in range(4)])
    xg = np.einsum("...ab,...sb->...sa", g, _cplx(x, X))
    xg = np.ascontiguousarray(np.stack([xg.real, xg.imag], axis=-1).reshape(-1))
    _load(qa, gauge_g, X, True)
    after = qa.contract_loop(xg, ip, QSQ, X[:3])
    assert _block_err(after, before) < 1e-12


_CHILD = """
import importlib, sys
import numpy as np
sys.path.insert(0, %r)
sys.path.insert(0, %r)
import oracle_api
qa = importlib.import_module("quda-qkxtm-multigrid_amd")
d = np.load(sys.argv[1])
X = [int(v) for v in d["X"]]
qa.init(0)
qa.load_gauge(d["gauge"], qa.gauge_param(X, t_boundary=qa.QUDA_ANTI_PERIODIC_T))
ip = qa.invert_param(qa.QUDA_TWISTED_MASS_DSLASH, float(d["kappa"]), 0.05, +1, "ee", 0, cuda_prec=8, solution_type=qa.QUDA_MAT_SOLUTION,
                     gamma_basis=qa.QUDA_UKQCD_GAMMA_BASIS)
np.save(sys.argv[2], qa.contract_loop(d["x"], ip, int(d["qsq"]), X[:3]))
qa.end()
"""


@pytest.mark.parametrize("X", LATTICES)
def test_unfused_chain_matches(qa, oracle, X, tmp_path):
    """QUDA_AMD_LOOP_FUSED=0 (covariant shifts and pairwise contractions in the reference's call order) in a child process"""
    gauge, _, x = _fields(oracle, X, True)
    _load(qa, gauge, X, True)
    fused = qa.contract_loop(x, _ip(qa, False), QSQ, X[:3])
    inp, out, script = tmp_path / "in.npz", tmp_path / "out.npy", tmp_path / "child.py"
    np.savez(str(inp), X=np.array(X), gauge=gauge, x=x, kappa=KAPPA, qsq=QSQ)
    script.write_text(_CHILD % (ROOT, os.path.join(ROOT, "tests")))
    r = subprocess.run([sys.executable, str(script), str(inp), str(out)], capture_output=True, text=True, timeout=300, env=dict(os.environ, QUDA_AMD_LOOP_FUSED="0"))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    chain = np.load(str(out))
    want = numpy_loops(x, _wilson(oracle, gauge, None, x, X), _lex_links(oracle, gauge, X), X, qa.loop_momenta(X[:3], QSQ))
    assert _block_err(chain, want) < 1e-12
    assert _block_err(chain, fused) < 1e-12


def test_chunked_driver_equals_unchunked_bit_for_bit(qa, oracle, tmp_path):
    """QUDA_AMD_LOOP_TCHUNK=3 in a child process: 8 time slices staged and projected in chunks of 3, 3 and 2, so the shared projection
    runs with t0 > 0 and nt > 1 together, as the production loops do once their staged blocks pass 2 GiB.  The summation order within
    a slice does not depend on the chunking, so the result equals the parent's single chunk in every bit"""
    X = LATTICES[1]
    gauge, _, x = _fields(oracle, X, True)
    _load(qa, gauge, X, True)
    whole = qa.contract_loop(x, _ip(qa, False), QSQ, X[:3])
    inp, out, script = tmp_path / "in.npz", tmp_path / "out.npy", tmp_path / "child.py"
    np.savez(str(inp), X=np.array(X), gauge=gauge, x=x, kappa=KAPPA, qsq=QSQ)
    script.write_text(_CHILD % (ROOT, os.path.join(ROOT, "tests")))
    r = subprocess.run([sys.executable, str(script), str(inp), str(out)], capture_output=True, text=True, timeout=300, env=dict(os.environ, QUDA_AMD_LOOP_TCHUNK="3"))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    chunked = np.load(str(out))
    assert chunked.shape == whole.shape and np.array_equal(chunked.view(np.float64).view(np.uint64), whole.view(np.float64).view(np.uint64))
    want = numpy_loops(x, _wilson(oracle, gauge, None, x, X), _lex_links(oracle, gauge, X), X, qa.loop_momenta(X[:3], QSQ))
    assert _block_err(chunked, want) < 1e-12


def test_twisted_mass_matches_numpy_where_a_share_holds_many_sites(qa, oracle):
    """12 x 10 x 14 x 4: a time slice has 1680 sites, so the 64 shares of the shared projection hold 26 or 27 and their 16 site lanes
    make a second trip, fed by the fused staging kernel.  Same restatement, same bound; the projection itself is held to a per-element
    bound in tests/test_momproj_gpu.py"""
    test_twisted_mass_matches_numpy(qa, oracle, (12, 10, 14, 4), True)
