"""The numpy reference of gauge molecular dynamics (tests/gauge_md_ref.py) against things that do not depend on it: the finite-difference
derivative of the action, gauge covariance, the unit gauge, the closed form of the momentum action, and the order of the leapfrog
integrator.  No GPU.  The leapfrog inputs (gauge_md_ref.LEAPFROG) are the ones tests/test_gauge_md_gpu.py runs through the C ABI."""
import numpy as np
import pytest

import gauge_md_ref as md
import gauge_obs_ref as ob
from synth import smooth_gauge

X = (4, 4, 4, 4)
LEAPFROG, leapfrog_inputs = md.LEAPFROG, md.leapfrog_inputs


@pytest.fixture(scope="module")
def warm(oracle):
    return ob.from_qdp(oracle, smooth_gauge(X, 0.35), X)


ACTIONS = {"wilson": [(md.plaquette_loop, 1.0)], "plaquette+rectangle": [(md.plaquette_loop, 5.0 / 3.0), (md.rectangle_loop, -1.0 / 12.0)]}


def test_the_enumerator_finds_six_staples_and_eighteen_rectangle_paths():
    paths, coeff = md.symanzik_paths()
    for mu in range(4):
        assert len(paths[mu]) == 24 and [len(p) for p in paths[mu]] == [3] * 6 + [5] * 18
        for p in paths[mu]:   # every path closes the link: the steps sum to -mu
            off = [0, 0, 0, 0]
            for s in p:
                off[s if s < 4 else 7 - s] += 1 if s < 4 else -1
            assert off == [-1 if d == mu else 0 for d in range(4)]
    assert coeff == [1.0 - 8.0 * (-1.0 / 12.0)] * 6 + [-1.0 / 12.0] * 18


@pytest.mark.parametrize("name", sorted(ACTIONS))
def test_force_is_the_derivative_of_the_action(warm, name):
    """d/d eps S(exp(eps Y) U) at 0 = -(beta/3) sum Re tr(Y U V) = (beta/3) sum Re tr(Y G) with G = force(U, 0, ..., eb3 = 1) = -TA(U V).
    Central differences are exact to O(eps^2): halving eps must cut the discrepancy to a quarter (0.3 allowed)."""
    beta = 5.5
    shapes = ACTIONS[name]
    paths, coeff = md.path_table(shapes)
    G = md.force(warm, np.zeros_like(warm), paths, coeff, 1.0)
    rng = np.random.default_rng(2)
    for trial in range(2):
        Y = md.random_momentum(rng, warm.shape[:-2])
        analytic = (beta / 3.0) * np.sum(np.einsum("...ij,...ji->...", Y, G).real)
        disc = []
        for eps in (1e-2, 5e-3):
            Sp = md.loop_action(md.update(warm, Y, eps), beta, shapes)
            Sm = md.loop_action(md.update(warm, Y, -eps), beta, shapes)
            disc.append(abs((Sp - Sm) / (2 * eps) - analytic))
        print("%s: dS = %.6e, discrepancy %.3e at eps = 1e-2, %.3e at 5e-3" % (name, analytic, disc[0], disc[1]))
        assert disc[0] < 1e-3 * abs(analytic)
        assert disc[1] <= 0.3 * disc[0]


def test_force_is_gauge_covariant_and_vanishes_on_the_unit_gauge(warm):
    paths, coeff = md.symanzik_paths()
    zero = np.zeros_like(warm)
    F = md.force(warm, zero, paths, coeff, 0.7)
    g = ob.random_su3(np.random.default_rng(5), warm.shape[1:-2])
    Fg = md.force(ob.gauge_transform(warm, g), zero, paths, coeff, 0.7)
    assert np.max(np.abs(Fg - g @ F @ ob._dag(g))) <= 1e-13 * np.max(np.abs(F))
    unit = np.broadcast_to(np.eye(3, dtype=np.complex128), warm.shape).copy()
    assert np.max(np.abs(md.force(unit, zero, paths, coeff, 0.7))) == 0.0
    # the anti-periodic sign cancels in every closed loop
    assert np.max(np.abs(md.force(ob.flip_time_boundary(warm), zero, paths, coeff, 0.7) - F)) <= 1e-14 * np.max(np.abs(F))
    # a zero coefficient skips its path
    c2 = list(coeff)
    c2[3] = 0.0
    p2 = [[p for i, p in enumerate(paths[mu]) if i != 3] for mu in range(4)]
    assert np.array_equal(md.force(warm, zero, paths, c2, 0.7), md.force(warm, zero, p2, coeff[:3] + coeff[4:], 0.7))


def test_momentum_action_and_packing():
    rng = np.random.default_rng(7)
    A = md.random_momentum(rng, (4, 5))
    want = 0.5 * np.einsum("...ij,...ij->...", np.conj(A), A).real - 4.0
    assert np.max(np.abs(md.mom_action_terms(A) - want)) <= 1e-14 * np.max(np.abs(want))
    assert abs(md.mom_action(A) - want.sum()) <= 1e-13 * np.abs(want).sum()
    assert np.array_equal(md.unpack(md.pack(A)), A)
    v = md.pack(A)
    assert np.array_equal(md.pack(md.unpack(v)), v) and np.all(v[..., 9] == 0)
    # <tr(A^dag A)/2> = 4 per link: the mean of the action per link is 0 within its standard error
    big = md.mom_action_terms(md.random_momentum(rng, (20000,)))
    assert abs(big.mean()) < 5 * big.std() / np.sqrt(big.size)


def test_taylor_branch_agrees_with_the_exact_one_at_small_dt(warm):
    """largest entry of dt A = 0.1, so its norm is at most 0.3 and the first neglected term of the eighth-order polynomial at most
    0.3^9 / 9! = 5.4e-11: the bound is 1e-10.  Observed 1.1e-14 (max over the 4^4 lattice), i.e. rounding; with the largest entry 1
    the truncation shows, observed 9.5e-6"""
    A = md.random_momentum(np.random.default_rng(3), warm.shape[:-2])
    A = A / np.max(np.abs(A))
    for conj in (False, True):
        d = np.max(np.abs(md.update(warm, A, 0.1, conj, True) - md.update(warm, A, 0.1, conj, False)))
        print("taylor vs exact at |dt A| = 0.1: %.3e" % d)
        assert d <= 1e-10
    d1 = np.max(np.abs(md.update(warm, A, 1.0, False, True) - md.update(warm, A, 1.0, False, False)))
    print("taylor vs exact at |dt A| = 1: %.3e" % d1)
    assert 1e-8 < d1 < 1e-4
    # conj_mom is the complex conjugate, not the Hermitian conjugate: exp(dt conj A) = conj(exp(dt A))
    E = md.update(np.broadcast_to(np.eye(3, dtype=np.complex128), warm.shape), A, 0.3, True, True)
    assert np.max(np.abs(E - np.conj(md.update(np.broadcast_to(np.eye(3, dtype=np.complex128), warm.shape), A, 0.3, False, True)))) <= 1e-14


def test_projection_returns_special_unitary_links(warm):
    noise = np.random.default_rng(9).standard_normal(warm.shape + (2,))
    P = md.project(warm @ (np.eye(3) + 1e-3 * (noise[..., 0] + 1j * noise[..., 1])))
    assert np.max(np.abs(ob._dag(P) @ P - np.eye(3))) <= 1e-14
    assert np.max(np.abs(np.linalg.det(P) - 1.0)) <= 1e-14
    assert np.max(np.abs(P - warm)) < 1e-2
    assert np.max(np.abs(md.project(warm) - warm)) <= 1e-14


def test_leapfrog_energy_violation_is_second_order(oracle):
    """tau = 0.5 on the 4^4 smooth_gauge(0.35) field at beta = 5.5, momenta from seed 11: dH = -4.986 at dt = 0.05 and -1.271 at
    0.025, ratio 3.92 (seeds 12 and 13 give 3.91 and 3.89)"""
    p = LEAPFROG
    U, A = leapfrog_inputs(oracle)
    paths, coeff = md.wilson_paths()
    H0 = md.mom_action(A) + md.wilson_action(U, p["beta"])
    dH = []
    for dt in p["dt"]:
        U1, A1 = md.leapfrog(U, A, paths, coeff, p["beta"], dt, int(round(p["tau"] / dt)))
        dH.append(md.mom_action(A1) + md.wilson_action(U1, p["beta"]) - H0)
    print("dH = %.6e, %.6e, ratio %.4f" % (dH[0], dH[1], dH[0] / dH[1]))
    assert 3.5 <= dH[0] / dH[1] <= 4.5
    # reversibility of the reference itself
    U1, A1 = md.leapfrog(U, A, paths, coeff, p["beta"], 0.05, 10)
    U2, _ = md.leapfrog(U1, -A1, paths, coeff, p["beta"], 0.05, 10)
    assert np.max(np.abs(U2 - U)) <= 1e-12
