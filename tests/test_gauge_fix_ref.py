"""The numpy reference of gauge fixing by overrelaxation (tests/gauge_fix_ref.py) pinned by properties that do not depend on how it
is written: theta is the squared gradient of F, the sweeps never lower F and never change a gauge-invariant quantity, a pure gauge
is fixed to the unit field, the returned transformation reproduces the fixed links, Coulomb gauge ignores the time links, and the
anti-periodic sign goes through untouched (no GPU needed)."""
import numpy as np
import pytest

import gauge_fix_ref as gf
import gauge_obs_ref as ob
from synth import smooth_gauge

X = (4, 4, 2, 6)   # x, y, z, t: an extent of 2, where x + mu and x - mu are the same site


def _lam():
    """the eight generators T_a = lambda_a / 2, tr T_a T_b = delta_ab / 2"""
    l = np.zeros((8, 3, 3), dtype=np.complex128)
    l[0][0, 1] = l[0][1, 0] = 1
    l[1][0, 1], l[1][1, 0] = -1j, 1j
    l[2][0, 0], l[2][1, 1] = 1, -1
    l[3][0, 2] = l[3][2, 0] = 1
    l[4][0, 2], l[4][2, 0] = -1j, 1j
    l[5][1, 2] = l[5][2, 1] = 1
    l[6][1, 2], l[6][2, 1] = -1j, 1j
    l[7] = np.diag([1, 1, -2]) / np.sqrt(3.0)
    return l / 2.0


@pytest.fixture(scope="module")
def hot():
    return ob.random_su3(np.random.default_rng(5), (4, X[3], X[2], X[1], X[0]))


@pytest.fixture(scope="module")
def warm(oracle):
    U = ob.from_qdp(oracle, smooth_gauge(X, 0.35), X)
    return ob.gauge_transform(U, ob.random_su3(np.random.default_rng(6), U.shape[1:5]))


def _delta(U, D):
    B = sum(ob._bwd(U[mu], mu) - U[mu] for mu in range(D))
    A = B - ob._dag(B)
    return A - np.trace(A, axis1=-2, axis2=-1)[..., None, None] * np.eye(3) / 3.0


@pytest.mark.parametrize("D", [4, 3])
def test_theta_is_the_squared_gradient_of_F(hot, D):
    """S = 3 D V F = sum Re tr U.  Under g(x) = exp(i eps T) at one site, dS/d eps = -(1/2) tr(i T Delta(x)); and with the eight
    generators T_a, tr(Delta Delta^dag) = 8 sum_a (dS/d eps_a)^2, so theta = (8 / 3V) sum_x sum_a (dS/d eps_a)^2"""
    U, T = hot, _lam()
    V = int(np.prod(X))
    Dl = _delta(U, D)
    grad = -0.5 * np.einsum("aij,...ji->...a", 1j * T, Dl)
    assert np.max(np.abs(grad.imag)) < 1e-13
    F, theta = gf.quality(U, D)
    assert abs(theta - 8.0 * np.sum(grad.real ** 2) / (3.0 * V)) <= 1e-12 * theta
    eps = 1e-5
    for site in [(0, 0, 0, 0), (5, 1, 3, 2), (2, 0, 1, 3)]:
        for a in range(8):
            S = []
            for e in (eps, -eps):
                g = np.zeros(U.shape[1:], dtype=np.complex128)
                g[...] = np.eye(3)
                g[site] = ob.exp_eigh(e * T[a])
                S.append(gf.quality(ob.gauge_transform(U, g), D)[0] * 3.0 * D * V)
            numeric = (S[0] - S[1]) / (2.0 * eps)
            assert abs(numeric - grad[site][a].real) <= 1e-8, (site, a, numeric, grad[site][a].real)


@pytest.mark.parametrize("omega", [1.0, 1.5, 1.7])
@pytest.mark.parametrize("D", [4, 3])
def test_sweeps_raise_F_and_keep_the_plaquettes(hot, D, omega):
    U = hot
    plaq0 = ob.plaq(U)
    F = gf.quality(U, D)[0]
    for it in range(6):
        for parity in (0, 1):
            U = gf.sweep(U, D, omega, parity)
        Fn = gf.quality(U, D)[0]
        assert Fn >= F, (it, Fn, F)
        F = Fn
        assert np.max(np.abs(ob.plaq(U) - plaq0)) <= 1e-13
    assert np.max(np.abs(U @ ob._dag(U) - np.eye(3))) <= 1e-13


def test_a_pure_gauge_is_fixed_to_F_equal_one():
    g = ob.random_su3(np.random.default_rng(8), (X[3], X[2], X[1], X[0]))
    unit = np.zeros((4,) + g.shape, dtype=np.complex128)
    unit[...] = np.eye(3)
    U, _, info = gf.fix(ob.gauge_transform(unit, g), 4, 1.5, 1e-26, 400, 4, 1)
    assert info[0] < 400
    assert abs(info[1] - 1.0) <= 1e-12 and abs(gf.quality(U, 4)[0] - 1.0) <= 1e-12


@pytest.mark.parametrize("D", [4, 3])
def test_the_transformation_reproduces_the_fixed_links(warm, D):
    U, G, info = gf.fix(warm, D, 1.5, 0.0, 9, 4, 1, transform=True)
    assert info[0] == 9
    assert np.max(np.abs(ob.gauge_transform(warm, G) - U)) <= 1e-12
    assert np.max(np.abs(ob.plaq(U) - ob.plaq(warm))) <= 1e-13


def test_coulomb_gauge_ignores_the_time_links_but_transforms_them(warm):
    other = np.array(warm)
    other[3] = ob.random_su3(np.random.default_rng(9), warm.shape[1:5])
    assert gf.quality(other, 3) == gf.quality(warm, 3)
    assert gf.quality(other, 4) != gf.quality(warm, 4)
    a, b = warm, other
    for parity in (0, 1):
        a, b = gf.sweep(a, 3, 1.5, parity), gf.sweep(b, 3, 1.5, parity)
    assert np.array_equal(a[:3], b[:3])
    assert np.max(np.abs(a[3] - warm[3])) > 1e-3


def test_the_anti_periodic_sign_is_taken_off_and_put_back(warm):
    U, G, info = gf.fix(warm, 4, 1.5, 0.0, 6, 4, 1, transform=True)
    Ua, Ga, infoa = gf.fix(ob.flip_time_boundary(warm), 4, 1.5, 0.0, 6, 4, 1, transform=True, antiperiodic=True)
    assert np.array_equal(Ua, ob.flip_time_boundary(U)) and np.array_equal(Ga, G) and infoa == info


def test_stopping_rules_and_the_refused_interval(warm):
    _, _, by_theta = gf.fix(warm, 4, 1.5, 1e-3, 400, 4, 1)
    assert by_theta[0] < 400 and by_theta[2] < 1e-3
    _, _, by_delta = gf.fix(warm, 4, 1.5, 1e-5, 400, 4, 0)
    assert by_delta[0] < 400 and by_delta[3] < 1e-5
    with pytest.raises(ValueError):
        gf.fix(warm, 4, 1.5, 0.0, 1, 0, 1)
