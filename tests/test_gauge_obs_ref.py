"""The numpy reference of the gauge observables (tests/gauge_obs_ref.py) pinned on its own, without a GPU: its plaquette against
the oracle's, and the exact properties of stout smearing and of the clover-leaf charge density.  Bounds: 1e-13 for the properties
of the links (unitarity, covariance; a prototype of this reference gave 7e-15 and 4e-15 on these lattices), 1e-14 for the gauge
invariance of q(x) (2.5e-17 measured, max|q| of a hot field is about 0.02)."""
import numpy as np
import pytest

import gauge_obs_ref as ref
from synth import smooth_gauge

LATTICES = [(4, 4, 4, 4), (6, 4, 2, 8)]


def _fields(oracle, X):
    hot, _, _ = oracle.make_fields(list(X), seed=31, antiperiodic_t=True, clover=False)
    return {"hot": ref.from_qdp(oracle, hot, X), "warm": ref.from_qdp(oracle, smooth_gauge(X, 0.35), X)}, hot


@pytest.fixture(scope="module", params=LATTICES, ids=lambda X: "x".join(map(str, X)))
def case(request, oracle):
    X = request.param
    fields, hot_qdp = _fields(oracle, X)
    g = ref.random_su3(np.random.default_rng(5), (X[3], X[2], X[1], X[0]))
    return X, fields, hot_qdp, g


def _unitarity(U):
    return np.max(np.abs(U @ np.conj(np.swapaxes(U, -1, -2)) - np.eye(3)))


def test_layout_round_trip_and_plaquette_match_the_oracle(case, oracle):
    X, fields, hot_qdp, _ = case
    assert np.array_equal(ref.to_qdp(oracle, fields["hot"], X), hot_qdp)
    assert np.max(np.abs(ref.plaq(fields["hot"]) - oracle.plaquette(hot_qdp, list(X)))) < 1e-13
    warm_qdp = ref.to_qdp(oracle, fields["warm"], X)
    assert np.max(np.abs(ref.plaq(fields["warm"]) - oracle.plaquette(warm_qdp, list(X)))) < 1e-13


@pytest.mark.parametrize("kind", ["hot", "warm"])
@pytest.mark.parametrize("ndir,n,rho", [(3, 3, 0.1), (4, 2, 0.12)])
def test_stout_is_unitary_and_gauge_covariant(case, kind, ndir, n, rho):
    X, fields, _, g = case
    U = fields[kind]
    S = ref.stout(U, rho, n, ndir)
    assert _unitarity(S) < 1e-13
    # the hot field carries the anti-periodic sign on its last time links (determinant -1 there), and smearing keeps it
    assert np.max(np.abs(np.linalg.det(ref.flip_time_boundary(S) if kind == "hot" else S) - 1.0)) < 1e-13
    Sg = ref.stout(ref.gauge_transform(U, g), rho, n, ndir)
    assert np.max(np.abs(Sg - ref.gauge_transform(S, g))) < 1e-13
    if ndir == 3:
        assert np.array_equal(S[3], U[3])   # time links untouched
    else:
        assert np.max(np.abs(S[3] - U[3])) > 1e-3
    # the smearing smooths: the spatial plaquette of the hot field rises
    if kind == "hot":
        assert ref.plaq(S)[1] > ref.plaq(U)[1]


@pytest.mark.parametrize("kind", ["hot", "warm"])
def test_charge_density_is_gauge_invariant(case, kind):
    X, fields, _, g = case
    U = fields[kind]
    q = ref.qdensity(U)
    assert q.shape == (X[3], X[2], X[1], X[0])
    assert np.max(np.abs(q)) > 1e-6
    assert np.max(np.abs(ref.qdensity(ref.gauge_transform(U, g)) - q)) < 1e-14
    # F_mu_nu is anti-Hermitian and transforms in the adjoint
    F, Fg = ref.fmunu(U), ref.fmunu(ref.gauge_transform(U, g))
    for a, b in zip(F, Fg):
        assert np.max(np.abs(a + np.conj(np.swapaxes(a, -1, -2)))) < 1e-15
        assert np.max(np.abs(b - g @ a @ np.conj(np.swapaxes(g, -1, -2)))) < 1e-13


def test_unit_gauge_is_a_fixed_point_with_zero_charge():
    X = (6, 4, 2, 8)
    U = np.zeros((4, X[3], X[2], X[1], X[0], 3, 3), dtype=np.complex128)
    U[...] = np.eye(3)
    assert np.array_equal(ref.stout(U, 0.1, 3, 3), U)
    assert np.array_equal(ref.stout(U, 0.12, 2, 4), U)
    q = ref.qdensity(U)
    assert np.all(q == 0.0) and q.sum() == 0.0
    assert np.array_equal(ref.plaq(U), np.ones(3))


def test_zero_steps_and_zero_rho_return_the_links(case):
    _, fields, _, _ = case
    U = fields["hot"]
    assert np.array_equal(ref.stout(U, 0.1, 0, 3), U)
    assert np.max(np.abs(ref.stout(U, 0.0, 2, 4) - U)) < 1e-15


def test_exp_eigh_against_the_power_series():
    rng = np.random.default_rng(11)
    Q = ref.random_hermitian_traceless(rng, 64, 0.7)
    E = ref.exp_eigh(Q)
    S, T = np.zeros_like(E), np.broadcast_to(np.eye(3, dtype=np.complex128), E.shape).copy()
    for k in range(1, 40):
        S += T
        T = T @ (1j * Q) / k
    assert np.max(np.abs(E - S)) < 1e-13
    assert np.max(np.abs(np.linalg.det(E) - 1.0)) < 1e-13
