"""CPU leg of tests/test_coarse_transfer_gpu.py: the oracle's R, P and block orthonormalisation (oracle/qo_mg.c) at 2-spin input with the
colour counts of the production hierarchy, tied to the few-line einsum / QR restatements of tests/transfer_ref.py to 1e-12; the comparison the
GPU tests make (rel < 2e-5 against the oracle) shown to catch the errors a lane-group restrictor can make; and the case table of the GPU tests
checked against the restated rules of the library, so that a case whose reach was worked out wrongly fails here, without a GPU."""
import numpy as np
import pytest

import oracle_api
import transfer_ref as tr

# (lattice, aggregates, Nc, Nvec, slots of restrict_small_kernel for that aggregate): 24 sites -> GS 32 -> 16 slots < 32 iterations;
# 16 sites -> GS 16 -> 32 slots > 4 iterations
SHAPES = [((2, 2, 2, 6), (2, 2, 2, 3), 24, 32, 16), ((4, 2, 2, 4), (2, 2, 2, 2), 8, 4, 32)]
IDS = ["2x24to32-2x2x2x3-on-2x2x2x6", "2x8to4-2x2x2x2-on-4x2x2x4"]
TOL = 2e-5   # the bar of the GPU tests


def rel(a, b):
    return float(np.max(np.abs(a - b)) / np.max(np.abs(b)))


def cvec(rng, shape):
    return rng.standard_normal(shape) + 1j * rng.standard_normal(shape)


class Env:
    pass


@pytest.fixture(scope="module", params=SHAPES, ids=IDS)
def env(request):
    e = Env()
    e.X, e.bs, e.Nc, e.Nv, e.nslots = request.param
    e.o = oracle_api.load()
    rng = np.random.default_rng(19)
    V, Vc = int(np.prod(e.X)), int(np.prod(e.X)) // int(np.prod(e.bs))
    e.geom = (list(e.X), list(e.bs), 2, e.Nc, e.Nv, 1)
    e.table = tr.aggregates(e.X, e.bs)
    e.B = cvec(rng, (V, 2, e.Nc, e.Nv))
    e.V = e.o.mg_block_orthogonalize(e.B, *e.geom)
    e.phi, e.eta = cvec(rng, (V, 2, e.Nc)), cvec(rng, (Vc, 2, e.Nv))
    e.R, e.P = e.o.mg_restrict(e.phi, e.V, *e.geom), e.o.mg_prolongate(e.eta, e.V, *e.geom)
    assert tr.route(int(np.prod(e.bs)), e.Nv)[2] == e.nslots
    return e


def test_oracle_against_einsum_and_qr(env):
    e = env
    assert np.max(np.abs(e.V - tr.block_qr(e.B, e.table))) < 1e-12
    assert np.max(np.abs(e.R - tr.restrict(e.phi, e.V, e.table))) < 1e-12
    assert np.max(np.abs(e.P - tr.prolongate(e.eta, e.V, e.table))) < 1e-12
    # the fp64 Gram-Schmidt of transfer_ref (whose complex64 twin sets the orthonormalisation bar of the GPU tests) is the oracle's
    M = tr.gram_schmidt(tr.block_matrices(e.B, e.table), np.complex128)
    assert np.max(np.abs(tr.from_block_matrices(M, e.table, 2, e.Nc) - e.V)) < 1e-12
    G = np.einsum("bmi,bmj->bij", M.conj(), M) - np.eye(e.Nv)
    assert np.max(np.abs(G)) < 1e-12


def test_single_parity_reference_is_the_restriction_of_the_masked_source(env):
    e = env
    Vh = len(e.phi) // 2
    both = 0
    for par in (0, 1):
        src = e.phi.copy()
        src[(1 - par) * Vh:(2 - par) * Vh] = 0
        both = both + e.o.mg_restrict(src, e.V, *e.geom)
    assert np.max(np.abs(both - e.R)) < 1e-12


@pytest.mark.parametrize("error", ["chirality", "swap", "leak", "drop"])
def test_the_comparison_catches_a_planted_error(env, error):
    e = env
    clean = tr.restrict_planted(e.phi, e.V, e.table, e.nslots)
    assert rel(clean, e.R) < 1e-12                    # the restrictor the errors are planted in is right without them
    if error == "drop" and e.Nv <= e.nslots:
        assert np.array_equal(tr.restrict_planted(e.phi, e.V, e.table, e.nslots, error), clean)   # one trip: nothing to drop at this shape
        return
    bad = tr.restrict_planted(e.phi, e.V, e.table, e.nslots, error)
    r = rel(bad, e.R)
    print("planted %s: rel %.2e against the bar %.0e" % (error, r, TOL))
    assert r > 1e3 * TOL, (error, r)


def test_a_prolongator_with_the_wrong_chirality_or_pair_order_is_caught(env):
    e = env
    half = np.concatenate([e.eta[:, :1], e.eta[:, :1]], axis=1)               # every fine spin fed from coarse chirality 0: (k / Nc) / 2
    swapped = e.eta.reshape(len(e.eta), 2, e.Nv // 2, 2)[..., ::-1].reshape(e.eta.shape)
    for name, eta in (("chirality", half), ("swap", swapped)):
        r = rel(tr.prolongate(eta, e.V, e.table), e.P)
        assert r > 1e3 * TOL, (name, r)


def test_a_source_that_is_zero_comes_back_zero(env):
    e = env
    assert not np.any(e.o.mg_restrict(np.zeros_like(e.phi), e.V, *e.geom))
    assert not np.any(e.o.mg_prolongate(np.zeros_like(e.eta), e.V, *e.geom))


@pytest.mark.parametrize("name", list(tr.CASES))
def test_case_table_follows_the_rules_of_the_library(name):
    """what every GPU case says it reaches on level 1, from the restated block fallback (Transfer::Transfer) and work-group rule (transfer.hip)"""
    X, req, nvec, _, (got, rt, gs, slots, trips) = tr.CASES[name]
    X1 = [X[d] // 4 for d in range(4)]
    assert tr.blocks_after_fallback(X, (4, 4, 4, 4)) == [4, 4, 4, 4]
    assert tr.blocks_after_fallback(X1, req) == list(got)
    assert tr.route(int(np.prod(got)), nvec[1]) == (rt, gs, slots, trips)
    if name.isupper():
        assert list(got) == list(req)                       # the lattices that reach the aggregates asked for
        assert all((X1[d] // got[d]) % 2 == 0 for d in range(4))


def test_no_blocking_leaves_an_odd_coarse_extent():
    """why Xc[d] == 1 (MaskArg::single, a coarse lattice with an extent of 1) cannot be reached through a hierarchy"""
    for L in (2, 4, 6, 8, 12):
        for b in (1, 2, 3, 4, 6):
            for d in (0, 3):
                Xf, bs = [4, 4, 4, 4], [1, 1, 1, 1]
                Xf[d], bs[d] = L, b
                g = tr.blocks_after_fallback(Xf, bs)[d]
                assert g == 0 or (Xf[d] % g == 0 and (Xf[d] // g) % 2 == 0), (L, b, d, g)
