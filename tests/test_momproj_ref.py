"""The reference of the momentum projection tests (tests/momproj_ref.py) checked on the CPU: project() against a naive complex128 DFT,
the float64 restatement of the kernel's order inside the derived bound on every case that tests/test_momproj_gpu.py runs, and eight
mutants of that restatement, each of which must leave the bound on a case of the table: the cases discriminate."""
import numpy as np
import pytest

import momproj_ref as R


def _naive(cs, X, gx, L, moms):
    Vs = X[0] * X[1] * X[2]
    z, y, x = np.meshgrid(np.arange(X[2]), np.arange(X[1]), np.arange(X[0]), indexing="ij")
    ph = np.stack([np.exp(-2j * np.pi * (n[0] * (x + gx[0]) / L[0] + n[1] * (y + gx[1]) / L[1] + n[2] * (z + gx[2]) / L[2])).reshape(Vs) for n in moms])
    c = cs.reshape(cs.shape[0], -1, Vs, 16)
    return np.einsum("ms,ktse->ktme", ph, c)


@pytest.mark.parametrize("cid", ["A0-b1.Lt2.t1.n1-m36", "D1-b1.Lt2.t1.n1-m9"])
def test_project_matches_a_naive_dft(cid):
    """the two small shapes, one of them with an origin off the lattice and L != X.  The naive phase argument is not reduced, so its
    rounding grows with it: below 2 pi x 300 for the components below 100 (2^-53 of that per direction and term: 1e-12 of sum |cs|
    covers it), up to 2 pi x 4 10^4 for the component near 10^4 (1e-10)"""
    c = R.case(cid)
    small = np.all(np.abs(c.moms) < 100, axis=1)
    want = _naive(c.cs, c.X, c.gx, c.L, c.moms)
    got = np.asarray(R.project(c.cs, c.X, c.gx, c.L, c.moms), dtype=np.complex128)
    err = np.abs(got - want) / c.sum_abs
    assert small.sum() >= 7 and not small.all()
    assert np.max(err[:, :, small]) < 1e-12 and np.max(err) < 1e-10


@pytest.mark.parametrize("cid", R.CASES)
def test_emulation_stays_inside_the_bound(cid):
    c = R.case(cid)
    got = R.emulate(c.acc, c.cs, c.t0, c.X, c.gx, c.L, c.moms)
    print("%s: K = %d, largest error %.2f x 2^-53 sum|cs|, %.4f of the bound" % (cid, R.K(c.Vs), c.units(got), c.excess(got)))
    assert c.excess(got) <= 1.0
    assert c.untouched_equal(got)
    for i, j in R.alias_pairs(c.moms, c.L):
        assert np.array_equal(got[:, :, i], got[:, :, j]), (i, j)


def test_the_momentum_lists_hold_what_the_cases_need():
    for shape in "ABDE":
        L = R.SHAPES[shape][2] or R.SHAPES[shape][0]
        for count in (8, 9, 36, 37):
            m = R.momenta(count, L)
            assert m.shape == (count, 3) and len({tuple(v) for v in m}) == count
            assert any(not v.any() for v in m) and any(np.abs(v).sum() == 1 for v in m)
            assert any(v.min() < 0 < v.max() for v in m)
            assert any(np.any(np.abs(v) > np.array(L) / 2) for v in m)
            assert R.alias_pairs(m, L)
            assert np.sum((np.abs(m) > 5000) & (np.abs(m) < 20000)) >= 1
    assert R.momenta(1, (12, 10, 14)).shape == (1, 3)
    assert len(R.CASES) <= 16


# the mutants of emulate(), each with the cases of the table that must catch it
MUTANT_CASES = {
    "lane_stride_8": ["B0-b3.Lt5.t2.n3-m9", "C0-b1.Lt2.t1.n1-m36"],
    "share_end_minus_1": ["B0-b3.Lt5.t2.n3-m9", "A0-b1.Lt2.t1.n1-m36"],
    "yz_swapped": ["B0-b3.Lt5.t2.n3-m9", "A0-b1.Lt2.t1.n1-m36"],
    "gx_ignored": ["A0-b1.Lt2.t1.n1-m36", "D0-b1.Lt2.t1.n1-m36", "D1-b1.Lt2.t1.n1-m9"],
    "phase_sign": ["B0-b1.Lt1.t0.n1-m1", "A0-b1.Lt2.t1.n1-m36"],
    "L_taken_as_X": ["D0-b1.Lt2.t1.n1-m36", "D1-b1.Lt2.t1.n1-m9"],
    "acc_overwritten": ["B0-b1.Lt1.t0.n1-m1", "A0-b1.Lt2.t1.n1-m36"],
    "slice_tl": ["B0-b3.Lt5.t2.n3-m9", "A0-b1.Lt2.t1.n1-m36"],
}


def test_eight_mutants_are_listed():
    assert set(MUTANT_CASES) == set(R.MUTANTS) and len(R.MUTANTS) == 8
    assert all(cid in R.CASES for cids in MUTANT_CASES.values() for cid in cids)


@pytest.mark.parametrize("mutant", R.MUTANTS)
def test_mutant_leaves_the_bound(mutant):
    """what the GPU test asserts (the bound on the touched slices, the other slices bit-identical) fails for the mutant on EVERY case
    listed for it, by a wide margin: the smallest honest effect is 1e-8 of sum |cs|, the bound 2e-14 of it"""
    for cid in MUTANT_CASES[mutant]:
        c = R.case(cid)
        got = R.emulate(c.acc, c.cs, c.t0, c.X, c.gx, c.L, c.moms, mutant=mutant)
        caught = c.excess(got) > 1.0 or not c.untouched_equal(got)
        print("%s on %s: %.3e of the bound, other slices %s" % (mutant, cid, c.excess(got), "kept" if c.untouched_equal(got) else "changed"))
        assert caught, (mutant, cid)
        assert c.excess(got) > 100.0, (mutant, cid, c.excess(got))
