"""The momentum projection that all contractions share (momentumProject, csrc/momproj.hip) through its test hook
qudaAmdMomentumProject, element by element against the longdouble reference and the derived bound of tests/momproj_ref.py, at the
smallest shapes where a share of a slice holds more sites than it has site lanes (so the lane loop makes further trips), with t0 > 0
and nt > 1 together, with an origin off the lattice and global extents that differ from the local ones, and on both sides of the
branch between the one-pass kernel (9 to 36 momenta, phase tables up to 64 KiB of LDS) and chunks of 8 momenta.

Every case asserts: each element of the touched slices within the bound of the reference; each element of the other slices
bit-identical to what went in; a second identical call returns the same bits; aliased momenta (n and n +- L) return the same bits."""
import importlib
import os
import subprocess
import sys

import numpy as np
import pytest

import momproj_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IN_PROCESS = [c for c in R.CASES if c[0] not in "EF"]
CHILD_CASES = [c for c in R.CASES if c[0] in "EF"]


@pytest.fixture(scope="module")
def qa():
    mod = importlib.import_module("quda-qkxtm-multigrid_amd")
    mod.init(0)
    yield mod
    mod.end()


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.complex128), np.ascontiguousarray(b, dtype=np.complex128)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def _check(c, got, again):
    print("%s: K = %d, largest error %.2f x 2^-53 sum|cs|, %.4f of the bound" % (c.id, R.K(c.Vs), c.units(got), c.excess(got)))
    assert got.shape == c.acc.shape
    assert c.excess(got) <= 1.0, c.excess(got)
    assert c.untouched_equal(got)
    assert _same_bits(got, again)
    pairs = R.alias_pairs(c.moms, c.L)
    assert pairs or len(c.moms) == 1
    for i, j in pairs:
        assert _same_bits(got[:, :, i], got[:, :, j]), (i, j, c.moms[i], c.moms[j])


@pytest.mark.parametrize("cid", IN_PROCESS)
def test_projection_within_the_bound(qa, cid):
    c = R.case(cid)
    got = qa.momentum_project(c.acc, c.cs, c.t0, c.moms, c.X, c.gx, c.L)
    again = qa.momentum_project(c.acc, c.cs, c.t0, c.moms, c.X, c.gx, c.L)
    _check(c, got, again)


_CHILD = """
import importlib, sys
import numpy as np
sys.path.insert(0, %r)
qa = importlib.import_module("quda-qkxtm-multigrid_amd")
d = np.load(sys.argv[1])
qa.init(0)
out = [qa.momentum_project(d["acc"], d["cs"], int(d["t0"]), d["moms"], d["X"], d["gx"], d["L"]) for call in range(2)]
np.save(sys.argv[2], np.stack(out))
qa.end()
"""


@pytest.mark.parametrize("cid", CHILD_CASES)
def test_largest_phase_tables_within_the_bound(cid, tmp_path):
    """X0 + Y + Z = 106: the 65 152 bytes of LDS at the edge of the one-pass branch; 108: the fall-back of 9 to 36 momenta to chunks of
    8.  In a child process of their own: a launch that the device refuses fails this test with the library's message"""
    c = R.case(cid)
    inp, out, script = tmp_path / "in.npz", tmp_path / "out.npy", tmp_path / "child.py"
    np.savez(str(inp), acc=c.acc, cs=c.cs, t0=c.t0, moms=c.moms, X=np.array(c.X), gx=np.array(c.gx), L=np.array(c.L))
    script.write_text(_CHILD % ROOT)
    r = subprocess.run([sys.executable, str(script), str(inp), str(out)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    got, again = np.load(str(out))
    _check(c, got, again)


@pytest.mark.parametrize("shape", ["B", "C"])
def test_every_site_is_counted_once(qa, shape):
    """zero momentum (as 0 and as whole multiples of L) and whole-number blocks: site s holds (s + 1) 2^e + i (Vs - s) 2^(15 - e) in entry
    e, plus Vs per slice and block, so every phase is exactly 1 and every partial sum a whole number below 2^53: the result equals the
    closed form, and a site counted twice or not at all shows as a whole number"""
    X = R.SHAPES[shape][0]
    Vs = X[0] * X[1] * X[2]
    nblk, Lt, t0, nt = 2, 3, 1, 2
    moms = np.array([(0, 0, 0), (X[0], -X[1], 2 * X[2]), (0, 3 * X[1], 0)], dtype=np.int32)
    s = np.arange(Vs, dtype=np.float64)[None, None, :, None]
    e = np.arange(16)[None, None, None, :]
    off = (Vs * (np.arange(nt)[None, :, None, None] + nt * np.arange(nblk)[:, None, None, None])).astype(np.float64)
    cs = (s + 1 + off) * 2.0 ** e + 1j * (Vs - s + off) * 2.0 ** (15 - e)
    acc = np.zeros((nblk, Lt, 3, 16), dtype=np.complex128)
    acc += (np.arange(nblk * Lt * 3 * 16).reshape(acc.shape) % 1001) - 500.0j
    tri = Vs * (Vs + 1) // 2
    want = acc.copy()
    for k in range(nblk):
        for tl in range(nt):
            o = Vs * (tl + nt * k)
            want[k, t0 + tl] += ((tri + Vs * o) * 2.0 ** np.arange(16) + 1j * (tri + Vs * o) * 2.0 ** (15 - np.arange(16)))[None, :]
    assert np.max(np.abs(want)) < 2.0 ** 52
    got = qa.momentum_project(acc, cs.reshape(nblk, nt * Vs, 16), t0, moms, X)
    assert np.array_equal(got, want), np.max(np.abs(got - want))


def test_slices_and_blocks_do_not_depend_on_the_launch(qa):
    """36 momenta on 12 x 10 x 14: three slices in one call equal three calls of one slice, three blocks in one call equal each alone"""
    c = R.case("B0-b3.Lt5.t2.n3-m36")
    one = qa.momentum_project(c.acc, c.cs, c.t0, c.moms, c.X, c.gx, c.L)
    by_slice = c.acc
    for tl in range(c.nt):
        by_slice = qa.momentum_project(by_slice, c.cs[:, tl * c.Vs:(tl + 1) * c.Vs], c.t0 + tl, c.moms, c.X, c.gx, c.L)
    assert _same_bits(by_slice, one)
    for k in range(c.nblk):
        alone = qa.momentum_project(c.acc[k:k + 1], c.cs[k:k + 1], c.t0, c.moms, c.X, c.gx, c.L)
        assert _same_bits(alone[0], one[k]), k


def test_a_momentum_gives_the_same_bits_wherever_it_stands(qa):
    """lists of 37 (five chunks of 8, every chunk position), 36 (the one-pass kernel, rotated by 5 places) and 8 entries (windows of
    the long list, so that a momentum stands at another chunk position): both instantiations of project_kernel, same bits"""
    c = R.case("B0-b3.Lt5.t2.n3-m36")
    moms = R.momenta(37, c.L)
    acc = np.random.default_rng(3).standard_normal((c.nblk, c.Lt, 37, 16, 2)) @ np.array([1, 1j])

    def run(idx):
        return qa.momentum_project(acc[:, :, idx], c.cs, c.t0, moms[idx], c.X, c.gx, c.L)

    full = run(np.arange(37))
    rot = np.roll(np.arange(36), 5)
    assert _same_bits(run(rot), full[:, :, rot])
    for first in (0, 3, 13, 29):
        idx = np.arange(first, first + 8)
        assert _same_bits(run(idx), full[:, :, idx]), first
