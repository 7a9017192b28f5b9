"""The eigensolver and the exact part of the loops on a lattice split over two processes (tools/eig_ranks.sh: two ranks on one GPU,
each under its own time limit): 4 x 4 x 4 x 8 split in t, smooth_gauge(X, 0.35), kappa 0.124, mu 0.005, nEv = 8, nKv = 32, Chebyshev
degree 20 on [0.2, 4.0], tol 1e-10.  The start vector is keyed by the global site index, so both runs start from the same vector; the
sums over the lattice are added in another order.  (Dense spectrum of the oracle's operator on this lattice: twelve values
0.01989 .. 0.02210, then 0.0526; the eighth and the ninth are 0.02142 and 0.02162.)

The eigenvalues of the two runs agree within r_i(one) + r_i(two) + 1e-13 (residual theorem, both against the same exact value); the
exact part of the loops of the eight vectors agrees to 1e-9 of each block's maximum: the vectors differ by rounding-level rotations
inside near-degenerate pairs, so this is not bit-identical."""
import importlib
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from synth import smooth_gauge  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
X = (4, 4, 4, 8)
P = dict(kappa=0.124, mu=0.005, nEv=8, nKv=32, PolyDeg=20, amin=0.2, amax=4.0, tol=1e-10, qsq=2)


@pytest.fixture(scope="module")
def qa():
    mod = importlib.import_module("quda-qkxtm-multigrid_amd")
    mod.init(0)
    yield mod
    mod.end()


def test_two_ranks_find_the_one_rank_pairs(qa, tmp_path):
    gauge = smooth_gauge(X, 0.35)
    tb = qa.QUDA_PERIODIC_T
    qa.load_gauge(gauge, qa.gauge_param(X, t_boundary=tb))
    ip = qa.invert_param(qa.QUDA_TWISTED_MASS_DSLASH, P["kappa"], P["mu"], +1, "ee", 0, cuda_prec=8, solution_type=qa.QUDA_MAT_SOLUTION)
    defl = qa.Deflation(ip, P["nEv"], P["nKv"], P["PolyDeg"], P["amin"], P["amax"], P["tol"])
    try:
        one = defl.exact_loop(P["nEv"], P["qsq"], X[:3])
        ev1, r1 = defl.evals.copy(), defl.residuals.copy()
        print("one process: %d restarts, largest residual %.3e" % (defl.restarts, r1.max()))
    finally:
        defl.close()
    inp = tmp_path / "inputs.npz"
    np.savez(str(inp), X=np.array(X), gauge=gauge, t_boundary=tb, **P)
    r = subprocess.run(["bash", os.path.join(ROOT, "tools", "eig_ranks.sh"), str(inp), str(tmp_path)], capture_output=True, text=True, timeout=300)
    logs = "".join(open(str(tmp_path / ("rank%d.log" % k))).read()[-1500:] for k in range(2) if (tmp_path / ("rank%d.log" % k)).exists())
    assert r.returncode == 0, r.stdout + r.stderr + logs
    for rank in range(2):
        got = np.load(str(tmp_path / ("rank%d.npz" % rank)))
        dev = np.abs(got["evals"] - ev1)
        print("rank %d: %d restarts, |lambda(two) - lambda(one)| max %.3e, residuals max %.3e" % (rank, int(got["restarts"]), dev.max(), got["residuals"].max()))
        assert np.all(dev <= r1 + got["residuals"] + 1e-13)
        err = max(np.max(np.abs(got["loops"][b] - one[b])) / np.max(np.abs(one[b])) for b in range(18))
        print("rank %d: exact part of the loops, worst block deviation %.3e of the block maximum" % (rank, err))
        assert err <= 1e-9, (rank, err)
