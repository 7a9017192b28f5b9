"""Loop contractions on a lattice split over two processes (tools/loop_ranks.sh: two ranks on one GPU, each under its own time
limit): time split 1x1x1x2 and space split 1x1x2x1.  The neighbours of x and phi across the cut come through the full-spinor ghost
exchange, every rank sums its spatial sub-volume with the global coordinates in the phases, places its time slices at their global
position and receives the full result; both ranks must return the one-rank result to 1e-12 relative to the largest entry of each
of the 18 blocks."""
import importlib
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def qa():
    mod = importlib.import_module("quda-qkxtm-multigrid_amd")
    mod.init(0)
    yield mod
    mod.end()


@pytest.mark.parametrize("antiperiodic", [True, False])
def test_two_ranks_return_the_one_rank_result(qa, oracle, tmp_path, antiperiodic):
    X = (4, 4, 4, 8)
    kappa, qsq = 0.13, 3
    gauge, _, _ = oracle.make_fields(list(X), seed=9, antiperiodic_t=antiperiodic, clover=False)
    V = int(np.prod(X))
    x = np.random.default_rng(29).standard_normal(V * 24)
    tb = qa.QUDA_ANTI_PERIODIC_T if antiperiodic else qa.QUDA_PERIODIC_T
    qa.load_gauge(gauge, qa.gauge_param(X, t_boundary=tb))
    ip = qa.invert_param(qa.QUDA_TWISTED_MASS_DSLASH, kappa, 0.05, +1, "ee", 0, cuda_prec=8, solution_type=qa.QUDA_MAT_SOLUTION,
                         gamma_basis=qa.QUDA_UKQCD_GAMMA_BASIS)
    one = qa.contract_loop(x, ip, qsq, X[:3])
    inp = tmp_path / "inputs.npz"
    np.savez(str(inp), X=np.array(X), gauge=gauge, x=x, kappa=kappa, qsq=qsq, t_boundary=tb)
    r = subprocess.run(["bash", os.path.join(ROOT, "tools", "loop_ranks.sh"), str(inp), str(tmp_path)], capture_output=True, text=True, timeout=300)
    logs = "".join(open(str(tmp_path / ("rank%d.log" % k))).read()[-1500:] for k in range(2) if (tmp_path / ("rank%d.log" % k)).exists())
    assert r.returncode == 0, r.stdout + r.stderr + logs
    for k in range(2):
        for rank in range(2):
            got = np.load(str(tmp_path / ("rank%d_grid%d.npz" % (rank, k))))["loops"]
            assert got.shape == one.shape
            err = max(np.max(np.abs(got[b] - one[b])) / np.max(np.abs(one[b])) for b in range(18))
            print("grid %d rank %d: worst block error %.3e" % (k, rank, err))
            assert err < 1e-12, (k, rank, err)
