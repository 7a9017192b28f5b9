"""Two-point contractions on a lattice split over two processes (tools/twop_ranks.sh: two ranks on one GPU, each under its own
time limit): time split 1x1x1x2 and space split 1x1x2x1.  Every rank places its time slices at their global position, sums its
spatial sub-volume with the global coordinates in the phases and receives the full result; both ranks must return the one-rank
result to 1e-12 relative to the largest entry of each (channel, flavour) block.  Sink smearing runs through the halo exchange."""
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


def _blockwise(got, want):
    g = np.moveaxis(got, (2, 3), (0, 1)).reshape(2, 10, -1)
    w = np.moveaxis(want, (2, 3), (0, 1)).reshape(2, 10, -1)
    return max(np.max(np.abs(g[f, c] - w[f, c])) / np.max(np.abs(w[f, c])) for f in range(2) for c in range(10))


def test_two_ranks_return_the_one_rank_result(qa, oracle, tmp_path):
    X = (4, 4, 4, 8)
    gauge, _, _ = oracle.make_fields(list(X), seed=5, antiperiodic_t=False, clover=False)
    g_lex = np.stack([oracle.eo_to_lex(np.ascontiguousarray(gauge[d]), list(X), 18) for d in range(4)])
    V = int(np.prod(X))
    rng = np.random.default_rng(23)
    up, dn = rng.standard_normal((12, V * 24)), rng.standard_normal((12, V * 24))
    src, qsq, nsmear, alpha = (1, 2, 3, 6), 3, 2, 0.7
    qa.load_gauge(gauge, qa.gauge_param(X, t_boundary=qa.QUDA_PERIODIC_T))
    mes1, bar1 = qa.contract_twop(up, dn, g_lex, src, qsq, nsmear, alpha)
    inp = tmp_path / "inputs.npz"
    np.savez(str(inp), X=np.array(X), gauge=gauge, gauge_lex=g_lex, up=up, dn=dn, src=np.array(src), qsq=qsq, nsmear=nsmear, alpha=alpha)
    r = subprocess.run(["bash", os.path.join(ROOT, "tools", "twop_ranks.sh"), str(inp), str(tmp_path)], capture_output=True, text=True, timeout=300)
    logs = "".join(open(str(tmp_path / ("rank%d.log" % k))).read()[-1500:] for k in range(2) if (tmp_path / ("rank%d.log" % k)).exists())
    assert r.returncode == 0, r.stdout + r.stderr + logs
    for k in range(2):
        for rank in range(2):
            d = np.load(str(tmp_path / ("rank%d_grid%d.npz" % (rank, k))))
            em, eb = _blockwise(d["mes"], mes1), _blockwise(d["bar"], bar1)
            assert em < 1e-12 and eb < 1e-12, (k, rank, em, eb)
