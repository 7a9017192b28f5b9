"""Three-point sequential sources and contractions on a lattice split over two processes (tools/threep_ranks.sh: two ranks on one
GPU, each under its own time limit): time split 1x1x1x2 and space split 1x1x2x1 on 4 x 4 x 4 x 8, both time boundaries.  Two
(source, tsink) cases: the sink slice wraps and lies on the first time rank, and it does not wrap and lies on the second, so each
rank of the time split once builds the source and once contributes zeros.  The neighbours of q and F across the cut come through
the full-spinor ghost exchange between the processes, the phases carry the global coordinates, the time slices go to their
global position and every rank receives the full result.  Every rank must return its block of the one-rank sequential source and
the one-rank local / noether[mu] / oneD[mu] to 1e-12 relative to the largest entry of each block, with the resident links (the
boundary sign on the first and last time rank) and with the links given by the caller."""
import importlib
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from test_twop_gpu import _lex_gauge  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = [(1, 2, 3, 6, 3), (3, 0, 1, 2, 3)]   # source x, y, z, t0 and tsink: global sink slices 1 (wraps) and 5


@pytest.fixture(scope="module")
def qa():
    mod = importlib.import_module("quda-qkxtm-multigrid_amd")
    mod.init(0)
    yield mod
    mod.end()


def _local(a, X, Xl, coords, per_site):
    g = a.reshape(a.shape[:-1] + (X[3], X[2], X[1], X[0], per_site))
    o = [coords[d] * Xl[d] for d in range(4)]
    b = g[..., o[3]:o[3] + Xl[3], o[2]:o[2] + Xl[2], o[1]:o[1] + Xl[1], o[0]:o[0] + Xl[0], :]
    return np.ascontiguousarray(b).reshape(a.shape[:-1] + (-1,))


def _block_err(got, want):
    errs = [np.max(np.abs(got[0] - want[0])) / np.max(np.abs(want[0]))]
    for mu in range(4):
        errs.append(np.max(np.abs(got[1][..., mu] - want[1][..., mu])) / np.max(np.abs(want[1][..., mu])))
        errs.append(np.max(np.abs(got[2][:, :, mu] - want[2][:, :, mu])) / np.max(np.abs(want[2][:, :, mu])))
    return max(errs)


@pytest.mark.parametrize("antiperiodic", [True, False])
def test_two_ranks_return_the_one_rank_result(qa, oracle, tmp_path, antiperiodic):
    X = (4, 4, 4, 8)
    qsq, nsmear, alpha = 3, 2, 0.7
    particle, part, pid = (qa.PROTON, 1, qa.G5G123) if antiperiodic else (qa.NEUTRON, 2, qa.G4)
    gauge, _, _ = oracle.make_fields(list(X), seed=9, antiperiodic_t=antiperiodic, clover=False)
    tb = qa.QUDA_ANTI_PERIODIC_T if antiperiodic else qa.QUDA_PERIODIC_T
    qa.load_gauge(gauge, qa.gauge_param(X, t_boundary=tb))
    g_lex = _lex_gauge(oracle, gauge, X)
    V = int(np.prod(X))
    rng = np.random.default_rng(31)
    up, dn, seq, fwd = (rng.standard_normal((12, V * 24)) for _ in range(4))
    one = []
    for c in CASES:
        src, tsink = c[:4], c[4]
        source = qa.threep_seq_source(up, dn, g_lex, src, tsink, pid, particle, part, nsmear, alpha)
        assert np.max(np.abs(source)) > 0
        one.append((source, qa.contract_threep(seq, fwd, None, src, qsq, tsink, particle, part), qa.contract_threep(seq, fwd, g_lex, src, qsq, tsink, particle, part)))
    inp = tmp_path / "inputs.npz"
    np.savez(str(inp), X=np.array(X), gauge=gauge, gauge_lex=g_lex, up=up, dn=dn, seq=seq, fwd=fwd, t_boundary=tb, qsq=qsq, nsmear=nsmear, alpha=alpha,
             particle=particle, part=part, projector=pid, cases=np.array(CASES))
    r = subprocess.run(["bash", os.path.join(ROOT, "tools", "threep_ranks.sh"), str(inp), str(tmp_path)], capture_output=True, text=True, timeout=300)
    logs = "".join(open(str(tmp_path / ("rank%d.log" % k))).read()[-1500:] for k in range(2) if (tmp_path / ("rank%d.log" % k)).exists())
    assert r.returncode == 0, r.stdout + r.stderr + logs
    worst = 0.0
    for k in range(2):
        for rank in range(2):
            got = np.load(str(tmp_path / ("rank%d_grid%d.npz" % (rank, k))))
            coords, Xl = [int(v) for v in got["coords"]], [int(v) for v in got["local_dims"]]
            for c in range(len(CASES)):
                source, resident, given = one[c]
                want = _local(source, X, Xl, coords, 24)
                assert got["source%d" % c].shape == want.shape
                errs = [np.max(np.abs(got["source%d" % c] - want)) / np.max(np.abs(source))]
                for tag, ref in (("resident", resident), ("given", given)):
                    mine = (got["local%d_%s" % (c, tag)], got["noether%d_%s" % (c, tag)], got["oneD%d_%s" % (c, tag)])
                    assert all(m.shape == w.shape for m, w in zip(mine, ref))
                    errs.append(_block_err(mine, ref))
                print("grid %d rank %d case %d: source %.3e, contraction resident links %.3e, given links %.3e" % ((k, rank, c) + tuple(errs)))
                worst = max(worst, max(errs))
    assert worst < 1e-12, worst
