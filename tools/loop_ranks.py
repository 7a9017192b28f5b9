#!/usr/bin/env python3
"""One rank of the loop-contraction check on a decomposed lattice (started by tools/loop_ranks.sh, env RANK / LOCAL_RANK /
WORLD_SIZE).  Reads the global inputs of tests/test_loop_ranks_gpu.py (links, one solution vector), cuts out this rank's
sub-lattice for the grids 1x1x1x2 (time) and 1x1x2x1 (space), runs qudaAmdContractLoop and saves what this rank received.

    python tools/loop_ranks.py inputs.npz outdir"""
import faulthandler
import importlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import multi_gpu as mg  # noqa: E402

GRIDS = ([1, 1, 1, 2], [1, 1, 2, 1])


def local_lex(a, X, Xl, coords, per_site):
    """(..., V*per_site) global lexicographic host field -> this rank's local lexicographic block"""
    lead = a.shape[:-1]
    g = a.reshape(lead + (X[3], X[2], X[1], X[0], per_site))
    o = [coords[d] * Xl[d] for d in range(4)]
    b = g[..., o[3]:o[3] + Xl[3], o[2]:o[2] + Xl[2], o[1]:o[1] + Xl[1], o[0]:o[0] + Xl[0], :]
    return np.ascontiguousarray(b).reshape(lead + (-1,))


def main():
    faulthandler.enable()
    inp, outdir = sys.argv[1], sys.argv[2]
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    qa = importlib.import_module("quda-qkxtm-multigrid_amd")
    d = np.load(inp)
    X = [int(v) for v in d["X"]]
    for k, grid in enumerate(GRIDS):
        dist = mg.setup(qa, rank, world, int(os.environ["LOCAL_RANK"]), X, grid=grid)
        Xl = dist.local_dims
        qa.load_gauge(mg.scatter_gauge(d["gauge"], X, grid, dist.coords), qa.gauge_param(Xl, t_boundary=int(d["t_boundary"])))
        x = local_lex(d["x"], X, Xl, dist.coords, 24)
        ip = qa.invert_param(qa.QUDA_TWISTED_MASS_DSLASH, float(d["kappa"]), 0.05, +1, "ee", 0, cuda_prec=8, solution_type=qa.QUDA_MAT_SOLUTION,
                             gamma_basis=qa.QUDA_UKQCD_GAMMA_BASIS)
        out = qa.contract_loop(x, ip, int(d["qsq"]), X[:3])
        np.savez(os.path.join(outdir, "rank%d_grid%d.npz" % (rank, k)), loops=out)
        print("rank %d grid %s: contracted, |loops| %.6e" % (rank, grid, np.max(np.abs(out))), flush=True)
        dist.finalize()


if __name__ == "__main__":
    main()
