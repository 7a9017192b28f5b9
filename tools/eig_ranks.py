#!/usr/bin/env python3
"""One rank of the eigensolver check on a lattice split in time (started by tools/eig_ranks.sh, env RANK / LOCAL_RANK / WORLD_SIZE).
Reads the global inputs of tests/test_eig_ranks_gpu.py (links and the eigensolver's parameters), cuts out this rank's sub-lattice for
the grid 1x1x1x2, runs qudaAmdNewDeflation and qudaAmdDeflationExactLoop and saves what this rank received.

    python tools/eig_ranks.py inputs.npz outdir"""
import faulthandler
import importlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import multi_gpu as mg  # noqa: E402

GRID = [1, 1, 1, 2]


def main():
    faulthandler.enable()
    inp, outdir = sys.argv[1], sys.argv[2]
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    qa = importlib.import_module("quda-qkxtm-multigrid_amd")
    d = np.load(inp)
    X = [int(v) for v in d["X"]]
    dist = mg.setup(qa, rank, world, int(os.environ["LOCAL_RANK"]), X, grid=GRID)
    qa.load_gauge(mg.scatter_gauge(d["gauge"], X, GRID, dist.coords), qa.gauge_param(dist.local_dims, t_boundary=int(d["t_boundary"])))
    ip = qa.invert_param(qa.QUDA_TWISTED_MASS_DSLASH, float(d["kappa"]), float(d["mu"]), +1, "ee", 0, cuda_prec=8, solution_type=qa.QUDA_MAT_SOLUTION)
    defl = qa.Deflation(ip, int(d["nEv"]), int(d["nKv"]), int(d["PolyDeg"]), float(d["amin"]), float(d["amax"]), float(d["tol"]))
    loops = defl.exact_loop(int(d["nEv"]), int(d["qsq"]), X[:3])
    np.savez(os.path.join(outdir, "rank%d.npz" % rank), evals=defl.evals, residuals=defl.residuals, restarts=defl.restarts, loops=loops)
    print("rank %d: %d restarts, lambda %.12e .. %.12e, largest residual %.3e" % (rank, defl.restarts, defl.evals[0], defl.evals[-1], defl.residuals.max()), flush=True)
    defl.close()
    dist.finalize()


if __name__ == "__main__":
    main()
