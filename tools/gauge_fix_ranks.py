#!/usr/bin/env python3
"""One rank of the gauge-fixing check on a lattice split in t over two processes (started by tools/gauge_fix_ranks.sh, env RANK /
LOCAL_RANK / WORLD_SIZE).  Reads the global inputs of tests/test_gauge_fix_gpu.py, cuts out this rank's sub-lattice, runs
qudaAmdGaugeFixOVR with the transformation and saves this rank's links, G and figures.

    python tools/gauge_fix_ranks.py inputs.npz outdir"""
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
    gp = qa.gauge_param(dist.local_dims, t_boundary=int(d["t_boundary"]))
    gauge = mg.scatter_gauge(d["gauge"], X, GRID, dist.coords)
    links, G, info = qa.gauge_fix_ovr(gp, int(d["gauge_dir"]), int(d["n_steps"]), float(d["omega"]), float(d["tolerance"]), int(d["reunit_interval"]),
                                      int(d["stop_theta"]), gauge=gauge, make_resident_gauge=True, transform=True)
    quality = qa.gauge_fix_quality(int(d["gauge_dir"]))   # of the fixed links, now resident
    np.savez(os.path.join(outdir, "rank%d.npz" % rank), links=links, G=G, info=np.array([info["iterations"], info["F"], info["theta"], info["delta"]]),
             quality=np.array(quality), coords=np.array(dist.coords))
    print("rank %d: %d iterations, F %.15e, theta %.6e" % (rank, info["iterations"], info["F"], info["theta"]), flush=True)
    dist.finalize()


if __name__ == "__main__":
    main()
