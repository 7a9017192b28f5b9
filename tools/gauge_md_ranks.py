#!/usr/bin/env python3
"""One rank of the gauge molecular-dynamics check on a lattice split in t over two processes (started by tools/gauge_md_ranks.sh,
env RANK / LOCAL_RANK / WORLD_SIZE).  Reads the global inputs of tests/test_gauge_md_gpu.py (links, momenta, path table), cuts out
this rank's sub-lattice, runs computeGaugeForceQuda, updateGaugeFieldQuda and momActionQuda and saves this rank's results.

    python tools/gauge_md_ranks.py inputs.npz outdir"""
import faulthandler
import importlib
import json
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
    paths, coeff = json.loads(str(d["paths"])), [float(c) for c in d["coeff"]]
    dist = mg.setup(qa, rank, world, int(os.environ["LOCAL_RANK"]), X, grid=GRID)
    Xl = dist.local_dims
    gp = qa.gauge_param(Xl, t_boundary=int(d["t_boundary"]))
    gauge = mg.scatter_gauge(d["gauge"], X, GRID, dist.coords)
    mom = mg.scatter_field(d["mom"].reshape(-1), X, GRID, dist.coords, 40).reshape(-1, 4, 10)
    qa.load_gauge(gauge, gp)
    force = qa.gauge_force(gp, paths, coeff, float(d["eb3"]), mom=mom, make_resident_mom=True)
    action = qa.mom_action(gp)                       # of the resident momentum, summed over the ranks
    links = qa.update_gauge(gp, float(d["dt"]), make_resident_gauge=True)
    plaq = qa.plaquette()                            # of the new resident links
    np.savez(os.path.join(outdir, "rank%d.npz" % rank), force=force, action=action, links=links, plaq=np.array(plaq), coords=np.array(dist.coords))
    print("rank %d: force, action %.12e, update done" % (rank, action), flush=True)
    dist.finalize()


if __name__ == "__main__":
    main()
