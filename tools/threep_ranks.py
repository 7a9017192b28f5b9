#!/usr/bin/env python3
"""One rank of the three-point check on a decomposed lattice (started by tools/threep_ranks.sh, env RANK / LOCAL_RANK /
WORLD_SIZE).  Reads the global inputs of tests/test_threep_ranks_gpu.py (links, two propagators, sequential and forward columns),
cuts out this rank's sub-lattice for the grids 1x1x1x2 (time) and 1x1x2x1 (space), runs qudaAmdThreepSeqSource and
qudaAmdContractThreep (resident links and given links) for every (source, tsink) case and saves what this rank received.

    python tools/threep_ranks.py inputs.npz outdir"""
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
    qsq, nsmear, alpha = int(d["qsq"]), int(d["nsmear"]), float(d["alpha"])
    particle, part, pid = int(d["particle"]), int(d["part"]), int(d["projector"])
    for k, grid in enumerate(GRIDS):
        dist = mg.setup(qa, rank, world, int(os.environ["LOCAL_RANK"]), X, grid=grid)
        Xl = dist.local_dims
        qa.load_gauge(mg.scatter_gauge(d["gauge"], X, grid, dist.coords), qa.gauge_param(Xl, t_boundary=int(d["t_boundary"])))
        g_lex = local_lex(d["gauge_lex"], X, Xl, dist.coords, 18)
        up, dn = local_lex(d["up"], X, Xl, dist.coords, 24), local_lex(d["dn"], X, Xl, dist.coords, 24)
        seq, fwd = local_lex(d["seq"], X, Xl, dist.coords, 24), local_lex(d["fwd"], X, Xl, dist.coords, 24)
        out = dict(coords=np.array(dist.coords), local_dims=np.array(Xl))
        for c, case in enumerate(d["cases"]):
            src, tsink = [int(v) for v in case[:4]], int(case[4])
            out["source%d" % c] = qa.threep_seq_source(up, dn, g_lex, src, tsink, pid, particle, part, nsmear, alpha)
            for tag, links in (("resident", None), ("given", g_lex)):
                loc, noe, one = qa.contract_threep(seq, fwd, links, src, qsq, tsink, particle, part)
                out["local%d_%s" % (c, tag)], out["noether%d_%s" % (c, tag)], out["oneD%d_%s" % (c, tag)] = loc, noe, one
            print("rank %d grid %s case %d: |source| %.6e |local| %.6e" % (rank, grid, c, np.max(np.abs(out["source%d" % c])), np.max(np.abs(loc))), flush=True)
        np.savez(os.path.join(outdir, "rank%d_grid%d.npz" % (rank, k)), **out)
        dist.finalize()


if __name__ == "__main__":
    main()
