"""Timing of the thick-restart Lanczos eigensolver (qudaAmdNewDeflation) per phase: filter, dots, updates, basis rotations.

    python tools/eig_timing.py [--lattice 16,16,16,32] [--lattice 32,32,32,32] [--nev 50] [--nkv 100] [--degree 20] [--out profiles/eig_timing.txt]

For every lattice the eigensolver runs twice in this one process with maxRestarts = 1 (two cycles: nKv steps, one compression to
nEv + (nKv - nEv) / 2 vectors, the remaining steps, the final rotation to nEv vectors), so both runs do the same work whatever the
spectrum: once on the panel kernels of csrc/eig.hip, once with QUDA_AMD_EIG_PANEL=0 on blas::multiDot / multiCaxpy in chunks of 20
fields and the rotation as k multiCaxpy sweeps.  Hot links (kernel times do not depend on the values); the times are device events
summed inside the library.  Each step runs under its own time limit (SIGALRM ends the process: nothing more is started on the GPU
after a step that hangs)."""
import argparse
import importlib
import os
import signal
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
qa = importlib.import_module("quda-qkxtm-multigrid_amd")
from synth import tiled_gauge  # noqa: E402


def _expired(signum, frame):
    sys.stderr.write("eig_timing: a step ran into its time limit; stopping\n")
    os._exit(124)


def step(limit, fn):
    signal.alarm(limit)
    try:
        return fn()
    finally:
        signal.alarm(0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lattice", action="append", default=None)
    ap.add_argument("--nev", type=int, default=50)
    ap.add_argument("--nkv", type=int, default=100)
    ap.add_argument("--degree", type=int, default=20)
    ap.add_argument("--limit", type=int, default=240, help="seconds per step")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "eig_timing.txt"))
    a = ap.parse_args()
    lattices = [tuple(int(v) for v in s.split(",")) for s in (a.lattice or ["16,16,16,32", "32,32,32,32"])]
    signal.signal(signal.SIGALRM, _expired)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    step(a.limit, lambda: qa.init(0))
    try:
        for X in lattices:
            name = "x".join(map(str, X))
            gauge = tiled_gauge(X)
            step(a.limit, lambda: qa.load_gauge(gauge, qa.gauge_param(X, t_boundary=qa.QUDA_PERIODIC_T)))
            ip = qa.invert_param(qa.QUDA_TWISTED_MASS_DSLASH, 0.124, 0.005, +1, "ee", 0, cuda_prec=8, solution_type=qa.QUDA_MAT_SOLUTION)
            res = {}
            for panel in (1, 0):
                os.environ["QUDA_AMD_EIG_PANEL"] = str(panel)
                d = step(a.limit, lambda: qa.Deflation(ip, a.nev, a.nkv, a.degree, 0.4, 3.2, 1e-10, isACC=True, maxRestarts=1))
                res[panel] = dict(d.timings)
                mv = d.matvecs
                d.close()
                t = res[panel]
                say("eig %s nEv=%d nKv=%d degree=%d %s: filter %.4f s (%d applications of A), dots %.4f s, updates %.4f s, rotations %.4f s"
                    % (name, a.nev, a.nkv, a.degree, "panel kernels  " if panel else "blas chunks 20 ", t["filter"], mv, t["dots"], t["updates"], t["rotations"]))
            say("eig %s: blas / panel  dots %.2f, updates %.2f, rotations %.2f" % (name, res[0]["dots"] / res[1]["dots"], res[0]["updates"] / res[1]["updates"],
                                                                             res[0]["rotations"] / res[1]["rotations"]))
        os.environ.pop("QUDA_AMD_EIG_PANEL", None)
    finally:
        qa.end()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
