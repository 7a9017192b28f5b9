"""Timing of gauge fixing by overrelaxation at 16^4 and 32^4 (fp64 links, one rank).

    python tools/gauge_fix_timing.py [--lattice 16,16,16,16 --lattice 32,32,32,32] [--steps 20] [--repeat 5] [--out profiles/gauge_fix_timing.json]

The figure is the compute time qudaAmdGaugeFixOVR reports: a host clock from the stream synchronisation after the links are extracted
to the one after the last projection, so copies to and from the host are outside it.  Links resident, tolerance 0, nothing returned.
Two runs of N = --steps iterations separate an iteration from a projection:
    A  reunit_interval = N:  N iterations + 1 projection        B  reunit_interval = 1:  N iterations + N projections
    projection = (B - A) / (N - 1),   iteration = (A - projection) / N
An iteration is two sweeps and one quality pass (the pass before the first iteration is spread over the N: 1/N of a pass too much).
Medians of --repeat runs after one warm-up run of every shape.  Landau (4 directions) and Coulomb (3), the direct sweep and the
transport formulation (QUDA_AMD_GAUGE_FIX_TRANSPORT=1).

Algorithmic bytes at the 192 bytes a matrix-field entry occupies: an iteration reads and writes every one of the 4 V links in each
of its two sweeps, 4 V x 192 x 2 x 2, and the quality pass reads the D V links that enter it once; a projection reads and writes
4 V links.  `of_8TBs` is those bytes over the time over 8 TB/s: how far the whole step, launches and reductions included, is from
streaming its data once at the HBM rate.  One JSON line.  Every call runs under its own time limit (SIGALRM ends the process: nothing
more is started on the GPU after a call that hangs)."""
import argparse
import importlib
import json
import os
import signal
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from synth import tiled_gauge  # noqa: E402

qa = importlib.import_module("quda-qkxtm-multigrid_amd")
PEAK = 8e12   # bytes per second


def _expired(signum, frame):
    sys.stderr.write("gauge_fix_timing: a call ran into its time limit; stopping\n")
    os._exit(124)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lattice", action="append", default=None)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--limit", type=int, default=120, help="seconds per call")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gauge_fix_timing.json"))
    a = ap.parse_args()
    lattices = [tuple(int(v) for v in s.split(",")) for s in (a.lattice or ["16,16,16,16", "32,32,32,32"])]
    N = a.steps
    if N < 2:
        raise SystemExit("--steps has to be at least 2")
    signal.signal(signal.SIGALRM, _expired)

    def guarded(fn):
        signal.alarm(a.limit)
        try:
            return fn()
        finally:
            signal.alarm(0)

    result = {"what": "gauge fixing by overrelaxation, fp64 links, one rank, ms (median of %d runs of %d iterations)" % (a.repeat, N), "lattices": {}}
    guarded(lambda: qa.init(0))
    try:
        for X in lattices:
            V = int(np.prod(X))
            gauge = tiled_gauge(X)
            gp = qa.gauge_param(X, t_boundary=qa.QUDA_PERIODIC_T)
            guarded(lambda: qa.load_gauge(gauge, gp))
            r = {}
            for name, gauge_dir, D in (("landau", 4, 4), ("coulomb", 3, 3)):
                for form in ("direct", "transport"):
                    os.environ["QUDA_AMD_GAUGE_FIX_TRANSPORT"] = "1" if form == "transport" else "0"

                    def compute_secs(reunit):
                        run = lambda: qa.gauge_fix_ovr(gp, gauge_dir, N, 1.5, 0.0, reunit, 1, return_gauge=False)[2]["secs"][1]
                        guarded(run)   # warm-up: code objects, buffers
                        return statistics.median(guarded(run) for _ in range(a.repeat))

                    tA, tB = compute_secs(N), compute_secs(1)
                    reunit = (tB - tA) / (N - 1)
                    iteration = (tA - reunit) / N
                    it_bytes = 4.0 * V * 192 * 2 * 2 + D * V * 192.0
                    key = "%s_%s" % (name, form)
                    r[key + "_iteration_ms"] = round(1e3 * iteration, 4)
                    r[key + "_iteration_of_8TBs"] = round(it_bytes / iteration / PEAK, 4)
                    r[key + "_reunit_ms"] = round(1e3 * reunit, 4)
                    r[key + "_reunit_of_8TBs"] = round(4.0 * V * 192 * 2 / reunit / PEAK, 4)
            os.environ["QUDA_AMD_GAUGE_FIX_TRANSPORT"] = "0"
            result["lattices"]["x".join(map(str, X))] = r
            print(json.dumps({"x".join(map(str, X)): r}), flush=True)
    finally:
        qa.end()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(json.dumps(result) + "\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
