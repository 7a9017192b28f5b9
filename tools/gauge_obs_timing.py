"""Timing of stout smearing and of the topological charge at 32^4 (fp64 links, unpartitioned).

    python tools/gauge_obs_timing.py [--lattice 32,32,32,32] [--steps 10] [--out profiles/gauge_obs_timing.txt] [--limit 240]

Wall-clock of the C entry points, best of --repeat (both calls end with a stream synchronisation): ms per stout step from the
difference of an n-step and a 0-step call (the 0-step call is the fixed cost: link extraction, the copy back through the host
loader), spatial and all four directions, and ms per qudaAmdQCharge.  The transport formulation is the one that also runs on a
decomposed lattice: a step of it is ~20 passes over a 3x3 matrix field per staple, so these figures are the price of that
generality, not a roofline.  Every step runs under its own time limit (SIGALRM ends the process: nothing more is started on
the GPU after a step that hangs)."""
import argparse
import importlib
import os
import signal
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from synth import tiled_gauge  # noqa: E402

qa = importlib.import_module("quda-qkxtm-multigrid_amd")


def _expired(signum, frame):
    sys.stderr.write("gauge_obs_timing: a step ran into its time limit; stopping\n")
    os._exit(124)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lattice", action="append", default=None)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--limit", type=int, default=240, help="seconds per step")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gauge_obs_timing.txt"))
    a = ap.parse_args()
    lattices = [tuple(int(v) for v in s.split(",")) for s in (a.lattice or ["32,32,32,32"])]
    signal.signal(signal.SIGALRM, _expired)
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    def timed(fn):
        signal.alarm(a.limit)
        try:
            t0 = time.perf_counter()
            fn()
            return time.perf_counter() - t0
        finally:
            signal.alarm(0)

    def best(fn):
        return min(timed(fn) for _ in range(a.repeat))

    timed(lambda: qa.init(0))
    try:
        for X in lattices:
            name = "x".join(map(str, X))
            gauge = tiled_gauge(X)
            timed(lambda: qa.load_gauge(gauge, qa.gauge_param(X, t_boundary=qa.QUDA_PERIODIC_T)))
            for label, st in (("spatial", False), ("all directions", True)):
                timed(lambda: qa.stout_smear(1, 0.1, st))   # warm-up: code objects
                t0 = best(lambda: qa.stout_smear(0, 0.1, st))
                tn = best(lambda: qa.stout_smear(a.steps, 0.1, st))
                say("stout %s %s: %.2f ms per step (%d steps %.1f ms, 0 steps %.1f ms: extraction and the copy back through the loader)"
                    % (name, label, 1e3 * (tn - t0) / a.steps, a.steps, 1e3 * tn, 1e3 * t0))
            timed(lambda: qa.q_charge(which=0))
            tq = best(lambda: qa.q_charge(which=0))
            say("charge %s: %.2f ms per call (six field strengths by leaf transport, density, fixed-order sum)" % (name, 1e3 * tq))
    finally:
        qa.end()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
