"""Timing of gauge molecular dynamics at 16^4 and 32^4 (fp64 links, one rank).

    python tools/gauge_md_timing.py [--lattice 16,16,16,16 --lattice 32,32,32,32] [--repeat 5] [--out profiles/gauge_md_timing.json]

Wall clock of the C entry points around calls that end in a stream synchronisation, links and momenta resident, nothing returned
to the host; the median of --repeat calls after one warm-up call of every shape.  Per lattice: ms per plaquette force and per
tree-level Symanzik force (plaquette + 1x2 rectangles), by the direct gather and by the transport formulation
(QUDA_AMD_GAUGE_FORCE_TRANSPORT=1), ms per link update and ms per momActionQuda.  The link update includes what makes the new links
resident: the copy of the four directions to the host and the reload of the precise, sloppy and preconditioner copies through the
loader.  GFLOP/s of a force counts 198 flops per 3x3 complex product and the products the paths need (length - 1 per path, plus one
per link for U V), nothing else.  One JSON line.  Every call runs under its own time limit (SIGALRM ends the process: nothing more
is started on the GPU after a call that hangs)."""
import argparse
import importlib
import json
import os
import signal
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from synth import tiled_gauge  # noqa: E402
import gauge_md_ref as md  # noqa: E402

qa = importlib.import_module("quda-qkxtm-multigrid_amd")


def _expired(signum, frame):
    sys.stderr.write("gauge_md_timing: a call ran into its time limit; stopping\n")
    os._exit(124)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lattice", action="append", default=None)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--limit", type=int, default=120, help="seconds per call")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gauge_md_timing.json"))
    a = ap.parse_args()
    lattices = [tuple(int(v) for v in s.split(",")) for s in (a.lattice or ["16,16,16,16", "32,32,32,32"])]
    signal.signal(signal.SIGALRM, _expired)

    def timed(fn):
        signal.alarm(a.limit)
        try:
            t0 = time.perf_counter()
            fn()
            return time.perf_counter() - t0
        finally:
            signal.alarm(0)

    def ms(fn):
        timed(fn)   # warm-up: code objects, buffers
        return 1e3 * statistics.median(timed(fn) for _ in range(a.repeat))

    tables = {"plaquette": md.wilson_paths(), "symanzik": md.symanzik_paths()}
    result = {"what": "gauge molecular dynamics, fp64 links, one rank, ms per call (median of %d)" % a.repeat, "lattices": {}}
    timed(lambda: qa.init(0))
    try:
        for X in lattices:
            V = int(np.prod(X))
            gauge = tiled_gauge(X)
            gp = qa.gauge_param(X, t_boundary=qa.QUDA_PERIODIC_T)
            timed(lambda: qa.load_gauge(gauge, gp))
            r = {}
            for name, (paths, coeff) in tables.items():
                products = sum(len(p) - 1 for p in paths[0]) + 1
                gflop = 198.0 * products * 4 * V * 1e-9
                for form in ("direct", "transport"):
                    os.environ["QUDA_AMD_GAUGE_FORCE_TRANSPORT"] = "1" if form == "transport" else "0"
                    # the first call creates the resident momentum (overwrite), the timed ones accumulate into it
                    timed(lambda: qa.gauge_force(gp, paths, coeff, 1e-3, overwrite=True, make_resident_mom=True, return_mom=False))
                    t = ms(lambda: qa.gauge_force(gp, paths, coeff, 1e-3, make_resident_mom=True, return_mom=False))
                    r["%s_force_%s_ms" % (name, form)] = round(t, 3)
                    r["%s_force_%s_gflops" % (name, form)] = round(gflop / (1e-3 * t), 1)
                r["%s_force_gflop" % name] = round(gflop, 2)
            os.environ["QUDA_AMD_GAUGE_FORCE_TRANSPORT"] = "0"
            r["mom_action_ms"] = round(ms(lambda: qa.mom_action(gp)), 3)
            r["link_update_exact_ms"] = round(ms(lambda: qa.update_gauge(gp, 1e-3, exact=True, make_resident_gauge=True, make_resident_mom=True, return_gauge=False)), 3)
            r["link_update_taylor_ms"] = round(ms(lambda: qa.update_gauge(gp, 1e-3, exact=False, make_resident_gauge=True, make_resident_mom=True, return_gauge=False)), 3)
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
