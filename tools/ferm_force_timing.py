"""Timing of the twisted-mass fermion force at 16^4 and 32^4 (fp64 links and spinors, one rank).

    python tools/ferm_force_timing.py [--lattice 16,16,16,16 --lattice 32,32,32,32] [--repeat 10] [--out profiles/ferm_force_timing.json]

Per lattice and nvector (1 and 8): ms of the whole qudaAmdComputeTMForce call (wall clock around the C entry point, which ends in a
stream synchronisation: upload of the nvector host solutions, construction of X and Y by the Dirac classes, the kernel) and ms of
the outer-product kernel alone (device events around its launches, qudaAmdFermForceLastKernelSecs), links and momentum resident,
nothing returned to the host; the median of --repeat calls after one warm-up call of every shape.  kernel_model_gbs divides the
bytes of the cost model of DESIGN §3 (per site: 576 B links, 640 B momentum read and written, and per pair 2 x 192 B own spinors plus
8 x 192 B neighbours) by the kernel time: a model figure, not a counter.  One JSON line.  Every call runs under its own time limit
(SIGALRM ends the process: nothing more is started on the GPU after a call that hangs)."""
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

qa = importlib.import_module("quda-qkxtm-multigrid_amd")


def _expired(signum, frame):
    sys.stderr.write("ferm_force_timing: a call ran into its time limit; stopping\n")
    os._exit(124)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lattice", action="append", default=None)
    ap.add_argument("--repeat", type=int, default=10)
    ap.add_argument("--limit", type=int, default=120, help="seconds per call")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ferm_force_timing.json"))
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

    kappa, mu = 0.13, 0.2
    result = {"what": "twisted-mass fermion force, fp64, even-even symmetric, one rank, ms per call (median of %d)" % a.repeat, "lattices": {}}
    timed(lambda: qa.init(0))
    try:
        for X in lattices:
            V = int(np.prod(X))
            gp = qa.gauge_param(X, t_boundary=qa.QUDA_ANTI_PERIODIC_T)
            gauge = tiled_gauge(X)
            timed(lambda: qa.load_gauge(gauge, gp))
            ip = qa.invert_param(qa.QUDA_TWISTED_MASS_DSLASH, kappa, mu, qa.QUDA_TWIST_PLUS, "ee", 0, solution_type=qa.QUDA_MATPCDAG_MATPC_SOLUTION)
            ip.solve_type = qa.QUDA_NORMOP_PC_SOLVE
            rng = np.random.default_rng(3)
            r = {}
            for nv in (1, 8):
                xs = [rng.standard_normal(V * 12) for _ in range(nv)]
                coeff = [1.0 / (k + 1) for k in range(nv)]
                # the first call creates the resident momentum (overwrite) and warms up; the timed ones accumulate into it
                timed(lambda: qa.tm_force(gp, ip, xs, coeff, 1e-3, overwrite=True, make_resident_mom=True, return_mom=False))
                call, kernel = [], []
                for _ in range(a.repeat):
                    call.append(timed(lambda: qa.tm_force(gp, ip, xs, coeff, 1e-3, make_resident_mom=True, return_mom=False)))
                    kernel.append(qa.ferm_force_kernel_secs())
                model_bytes = V * (576.0 + 640.0 + nv * (2 + 8) * 192.0)
                k = statistics.median(kernel)
                r["nvector_%d" % nv] = {"call_ms": round(1e3 * statistics.median(call), 3), "kernel_ms": round(1e3 * k, 4),
                                        "kernel_model_bytes": int(model_bytes), "kernel_model_gbs": round(model_bytes / k * 1e-9, 1)}
            result["lattices"]["x".join(map(str, X))] = r
            print(json.dumps({"x".join(map(str, X)): r}), flush=True)
    finally:
        qa.end()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(json.dumps(result) + "\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
