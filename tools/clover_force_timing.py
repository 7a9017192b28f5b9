"""Timing of the twisted-clover force at 16^4 and 32^4 (fp64 links, spinors and clover term, one rank).

    python tools/clover_force_timing.py [--lattice 16,16,16,16 --lattice 32,32,32,32] [--repeat 10] [--out profiles/clover_force_timing.json]

Per lattice: ms of the derivative kernel and of the sigma-trace kernel alone (device events around their launches,
qudaAmdFermForceLastKernelSecs after qudaAmdCloverDerivativeForce / qudaAmdCloverSigmaTrace), of the whole qudaAmdCloverLogDetForce call, and
per nvector (1 and 8) ms of the sigma outer product kernel alone (after qudaAmdCloverSigmaOprod), of all kernels of a twisted-clover
qudaAmdComputeTMForce (hop outer product, sigma outer product, derivative) and of that whole call (wall clock around the C entry point,
which ends in a stream synchronisation: upload of the host solutions, construction of X and Y, the kernels); links, clover term and
momentum resident, no momentum returned to the host; the median of --repeat calls after one warm-up call of every shape.
deriv_model_gbs divides the upper byte count of the cost model of DESIGN §3 "Twisted-clover force" (per site 76 links of 144 B, 96
tensor matrices of 192 B, 640 B momentum read and written) by the kernel time: a model figure, not a counter.  One JSON line.  Every call
runs under its own time limit (SIGALRM ends the process: nothing more is started on the GPU after a call that hangs)."""
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
    sys.stderr.write("clover_force_timing: a call ran into its time limit; stopping\n")
    os._exit(124)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lattice", action="append", default=None)
    ap.add_argument("--repeat", type=int, default=10)
    ap.add_argument("--limit", type=int, default=120, help="seconds per call")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "clover_force_timing.json"))
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

    def median_of(fn):
        """(median wall seconds, median kernel seconds) of --repeat calls after one warm-up call"""
        timed(fn)
        wall, kernel = [], []
        for _ in range(a.repeat):
            wall.append(timed(fn))
            kernel.append(qa.ferm_force_kernel_secs())
        return statistics.median(wall), statistics.median(kernel)

    kappa, mu = 0.13, 0.2
    ms = lambda s, digits=4: round(1e3 * s, digits)
    result = {"what": "twisted-clover force, fp64, even-even symmetric, one rank, ms per call (median of %d)" % a.repeat, "lattices": {}}
    timed(lambda: qa.init(0))
    try:
        for X in lattices:
            V = int(np.prod(X))
            gp = qa.gauge_param(X, t_boundary=qa.QUDA_ANTI_PERIODIC_T)
            gauge = tiled_gauge(X)
            timed(lambda: qa.load_gauge(gauge, gp))
            ip = qa.invert_param(qa.QUDA_TWISTED_CLOVER_DSLASH, kappa, mu, qa.QUDA_TWIST_PLUS, "ee", 0, solution_type=qa.QUDA_MATPCDAG_MATPC_SOLUTION)
            ip.solve_type = qa.QUDA_NORMOP_PC_SOLVE
            ip.clover_coeff = kappa * 1.57551
            timed(lambda: qa.load_clover(None, None, ip))
            rng = np.random.default_rng(3)
            tensor = rng.standard_normal((V, 6, 3, 3, 2))
            # the first call creates the resident momentum (overwrite); the timed ones accumulate into it
            timed(lambda: qa.clover_derivative_force(gp, tensor, 1e-3, overwrite=True, make_resident_mom=True, return_mom=False))
            _, deriv = median_of(lambda: qa.clover_derivative_force(gp, tensor, 1e-3, make_resident_mom=True, return_mom=False))
            _, trace = median_of(lambda: qa.clover_sigma_trace(ip, 1.0, 1.0, V))
            logdet, logdet_kernels = median_of(lambda: qa.clover_logdet_force(gp, ip, 1e-3, 0.0, -1.0, make_resident_mom=True, return_mom=False))
            model_bytes = V * (76 * 144.0 + 96 * 192.0 + 640.0)
            r = {"deriv_kernel_ms": ms(deriv), "deriv_model_bytes": int(model_bytes), "deriv_model_gbs": round(model_bytes / deriv * 1e-9, 1),
                 "trace_kernel_ms": ms(trace), "logdet_call_ms": ms(logdet, 3), "logdet_kernels_ms": ms(logdet_kernels)}
            full_ip = qa.invert_param(qa.QUDA_TWISTED_CLOVER_DSLASH, kappa, mu, qa.QUDA_TWIST_PLUS, "ee", 0, solution_type=qa.QUDA_MAT_SOLUTION)
            for nv in (1, 8):
                xs = [rng.standard_normal(V * 12) for _ in range(nv)]
                coeff = [1.0 / (k + 1) for k in range(nv)]
                call, kernels = median_of(lambda: qa.tm_force(gp, ip, xs, coeff, 1e-3, make_resident_mom=True, return_mom=False))
                fx, fy = [rng.standard_normal(V * 24) for _ in range(nv)], [rng.standard_normal(V * 24) for _ in range(nv)]
                _, oprod = median_of(lambda: qa.clover_sigma_oprod(full_ip, fx, fy, np.ones((nv, 2)), V))
                r["nvector_%d" % nv] = {"tm_force_call_ms": ms(call, 3), "tm_force_kernels_ms": ms(kernels), "sigma_oprod_kernel_ms": ms(oprod)}
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
