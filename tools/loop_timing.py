"""Timing of the loop contractions (qudaAmdContractLoop): one random vector, no solves.

    python tools/loop_timing.py [--lattice 16,16,16,32] [--lattice 32,32,32,32] [--qsq 4] [--limit 120]

For every lattice the fused stencil path and the unfused chain (QUDA_AMD_LOOP_FUSED=0: covariant shifts and pairwise contractions
in the reference's call order) run in this one process, each step under its own time limit (SIGALRM ends the process: nothing
more is started on the GPU after a step that hangs).  Prints the device-event times of phi = g5 D_W x, of the stencil (or chain)
and of the projection, the achieved bytes/s of the stencil against its compulsory traffic, and the wall time of the call with
the host upload."""
import argparse
import importlib
import os
import signal
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
qa = importlib.import_module("quda-qkxtm-multigrid_amd")

# per site: the stencil must read x and phi once (2 x 192 B) and the 8 links (8 x 144 B) and write 18 x 16 complex (4608 B); what it
# requests is 18 spinors (the site and its 8 neighbours, x and phi: 3456 B) + the links; the projection reads the 4608 B back
BYTES_COMPULSORY = 2 * 192 + 8 * 144 + 288 * 16
BYTES_REQUESTED = 18 * 192 + 8 * 144 + 288 * 16
# flops: per (mu, sign) task 4 colour-matrix products on 4 spins (66 each) and 4 building blocks (16 x 3 complex multiply-adds of 8)
FLOP_SITE = 8 * (4 * 4 * 66 + 4 * 16 * 3 * 8) + 2 * 16 * 3 * 8
SOLVE_SHARE_32 = 0.171 / 12   # README: 12 lockstep solves at 32^4 in 0.171 s


def _expired(signum, frame):
    sys.stderr.write("loop_timing: a step ran into its time limit; stopping\n")
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
    ap.add_argument("--qsq", type=int, default=4)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--limit", type=int, default=120, help="seconds per step")
    a = ap.parse_args()
    lattices = [tuple(int(v) for v in s.split(",")) for s in (a.lattice or ["16,16,16,32", "32,32,32,32"])]
    signal.signal(signal.SIGALRM, _expired)
    step(a.limit, lambda: qa.init(0))
    try:
        for X in lattices:
            V = int(np.prod(X))
            gauge = np.zeros((4, V, 18))
            gauge[:, :, [0, 8, 16]] = 1.0   # unit links: only the geometry matters here
            gauge = gauge.reshape(4, V * 18)
            step(a.limit, lambda: qa.load_gauge(gauge, qa.gauge_param(X, t_boundary=qa.QUDA_ANTI_PERIODIC_T)))
            x = np.random.default_rng(0).standard_normal(V * 24)
            ip = qa.invert_param(qa.QUDA_TWISTED_MASS_DSLASH, 0.13, 0.01, +1, "ee", 0, cuda_prec=8, solution_type=qa.QUDA_MAT_SOLUTION,
                                 gamma_basis=qa.QUDA_UKQCD_GAMMA_BASIS)
            nm = len(qa.loop_momenta(X[:3], a.qsq))
            name = "x".join(map(str, X))
            res = {}
            for fused in (1, 0):
                os.environ["QUDA_AMD_LOOP_FUSED"] = str(fused)
                best, wall = None, 1e30
                for _ in range(a.repeat):
                    t0 = time.perf_counter()
                    step(a.limit, lambda: qa.contract_loop(x, ip, a.qsq, X[:3]))
                    wall = min(wall, time.perf_counter() - t0)
                    t = qa.loop_last_timings()
                    if best is None or t["total"] < best["total"]:
                        best = t
                res[fused] = best
                extra = ""
                if fused:
                    extra = "; stencil %.2f TB/s compulsory (%d B/site), %.2f TB/s requested (%d B/site), %.2f Tflop/s" % (
                        V * BYTES_COMPULSORY / best["stencil"] / 1e12, BYTES_COMPULSORY, V * BYTES_REQUESTED / best["stencil"] / 1e12, BYTES_REQUESTED,
                        V * FLOP_SITE / best["stencil"] / 1e12)
                print("loop %s Q_sq=%d Nmoms=%d %s: phi %.5f s, %s %.5f s, projection %.5f s, device total %.5f s, call with host upload %.4f s%s"
                      % (name, a.qsq, nm, "fused  " if fused else "unfused", best["phi"], "stencil" if fused else "chain  ", best["stencil"], best["projection"],
                         best["total"], wall, extra), flush=True)
            print("loop %s: unfused / fused device total = %.2f" % (name, res[0]["total"] / res[1]["total"]), flush=True)
            if tuple(X) == (32, 32, 32, 32):
                print("loop %s: contraction %.4f s per vector against %.4f s per vector of the lockstep solve (0.171 s / 12)" % (name, res[1]["total"], SOLVE_SHARE_32),
                      flush=True)
        os.environ.pop("QUDA_AMD_LOOP_FUSED", None)
    finally:
        qa.end()


if __name__ == "__main__":
    main()
