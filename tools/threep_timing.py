"""Timing of the three-point contraction (qudaAmdContractThreep): random sequential and forward columns, no solves.

    python tools/threep_timing.py [--lattice 16,16,16,32] [--lattice 32,32,32,32] [--qsq 4] [--limit 120] [--out profiles/threep_timing.txt]

Every step runs under its own time limit (SIGALRM ends the process: nothing more is started on the GPU after a step that hangs).
Prints, and writes to --out, the device-event times of the ghost exchange, the stencil and the projection, the achieved bytes/s of
the stencil against its compulsory and its requested traffic, its flop rate, and the wall time of the call with the host upload of
the 24 columns."""
import argparse
import importlib
import os
import signal
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
qa = importlib.import_module("quda-qkxtm-multigrid_amd")

# per site: the stencil must read the 24 columns once (24 x 192 B) and the 8 link blocks (8 x 144 B) and write 9 x 16 complex (2304 B);
# what it requests: the S0 task 24 spinors, each of the 8 (direction, A + D | B + C) tasks 4 spinors per column and 2 links
BYTES_COMPULSORY = 24 * 192 + 8 * 144 + 9 * 256
BYTES_REQUESTED = (24 + 8 * 4 * 12) * 192 + 16 * 144 + 9 * 256
# flops: a 4 x 4 colour-summed block is 16 x 3 complex multiply-adds of 8, a colour-matrix product on 4 spins 4 x 66
FLOP_SITE = 8 * 12 * 2 * (4 * 66 + 16 * 3 * 8) + 12 * 16 * 3 * 8


def _expired(signum, frame):
    sys.stderr.write("threep_timing: a step ran into its time limit; stopping\n")
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
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "threep_timing.txt"))
    a = ap.parse_args()
    lattices = [tuple(int(v) for v in s.split(",")) for s in (a.lattice or ["16,16,16,32", "32,32,32,32"])]
    signal.signal(signal.SIGALRM, _expired)
    lines = []
    step(a.limit, lambda: qa.init(0))
    try:
        for X in lattices:
            V = int(np.prod(X))
            gauge = np.zeros((4, V, 18))
            gauge[:, :, [0, 8, 16]] = 1.0   # unit links: only the geometry matters here
            gauge = gauge.reshape(4, V * 18)
            step(a.limit, lambda: qa.load_gauge(gauge, qa.gauge_param(X, t_boundary=qa.QUDA_ANTI_PERIODIC_T)))
            rng = np.random.default_rng(0)
            seq, fwd = rng.standard_normal((12, V * 24)), rng.standard_normal((12, V * 24))
            nm = len(qa.twop_momenta(a.qsq))
            best, wall = None, 1e30
            for _ in range(a.repeat):
                t0 = time.perf_counter()
                step(a.limit, lambda: qa.contract_threep(seq, fwd, None, (1, 2, 3, 5), a.qsq, 4, qa.PROTON, 1))
                wall = min(wall, time.perf_counter() - t0)
                t = qa.threep_last_timings()
                if best is None or t["stencil"] + t["projection"] < best["stencil"] + best["projection"]:
                    best = t
            lines.append("threep %s Q_sq=%d Nmoms=%d: ghost exchange %.5f s, stencil %.5f s, projection %.5f s, call with host upload %.4f s; "
                         "stencil %.2f TB/s compulsory (%d B/site), %.2f TB/s requested (%d B/site), %.2f Tflop/s (%d flop/site)"
                         % ("x".join(map(str, X)), a.qsq, nm, best["ghost"], best["stencil"], best["projection"], wall, V * BYTES_COMPULSORY / best["stencil"] / 1e12,
                            BYTES_COMPULSORY, V * BYTES_REQUESTED / best["stencil"] / 1e12, BYTES_REQUESTED, V * FLOP_SITE / best["stencil"] / 1e12, FLOP_SITE))
            print(lines[-1], flush=True)
    finally:
        qa.end()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
