"""Timing of the two-point contractions (qudaAmdContractTwop): random propagators, no solves, no smearing.

    python tools/twop_timing.py [--lattice 16,16,16,32] [--lattice ...] [--qsq 0 --qsq 4]

Prints the wall time of one contraction call (upload of the 24 host columns, rotation, contractions, projection) and the cost
model of the kernels per site.  Run it under `rocprofv3 --kernel-trace --stats` for the per-kernel times."""
import argparse
import importlib
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
qa = importlib.import_module("quda-qkxtm-multigrid_amd")

# cost model per site (complex multiply-add = 8 flops): mesons 2 x 10 channels x 16 spin pairs x 9 colours;
# baryons: 50 Wick terms per flavour (31 chains, 19 traces) x 36 colour pairs; a chain is 16 (diquark) + 64 + 64 cmadds, a trace 16 + 16 + 16
FLOP_MES = 2 * 10 * 16 * 9 * 8
FLOP_BAR = 2 * 36 * (31 * (16 + 64 + 64) + 19 * (16 + 16 + 16)) * 8
BYTES_PROP = 2 * 144 * 16           # both propagators, read once per site (ideal caching)
BYTES_OUT = 340 * 16                # per-site correlator values written and read back by the projection


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lattice", action="append", default=None)
    ap.add_argument("--qsq", action="append", type=int, default=None)
    ap.add_argument("--repeat", type=int, default=2)
    a = ap.parse_args()
    lattices = [tuple(int(v) for v in s.split(",")) for s in (a.lattice or ["16,16,16,32", "24,24,24,48"])]
    qsqs = a.qsq if a.qsq is not None else [0, 4]
    qa.init(0)
    try:
        for X in lattices:
            V = int(np.prod(X))
            gauge = np.zeros((4, V, 18))
            gauge[:, :, [0, 8, 16]] = 1.0   # unit links: only the geometry matters here
            gauge = gauge.reshape(4, V * 18)
            qa.load_gauge(gauge, qa.gauge_param(X, t_boundary=qa.QUDA_PERIODIC_T))
            rng = np.random.default_rng(0)
            up, dn = rng.standard_normal((12, V * 24)), rng.standard_normal((12, V * 24))
            for q in qsqs:
                nm = len(qa.twop_momenta(q))
                best = 1e30
                for _ in range(a.repeat):
                    t0 = time.perf_counter()
                    qa.contract_twop(up, dn, None, (0, 0, 0, 0), q, 0, 0.0)
                    best = min(best, time.perf_counter() - t0)
                flops = V * (FLOP_MES + FLOP_BAR) + V * 340 * nm * 8
                print("twop %s Q_sq=%d Nmoms=%d: %.4f s per call (host upload included); model %.3e flop (%.1f Mflop/site), %.3e bytes"
                      % ("x".join(map(str, X)), q, nm, best, flops, flops / V / 1e6, V * (BYTES_PROP + 2 * BYTES_OUT)), flush=True)
    finally:
        qa.end()


if __name__ == "__main__":
    main()
