"""Timing of CG and multi-shift CG: twisted mass, even-odd normal operator, 16^3 x 32 and 32^4.

    python tools/cg_timing.py [--lattice 16,16,16,32] [--lattice 32,32,32,32] [--out profiles/cg_timing.txt] [--limit 240]

For every lattice and precision set (fp64, fp64 with fp32 sloppy, fp64 with 16-bit sloppy), best of --repeat:
  * seconds per CG iteration of invertQuda (solver seconds / iterations), next to a device-event timed loop of the sloppy M^dag M
    (the stencil share) and of the three fused sweeps of an iteration on sloppy fields (the BLAS share);
  * the fused sweeps against the sequence of one-purpose blas:: calls they replace, and the multi-shift update of 1 / 4 / 12 shifts
    against axpy + axpby per shift, with the field passes of each form and the achieved bytes/s;
  * invertMultiShiftQuda with 1, 4 and 12 shifts against as many single-shift solves.
Every step runs under its own time limit (SIGALRM ends the process: nothing more is started on the GPU after a step that hangs)."""
import argparse
import importlib
import os
import signal
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from synth import smooth_gauge_cayley  # noqa: E402

qa = importlib.import_module("quda-qkxtm-multigrid_amd")

KAPPA, MU, TOL = 0.124, 0.005, 1e-10
PRECISIONS = [("fp64", 8, 1e-4), ("fp64/fp32", 4, 1e-4), ("fp64/16-bit", 2, 0.1)]   # name, sloppy precision, reliable_delta
# field passes (reads + writes of one parity field) of the vector work of one CG iteration
PASSES_FUSED = 2 + 3 + 5          # reDotProduct, axpyCGNorm, axpyZpbx
PASSES_UNFUSED = 2 + 3 + 1 + 2 + 3 + 3   # reDotProduct, axpy, norm2, reDotProduct, axpy, xpay
BYTES_SITE = {8: 192, 4: 96, 2: 52}   # one spinor site: 24 reals (+ the fp32 scale of a 16-bit site)


def _expired(signum, frame):
    sys.stderr.write("cg_timing: a step ran into its time limit; stopping\n")
    os._exit(124)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lattice", action="append", default=None)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--limit", type=int, default=240, help="seconds per step")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cg_timing.txt"))
    a = ap.parse_args()
    lattices = [tuple(int(v) for v in s.split(",")) for s in (a.lattice or ["16,16,16,32", "32,32,32,32"])]
    signal.signal(signal.SIGALRM, _expired)
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    def step(fn):
        signal.alarm(a.limit)
        try:
            return fn()
        finally:
            signal.alarm(0)

    def best(fn):
        return min(step(fn) for _ in range(a.repeat))

    def cg_param(sloppy, delta, maxiter=5000):
        ip = qa.invert_param(qa.QUDA_TWISTED_MASS_DSLASH, KAPPA, MU, +1, "ee", 0, cuda_prec=8, prec_sloppy=sloppy,
                             solution_type=qa.QUDA_MATPCDAG_MATPC_SOLUTION)
        ip.solve_type, ip.inv_type, ip.tol, ip.maxiter, ip.reliable_delta = qa.QUDA_NORMOP_PC_SOLVE, qa.QUDA_CG_INVERTER, TOL, maxiter, delta
        return ip

    step(lambda: qa.init(0))
    try:
        for X in lattices:
            name = "x".join(map(str, X))
            Vh = int(np.prod(X)) // 2
            gauge = smooth_gauge_cayley(X, 0.35)
            b = np.random.default_rng(5).random(Vh * 24)
            for pname, sloppy, delta in PRECISIONS:
                step(lambda: qa.load_gauge(gauge, qa.gauge_param(X, cuda_prec=8, prec_sloppy=sloppy, t_boundary=qa.QUDA_PERIODIC_T)))
                ip = cg_param(sloppy, delta)

                def solve():
                    qa.invert(b, ip)
                    return ip.secs / max(ip.iter, 1)
                step(solve)   # warm-up: code objects, launch-parameter search
                per_iter = best(solve)
                iters, res = ip.iter, ip.true_res
                # the same operator and the same sweeps on sloppy fields, device-event timed
                d = qa.Dirac(ip, pc=True, which=1)
                f = [qa.Spinor(sloppy, qa.QUDA_PARITY_SITE_SUBSET).load(np.random.default_rng(i).standard_normal(Vh * 24), ip) for i in range(4)]
                step(lambda: d.time_MdagM(f[0], f[1], 5))
                t_op = best(lambda: d.time_MdagM(f[0], f[1], 50))
                L = qa.lib()
                step(lambda: (L.qudaAmdTimeCGBlas(1, f[0].h, f[1].h, f[2].h, f[3].h, 5), L.qudaAmdTimeCGBlas(0, f[0].h, f[1].h, f[2].h, f[3].h, 5)))
                t_fused = best(lambda: L.qudaAmdTimeCGBlas(1, f[0].h, f[1].h, f[2].h, f[3].h, 50))
                t_unfused = best(lambda: L.qudaAmdTimeCGBlas(0, f[0].h, f[1].h, f[2].h, f[3].h, 50))
                fb = Vh * BYTES_SITE[sloppy]
                say("cg %s %s: %d iterations to %.1e, %.1f us per iteration = M^dag M %.1f us + fused BLAS %.1f us + %.1f us rest (host round trips, reliable updates)"
                    % (name, pname, iters, res, 1e6 * per_iter, 1e6 * t_op, 1e6 * t_fused, 1e6 * (per_iter - t_op - t_fused)))
                say("cg %s %s: BLAS of one iteration fused %.1f us (%d passes, %.2f TB/s) against unfused %.1f us (%d passes, %.2f TB/s): %.2f x"
                    % (name, pname, 1e6 * t_fused, PASSES_FUSED, PASSES_FUSED * fb / t_fused / 1e12, 1e6 * t_unfused, PASSES_UNFUSED,
                       PASSES_UNFUSED * fb / t_unfused / 1e12, t_unfused / t_fused))
                for k in (1, 4, 12):
                    xs = [qa.Spinor(sloppy, qa.QUDA_PARITY_SITE_SUBSET).load(np.zeros(Vh * 24), ip) for _ in range(k)]
                    ps = [qa.Spinor(sloppy, qa.QUDA_PARITY_SITE_SUBSET).load(b, ip) for _ in range(k)]
                    hx, hp = (qa._p * k)(*[s.h for s in xs]), (qa._p * k)(*[s.h for s in ps])
                    step(lambda: (L.qudaAmdTimeMultiShift(1, k, hx, hp, f[0].h, 5), L.qudaAmdTimeMultiShift(0, k, hx, hp, f[0].h, 5)))
                    t_ms = best(lambda: L.qudaAmdTimeMultiShift(1, k, hx, hp, f[0].h, 50))
                    t_seq = best(lambda: L.qudaAmdTimeMultiShift(0, k, hx, hp, f[0].h, 50))
                    sweeps = -(-k // qa.multi_shift_chunk())
                    say("cg %s %s: multi-shift update k = %2d fused %.1f us (%d passes, %.2f TB/s) against per-shift %.1f us (%d passes, %.2f TB/s): %.2f x, model %.2f x"
                        % (name, pname, k, 1e6 * t_ms, 4 * k + sweeps, (4 * k + sweeps) * fb / t_ms / 1e12, 1e6 * t_seq, 6 * k, 6 * k * fb / t_seq / 1e12,
                           t_seq / t_ms, 6.0 * k / (4 * k + sweeps)))
                    for s in xs + ps:
                        s.free()
                for s in f:
                    s.free()
                d.free()
                for k in (1, 4, 12):
                    offsets = [0.0] if k == 1 else list(np.geomspace(1e-3, 1.0, k))
                    ipm = cg_param(sloppy, delta)

                    def multi():
                        qa.invert_multi_shift(b, ipm, offsets, [TOL] * k)
                        return ipm.secs

                    def sequential():
                        total = 0.0
                        for s in offsets:
                            qa.invert_multi_shift(b, ipm, [s], [TOL])
                            total += ipm.secs
                        return total
                    step(multi)
                    t_multi = best(multi)
                    it_multi = ipm.iter
                    t_seq = best(sequential)
                    say("cg %s %s: %2d shifts in one multi-shift solve %.4f s (%d iterations, refinement included) against %d single-shift solves %.4f s: %.2f x"
                        % (name, pname, k, t_multi, it_multi, k, t_seq, t_seq / t_multi))
    finally:
        qa.end()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
