"""Timing of the non-degenerate twisted-mass doublet stencil: fused against composed against two degenerate launches.

    python tools/ndeg_timing.py --parent-lib <libquda.so of the parent commit> [--lattice 32,32,32,32] [--lattice 16,16,16,32]
                                [--out profiles/ndeg_timing.txt] [--limit 240]

For every lattice and (precision, link reconstruction) in fp64 / fp32 / 16-bit with 18-real links and fp64 with 12 and 8, best of --repeat
alternating rounds of device-event timed loops (qudaAmdTimeDslash):
  (a) A^-1 D on a parity doublet by the fused doublet stencil (tune key ndeg_fused = 1), by the composed form (ndeg_fused = 0: two
      single-flavour launches on the flavour views plus the flavour-mixing site pass), and two launches of the degenerate A^-1 D
      (flavours +1 and -1) on single-flavour fields; the three are applied in turn inside every round.  With --parent-lib the degenerate
      launches are those of THAT library — a build of the commit before the doublet, which is the yardstick the fused stencil has to beat:
      a child process loads it through QUDA_AMD_LIBRARY, holds the same gauge field and its own fields on the same device, and times its
      two launches when this process asks for them, between the composed leg and the next round's fused leg (one process at a time uses
      the device).  Without --parent-lib the degenerate launches come from the library this process has loaded, and the output says so;
  (b) microseconds per CG iteration of a doublet even-odd solve (invertQuda, NORMOP_PC) and the share of the stencil in it (M^dag M loop);
  (c) the algorithmic bytes per checkerboard site of each form and the ratio the byte model predicts (8 R P + 96 P for the fused stencil
      against 2 (8 R P + 48 P); 16-bit sites carry a 4-byte scale each).
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

KAPPA, MU, EPS, TOL = 0.124, 0.005, 0.2, 1e-10
CONFIGS = [("fp64 R18", 8, 18), ("fp32 R18", 4, 18), ("16-bit R18", 2, 18), ("fp64 R12", 8, 12), ("fp64 R8", 8, 8)]


def bytes_fused(P, R):
    return 8 * R * P + 96 * P + (16 if P == 2 else 0)


def bytes_degenerate(P, R):
    return 8 * R * P + 48 * P + (8 if P == 2 else 0)


_child = None   # the process of the degenerate leg (--parent-lib)


def _expired(signum, frame):
    sys.stderr.write("ndeg_timing: a step ran into its time limit; stopping\n")
    if _child is not None:
        _child.kill()
    os._exit(124)


def degenerate_child():
    """the degenerate leg in a process of its own (its library: QUDA_AMD_LIBRARY).  Commands on stdin, one answer line each on stdout:
    `load X Y Z T prec recon` -> ok, `time n` -> seconds of the two launches (+1, -1) per application, `quit`"""
    out = os.fdopen(os.dup(1), "w")
    os.dup2(2, 1)   # whatever the library prints goes to stderr, the answers keep the pipe
    qa.init(0)
    ds, fields = [], []
    try:
        for line in sys.stdin:
            w = line.split()
            if not w or w[0] == "quit":
                break
            if w[0] == "load":
                X, prec, recon = tuple(int(v) for v in w[1:5]), int(w[5]), int(w[6])
                for f in fields:
                    f.free()
                for d in ds:
                    d.free()
                qa.load_gauge(smooth_gauge_cayley(X, 0.35), qa.gauge_param(X, cuda_prec=prec, recon=recon, t_boundary=qa.QUDA_PERIODIC_T))
                ips = [qa.invert_param(qa.QUDA_TWISTED_MASS_DSLASH, KAPPA, MU, f, "ee", 0, cuda_prec=prec) for f in (+1, -1)]
                ds = [qa.Dirac(ip, pc=True) for ip in ips]
                src = np.random.default_rng(5).standard_normal(int(np.prod(X)) // 2 * 24)
                fields = [qa.Spinor(prec).load(src, ips[0]), qa.Spinor(prec)]
                out.write("ok\n")
            elif w[0] == "time":
                n = int(w[1])
                out.write("%.9e\n" % (ds[0].time_dslash(fields[1], fields[0], 0, n) + ds[1].time_dslash(fields[1], fields[0], 0, n)))
            out.flush()
    finally:
        qa.end()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None, help="libquda.so of the commit before the doublet: its degenerate stencil is the yardstick")
    ap.add_argument("--degenerate-child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--lattice", action="append", default=None)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--niter", type=int, default=50)
    ap.add_argument("--limit", type=int, default=240, help="seconds per step")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ndeg_timing.txt"))
    a = ap.parse_args()
    if a.degenerate_child:
        return degenerate_child()
    lattices = [tuple(int(v) for v in s.split(",")) for s in (a.lattice or ["32,32,32,32", "16,16,16,32"])]
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

    def fused(on):
        qa.lib().qudaAmdSetDslashTune(b"ndeg_fused", on)

    DBL = qa.QUDA_TWIST_NONDEG_DOUBLET
    global _child
    child = None
    if a.parent_lib:
        import subprocess
        child = _child = subprocess.Popen([sys.executable, os.path.abspath(__file__), "--degenerate-child"], stdin=subprocess.PIPE, stdout=subprocess.PIPE, text=True,
                                 env=dict(os.environ, QUDA_AMD_LIBRARY=os.path.abspath(a.parent_lib)))

    def ask(text):
        child.stdin.write(text + "\n")
        child.stdin.flush()
        answer = child.stdout.readline().strip()
        if not answer:
            raise RuntimeError("the degenerate-leg process ended (command: %s)" % text)
        return answer
    say("ndeg: degenerate launches from %s" % ("the parent library " + a.parent_lib if child else "THIS library (no --parent-lib): a slowdown of the degenerate stencil itself would not show"))
    step(lambda: qa.init(0))
    try:
        for X in lattices:
            name = "x".join(map(str, X))
            Vh = int(np.prod(X)) // 2
            gauge = smooth_gauge_cayley(X, 0.35)
            rng = np.random.default_rng(5)
            src2, src1 = rng.standard_normal(2 * Vh * 24), rng.standard_normal(Vh * 24)
            for cname, prec, recon in CONFIGS:
                step(lambda: qa.load_gauge(gauge, qa.gauge_param(X, cuda_prec=prec, recon=recon, t_boundary=qa.QUDA_PERIODIC_T)))
                if child:
                    step(lambda: ask("load %d %d %d %d %d %d" % (X + (prec, recon))))
                ipd = qa.invert_param(qa.QUDA_TWISTED_MASS_DSLASH, KAPPA, MU, DBL, "ee", 0, cuda_prec=prec, epsilon=EPS)
                ips = [qa.invert_param(qa.QUDA_TWISTED_MASS_DSLASH, KAPPA, MU, f, "ee", 0, cuda_prec=prec) for f in (+1, -1)]
                dd, ds = qa.Dirac(ipd, pc=True), [qa.Dirac(ip, pc=True) for ip in ips]
                i2, o2 = qa.Spinor(prec, flavor=DBL).load(src2, ipd), qa.Spinor(prec, flavor=DBL)
                i1, o1 = qa.Spinor(prec).load(src1, ips[0]), qa.Spinor(prec)
                t = {"fused": [], "composed": [], "degenerate": []}

                def round_(n):
                    fused(1)
                    tf = dd.time_dslash(o2, i2, 0, n)
                    fused(0)
                    tc = dd.time_dslash(o2, i2, 0, n)
                    if child:
                        qa.lib().qudaAmdDeviceSynchronize()
                        td = float(ask("time %d" % n))
                    else:
                        td = ds[0].time_dslash(o1, i1, 0, n) + ds[1].time_dslash(o1, i1, 0, n)
                    return tf, tc, td
                step(lambda: round_(5))   # warm-up
                for _ in range(a.repeat):
                    tf, tc, td = step(lambda: round_(a.niter))
                    t["fused"].append(tf); t["composed"].append(tc); t["degenerate"].append(td)
                fused(-1)
                tf, tc, td = (min(t[k]) for k in ("fused", "composed", "degenerate"))
                bf, bd = bytes_fused(prec, recon), 2 * bytes_degenerate(prec, recon)
                say("ndeg %s %s: A^-1 D fused %.1f us (%d B/site, %.2f TB/s), composed %.1f us, two degenerate launches %.1f us (%d B/site, %.2f TB/s)"
                    % (name, cname, 1e6 * tf, bf, bf * Vh / tf / 1e12, 1e6 * tc, 1e6 * td, bd, bd * Vh / td / 1e12))
                say("ndeg %s %s: fused / two degenerate = %.3f (byte model %.3f), composed / two degenerate = %.3f"
                    % (name, cname, tf / td, bf / bd, tc / td))
                for f in (i2, o2, i1, o1):
                    f.free()
                for d in [dd] + ds:
                    d.free()
            # (b) a doublet even-odd CG solve in fp64 and its stencil share
            step(lambda: qa.load_gauge(gauge, qa.gauge_param(X, cuda_prec=8, t_boundary=qa.QUDA_PERIODIC_T)))
            ip = qa.invert_param(qa.QUDA_TWISTED_MASS_DSLASH, KAPPA, MU, DBL, "ee", 0, cuda_prec=8, solution_type=qa.QUDA_MATPCDAG_MATPC_SOLUTION, epsilon=EPS)
            ip.solve_type, ip.inv_type, ip.tol, ip.maxiter = qa.QUDA_NORMOP_PC_SOLVE, qa.QUDA_CG_INVERTER, TOL, 5000
            b = np.random.default_rng(7).random(2 * Vh * 24)
            for form, on in (("fused", 1), ("composed", 0)):
                fused(on)

                def solve():
                    qa.invert(b, ip)
                    return ip.secs / max(ip.iter, 1)
                step(solve)
                per_iter = min(step(solve) for _ in range(3))
                d = qa.Dirac(ip, pc=True)
                x, y = qa.Spinor(8, flavor=DBL).load(b, ip), qa.Spinor(8, flavor=DBL)
                step(lambda: d.time_MdagM(y, x, 5))
                t_op = min(step(lambda: d.time_MdagM(y, x, a.niter)) for _ in range(3))
                say("ndeg %s fp64 CG (%s): %d iterations to %.1e, %.1f us per iteration, M^dag M %.1f us = %.0f %% of it"
                    % (name, form, ip.iter, ip.true_res, 1e6 * per_iter, 1e6 * t_op, 100 * t_op / per_iter))
                x.free(); y.free(); d.free()
            fused(-1)
    finally:
        if child:
            try:
                child.stdin.write("quit\n")
                child.stdin.flush()
                child.wait(timeout=60)
            except Exception:
                child.kill()
        qa.end()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
