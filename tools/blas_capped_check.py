#!/usr/bin/env python3
"""The BLAS kernel checks of tests/test_blas_kernels_gpu.py under a grid cap.

The cap of the BLAS grids (QUDA_AMD_BLAS_BLOCKS, default 512 work-groups) is read once per process, and on the lattices of the test suite it
never binds, so the suite's own process drives neither a second trip of the 4-way unrolled loop of blas_kernel nor its mixed live / dead
tail.  Run this with QUDA_AMD_BLAS_BLOCKS=1 or 2: on the full 6x6x4x2 field one work-group makes four trips over the 3456 fp64 chunks (the
last group with a partly live u = 1 lane and dead u = 2, 3), two over the 1728 fp32 chunks and two of the site loop over the 288 sites of a
16-bit field; two work-groups run the same loops with more than one block in the completion-counter reduction and a live group across the
switch between the parity segments.

Runs every single-field, aliased, device-scalar, multi-field and heavy-quark check in fp64, fp32 and 16 bits, prints one
    OK <op> <prec> <error> <bound>
line per check (the comparison of the call that came closest to its bound) and exits nonzero at the first failure.

    QUDA_AMD_BLAS_BLOCKS=1 python tools/blas_capped_check.py"""
import importlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import blas_ref as R  # noqa: E402
import test_blas_kernels_gpu as T  # noqa: E402

LATTICE = "6x6x4x2-full"


def main():
    qa = importlib.import_module("quda-qkxtm-multigrid_amd")
    print("cap %s on %s" % (os.environ.get("QUDA_AMD_BLAS_BLOCKS", "default"), LATTICE))
    qa.init(0)
    status = 0
    try:
        for prec in T.PRECS:
            def ok(op, rec):
                print("OK %s %d %.3e %.3e" % (op, prec, rec[1], rec[2]), flush=True)

            def fields(seed):
                return T.Fields(qa, LATTICE, prec, seed)

            for op in T.SINGLE_OPS:
                ok(op, T.check_single(qa, fields(31), op))
            ok("xmyz", T.check_single(qa, fields(32), "xmyz", alias="yz"))
            ok("caxpy", T.check_single(qa, fields(33), "caxpy", alias="xy"))
            ok("cDotProduct", T.check_self_dot(qa, fields(34)))
            for op in sorted(T.DEV_OPS):
                ok(op + "Dev", T.check_dev(qa, fields(35), op))
                ok(op + "Dev", T.check_dev(qa, fields(36), op, breakdown=True))
            T.check_multi_supported(qa, fields(37))
            ok("multiSupported", ("", 0.0, 0.0))
            ok("HeavyQuarkResidualNorm", T.check_heavy_quark(qa, fields(130)))
            if prec == 2:
                continue
            for k in T.MULTI_K:
                ok("multiDot", T.check_multi_dot(qa, fields(40 + k), k))
                ok("multiCaxpyResidual", T.check_multi_caxpy(qa, fields(70 + k), k, True))
                ok("multiCaxpy", T.check_multi_caxpy(qa, fields(100 + k), k, False))
    except R.Mismatch as e:
        print("FAILED %s" % e, flush=True)
        status = 1
    finally:
        qa.end()
    return status


if __name__ == "__main__":
    sys.exit(main())
