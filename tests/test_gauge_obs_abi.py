"""CPU-side check of the stout-smearing / topological-charge boundary: the shared library exports the five entry points (nm -D),
the headers declare them with the reference's signatures, and the binding lists and wraps them (no GPU needed)."""
import ctypes as C
import importlib
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
qa = importlib.import_module("quda-qkxtm-multigrid_amd")

QUDA_H = ["performSTOUTnStep", "qChargeCuda"]
EXT_H = ["qudaAmdStoutSmear", "qudaAmdQCharge", "qudaAmdSu3ExpIQ"]


def test_nm_shows_the_five_symbols():
    so = os.path.join(ROOT, "quda-qkxtm-multigrid_amd", "lib", "libquda.so")
    out = subprocess.check_output(["nm", "-D", "--defined-only", so]).decode()
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    missing = [s for s in QUDA_H + EXT_H if s not in exported]
    assert not missing, missing
    L = qa.lib()
    assert all(hasattr(L, s) for s in QUDA_H + EXT_H)


def test_headers_declare_them_and_the_binding_lists_them():
    quda_h = open(os.path.join(ROOT, "include", "quda.h")).read()
    ext_h = open(os.path.join(ROOT, "include", "quda_amd_ext.h")).read()
    assert re.search(r"\bvoid\s+performSTOUTnStep\s*\(\s*unsigned int nSteps,\s*double rho\s*\)\s*;", quda_h)
    assert re.search(r"\bdouble\s+qChargeCuda\s*\(\s*(void)?\s*\)\s*;", quda_h)
    assert re.search(r"\bvoid\s+qudaAmdStoutSmear\s*\(\s*unsigned int nSteps,\s*double rho,\s*int smear_time\s*\)\s*;", ext_h)
    assert re.search(r"\bdouble\s+qudaAmdQCharge\s*\(\s*double \*h_density,\s*int lexicographic,\s*int which\s*\)\s*;", ext_h)
    assert re.search(r"\bvoid\s+qudaAmdSu3ExpIQ\s*\(\s*int n,\s*const double \*q,\s*double \*out\s*\)\s*;", ext_h)
    for s in QUDA_H:
        assert s in qa.QUDA_H_SYMBOLS
    for s in EXT_H:
        assert s in qa.EXT_H_SYMBOLS


def test_binding_has_the_wrappers_and_return_types():
    for name in ("perform_stout", "stout_smear", "q_charge", "su3_exp_iq"):
        assert callable(getattr(qa, name)), name
    L = qa.lib()
    assert L.qChargeCuda.restype is C.c_double and L.qudaAmdQCharge.restype is C.c_double
    assert L.performSTOUTnStep.argtypes == [C.c_uint, C.c_double]
    assert L.qudaAmdStoutSmear.argtypes == [C.c_uint, C.c_double, C.c_int]
    assert len(L.qudaAmdQCharge.argtypes) == 3 and len(L.qudaAmdSu3ExpIQ.argtypes) == 3
