"""CPU-side check of the gauge-fixing boundary: include/quda.h declares computeGaugeFixingOVRQuda with the reference's prototype
token for token, the shared library exports it and the two extension calls (nm -D), and the binding declares and wraps them (no GPU
needed)."""
import ctypes as C
import importlib
import inspect
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
qa = importlib.import_module("quda-qkxtm-multigrid_amd")

# the prototype of the reference's include/quda.h (line 998), as a token list
PROTOTYPE = ("int computeGaugeFixingOVRQuda ( void * gauge , const unsigned int gauge_dir , const unsigned int Nsteps , "
             "const unsigned int verbose_interval , const double relax_boost , const double tolerance , const unsigned int reunit_interval , "
             "const unsigned int stopWtheta , QudaGaugeParam * param , double * timeinfo ) ;")
SYMBOLS = ("computeGaugeFixingOVRQuda", "qudaAmdGaugeFixOVR", "qudaAmdGaugeFixQuality")
REFERENCE_H = "/root/reference/include/quda.h"


def _tokens(header, name):
    txt = re.sub(r"/\*.*?\*/", " ", open(header).read(), flags=re.S)
    txt = re.sub(r"//[^\n]*", " ", txt)
    m = re.search(r"\b(?:int|void|double)\s+%s\s*\([^;{]*\)\s*;" % name, txt)
    assert m, "%s is not declared in %s" % (name, header)
    return re.findall(r"\w+|[^\w\s]", m.group(0))


def test_prototype_matches_the_reference_token_for_token():
    name = "computeGaugeFixingOVRQuda"
    assert _tokens(os.path.join(ROOT, "include", "quda.h"), name) == PROTOTYPE.split()
    if os.path.isfile(REFERENCE_H):   # where the reference tree is present, the table above is checked against it too
        assert _tokens(REFERENCE_H, name) == PROTOTYPE.split()
    assert name in qa.QUDA_H_SYMBOLS
    assert "qudaAmdGaugeFixOVR" in qa.EXT_H_SYMBOLS and "qudaAmdGaugeFixQuality" in qa.EXT_H_SYMBOLS
    for ext in SYMBOLS[1:]:
        _tokens(os.path.join(ROOT, "include", "quda_amd_ext.h"), ext)


def test_nm_shows_the_three_symbols():
    so = os.path.join(ROOT, "quda-qkxtm-multigrid_amd", "lib", "libquda.so")
    out = subprocess.check_output(["nm", "-D", "--defined-only", so]).decode()
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    missing = [s for s in SYMBOLS if s not in exported]
    assert not missing, missing


def test_binding_declares_and_wraps_them():
    L = qa.lib()
    gp, u, d, p = C.POINTER(qa.QudaGaugeParam), C.c_uint, C.c_double, C.c_void_p
    assert L.computeGaugeFixingOVRQuda.restype is C.c_int
    assert L.computeGaugeFixingOVRQuda.argtypes == [p, u, u, u, d, d, u, u, gp, C.POINTER(d)]
    assert L.qudaAmdGaugeFixOVR.restype is C.c_int
    assert L.qudaAmdGaugeFixOVR.argtypes == [p, u, u, u, d, d, u, u, gp, C.POINTER(d), p, C.POINTER(d)]
    assert L.qudaAmdGaugeFixQuality.restype is None and L.qudaAmdGaugeFixQuality.argtypes == [u, C.POINTER(d)]
    assert list(inspect.signature(qa.gauge_fix_ovr).parameters) == ["gp", "gauge_dir", "n_steps", "relax_boost", "tolerance", "reunit_interval", "stop_theta",
                                                                   "gauge", "make_resident_gauge", "return_gauge", "transform", "verbose_interval"]
    assert list(inspect.signature(qa.gauge_fix_quality).parameters) == ["gauge_dir"]
