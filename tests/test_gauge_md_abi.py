"""CPU-side check of the gauge molecular-dynamics boundary: include/quda.h declares the four entry points with the reference's
prototypes token for token, the shared library exports them (nm -D), and the binding declares and wraps them (no GPU needed)."""
import ctypes as C
import importlib
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
qa = importlib.import_module("quda-qkxtm-multigrid_amd")

# the prototypes of the reference's include/quda.h (lines 778, 793, 815, 825), as token lists
PROTOTYPES = {
    "computeGaugeForceQuda": "int computeGaugeForceQuda ( void * mom , void * sitelink , int * * * input_path_buf , int * path_length , double * loop_coeff , "
                             "int num_paths , int max_length , double dt , QudaGaugeParam * qudaGaugeParam ) ;",
    "updateGaugeFieldQuda": "void updateGaugeFieldQuda ( void * gauge , void * momentum , double dt , int conj_mom , int exact , QudaGaugeParam * param ) ;",
    "projectSU3Quda": "void projectSU3Quda ( void * gauge_h , double tol , QudaGaugeParam * param ) ;",
    "momActionQuda": "double momActionQuda ( void * momentum , QudaGaugeParam * param ) ;",
}
REFERENCE_H = "/root/reference/include/quda.h"


def _tokens(header, name):
    txt = re.sub(r"/\*.*?\*/", " ", open(header).read(), flags=re.S)
    txt = re.sub(r"//[^\n]*", " ", txt)
    m = re.search(r"\b(?:int|void|double)\s+%s\s*\([^;{]*\)\s*;" % name, txt)
    assert m, "%s is not declared in %s" % (name, header)
    return re.findall(r"\w+|[^\w\s]", m.group(0))


def test_prototypes_match_the_reference_token_for_token():
    for name, proto in PROTOTYPES.items():
        assert _tokens(os.path.join(ROOT, "include", "quda.h"), name) == proto.split(), name
        if os.path.isfile(REFERENCE_H):   # where the reference tree is present, the table above is checked against it too
            assert _tokens(REFERENCE_H, name) == proto.split(), name
        assert name in qa.QUDA_H_SYMBOLS


def test_nm_shows_the_four_symbols():
    so = os.path.join(ROOT, "quda-qkxtm-multigrid_amd", "lib", "libquda.so")
    out = subprocess.check_output(["nm", "-D", "--defined-only", so]).decode()
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    missing = [s for s in PROTOTYPES if s not in exported]
    assert not missing, missing


def test_binding_declares_and_wraps_them():
    for name in ("gauge_force", "update_gauge", "mom_action", "project_su3"):
        assert callable(getattr(qa, name)), name
    L = qa.lib()
    gp = C.POINTER(qa.QudaGaugeParam)
    assert L.computeGaugeForceQuda.restype is C.c_int
    assert L.computeGaugeForceQuda.argtypes == [C.c_void_p, C.c_void_p, C.POINTER(C.POINTER(C.POINTER(C.c_int))), C.POINTER(C.c_int), C.POINTER(C.c_double),
                                                C.c_int, C.c_int, C.c_double, gp]
    assert L.updateGaugeFieldQuda.restype is None
    assert L.updateGaugeFieldQuda.argtypes == [C.c_void_p, C.c_void_p, C.c_double, C.c_int, C.c_int, gp]
    assert L.projectSU3Quda.restype is None and L.projectSU3Quda.argtypes == [C.c_void_p, C.c_double, gp]
    assert L.momActionQuda.restype is C.c_double and L.momActionQuda.argtypes == [C.c_void_p, gp]
