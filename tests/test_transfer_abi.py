"""CPU-side check of the transfer test hook: the library exports qudaAmdMultigridApplyTransfer, which tests/test_transfer_gpu.py goes
through, include/quda_amd_ext.h declares it, and the binding lists and wraps it with one code per operation the header documents (no GPU
needed: dlopen + dlsym)."""
import importlib
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
qa = importlib.import_module("quda-qkxtm-multigrid_amd")

HOOK = "qudaAmdMultigridApplyTransfer"


def test_library_exports_the_hook():
    assert hasattr(qa.lib(), HOOK)


def test_header_declares_it_and_the_binding_lists_it():
    ext_h = open(os.path.join(ROOT, "include", "quda_amd_ext.h")).read()
    assert re.search(r"\bvoid %s\s*\(void \*\w+, int level, int op, int parity, float \*h_out, const float \*h_in\)" % HOOK, ext_h)
    assert HOOK in qa.EXT_H_SYMBOLS
    assert len(getattr(qa.lib(), HOOK).argtypes) == 6


def test_binding_wraps_every_operation_of_the_header():
    assert callable(qa.Multigrid.apply_transfer)
    ext_h = open(os.path.join(ROOT, "include", "quda_amd_ext.h")).read()
    doc = ext_h[ext_h.index("The transfer operators of `level` one by one"):ext_h.index("void %s" % HOOK)]
    ops = dict((name, int(code)) for code, name in re.findall(r"op (\d)\s+(\w+)", doc))
    ops["P4Block+"] = int(re.search(r"op (\d): accumulate = 1", doc).group(1))
    assert ops == qa.Multigrid.TRANSFER_OPS, (ops, qa.Multigrid.TRANSFER_OPS)
    src = open(os.path.join(ROOT, "quda-qkxtm-multigrid_amd", "csrc", "mg_introspect.cpp")).read()
    body = src[src.index("void %s" % HOOK):]
    for fn in ("R", "P", "R4", "P4", "R4Block", "P4Block", "setSiteSubset"):
        assert re.search(r"T->%s\(" % fn, body), fn
