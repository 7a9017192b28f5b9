"""CPU-side check of the BLAS test hooks: the library exports the qudaAmdBlas* entry points tests/test_blas_kernels_gpu.py and
tools/blas_capped_check.py go through, include/quda_amd_ext.h declares them, and the binding lists and wraps them (no GPU needed:
dlopen + dlsym).  Every operation the reference of tests/blas_ref.py knows is named in the header's list of the dispatcher, and in the
dispatcher itself."""
import importlib
import os
import re

import blas_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
qa = importlib.import_module("quda-qkxtm-multigrid_amd")

EXT_H = ["qudaAmdBlasApply", "qudaAmdBlasDevUpdate", "qudaAmdBlasMultiSupported", "qudaAmdBlasMultiDot", "qudaAmdBlasMultiCaxpyResidual",
         "qudaAmdBlasMultiCaxpy", "qudaAmdBlasHeavyQuarkResidualNorm"]


def test_library_exports_the_blas_hooks():
    L = qa.lib()
    missing = [s for s in EXT_H if not hasattr(L, s)]
    assert not missing, missing


def test_header_declares_them_and_the_binding_lists_them():
    ext_h = open(os.path.join(ROOT, "include", "quda_amd_ext.h")).read()
    for s in EXT_H:
        assert re.search(r"\b%s\s*\(" % s, ext_h), s
        assert s in qa.EXT_H_SYMBOLS
        assert getattr(qa.lib(), s).argtypes is not None, s


def test_binding_has_the_wrappers():
    for name in ("blas_apply", "blas_dev_update", "multi_supported", "multi_dot", "multi_caxpy_residual", "multi_caxpy", "heavy_quark_residual_norm"):
        assert callable(getattr(qa, name)), name


def test_dispatcher_and_reference_name_the_same_operations():
    """every operation with a numpy reference is dispatched by name, documented in the header, and declared in namespace blas"""
    ext_h = open(os.path.join(ROOT, "include", "quda_amd_ext.h")).read()
    blas_h = open(os.path.join(ROOT, "include", "blas.h")).read()
    src = open(os.path.join(ROOT, "quda-qkxtm-multigrid_amd", "csrc", "interface.cpp")).read()
    doc = ext_h[ext_h.index("qudaAmdBlasApply calls"):ext_h.index("int qudaAmdBlasApply")]
    for op in blas_ref.OPERANDS:
        assert 'is("%s")' % op in src, op
        assert re.search(r"\b%s\b" % op, doc), op
        assert re.search(r"\b%s\s*\(" % op, blas_h), op
    dispatched = set(re.findall(r'is\("(\w+)"\)', src))
    assert dispatched == set(blas_ref.OPERANDS), dispatched ^ set(blas_ref.OPERANDS)
    for op in ("caxpyXmazDev", "caxXmazDev", "caxInitDev"):
        assert '"%s"' % op in src and re.search(r"\b%s\s*\(" % op, blas_h), op
