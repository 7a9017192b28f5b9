"""CPU-side check of the projection's test hook: the library exports qudaAmdMomentumProject, which tests/test_momproj_gpu.py goes
through, include/quda_amd_ext.h declares it, and the binding lists and wraps it (no GPU needed: dlopen + dlsym).  The constants that the
reference of tests/momproj_ref.py restates are the kernel's."""
import importlib
import os
import re

import numpy as np
import pytest

import momproj_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
qa = importlib.import_module("quda-qkxtm-multigrid_amd")

HOOK = "qudaAmdMomentumProject"


def test_library_exports_the_hook():
    assert hasattr(qa.lib(), HOOK)


def test_header_declares_it_and_the_binding_lists_it():
    ext_h = open(os.path.join(ROOT, "include", "quda_amd_ext.h")).read()
    assert re.search(r"\bvoid\s+%s\s*\(double \*h_acc, const double \*h_cs, int nblk, int t0, int nt, int Lt, const int \*moms, int Nm," % HOOK, ext_h)
    assert HOOK in qa.EXT_H_SYMBOLS
    assert len(getattr(qa.lib(), HOOK).argtypes) == 11
    assert getattr(qa.lib(), HOOK).restype is None


def test_binding_has_the_wrapper_and_it_checks_shapes():
    assert callable(qa.momentum_project)
    acc, cs = np.zeros((1, 2, 3, 16), complex), np.zeros((1, 48, 16), complex)
    moms = np.zeros((3, 3), np.int32)
    with pytest.raises(ValueError):      # slice 2 of 2
        qa.momentum_project(acc, cs, 2, moms, (6, 4, 2))
    with pytest.raises(ValueError):      # 48 sites are no whole number of slices of 5 x 4 x 2
        qa.momentum_project(acc, cs, 0, moms, (5, 4, 2))
    with pytest.raises(ValueError):      # two momenta for an accumulator of three
        qa.momentum_project(acc, cs, 0, moms[:2], (6, 4, 2))


def test_the_reference_restates_the_kernels_constants():
    src = open(os.path.join(ROOT, "quda-qkxtm-multigrid_amd", "csrc", "momproj.hip")).read()
    assert re.search(r"NPART = %d\b" % momproj_ref.NPART, src) and re.search(r"NLANE = %d\b" % momproj_ref.NLANE, src)
    assert re.search(r"MB_SMALL = 8, MB_LARGE = 36\b", src)
