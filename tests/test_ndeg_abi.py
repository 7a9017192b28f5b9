"""The non-degenerate doublet in the library's surface: exported symbol, header, binding, parameter helper (no GPU needed)."""
import importlib
import inspect
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _qa():
    return importlib.import_module("quda-qkxtm-multigrid_amd")


def test_library_exports_the_doublet_twist():
    qa = _qa()
    out = subprocess.run(["nm", "-D", "--defined-only", qa.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert any(line.split()[-1] == "qudaAmdNdegTwist" for line in out.splitlines() if line.strip())


def test_header_declares_and_binding_lists_it():
    qa = _qa()
    header = open(os.path.join(ROOT, "include", "quda_amd_ext.h")).read()
    assert "void qudaAmdNdegTwist(void *out, const void *in, double kappa, double mu, double epsilon, int dagger, int inverse);" in header
    assert "qudaAmdNdegTwist" in qa.EXT_H_SYMBOLS
    assert callable(qa.ndeg_twist)


def test_invert_param_takes_epsilon():
    qa = _qa()
    assert inspect.signature(qa.invert_param).parameters["epsilon"].default == 0.0
    ip = qa.invert_param(qa.QUDA_TWISTED_MASS_DSLASH, 0.12, 0.3, qa.QUDA_TWIST_NONDEG_DOUBLET, "ee", 0, epsilon=0.2)
    assert ip.epsilon == 0.2 and ip.twist_flavor == 2
    assert qa.invert_param().epsilon == 0.0


def test_doublet_flavour_constant_is_the_header_enum():
    """the binding's constant is the value of QUDA_TWIST_NONDEG_DOUBLET in include/enum_quda.h, and Spinor / Dirac / ndeg_twist take it
    (fields are created with it in tests/test_ndeg_gpu.py)"""
    import re
    qa = _qa()
    enum = open(os.path.join(ROOT, "include", "enum_quda.h")).read()
    m = re.search(r"QUDA_TWIST_NONDEG_DOUBLET\s*=\s*([+-]?\d+)", enum)
    assert m and int(m.group(1)) == qa.QUDA_TWIST_NONDEG_DOUBLET == 2
    assert inspect.signature(qa.Spinor.__init__).parameters["flavor"].default == qa.QUDA_TWIST_PLUS
    assert list(inspect.signature(qa.ndeg_twist).parameters) == ["out", "inp", "kappa", "mu", "epsilon", "dagger", "inverse"]
