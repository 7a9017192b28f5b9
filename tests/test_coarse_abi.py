"""CPU-side check of the coarse-operator test hooks that tests/test_coarse_pc_gpu.py goes through: the library exports them, include/
quda_amd_ext.h declares them with the prototypes the bindings assume, and the bindings wrap every link set and Schur operation the header
documents (no GPU needed: dlopen + dlsym)."""
import importlib
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
qa = importlib.import_module("quda-qkxtm-multigrid_amd")

PROTOTYPES = {
    "qudaAmdMultigridGetCoarseSiteLinks": r"void %s\s*\(void \*\w+, int level, int which, float \*h_out\)",
    "qudaAmdMultigridCoarseApply": r"int %s\s*\(void \*\w+, int level, int which, int mmask, int parity, float \*h_out, const float \*h_in\)",
    "qudaAmdMultigridCoarsePC": r"int %s\s*\(void \*\w+, int level, int impl, int op, int parity, int nrhs, float \*h_out, const float \*h_in\)",
    "qudaAmdCoarseInvertSites": r"void %s\s*\(int n, int nsites, const float \*h_X, float \*h_Xinv, float \*h_hat, const float \*h_H, int \*fail\)",
}


def header():
    return open(os.path.join(ROOT, "include", "quda_amd_ext.h")).read()


@pytest.mark.parametrize("hook", sorted(PROTOTYPES))
def test_library_exports_the_hook_and_the_header_declares_what_the_binding_assumes(hook):
    assert hasattr(qa.lib(), hook)
    proto = re.search(r"\b" + PROTOTYPES[hook] % hook, header())
    assert proto, hook
    assert hook in qa.EXT_H_SYMBOLS
    fn = getattr(qa.lib(), hook)
    assert len(fn.argtypes) == proto.group(0).count(",") + 1
    assert (fn.restype is None) == proto.group(0).startswith("void")


def test_bindings_wrap_every_link_set_and_operation_of_the_header():
    txt = header()
    doc = txt[txt.index("The even-odd preconditioned coarse operator piece by piece"):txt.index("void qudaAmdMultigridGetCoarseSiteLinks")]
    assert re.search(r"which 0: the links \(8 = X\), 1: the\s+\*?\s*preconditioned links", doc) and "2 / 3" in doc
    assert qa.Multigrid.SITE_LINKS == {"links": 0, "hat": 1, "links16": 2, "hat16": 3}
    ops = dict((name, int(code)) for code, name in re.findall(r"op (\d): (Mhat|prepare|reconstruct)", doc))
    assert ops == {"Mhat": 0, "prepare": 1, "reconstruct": 2}
    assert qa.Multigrid.PC_OPS == {"M": 0, "prepare": 1, "reconstruct": 2}
    for name in ("coarse_site_links", "coarse_apply", "coarse_pc"):
        assert callable(getattr(qa.Multigrid, name))
    assert callable(qa.coarse_invert_sites)


def test_hooks_call_the_library_code_and_do_not_copy_it():
    csrc = os.path.join(ROOT, "quda-qkxtm-multigrid_amd", "csrc")
    src = open(os.path.join(csrc, "mg_introspect.cpp")).read()
    body = src[src.index("void qudaAmdMultigridGetCoarseSiteLinks"):]
    for call in (r"applyCoarse\(", r"blockCoarseSchurPiece\(", r"coarseInvertHat\(", r"pc->M\(", r"pc->prepare\(", r"pc->reconstruct\("):
        assert re.search(call, body), call
    block = open(os.path.join(csrc, "block_coarse_cycle.cpp")).read()
    start = block.index("int blockCoarseSchurPiece")
    piece = block[start:block.index("\n}\n", start)]   # to the end of that function
    for call in (r"bc\.matpc\(", r"bc\.prepare\(", r"bc\.reconstruct\("):
        assert re.search(call, piece), call
    coarse = open(os.path.join(csrc, "coarse.hip")).read()
    hat_links = coarse[coarse.index("const CoarseGauge &DiracCoarse::HatLinks() const {"):coarse.index("DiracCoarse::DiracCoarse(const DiracParam &p)")]
    assert "coarseInvertHat(" in hat_links and "errorQuda(" in hat_links   # HatLinks still stops on a singular X
    assert coarse.count("hipLaunchKernelGGL(coarse_invert_kernel") == 1
