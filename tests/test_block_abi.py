"""CPU-side check of the block-field test hooks: the library exports the qudaAmdBlock* entry points tests/test_block_kernels_gpu.py and
tests/test_fine_stencil_gpu.py go through (with qudaAmdCloverTwistDense), include/quda_amd_ext.h declares them, and the binding lists and
wraps them (no GPU needed: dlopen + dlsym).  Every operation the reference of tests/block_ref.py knows is dispatched by name in csrc/block_hooks.cpp, named in the header's list of the dispatcher, declared
in namespace blockblas of include/block.h, and has its operands mapped to slots by the binding."""
import importlib
import os
import re

import block_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
qa = importlib.import_module("quda-qkxtm-multigrid_amd")

EXT_H = ["qudaAmdBlockFieldCreate", "qudaAmdBlockFieldDestroy", "qudaAmdBlockFieldLoad", "qudaAmdBlockFieldSave", "qudaAmdBlockBlasApply",
         "qudaAmdBlockMrUpdate", "qudaAmdBlockPack", "qudaAmdBlockUnpack", "qudaAmdBlockPackParity", "qudaAmdBlockUnpackParity",
         "qudaAmdBlockGhostPanels", "qudaAmdBlockFineApply", "qudaAmdCloverTwistDense", "qudaAmdBlockFineApplySite"]


def test_library_exports_the_block_hooks():
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
    for name in ("BlockField", "block_blas_apply", "block_mr_update", "block_pack", "block_unpack", "block_pack_parity", "block_unpack_parity",
                 "block_ghost_panels", "block_fine_apply", "clover_twist_dense", "block_fine_apply_site"):
        assert callable(getattr(qa, name)), name


def test_dispatcher_and_reference_name_the_same_operations():
    ext_h = open(os.path.join(ROOT, "include", "quda_amd_ext.h")).read()
    block_h = open(os.path.join(ROOT, "include", "block.h")).read()
    src = open(os.path.join(ROOT, "quda-qkxtm-multigrid_amd", "csrc", "block_hooks.cpp")).read()
    doc = ext_h[ext_h.index("qudaAmdBlockBlasApply calls"):ext_h.index("int qudaAmdBlockBlasApply")]
    ns = block_h[block_h.index("namespace blockblas {"):block_h.index("}  // namespace blockblas")]
    for op, names in block_ref.OPERANDS.items():
        assert 'is("%s")' % op in src, op
        assert re.search(r"\b%s\b" % op, doc), op
        assert re.search(r"\bvoid %s\s*\(" % op, ns), op
        assert sorted(qa.BLOCK_BLAS_SLOTS[op]) == sorted(names), op
        assert len(set(qa.BLOCK_BLAS_SLOTS[op].values())) == len(names) and set(qa.BLOCK_BLAS_SLOTS[op].values()) <= set("xyzwu"), op
    dispatched = set(re.findall(r'is\("(\w+)"\)', src))
    assert dispatched == set(block_ref.OPERANDS), dispatched ^ set(block_ref.OPERANDS)
    for fn in ("mrUpdateDev", "mr2UpdateDev"):
        assert re.search(r"\bblockblas::%s\s*\(" % fn, src) and re.search(r"\bvoid %s\s*\(" % fn, ns), fn
    for fn in ("blockPack", "blockUnpack", "blockPackParity", "blockUnpackParity"):
        assert re.search(r"\b%s\s*\(" % fn, src) and re.search(r"\bvoid %s\s*\(" % fn, block_h), fn
