"""quda-qkxtm-multigrid_amd — MI355X-native twisted-mass Dslash / multigrid library behind the QUDA C ABI.

This package is only the Python-side binding used by tests and bench.py: ctypes mirrors of the PODs in
include/quda.h (field-for-field, the ABI of reference include/quda.h:25-409) and thin wrappers over the
extern "C" entry points of lib/libquda.so (built from csrc/ by `make`, see __graft_entry__.build()).
There is NO CPU fallback: importing works without a GPU (so the symbol table can be checked), but any
compute call needs a gfx950 device, and a missing library raises immediately.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("QUDA_AMD_LIBRARY") or os.path.join(_HERE, "lib", "libquda.so")   # override: A/B timing of two builds
INCLUDE_DIR = os.path.join(os.path.dirname(_HERE), "include")

# ---- enum values (include/quda.h) ----
QUDA_INVALID_ENUM = -(2**31)
QUDA_CPU_FIELD_LOCATION, QUDA_CUDA_FIELD_LOCATION = 1, 2
QUDA_HALF_PRECISION, QUDA_SINGLE_PRECISION, QUDA_DOUBLE_PRECISION = 2, 4, 8
QUDA_RECONSTRUCT_NO, QUDA_RECONSTRUCT_12, QUDA_RECONSTRUCT_8 = 18, 12, 8
QUDA_WILSON_LINKS = 0
QUDA_QDP_GAUGE_ORDER = 5
QUDA_MILC_GAUGE_ORDER = 8
QUDA_ANTI_PERIODIC_T, QUDA_PERIODIC_T = -1, 1
QUDA_GAUGE_FIXED_NO = 0
QUDA_WILSON_DSLASH, QUDA_TWISTED_MASS_DSLASH, QUDA_TWISTED_CLOVER_DSLASH = 0, 7, 8
QUDA_CG_INVERTER, QUDA_BICGSTAB_INVERTER, QUDA_GCR_INVERTER, QUDA_MR_INVERTER, QUDA_MG_INVERTER = 0, 1, 2, 3, 15
QUDA_MAT_SOLUTION, QUDA_MATDAG_MAT_SOLUTION, QUDA_MATPC_SOLUTION, QUDA_MATPC_DAG_SOLUTION, QUDA_MATPCDAG_MATPC_SOLUTION = 0, 1, 2, 3, 4
QUDA_DIRECT_SOLVE, QUDA_NORMOP_SOLVE, QUDA_DIRECT_PC_SOLVE, QUDA_NORMOP_PC_SOLVE = 0, 1, 2, 3
QUDA_MG_CYCLE_VCYCLE, QUDA_MG_CYCLE_FCYCLE, QUDA_MG_CYCLE_WCYCLE, QUDA_MG_CYCLE_RECURSIVE = 0, 1, 2, 3
QUDA_ADDITIVE_SCHWARZ = 0
QUDA_L2_RELATIVE_RESIDUAL = 1
QUDA_MATPC_EVEN_EVEN, QUDA_MATPC_ODD_ODD, QUDA_MATPC_EVEN_EVEN_ASYMMETRIC, QUDA_MATPC_ODD_ODD_ASYMMETRIC = 0, 1, 2, 3
MATPC = {"ee": 0, "oo": 1, "eeasym": 2, "ooasym": 3}
QUDA_DAG_NO, QUDA_DAG_YES = 0, 1
QUDA_KAPPA_NORMALIZATION, QUDA_MASS_NORMALIZATION, QUDA_ASYMMETRIC_MASS_NORMALIZATION = 0, 1, 2
QUDA_DEFAULT_NORMALIZATION = 0
QUDA_PRESERVE_SOURCE_NO, QUDA_PRESERVE_SOURCE_YES = 0, 1
QUDA_DIRAC_ORDER, QUDA_QDP_DIRAC_ORDER = 1, 2
QUDA_PACKED_CLOVER_ORDER = 5
QUDA_SILENT, QUDA_SUMMARIZE, QUDA_VERBOSE, QUDA_DEBUG_VERBOSE = 0, 1, 2, 3
QUDA_TUNE_NO = 0
QUDA_EVEN_PARITY, QUDA_ODD_PARITY = 0, 1
QUDA_PARITY_SITE_SUBSET, QUDA_FULL_SITE_SUBSET = 1, 2
QUDA_DEGRAND_ROSSI_GAMMA_BASIS, QUDA_UKQCD_GAMMA_BASIS = 0, 1
QUDA_TWIST_MINUS, QUDA_TWIST_PLUS, QUDA_TWIST_NO = -1, 1, 0
QUDA_TWIST_NONDEG_DOUBLET = 2   # two-flavour fields, host layout [flavour 1][flavour 2] per parity
QUDA_USE_INIT_GUESS_NO, QUDA_USE_INIT_GUESS_YES = 0, 1
QUDA_COMPUTE_NULL_VECTOR_NO, QUDA_COMPUTE_NULL_VECTOR_YES = 0, 1
QUDA_BOOLEAN_NO, QUDA_BOOLEAN_YES = 0, 1

QUDA_MAX_DIM, QUDA_MAX_MULTI_SHIFT, QUDA_MAX_DWF_LS, QUDA_MAX_MG_LEVEL = 6, 32, 128, 4

_i, _d, _p = C.c_int, C.c_double, C.c_void_p


class QudaGaugeParam(C.Structure):
    _fields_ = [("location", _i), ("X", _i * 4), ("anisotropy", _d), ("tadpole_coeff", _d), ("scale", _d), ("type", _i),
                ("gauge_order", _i), ("t_boundary", _i), ("cpu_prec", _i), ("cuda_prec", _i), ("reconstruct", _i),
                ("cuda_prec_sloppy", _i), ("reconstruct_sloppy", _i), ("cuda_prec_precondition", _i),
                ("reconstruct_precondition", _i), ("gauge_fix", _i), ("ga_pad", _i), ("site_ga_pad", _i), ("staple_pad", _i),
                ("llfat_ga_pad", _i), ("mom_ga_pad", _i), ("gaugeGiB", _d), ("preserve_gauge", _i),
                ("staggered_phase_type", _i), ("staggered_phase_applied", _i), ("i_mu", _d), ("overlap", _i),
                ("overwrite_mom", _i), ("use_resident_gauge", _i), ("use_resident_mom", _i), ("make_resident_gauge", _i),
                ("make_resident_mom", _i), ("return_result_gauge", _i), ("return_result_mom", _i)]


class QudaInvertParam(C.Structure):
    _fields_ = [("input_location", _i), ("output_location", _i), ("dslash_type", _i), ("inv_type", _i), ("mass", _d),
                ("kappa", _d), ("m5", _d), ("Ls", _i), ("b_5", _d * QUDA_MAX_DWF_LS), ("c_5", _d * QUDA_MAX_DWF_LS), ("mu", _d),
                ("epsilon", _d), ("twist_flavor", _i), ("tol", _d), ("tol_restart", _d), ("tol_hq", _d), ("true_res", _d),
                ("true_res_hq", _d), ("maxiter", _i), ("reliable_delta", _d), ("use_sloppy_partial_accumulator", _i),
                ("max_res_increase", _i), ("max_res_increase_total", _i), ("heavy_quark_check", _i), ("pipeline", _i),
                ("num_offset", _i), ("num_src", _i), ("overlap", _i), ("offset", _d * QUDA_MAX_MULTI_SHIFT),
                ("tol_offset", _d * QUDA_MAX_MULTI_SHIFT), ("tol_hq_offset", _d * QUDA_MAX_MULTI_SHIFT),
                ("true_res_offset", _d * QUDA_MAX_MULTI_SHIFT), ("iter_res_offset", _d * QUDA_MAX_MULTI_SHIFT),
                ("true_res_hq_offset", _d * QUDA_MAX_MULTI_SHIFT), ("solution_type", _i), ("solve_type", _i), ("matpc_type", _i),
                ("dagger", _i), ("mass_normalization", _i), ("solver_normalization", _i), ("preserve_source", _i),
                ("cpu_prec", _i), ("cuda_prec", _i), ("cuda_prec_sloppy", _i), ("cuda_prec_precondition", _i),
                ("dirac_order", _i), ("gamma_basis", _i), ("clover_location", _i), ("clover_cpu_prec", _i),
                ("clover_cuda_prec", _i), ("clover_cuda_prec_sloppy", _i), ("clover_cuda_prec_precondition", _i),
                ("clover_order", _i), ("use_init_guess", _i), ("clover_coeff", _d), ("compute_clover_trlog", _i),
                ("trlogA", _d * 2), ("compute_clover", _i), ("compute_clover_inverse", _i), ("return_clover", _i),
                ("return_clover_inverse", _i), ("verbosity", _i), ("sp_pad", _i), ("cl_pad", _i), ("iter", _i),
                ("spinorGiB", _d), ("cloverGiB", _d), ("gflops", _d), ("secs", _d), ("tune", _i), ("Nsteps", _i),
                ("gcrNkrylov", _i), ("inv_type_precondition", _i), ("preconditioner", _p), ("preconditionerUP", _p),
                ("preconditionerDN", _p), ("dslash_type_precondition", _i), ("verbosity_precondition", _i),
                ("tol_precondition", _d), ("maxiter_precondition", _i), ("omega", _d), ("precondition_cycle", _i),
                ("schwarz_type", _i), ("residual_type", _i), ("cuda_prec_ritz", _i), ("nev", _i), ("max_search_dim", _i),
                ("rhs_idx", _i), ("deflation_grid", _i), ("use_reduced_vector_set", _i), ("eigenval_tol", _d),
                ("use_cg_updates", _i), ("cg_iterref_tol", _d), ("eigcg_max_restarts", _i), ("max_restart_num", _i),
                ("inc_tol", _d), ("make_resident_solution", _i), ("use_resident_solution", _i)]


class QudaMultigridParam(C.Structure):
    _L = QUDA_MAX_MG_LEVEL
    _fields_ = [("invert_param", C.POINTER(QudaInvertParam)), ("n_level", _i), ("geo_block_size", (_i * QUDA_MAX_DIM) * _L),
                ("spin_block_size", _i * _L), ("n_vec", _i * _L), ("smoother", _i * _L), ("coarse_grid_solution_type", _i * _L),
                ("smoother_solve_type", _i * _L), ("cycle_type", _i * _L), ("nu_pre", _i * _L), ("nu_post", _i * _L),
                ("smoother_tol", _d * _L), ("setup_maxiter", _i), ("setup_tol", _d), ("omega", _d * _L),
                ("global_reduction", _i * _L), ("location", _i * _L), ("compute_null_vector", _i), ("generate_all_levels", _i),
                ("run_verify", _i), ("vec_infile", C.c_char * 256), ("vec_outfile", C.c_char * 256), ("gflops", _d), ("secs", _d),
                ("delta_muPR", _d), ("delta_kappaPR", _d), ("delta_cswPR", _d), ("delta_muCG", _d), ("delta_kappaCG", _d),
                ("delta_cswCG", _d)]


# every extern "C" symbol include/quda.h and include/quda_amd_ext.h declare
QUDA_H_SYMBOLS = ["setVerbosityQuda", "initCommsGridQuda", "initQudaDevice", "initQudaMemory", "initQuda", "endQuda",
                  "newQudaGaugeParam", "newQudaInvertParam", "newQudaMultigridParam", "printQudaGaugeParam", "printQudaInvertParam",
                  "printQudaMultigridParam", "loadGaugeQuda", "freeGaugeQuda", "performSTOUTnStep", "qChargeCuda", "computeGaugeForceQuda", "updateGaugeFieldQuda", "projectSU3Quda", "momActionQuda",
                  "computeGaugeFixingOVRQuda",
                  "loadCloverQuda", "freeCloverQuda", "invertQuda", "invertMultiSrcQuda", "invertMultiShiftQuda",
                  "newMultigridQuda", "destroyMultigridQuda", "dslashQuda", "cloverQuda", "MatQuda", "MatDagMatQuda", "openMagma",
                  "closeMagma"]
EXT_H_SYMBOLS = ["qudaAmdSpinorCreate", "qudaAmdSpinorDestroy", "qudaAmdSpinorLoad", "qudaAmdSpinorSave", "qudaAmdSpinorCopy",
                 "qudaAmdSpinorSetTwist", "qudaAmdDiracCreate", "qudaAmdDiracDestroy", "qudaAmdDiracDslash", "qudaAmdDiracDslashXpay",
                 "qudaAmdDiracM", "qudaAmdDiracMdag", "qudaAmdDiracMdagM", "qudaAmdDiracFlops", "qudaAmdTimeDslash", "qudaAmdTimeM",
                 "qudaAmdBlasNorm2", "qudaAmdBlasCDot", "qudaAmdBlasAxpy", "qudaAmdDslashBytesPerSite", "qudaAmdDslashFlopsPerSite",
                 "qudaAmdSetPartitionMask", "qudaAmdComputeStream", "qudaAmdDeviceSynchronize", "qudaAmdHaloTransport", "qudaAmdHaloWireFormat", "qudaAmdSetDslashTune", "qudaAmdCommGetUniqueId",
                 "qudaAmdCommInit", "qudaAmdCommRank", "qudaAmdCommSize", "qudaAmdCommCoords", "qudaAmdCommBarrier", "qudaAmdCommAllreduce", "qudaAmdCommAllreduceMax",
                 "qudaAmdMultigridVerify", "qudaAmdMultigridCycle", "qudaAmdTimeAxpy", "qudaAmdMultigridLevels", "qudaAmdMultigridLevelInfo",
                 "qudaAmdMultigridSetHalfStorage", "qudaAmdMultigridGetNullVector", "qudaAmdMultigridGetV", "qudaAmdMultigridGetCoarseLinks", "qudaAmdMultigridApply", "qudaAmdMultigridApplyTransfer", "qudaAmdMultigridApplyBlock",
                 "qudaAmdMultigridTimeApply", "qudaAmdMultigridTimeTransfer", "qudaAmdSetExitLine", "qudaAmdDiracPrepare", "qudaAmdDiracReconstruct", "qudaAmdSpinorRawInfo", "qudaAmdGaugeRawInfo", "qudaAmdCloverRawInfo", "qudaAmdRawDeviceCopy",
                 "qudaAmdSetSolutionSink", "qudaAmdCommStats", "qudaAmdDescribeHaloError", "qudaAmdMultigridOrthoFallbackBlocks", "qudaAmdProfileMarker", "qudaAmdAccountStart", "qudaAmdAccountDump", "qudaAmdWriteSpinorFields", "qudaAmdReadSpinorFields", "qudaAmdMultigridRefine", "qudaAmdMultigridSetFused", "qudaAmdMultigridFusedStats", "qudaAmdMultiSrcStats", "qudaAmdTwopMomenta", "qudaAmdTwopTimeExtent", "qudaAmdContractTwop", "qudaAmdSetTwopOutput",
                 "qudaAmdLoopMomenta", "qudaAmdContractLoop", "qudaAmdSetLoopOutput", "qudaAmdLoopLastTimings", "qudaAmdMomentumProject",
                 "qudaAmdNewDeflation", "qudaAmdDestroyDeflation", "qudaAmdDeflationInfo", "qudaAmdDeflationTimings", "qudaAmdDeflationGetVector", "qudaAmdDeflationProject",
                 "qudaAmdDeflationExactLoop", "qudaAmdHostSymmetricEig", "qudaAmdGcrBackSubstitute", "qudaAmdRotateBasis", "qudaAmdBlockDot", "qudaAmdBlockAxpy", "qudaAmdLastEigenvalues",
                 "qudaAmdBlasAxpyCGNorm", "qudaAmdBlasAxpyZpbx", "qudaAmdBlasTripleCGReduction", "qudaAmdBlasAxpyReDot", "qudaAmdBlasMultiShiftUpdate",
                 "qudaAmdBlasMultiShiftChunk", "qudaAmdDiracMdagMShift", "qudaAmdTimeMdagM", "qudaAmdTimeCGBlas", "qudaAmdTimeMultiShift",
                 "qudaAmdNdegTwist", "qudaAmdStoutSmear", "qudaAmdQCharge", "qudaAmdSu3ExpIQ",
                 "qudaAmdBlasApply", "qudaAmdBlasDevUpdate", "qudaAmdBlasMultiSupported", "qudaAmdBlasMultiDot", "qudaAmdBlasMultiCaxpyResidual",
                 "qudaAmdBlasMultiCaxpy", "qudaAmdBlasHeavyQuarkResidualNorm",
                 "qudaAmdBlockFieldCreate", "qudaAmdBlockFieldDestroy", "qudaAmdBlockFieldLoad", "qudaAmdBlockFieldSave", "qudaAmdBlockBlasApply",
                 "qudaAmdBlockMrUpdate", "qudaAmdBlockPack", "qudaAmdBlockUnpack", "qudaAmdBlockPackParity", "qudaAmdBlockUnpackParity",
                 "qudaAmdBlockGhostPanels", "qudaAmdBlockFineApply", "qudaAmdCloverTwistDense", "qudaAmdBlockFineApplySite",
                 "qudaAmdMultigridGetCoarseSiteLinks", "qudaAmdMultigridCoarseApply", "qudaAmdMultigridCoarsePC", "qudaAmdCoarseInvertSites",
                 "qudaAmdFermionOprodForce", "qudaAmdComputeTMForce", "qudaAmdFermForceLastKernelSecs",
                 "qudaAmdCloverSigmaOprod", "qudaAmdCloverSigmaTrace", "qudaAmdCloverDerivativeForce", "qudaAmdCloverLogDetForce",
                 "qudaAmdGaugeFixOVR", "qudaAmdGaugeFixQuality"]

_lib = None


class QudaAmdSourceParam(C.Structure):
    """include/quda_amd_ext.h: the source description of the QKXTM solve loop"""
    _fields_ = [("sourcePosition", C.c_int * 4), ("nsmearGauss", C.c_int), ("alphaGauss", C.c_double)]


class QudaAmdTwopParam(C.Structure):
    """include/quda_amd_ext.h: source and sink description of the two-point contractions"""
    _fields_ = [("sourcePosition", C.c_int * 4), ("Q_sq", C.c_int), ("nsmearGauss", C.c_int), ("alphaGauss", C.c_double)]


class QudaAmdThreepParam(C.Structure):
    """include/quda_amd_ext.h: source, sink, projector and flavour assignment of the three-point functions"""
    _fields_ = [("sourcePosition", C.c_int * 4), ("Q_sq", C.c_int), ("tsinkSource", C.c_int), ("projector", C.c_int), ("particle", C.c_int),
                ("part", C.c_int), ("nsmearGauss", C.c_int), ("alphaGauss", C.c_double)]


class QudaAmdEigParam(C.Structure):
    """include/quda_amd_ext.h: the thick-restart Lanczos eigensolver behind the exact deflation of the loops"""
    _fields_ = [("nEv", C.c_int), ("nKv", C.c_int), ("PolyDeg", C.c_int), ("isACC", C.c_int), ("maxRestarts", C.c_int),
                ("amin", C.c_double), ("amax", C.c_double), ("tol", C.c_double)]


# include/qudaQKXTM_Kepler_utils.h: enum WHICHPARTICLE, enum WHICHPROJECTOR
PROTON, NEUTRON = 0, 1
G4, G5G123, G5G1, G5G2, G5G3 = 0, 1, 2, 3, 4


def lib():
    """The loaded libquda.so; raises if the HIP extension has not been built (no fallback)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError("%s is missing: build it with `make -C %s` (or __graft_entry__.build()); "
                               "there is no CPU fallback" % (LIB_PATH, _HERE))
        L = C.CDLL(LIB_PATH, mode=C.RTLD_GLOBAL)
        L.newQudaGaugeParam.restype = QudaGaugeParam
        L.newQudaInvertParam.restype = QudaInvertParam
        L.newQudaMultigridParam.restype = QudaMultigridParam
        L.newMultigridQuda.restype = _p
        L.newMultigridQuda.argtypes = [C.POINTER(QudaMultigridParam)]
        L.destroyMultigridQuda.argtypes = [_p]
        for name in ("qudaAmdSpinorCreate", "qudaAmdDiracCreate", "qudaAmdComputeStream"):
            getattr(L, name).restype = _p
        L.qudaAmdSpinorCreate.argtypes = [_i, _i, _i]
        L.qudaAmdSpinorDestroy.argtypes = [_p]
        L.qudaAmdSpinorLoad.argtypes = [_p, _p, C.POINTER(QudaInvertParam)]
        L.qudaAmdSpinorSave.argtypes = [_p, _p, C.POINTER(QudaInvertParam)]
        L.qudaAmdSpinorCopy.argtypes = [_p, _p]
        L.qudaAmdSpinorSetTwist.argtypes = [_p, _i]
        if hasattr(L, "qudaAmdNdegTwist"):   # absent from a build of an earlier commit loaded through QUDA_AMD_LIBRARY (tools/ndeg_timing.py --parent-lib)
            L.qudaAmdNdegTwist.argtypes = [_p, _p, _d, _d, _d, _i, _i]
            L.qudaAmdNdegTwist.restype = None
        L.qudaAmdDiracCreate.argtypes = [C.POINTER(QudaInvertParam), _i, _i]
        L.qudaAmdDiracDestroy.argtypes = [_p]
        L.qudaAmdDiracDslash.argtypes = [_p, _p, _p, _i]
        L.qudaAmdDiracDslashXpay.argtypes = [_p, _p, _p, _i, _p, _d]
        for name in ("qudaAmdDiracM", "qudaAmdDiracMdag", "qudaAmdDiracMdagM"):
            getattr(L, name).argtypes = [_p, _p, _p]
        L.qudaAmdDiracFlops.argtypes = [_p]
        L.qudaAmdDiracFlops.restype = C.c_ulonglong
        L.qudaAmdTimeDslash.argtypes = [_p, _p, _p, _i, _i]
        L.qudaAmdTimeDslash.restype = _d
        L.qudaAmdTimeM.argtypes = [_p, _p, _p, _i]
        L.qudaAmdTimeM.restype = _d
        L.qudaAmdBlasNorm2.argtypes = [_p]
        L.qudaAmdBlasNorm2.restype = _d
        L.qudaAmdBlasCDot.argtypes = [_p, _p, C.POINTER(_d)]
        L.qudaAmdBlasAxpy.argtypes = [_d, _p, _p]
        L.qudaAmdDslashBytesPerSite.argtypes = [C.POINTER(QudaInvertParam), _i, _i]
        L.qudaAmdDslashBytesPerSite.restype = C.c_longlong
        L.qudaAmdDslashFlopsPerSite.argtypes = [C.POINTER(QudaInvertParam), _i]
        L.qudaAmdDslashFlopsPerSite.restype = C.c_longlong
        L.dslashQuda.argtypes = [_p, _p, C.POINTER(QudaInvertParam), _i]
        L.MatQuda.argtypes = [_p, _p, C.POINTER(QudaInvertParam)]
        L.MatDagMatQuda.argtypes = [_p, _p, C.POINTER(QudaInvertParam)]
        L.invertQuda.argtypes = [_p, _p, C.POINTER(QudaInvertParam)]
        L.invertMultiSrcQuda.argtypes = [_p, _p, C.POINTER(QudaInvertParam)]
        L.invertMultiSrcQuda.restype = None
        L.invertMultiShiftQuda.argtypes = [_p, _p, C.POINTER(QudaInvertParam)]
        L.invertMultiShiftQuda.restype = None
        L.qudaAmdBlasAxpyCGNorm.argtypes = [_d, _p, _p, C.POINTER(_d)]
        L.qudaAmdBlasAxpyCGNorm.restype = None
        L.qudaAmdBlasAxpyZpbx.argtypes = [_d, _p, _p, _p, _d]
        L.qudaAmdBlasAxpyZpbx.restype = None
        L.qudaAmdBlasTripleCGReduction.argtypes = [_p, _p, _p, C.POINTER(_d)]
        L.qudaAmdBlasTripleCGReduction.restype = None
        L.qudaAmdBlasAxpyReDot.argtypes = [_d, _p, _p]
        L.qudaAmdBlasAxpyReDot.restype = _d
        L.qudaAmdBlasMultiShiftUpdate.argtypes = [_i, C.POINTER(_p), C.POINTER(_p), _p, C.POINTER(_d), C.POINTER(_d), C.POINTER(_d)]
        L.qudaAmdBlasMultiShiftUpdate.restype = None
        L.qudaAmdBlasMultiShiftChunk.argtypes = []
        L.qudaAmdBlasMultiShiftChunk.restype = _i
        L.qudaAmdBlasApply.argtypes = [C.c_char_p, C.POINTER(_d), _p, _p, _p, _p, C.POINTER(_d)]
        L.qudaAmdBlasApply.restype = _i
        L.qudaAmdBlasDevUpdate.argtypes = [C.c_char_p, _d, _p, _p, _p, _p, _p, _p]
        L.qudaAmdBlasDevUpdate.restype = None
        L.qudaAmdBlasMultiSupported.argtypes = [_p, _i]
        L.qudaAmdBlasMultiSupported.restype = _i
        L.qudaAmdBlasMultiDot.argtypes = [_i, C.POINTER(_p), _p, _p, C.POINTER(_d), C.POINTER(_d), C.POINTER(_d)]
        L.qudaAmdBlasMultiDot.restype = None
        L.qudaAmdBlasMultiCaxpyResidual.argtypes = [_i, C.POINTER(_p), C.POINTER(_d), _d, _p, C.POINTER(_d), _p, C.POINTER(_d)]
        L.qudaAmdBlasMultiCaxpyResidual.restype = None
        L.qudaAmdBlasMultiCaxpy.argtypes = [_i, C.POINTER(_p), C.POINTER(_d), _p]
        L.qudaAmdBlasMultiCaxpy.restype = None
        L.qudaAmdBlasHeavyQuarkResidualNorm.argtypes = [_p, _p, C.POINTER(_d)]
        L.qudaAmdBlasHeavyQuarkResidualNorm.restype = None
        if hasattr(L, "qudaAmdBlockFieldCreate"):   # absent from a build of an earlier commit loaded through QUDA_AMD_LIBRARY
            L.qudaAmdBlockFieldCreate.argtypes = [_i, _i, _i, _i]
            L.qudaAmdBlockFieldCreate.restype = _p
            L.qudaAmdBlockFieldDestroy.argtypes = [_p]
            L.qudaAmdBlockFieldDestroy.restype = None
            L.qudaAmdBlockFieldLoad.argtypes = [_p, _p]
            L.qudaAmdBlockFieldLoad.restype = None
            L.qudaAmdBlockFieldSave.argtypes = [_p, _p]
            L.qudaAmdBlockFieldSave.restype = None
            L.qudaAmdBlockBlasApply.argtypes = [C.c_char_p, _p, _p, _p, _p, _p, _p, _p, _p, _p]
            L.qudaAmdBlockBlasApply.restype = _i
            L.qudaAmdBlockMrUpdate.argtypes = [_i, _d, _i, _i, _p, _p, _p, _p, _p, _p, _p]
            L.qudaAmdBlockMrUpdate.restype = None
            for name in ("qudaAmdBlockPack", "qudaAmdBlockUnpack", "qudaAmdBlockPackParity"):
                getattr(L, name).argtypes = [_p, C.POINTER(_p), _i, _i]
                getattr(L, name).restype = None
            L.qudaAmdBlockUnpackParity.argtypes = [_p, C.POINTER(_p), _i]
            L.qudaAmdBlockUnpackParity.restype = None
            L.qudaAmdBlockGhostPanels.argtypes = [_i]
            L.qudaAmdBlockGhostPanels.restype = _i
            L.qudaAmdBlockFineApply.argtypes = [_p, _p, _p, _p, _i, _d, _d, _d, _d, _i, _i, _p]
            L.qudaAmdBlockFineApply.restype = None
        if hasattr(L, "qudaAmdBlockFineApplySite"):
            L.qudaAmdCloverTwistDense.argtypes = [_i, _d, _i, _p]
            L.qudaAmdCloverTwistDense.restype = None
            L.qudaAmdBlockFineApplySite.argtypes = [_p, _p, _p, _i, _d, _d, _d, _d, _i, _d, _i]
            L.qudaAmdBlockFineApplySite.restype = _i
        L.qudaAmdDiracMdagMShift.argtypes = [_p, _p, _p, _d]
        L.qudaAmdDiracMdagMShift.restype = None
        L.qudaAmdTimeMdagM.argtypes = [_p, _p, _p, _i]
        L.qudaAmdTimeMdagM.restype = _d
        L.qudaAmdTimeCGBlas.argtypes = [_i, _p, _p, _p, _p, _i]
        L.qudaAmdTimeCGBlas.restype = _d
        L.qudaAmdTimeMultiShift.argtypes = [_i, _i, C.POINTER(_p), C.POINTER(_p), _p, _i]
        L.qudaAmdTimeMultiShift.restype = _d
        L.cloverQuda.argtypes = [_p, _p, C.POINTER(QudaInvertParam), C.POINTER(_i), _i]
        L.loadGaugeQuda.argtypes = [_p, C.POINTER(QudaGaugeParam)]
        L.loadCloverQuda.argtypes = [_p, _p, C.POINTER(QudaInvertParam)]
        L.qudaAmdCommInit.argtypes = [_p, _i, _i]
        L.qudaAmdCommGetUniqueId.argtypes = [_p]
        L.initCommsGridQuda.argtypes = [_i, C.POINTER(_i), _p, _p]
        L.qudaAmdSetPartitionMask.argtypes = [_i]
        L.qudaAmdSpinorRawInfo.argtypes = [_p, C.POINTER(C.c_longlong)]
        L.qudaAmdGaugeRawInfo.argtypes = [_i, C.POINTER(C.c_longlong)]
        L.qudaAmdCloverRawInfo.argtypes = [_i, C.POINTER(C.c_longlong)]
        L.qudaAmdRawDeviceCopy.argtypes = [_p, C.c_longlong, C.c_size_t]
        L.qudaAmdSetDslashTune.argtypes = [C.c_char_p, _i]
        L.qudaAmdMultigridVerify.argtypes = [_p, C.POINTER(_d)]
        L.qudaAmdMultigridCycle.argtypes = [_p, _p, _p, C.POINTER(QudaInvertParam)]
        L.qudaAmdTimeAxpy.argtypes = [_d, _p, _p, _i]
        L.qudaAmdTimeAxpy.restype = _d
        L.qudaAmdMultigridSetHalfStorage.argtypes = [_p, _i]
        L.qudaAmdMultigridLevels.argtypes = [_p]
        L.qudaAmdMultigridOrthoFallbackBlocks.argtypes = [_p, _i]
        L.qudaAmdMultigridRefine.argtypes = [_p, _i, _i]
        L.qudaAmdMultigridRefine.restype = _d
        L.qudaAmdProfileMarker.argtypes = [_i]
        L.qudaAmdAccountDump.argtypes = [C.c_char_p]
        L.qudaAmdCommStats.argtypes = [C.POINTER(C.c_longlong)]
        L.qudaAmdDescribeHaloError.argtypes = [C.c_char_p, _i]
        L.qudaAmdMultigridLevelInfo.argtypes = [_p, _i, C.POINTER(_i)]
        L.qudaAmdMultigridGetNullVector.argtypes = [_p, _i, _i, _p]
        L.qudaAmdMultigridGetV.argtypes = [_p, _i, _p]
        L.qudaAmdMultigridGetCoarseLinks.argtypes = [_p, _i, _p, _p]
        L.qudaAmdMultigridApply.argtypes = [_p, _i, _i, _p, _p]
        L.qudaAmdMultigridApplyTransfer.argtypes = [_p, _i, _i, _i, _p, _p]
        L.qudaAmdMultigridGetCoarseSiteLinks.argtypes = [_p, _i, _i, _p]
        L.qudaAmdMultigridGetCoarseSiteLinks.restype = None
        L.qudaAmdMultigridCoarseApply.argtypes = [_p, _i, _i, _i, _i, _p, _p]
        L.qudaAmdMultigridCoarseApply.restype = _i
        L.qudaAmdMultigridCoarsePC.argtypes = [_p, _i, _i, _i, _i, _i, _p, _p]
        L.qudaAmdMultigridCoarsePC.restype = _i
        L.qudaAmdCoarseInvertSites.argtypes = [_i, _i, _p, _p, _p, _p, C.POINTER(_i)]
        L.qudaAmdCoarseInvertSites.restype = None
        L.qudaAmdMultigridSetFused.argtypes = [_i]
        L.qudaAmdMultigridSetFused.restype = None
        L.qudaAmdMultigridFusedStats.argtypes = [_p, _i, _p]
        L.qudaAmdMultigridFusedStats.restype = _i
        L.qudaAmdMultigridApplyBlock.argtypes = [_p, _i, _i, _p, _p, _i]
        L.qudaAmdMultigridApplyBlock.restype = _d
        L.qudaAmdMultigridTimeApply.argtypes = [_p, _i, _i]
        L.qudaAmdMultigridTimeApply.restype = _d
        L.qudaAmdMultigridTimeTransfer.argtypes = [_p, _i, _i, _i]
        L.qudaAmdMultigridTimeTransfer.restype = _d
        L.qudaAmdSetExitLine.argtypes = [C.c_char_p, _i]
        L.qudaAmdSetExitLine.restype = None
        L.qudaAmdDiracPrepare.argtypes = [_p, _p, _p, _p, _i]
        L.qudaAmdDiracPrepare.restype = None
        L.qudaAmdDiracReconstruct.argtypes = [_p, _p, _p, _i]
        L.qudaAmdDiracReconstruct.restype = None
        L.qudaAmdReadLimeGauge.argtypes = [C.POINTER(_p), C.c_char_p, C.POINTER(QudaGaugeParam), C.POINTER(QudaInvertParam), C.POINTER(_i)]
        L.qudaAmdWriteLimeGauge.argtypes = [C.POINTER(_p), C.c_char_p, C.POINTER(QudaGaugeParam), C.c_char_p]
        L.plaqQuda.argtypes = [C.POINTER(_d)]
        L.performAPEnStep.argtypes = [C.c_uint, _d]
        L.performSTOUTnStep.argtypes = [C.c_uint, _d]
        L.performSTOUTnStep.restype = None
        L.qChargeCuda.argtypes = []
        L.qChargeCuda.restype = _d
        L.qudaAmdStoutSmear.argtypes = [C.c_uint, _d, _i]
        L.qudaAmdStoutSmear.restype = None
        L.qudaAmdQCharge.argtypes = [_p, _i, _i]
        L.qudaAmdQCharge.restype = _d
        L.qudaAmdSu3ExpIQ.argtypes = [_i, _p, _p]
        L.qudaAmdSu3ExpIQ.restype = None
        L.saveGaugeQuda.argtypes = [_p, C.POINTER(QudaGaugeParam)]
        L.qudaAmdSaveSmearedGauge.argtypes = [C.POINTER(_p), _i]
        L.computeGaugeForceQuda.argtypes = [_p, _p, C.POINTER(C.POINTER(C.POINTER(_i))), C.POINTER(_i), C.POINTER(_d), _i, _i, _d, C.POINTER(QudaGaugeParam)]
        L.computeGaugeForceQuda.restype = _i
        L.updateGaugeFieldQuda.argtypes = [_p, _p, _d, _i, _i, C.POINTER(QudaGaugeParam)]
        L.updateGaugeFieldQuda.restype = None
        L.projectSU3Quda.argtypes = [_p, _d, C.POINTER(QudaGaugeParam)]
        L.projectSU3Quda.restype = None
        L.momActionQuda.argtypes = [_p, C.POINTER(QudaGaugeParam)]
        L.momActionQuda.restype = _d
        _u = C.c_uint
        L.computeGaugeFixingOVRQuda.argtypes = [_p, _u, _u, _u, _d, _d, _u, _u, C.POINTER(QudaGaugeParam), C.POINTER(_d)]
        L.computeGaugeFixingOVRQuda.restype = _i
        L.qudaAmdGaugeFixOVR.argtypes = [_p, _u, _u, _u, _d, _d, _u, _u, C.POINTER(QudaGaugeParam), C.POINTER(_d), _p, C.POINTER(_d)]
        L.qudaAmdGaugeFixOVR.restype = _i
        L.qudaAmdGaugeFixQuality.argtypes = [_u, C.POINTER(_d)]
        L.qudaAmdGaugeFixQuality.restype = None
        L.qudaAmdFermionOprodForce.argtypes = [_p, C.POINTER(_p), C.POINTER(_p), C.POINTER(_d), _i, C.POINTER(QudaGaugeParam), C.POINTER(QudaInvertParam)]
        L.qudaAmdFermionOprodForce.restype = None
        L.qudaAmdComputeTMForce.argtypes = [_p, _d, C.POINTER(_p), C.POINTER(_d), _i, C.POINTER(QudaGaugeParam), C.POINTER(QudaInvertParam)]
        L.qudaAmdComputeTMForce.restype = None
        L.qudaAmdFermForceLastKernelSecs.argtypes = []
        L.qudaAmdFermForceLastKernelSecs.restype = _d
        L.qudaAmdCloverSigmaOprod.argtypes = [C.POINTER(_d), C.POINTER(_p), C.POINTER(_p), C.POINTER(_d), _i, C.POINTER(QudaInvertParam)]
        L.qudaAmdCloverSigmaOprod.restype = None
        L.qudaAmdCloverSigmaTrace.argtypes = [C.POINTER(_d), _d, _d, C.POINTER(QudaInvertParam)]
        L.qudaAmdCloverSigmaTrace.restype = None
        L.qudaAmdCloverDerivativeForce.argtypes = [_p, C.POINTER(_d), _d, C.POINTER(QudaGaugeParam)]
        L.qudaAmdCloverDerivativeForce.restype = None
        L.qudaAmdCloverLogDetForce.argtypes = [_p, _d, _d, _d, C.POINTER(QudaGaugeParam), C.POINTER(QudaInvertParam)]
        L.qudaAmdCloverLogDetForce.restype = None
        L.qudaAmdGaussianSmear.argtypes = [_p, _p, C.POINTER(_p), _i, _d]
        L.qudaAmdCalcMGPropagators.argtypes = [_p, _p, C.POINTER(_p), C.POINTER(QudaInvertParam), C.POINTER(QudaAmdSourceParam)]
        L.qudaAmdTwopMomenta.argtypes = [_i, C.POINTER(_i), _i]
        L.qudaAmdTwopMomenta.restype = _i
        L.qudaAmdTwopTimeExtent.argtypes = []
        L.qudaAmdTwopTimeExtent.restype = _i
        L.qudaAmdContractTwop.argtypes = [_p, _p, _p, _p, C.POINTER(_p), C.POINTER(QudaAmdTwopParam)]
        L.qudaAmdContractTwop.restype = None
        L.qudaAmdSetTwopOutput.argtypes = [_i]
        L.qudaAmdSetTwopOutput.restype = None
        L.qudaAmdLoopMomenta.argtypes = [C.POINTER(_i), _i, C.POINTER(_i), _i]
        L.qudaAmdLoopMomenta.restype = _i
        L.qudaAmdContractLoop.argtypes = [_p, _p, C.POINTER(QudaInvertParam), _i]
        L.qudaAmdContractLoop.restype = None
        L.qudaAmdSetLoopOutput.argtypes = [_i]
        L.qudaAmdSetLoopOutput.restype = None
        L.qudaAmdLoopLastTimings.argtypes = [C.POINTER(_d)]
        L.qudaAmdLoopLastTimings.restype = None
        L.qudaAmdMomentumProject.argtypes = [_p, _p, _i, _i, _i, _i, C.POINTER(_i), _i, C.POINTER(_i), C.POINTER(_i), C.POINTER(_i)]
        L.qudaAmdMomentumProject.restype = None
        L.qudaAmdNewDeflation.argtypes = [C.POINTER(QudaInvertParam), C.POINTER(QudaAmdEigParam)]
        L.qudaAmdNewDeflation.restype = _p
        L.qudaAmdDestroyDeflation.argtypes = [_p]
        L.qudaAmdDestroyDeflation.restype = None
        L.qudaAmdDeflationInfo.argtypes = [_p, C.POINTER(_d), C.POINTER(_d), C.POINTER(_i), C.POINTER(_i)]
        L.qudaAmdDeflationInfo.restype = _i
        L.qudaAmdDeflationTimings.argtypes = [_p, C.POINTER(_d)]
        L.qudaAmdDeflationTimings.restype = None
        L.qudaAmdDeflationGetVector.argtypes = [_p, _i, _p]
        L.qudaAmdDeflationGetVector.restype = None
        L.qudaAmdDeflationProject.argtypes = [_p, _i, _p, _p]
        L.qudaAmdDeflationProject.restype = None
        L.qudaAmdDeflationExactLoop.argtypes = [_p, _i, _p, _i]
        L.qudaAmdDeflationExactLoop.restype = None
        L.qudaAmdHostSymmetricEig.argtypes = [_i, _p, _p, _p]
        L.qudaAmdHostSymmetricEig.restype = None
        if hasattr(L, "qudaAmdGcrBackSubstitute"):   # absent from a build of an earlier commit loaded through QUDA_AMD_LIBRARY
            L.qudaAmdGcrBackSubstitute.argtypes = [_i, _i, _p, _p, _p, _p]
            L.qudaAmdGcrBackSubstitute.restype = None
        L.qudaAmdRotateBasis.argtypes = [_p, _i, _i, _p, C.POINTER(_i)]
        L.qudaAmdRotateBasis.restype = None
        L.qudaAmdBlockDot.argtypes = [_p, _p, _i, _p, C.POINTER(_i)]
        L.qudaAmdBlockDot.restype = None
        L.qudaAmdBlockAxpy.argtypes = [_p, _p, _p, _i, C.POINTER(_i)]
        L.qudaAmdBlockAxpy.restype = None
        L.qudaAmdLastEigenvalues.argtypes = [C.POINTER(_d), _i]
        L.qudaAmdLastEigenvalues.restype = _i
        L.qudaAmdThreepSeqSource.argtypes = [_p, _p, _p, C.POINTER(_p), C.POINTER(QudaAmdThreepParam)]
        L.qudaAmdThreepSeqSource.restype = None
        L.qudaAmdContractThreep.argtypes = [_p, _p, _p, _p, _p, C.POINTER(_p), C.POINTER(QudaAmdThreepParam)]
        L.qudaAmdContractThreep.restype = None
        L.qudaAmdThreepOperator.argtypes = [_i, _i, C.POINTER(_d)]
        L.qudaAmdThreepOperator.restype = None
        L.qudaAmdThreepProjector.argtypes = [_i, _i, C.POINTER(_d)]
        L.qudaAmdThreepProjector.restype = None
        L.qudaAmdSetThreepOutput.argtypes = [_i]
        L.qudaAmdSetThreepOutput.restype = None
        L.qudaAmdThreepLastTimings.argtypes = [C.POINTER(_d)]
        L.qudaAmdThreepLastTimings.restype = None
        _lib = L
    return _lib


def _vp(a):
    return a.ctypes.data_as(_p) if a is not None else None


# ---- helpers written the way the reference's tests set things up (tests/dslash_test.cpp:84-200) ----
def gauge_param(X, cpu_prec=QUDA_DOUBLE_PRECISION, cuda_prec=QUDA_DOUBLE_PRECISION, recon=QUDA_RECONSTRUCT_NO,
                prec_sloppy=None, recon_sloppy=None, prec_precondition=None, t_boundary=QUDA_ANTI_PERIODIC_T, recon_precondition=None):
    gp = lib().newQudaGaugeParam()
    for d in range(4):
        gp.X[d] = int(X[d])
    gp.anisotropy = 1.0
    gp.type = QUDA_WILSON_LINKS
    gp.gauge_order = QUDA_QDP_GAUGE_ORDER
    gp.t_boundary = t_boundary
    gp.cpu_prec = cpu_prec
    gp.cuda_prec = cuda_prec
    gp.reconstruct = recon
    gp.cuda_prec_sloppy = prec_sloppy or cuda_prec
    gp.reconstruct_sloppy = recon_sloppy or recon
    gp.cuda_prec_precondition = prec_precondition or gp.cuda_prec_sloppy
    gp.reconstruct_precondition = recon_precondition or gp.reconstruct_sloppy
    gp.gauge_fix = QUDA_GAUGE_FIXED_NO
    gp.ga_pad = 0
    return gp


def invert_param(dslash_type=QUDA_TWISTED_MASS_DSLASH, kappa=0.1, mu=0.01, flavor=QUDA_TWIST_PLUS, matpc="ee", dagger=0,
                 cpu_prec=QUDA_DOUBLE_PRECISION, cuda_prec=QUDA_DOUBLE_PRECISION, prec_sloppy=None, prec_precondition=None,
                 solution_type=QUDA_MATPC_SOLUTION, gamma_basis=QUDA_DEGRAND_ROSSI_GAMMA_BASIS, dirac_order=QUDA_DIRAC_ORDER, epsilon=0.0):
    ip = lib().newQudaInvertParam()
    ip.dslash_type = dslash_type
    ip.kappa = kappa
    ip.mu = mu
    ip.epsilon = epsilon   # flavour splitting of the non-degenerate doublet (flavor=QUDA_TWIST_NONDEG_DOUBLET)
    ip.mass = 0.5 / kappa - 4.0
    ip.twist_flavor = flavor if dslash_type != QUDA_WILSON_DSLASH else QUDA_TWIST_NO
    ip.matpc_type = MATPC[matpc] if isinstance(matpc, str) else matpc
    ip.dagger = dagger
    ip.solution_type = solution_type
    ip.solve_type = QUDA_DIRECT_PC_SOLVE
    ip.mass_normalization = QUDA_KAPPA_NORMALIZATION
    ip.cpu_prec = cpu_prec
    ip.cuda_prec = cuda_prec
    ip.cuda_prec_sloppy = prec_sloppy or cuda_prec
    ip.cuda_prec_precondition = prec_precondition or ip.cuda_prec_sloppy
    ip.gamma_basis = gamma_basis
    ip.dirac_order = dirac_order
    ip.clover_cpu_prec = cpu_prec
    ip.clover_cuda_prec = cuda_prec
    ip.clover_cuda_prec_sloppy = ip.cuda_prec_sloppy
    ip.clover_cuda_prec_precondition = ip.cuda_prec_precondition
    ip.clover_order = QUDA_PACKED_CLOVER_ORDER
    ip.clover_coeff = 0.0
    ip.input_location = ip.output_location = QUDA_CPU_FIELD_LOCATION
    ip.tune = QUDA_TUNE_NO
    ip.sp_pad = ip.cl_pad = 0
    ip.verbosity = QUDA_SILENT
    ip.inv_type = QUDA_GCR_INVERTER
    ip.inv_type_precondition = QUDA_INVALID_ENUM
    ip.tol = 1e-10
    ip.maxiter = 1000
    ip.reliable_delta = 1e-4
    ip.gcrNkrylov = 20
    ip.use_init_guess = QUDA_USE_INIT_GUESS_NO
    ip.preserve_source = QUDA_PRESERVE_SOURCE_YES
    ip.residual_type = QUDA_L2_RELATIVE_RESIDUAL
    return ip


COMM_STATS_KEYS = ("fine_peer_store_exchanges", "fine_staged_exchanges", "coarse_peer_store_exchanges", "coarse_staged_exchanges",
                   "in_kernel_allreduces", "collective_allreduces", "fallbacks_to_staged", "block_exchanges")


def comm_stats():
    """this process' transport counters since initQuda (include/quda_amd_ext.h qudaAmdCommStats)"""
    a = (C.c_longlong * 8)()
    lib().qudaAmdCommStats(a)
    return dict(zip(COMM_STATS_KEYS, [int(v) for v in a]))


def halo_error_text():
    buf = C.create_string_buffer(1024)
    return buf.value.decode() if lib().qudaAmdDescribeHaloError(buf, 1024) else None


def init(device=0, verbosity=QUDA_SILENT):
    lib().setVerbosityQuda(verbosity, b"", None)
    lib().initQuda(int(device))


def end():
    lib().endQuda()


def load_gauge(gauge, gp):
    """gauge: (4, V*18) float64/float32 array in QDP order (even sites then odd)."""
    gauge = np.ascontiguousarray(gauge)
    ptrs = (_p * 4)(*[gauge[d].ctypes.data_as(_p) for d in range(4)])
    lib().loadGaugeQuda(C.cast(ptrs, _p), C.byref(gp))
    return gp


def load_clover(clover, clover_inv, ip):
    """loadCloverQuda; clover = clover_inv = None: the clover term is built on the device from the resident links with
    ip.clover_coeff (reference lib/interface_quda.cpp:743-747)"""
    lib().loadCloverQuda(_vp(clover) if clover is not None else None, _vp(clover_inv) if clover_inv is not None else None, C.byref(ip))


def dslash(h_in, ip, parity):
    out = np.empty_like(h_in)
    lib().dslashQuda(_vp(out), _vp(h_in), C.byref(ip), int(parity))
    return out


def mat(h_in, ip):
    out = np.empty_like(h_in)
    lib().MatQuda(_vp(out), _vp(h_in), C.byref(ip))
    return out


def matdagmat(h_in, ip):
    out = np.empty_like(h_in)
    lib().MatDagMatQuda(_vp(out), _vp(h_in), C.byref(ip))
    return out


def invert(h_b, ip, out=None):
    """invertQuda; out: an existing solution array of the caller (as a C caller has one) — a fresh numpy array is untouched memory, and its page
    faults (0.1 s for the 2 GB solution of a 48^3 x 96 lattice) would be charged to the download of the solution"""
    x = np.zeros_like(h_b) if out is None else out
    lib().invertQuda(_vp(x), _vp(h_b), C.byref(ip))
    return x


def invert_multi_shift(h_b, ip, offsets, tols, out=None):
    """invertMultiShiftQuda: (A + offsets[i]) x_i = h_b, A = M^dag M of ip (NORMOP solve types, CG), for ascending offsets with the
    tolerances tols[i]; returns the list of solutions.  ip.num_offset, ip.offset[] and ip.tol_offset[] are set here; the per-shift
    residuals are left in ip.true_res_offset[] / ip.iter_res_offset[], the total iteration count in ip.iter"""
    n = len(offsets)
    if len(tols) != n or not 1 <= n <= QUDA_MAX_MULTI_SHIFT:
        raise ValueError("one tolerance per offset, 1 <= number of offsets <= %d" % QUDA_MAX_MULTI_SHIFT)
    b = np.ascontiguousarray(h_b)
    xs = out if out is not None else [np.zeros_like(b) for _ in range(n)]
    if len(xs) != n or any(x.shape != b.shape or x.dtype != b.dtype or not x.flags.c_contiguous for x in xs):
        raise ValueError("out must hold one contiguous array per offset, of the source's shape and type")
    ip.num_offset = n
    for i in range(n):
        ip.offset[i], ip.tol_offset[i] = float(offsets[i]), float(tols[i])
    px = (_p * n)(*[_vp(x) for x in xs])
    lib().invertMultiShiftQuda(px, _vp(b), C.byref(ip))
    return xs


def multi_shift_chunk():
    """qudaAmdBlasMultiShiftChunk: shifts one sweep of Spinor.multi_shift_update covers"""
    return int(lib().qudaAmdBlasMultiShiftChunk())


def multi_shift_update(x, p, r, alpha, beta, zeta):
    """qudaAmdBlasMultiShiftUpdate on lists of Spinor: x[i] += alpha[i] p[i] ; p[i] = zeta[i] r + beta[i] p[i]"""
    k = len(x)
    if not (len(p) == len(alpha) == len(beta) == len(zeta) == k):
        raise ValueError("x, p, alpha, beta, zeta must have one entry per shift")
    hx, hp = (_p * max(k, 1))(*[f.h for f in x]), (_p * max(k, 1))(*[f.h for f in p])
    a, b, z = [(_d * max(k, 1))(*[float(v) for v in c]) for c in (alpha, beta, zeta)]
    lib().qudaAmdBlasMultiShiftUpdate(k, hx, hp, r.h, a, b, z)


def blas_apply(op, coeff=(), x=None, y=None, z=None, w=None):
    """qudaAmdBlasApply: the function of namespace blas named op (include/blas.h) on Spinors named as there; coeff as quda_amd_ext.h lays
    it out (complex a, complex b as four reals; real a, b first; cabxpyAx: a, unused, re b, im b).  Returns the tuple of its sums"""
    c = (_d * 4)(*([float(v) for v in coeff] + [0.0] * (4 - len(coeff))))
    r = (_d * 3)()
    n = lib().qudaAmdBlasApply(op.encode(), c, *[f.h if f is not None else None for f in (x, y, z, w)], r)
    return tuple(r[i] for i in range(n))


def blas_dev_update(op, omega, p, q, x, y, z, w=None):
    """qudaAmdBlasDevUpdate: cDotProductNormADev(p, q), then caxpyXmazDev / caxXmazDev / caxInitDev (op) with alpha = omega (p, q) / |p|^2
    taken from device memory"""
    lib().qudaAmdBlasDevUpdate(op.encode(), float(omega), p.h, q.h, x.h, y.h, z.h, w.h if w is not None else None)


def _complex_list(c):
    k = len(c)
    a = (_d * (2 * max(k, 1)))()
    for i, v in enumerate(c):
        a[2 * i], a[2 * i + 1] = complex(v).real, complex(v).imag
    return a


def multi_supported(field, k):
    """qudaAmdBlasMultiSupported: can k fields of this precision go through the multi-field kernels"""
    return bool(lib().qudaAmdBlasMultiSupported(field.h, int(k)))


def multi_dot(f, y, r):
    """qudaAmdBlasMultiDot: ([(f_i, y)], (y, r), |y|^2) in one sweep"""
    k = len(f)
    beta, yr, yn = (_d * (2 * max(k, 1)))(), (_d * 2)(), (_d * 1)()
    lib().qudaAmdBlasMultiDot(k, (_p * max(k, 1))(*[g.h for g in f]), y.h, r.h, beta, yr, yn)
    return [complex(beta[2 * i], beta[2 * i + 1]) for i in range(k)], complex(yr[0], yr[1]), yn[0]


def multi_caxpy_residual(c, f, scale, y, a, r):
    """qudaAmdBlasMultiCaxpyResidual: y <- scale (y + sum_i c_i f_i) ; r <- r - a y ; returns (|r|^2, |y|^2)"""
    k = len(f)
    if len(c) != k:
        raise ValueError("one coefficient per field")
    s = (_d * 2)()
    lib().qudaAmdBlasMultiCaxpyResidual(k, (_p * max(k, 1))(*[g.h for g in f]), _complex_list(c), float(scale), y.h, _complex_list([a]), r.h, s)
    return s[0], s[1]


def multi_caxpy(c, f, y):
    """qudaAmdBlasMultiCaxpy: y <- y + sum_i c_i f_i"""
    k = len(f)
    if len(c) != k:
        raise ValueError("one coefficient per field")
    lib().qudaAmdBlasMultiCaxpy(k, (_p * max(k, 1))(*[g.h for g in f]), _complex_list(c), y.h)


def heavy_quark_residual_norm(x, r):
    """qudaAmdBlasHeavyQuarkResidualNorm: (|x|^2, |r|^2, mean over sites of |r(site)|^2 / |x(site)|^2)"""
    s = (_d * 3)()
    lib().qudaAmdBlasHeavyQuarkResidualNorm(x.h, r.h, s)
    return s[0], s[1], s[2]


class BlockField:
    """qudaAmdBlockField*: a multi-right-hand-side field (include/block.h) of nsites panels of ncomp x nrhs complex numbers and nghost ghost
    panels, free of any lattice.  load / save move the raw device image: float32, (nsites + nghost) * ncomp * nrhs * 2 reals in device order"""

    def __init__(self, nsites, ncomp, nrhs, nghost=0):
        self.nsites, self.ncomp, self.nrhs, self.nghost = int(nsites), int(ncomp), int(nrhs), int(nghost)
        self.nreal = 2 * (self.nsites + self.nghost) * self.ncomp * self.nrhs
        self.h = lib().qudaAmdBlockFieldCreate(self.nsites, self.ncomp, self.nrhs, self.nghost)

    def load(self, image):
        image = np.ascontiguousarray(image, dtype=np.float32)
        if image.size != self.nreal:
            raise ValueError("device image of %d reals, the field holds %d" % (image.size, self.nreal))
        lib().qudaAmdBlockFieldLoad(self.h, _vp(image))
        return self

    def save(self):
        out = np.empty(self.nreal, dtype=np.float32)
        lib().qudaAmdBlockFieldSave(self.h, _vp(out))
        return out

    def free(self):
        if self.h:
            lib().qudaAmdBlockFieldDestroy(self.h)
            self.h = None


# operand of include/block.h -> slot of qudaAmdBlockBlasApply (quda_amd_ext.h)
BLOCK_BLAS_SLOTS = {"norm2": {"x": "x"}, "cDot": {"x": "x", "y": "y"}, "caxpy": {"x": "x", "y": "y"}, "cDotNormA": {"t": "x", "r": "y"},
                    "bicgstabUpdate": {"p": "x", "r": "y", "x": "z", "t": "w", "r0": "u"}, "cxpaypbz": {"r": "x", "v": "y", "p": "z"},
                    "bicgstabDots": {"t": "x", "s": "y", "r0": "u"}, "bicgstabFused": {"p": "x", "r": "y", "x": "z", "t": "w", "v": "u"},
                    "xmy": {"x": "x", "y": "y"}, "negate": {"x": "x"}, "copy": {"src": "x", "dst": "y"}, "zero": {"x": "x"}}


def block_blas_apply(op, a=None, b=None, c=None, **fields):
    """qudaAmdBlockBlasApply: blockblas::<op> on BlockFields given under their names in include/block.h (BLOCK_BLAS_SLOTS); a, b, c: one
    complex coefficient per right-hand side, in the order of the function's coefficient arguments.  Returns the sums as an array [sum][rhs]"""
    slots = BLOCK_BLAS_SLOTS[op]
    if set(fields) != set(slots):
        raise ValueError("%s takes the operands %s" % (op, sorted(slots)))
    h = {slots[n]: f.h for n, f in fields.items()}
    nrhs = next(iter(fields.values())).nrhs
    co = [None if v is None else _complex_list(list(v)) for v in (a, b, c)]
    if any(v is not None and len(v) != nrhs for v in (a, b, c)):
        raise ValueError("one coefficient per right-hand side")
    r = (_d * (8 * 32))()
    n = lib().qudaAmdBlockBlasApply(op.encode(), co[0], co[1], co[2], *[h.get(k) for k in "xyzwu"], r)
    return np.array(r[:n * nrhs], dtype=np.float64).reshape(n, nrhs)


def block_mr_update(steps, omega, fresh, need_residual, s3, s7, x, r, rin, w1, w2=None):
    """qudaAmdBlockMrUpdate: blockblas::mrUpdateDev (steps 1) / mr2UpdateDev (steps 2) with the sums s3[3][nrhs], s7[7][nrhs] given by the caller"""
    s3 = np.ascontiguousarray(s3, dtype=np.float64).reshape(-1)
    s7 = None if s7 is None else np.ascontiguousarray(s7, dtype=np.float64).reshape(-1)
    if s3.size != 3 * x.nrhs or (s7 is not None and s7.size != 7 * x.nrhs):
        raise ValueError("s3 holds 3 and s7 7 sums per right-hand side")
    lib().qudaAmdBlockMrUpdate(int(steps), float(omega), int(bool(fresh)), int(bool(need_residual)), _vp(s3), None if s7 is None else _vp(s7),
                               x.h, r.h, rin.h, w1.h, w2.h if w2 is not None else None)


def _spinor_handles(spinors):
    return (_p * max(len(spinors), 1))(*[f.h if f is not None else None for f in spinors])


def block_pack(block, spinors, parity=-1):
    """qudaAmdBlockPack: full fp32 Spinors -> the columns of block (parity -1: both halves, 0 / 1: that half only)"""
    lib().qudaAmdBlockPack(block.h, _spinor_handles(spinors), len(spinors), int(parity))


def block_unpack(block, spinors, parity=-1):
    lib().qudaAmdBlockUnpack(block.h, _spinor_handles(spinors), len(spinors), int(parity))


def block_pack_parity(block, spinors, accumulate=False):
    """qudaAmdBlockPackParity: single-parity fp32 Spinors (None: a column of zeros) -> the first len(spinors) columns of a 12-component block"""
    lib().qudaAmdBlockPackParity(block.h, _spinor_handles(spinors), len(spinors), int(bool(accumulate)))


def block_unpack_parity(block, spinors):
    """qudaAmdBlockUnpackParity: the columns of block -> single-parity fp32 Spinors (None: that column is skipped)"""
    lib().qudaAmdBlockUnpackParity(block.h, _spinor_handles(spinors), len(spinors))


def block_ghost_panels(parity_field=True):
    """qudaAmdBlockGhostPanels: ghost panels a hop input of the multi-right-hand-side stencil carries under the current partition"""
    return int(lib().qudaAmdBlockGhostPanels(int(bool(parity_field))))


def block_fine_apply(out, in_same, in_other, parity, s0, a0, k1, a1, mode=0, dot_a=None, device_sums=False):
    """qudaAmdBlockFineApply: one parity launch of the multi-right-hand-side fine stencil on the resident fp32 links; mode 1, 2, 3: returns
    its epilogue sums [sum][rhs] (through fineBlockDotsFinishDev if device_sums), mode 0: None"""
    ns = {0: 0, 1: 2, 2: 7, 3: 3}[int(mode)]
    sums = np.zeros(max(ns, 1) * out.nrhs, dtype=np.float64)
    lib().qudaAmdBlockFineApply(out.h, in_same.h if in_same is not None else None, in_other.h, dot_a.h if dot_a is not None else None, int(parity),
                                float(s0), float(a0), float(k1), float(a1), int(mode), int(bool(device_sums)), _vp(sums))
    return sums.reshape(-1, out.nrhs) if ns else None


def clover_twist_dense(parity, a, inverse, vh):
    """qudaAmdCloverTwistDense: the dense site matrices A + i a s (s = +1 / -1 for the upper / lower chirality) of one parity of the resident
    fp32 clover field, or their inverses, as complex64 [vh][2][6][6]"""
    out = np.empty(int(vh) * 2 * 72, dtype=np.float32)
    lib().qudaAmdCloverTwistDense(int(parity), float(a), int(bool(inverse)), _vp(out))
    return out.view(np.complex64).reshape(int(vh), 2, 6, 6)


def block_fine_apply_site(out, in_same, in_other, parity, s0, a0, k1, a1, tmode=0, a=0.0, inverse=False):
    """qudaAmdBlockFineApplySite: one parity launch of the multi-right-hand-side fine stencil with the dense site matrices of the output parity
    on the hop sum (tmode 1) or on in_same (tmode 2), none with tmode 0.  Returns the flag word: bit 0 = XCD plane-tiled work-group order"""
    return int(lib().qudaAmdBlockFineApplySite(out.h, in_same.h if in_same is not None else None, in_other.h, int(parity), float(s0), float(a0),
                                               float(k1), float(a1), int(tmode), float(a), int(bool(inverse))))


def multi_src_stats():
    """qudaAmdMultiSrcStats: counters of the lockstep multi-source path since start-up"""
    a = (C.c_longlong * 4)()
    lib().qudaAmdMultiSrcStats(a)
    return dict(block_cycles=int(a[0]), block_smoothed=int(a[1]), quad_transfers=int(a[2]), solves=int(a[3]))


def invert_multi_src(h_bs, ip, out=None):
    """invertMultiSrcQuda: the sources h_bs[i] through one lockstep solve; returns the list of solutions (ip.num_src is set here).
    out: a list of arrays to receive the solutions (as invert(..., out=))"""
    bs = [np.ascontiguousarray(b) for b in h_bs]
    xs = out if out is not None else [np.zeros_like(b) for b in bs]
    if len(xs) != len(bs) or any(x.shape != b.shape or x.dtype != b.dtype or not x.flags.c_contiguous for x, b in zip(xs, bs)):
        raise ValueError("out must hold one contiguous array per source, of the source's shape and type")
    n = len(bs)
    ip.num_src = n
    pb = (_p * n)(*[_vp(b) for b in bs])
    px = (_p * n)(*[_vp(x) for x in xs])
    lib().invertMultiSrcQuda(px, pb, C.byref(ip))
    return xs


def read_lime_gauge(fname, gp, grid=(1, 1, 1, 1), ip=None, local_volume=None):
    """qudaAmdReadLimeGauge: this rank's sub-block of an ILDG configuration as (4, V_local*18) QDP even-odd arrays; sets gp.X"""
    if local_volume is None:
        raise ValueError("local_volume (sites of this rank's sub-lattice) is needed to size the arrays")
    out = np.zeros((4, int(local_volume) * 18))
    ptr = (_p * 4)(*[_vp(out[d]) for d in range(4)])
    lib().qudaAmdReadLimeGauge(ptr, str(fname).encode(), C.byref(gp), C.byref(ip) if ip is not None else None, (_i * 4)(*[int(v) for v in grid]))
    return out


def write_lime_gauge(fname, gauge, gp, xlf_info=None):
    keep = [np.ascontiguousarray(gauge[d], dtype=np.float64) for d in range(4)]
    ptr = (_p * 4)(*[_vp(a) for a in keep])
    lib().qudaAmdWriteLimeGauge(ptr, str(fname).encode(), C.byref(gp), xlf_info.encode() if xlf_info else None)


def plaquette():
    """plaqQuda: (total, spatial, temporal) plaquette averages of the resident links"""
    pl = (_d * 3)()
    lib().plaqQuda(pl)
    return tuple(pl)


def perform_ape(n_steps, alpha):
    lib().performAPEnStep(int(n_steps), float(alpha))


def perform_stout(n_steps, rho):
    """performSTOUTnStep: stout-smear the resident spatial links into the library's smeared field (save_smeared_gauge reads it)"""
    lib().performSTOUTnStep(int(n_steps), float(rho))


def stout_smear(n_steps, rho, smear_time=False):
    """qudaAmdStoutSmear: as perform_stout; smear_time=True smears all four directions with the staples of all six planes"""
    lib().qudaAmdStoutSmear(int(n_steps), float(rho), int(bool(smear_time)))


def q_charge(density=False, lexicographic=False, which=-1):
    """qChargeCuda / qudaAmdQCharge: the topological charge of the smeared field if one is resident, else of the resident links
    (which=-1), of the resident links (0) or of the smeared field (1).  density=True: returns (Q, q) with q(x) of the local lattice,
    even sites then odd or lexicographic"""
    if not density:
        if which == -1:
            return float(lib().qChargeCuda())
        return float(lib().qudaAmdQCharge(None, 0, int(which)))
    q = np.zeros(2 * gauge_raw_info(0)["Vh"])   # the smeared field has the lattice of the resident links
    Q = lib().qudaAmdQCharge(_vp(q), int(bool(lexicographic)), int(which))
    return float(Q), q


def su3_exp_iq(q):
    """qudaAmdSu3ExpIQ: exp(iq) of traceless Hermitian matrices q[..., 3, 3] (complex) through the stout kernel's device function"""
    q = np.asarray(q, dtype=np.complex128)
    flat = np.ascontiguousarray(np.stack([q.real, q.imag], axis=-1).reshape(-1, 18))
    out = np.zeros_like(flat)
    lib().qudaAmdSu3ExpIQ(int(flat.shape[0]), _vp(flat), _vp(out))
    out = out.reshape(q.shape + (2,))
    return out[..., 0] + 1j * out[..., 1]


def save_gauge(gp):
    """saveGaugeQuda: the resident links in host QDP order, (4, V*18) float64"""
    V = int(np.prod([gp.X[d] for d in range(4)]))
    out = np.zeros((4, V * 18))
    ptr = (_p * 4)(*[_vp(out[d]) for d in range(4)])
    lib().saveGaugeQuda(C.cast(ptr, _p), C.byref(gp))
    return out


def _md_param(gp, **flags):
    """a copy of gp with the residency flags of the molecular-dynamics calls set (all 0 unless named)"""
    q = QudaGaugeParam.from_buffer_copy(gp)
    for name in ("overwrite_mom", "use_resident_gauge", "use_resident_mom", "make_resident_gauge", "make_resident_mom",
                 "return_result_gauge", "return_result_mom"):
        setattr(q, name, int(bool(flags.pop(name, 0))))
    if flags:
        raise TypeError("unknown flags %s" % sorted(flags))
    return q


def _qdp_ptrs(gauge):
    return C.cast((_p * 4)(*[_vp(gauge[d]) for d in range(4)]), _p)


def gauge_force(gp, paths, coeff, eb3, gauge=None, mom=None, overwrite=False, make_resident_gauge=False, make_resident_mom=False,
                return_mom=True, max_length=None):
    """computeGaugeForceQuda: mom <- TA(mom - eb3 U V).  paths[mu][i] is the i-th path (a list of steps 0..7) of direction mu, coeff[i]
    its coefficient.  gauge: (4, V*18) host QDP links, None: the resident links.  mom: (V, 4, 10) host momentum, None: the resident
    momentum (or, with overwrite, none at all).  Returns the new momentum unless return_mom is False"""
    n = len(coeff)
    lengths = [len(paths[0][i]) for i in range(n)]
    maxlen = max(lengths + [1])
    rows = [[(_i * maxlen)(*[int(s) for s in paths[mu][i]]) for i in range(n)] for mu in range(4)]
    per_dir = [(C.POINTER(_i) * max(n, 1))(*[C.cast(r, C.POINTER(_i)) for r in rows[mu]]) for mu in range(4)]
    buf = (C.POINTER(C.POINTER(_i)) * 4)(*[C.cast(a, C.POINTER(C.POINTER(_i))) for a in per_dir])
    V = int(np.prod([gp.X[d] for d in range(4)]))
    use_res_mom = mom is None and not overwrite
    out = np.zeros((V, 4, 10)) if mom is None else np.ascontiguousarray(mom, dtype=np.float64).reshape(V, 4, 10).copy()
    q = _md_param(gp, overwrite_mom=overwrite, use_resident_gauge=gauge is None, use_resident_mom=use_res_mom,
                  make_resident_gauge=make_resident_gauge, make_resident_mom=make_resident_mom, return_result_mom=return_mom)
    if gauge is not None:
        gauge = [np.ascontiguousarray(gauge[d], dtype=np.float64) for d in range(4)]
    lib().computeGaugeForceQuda(_vp(out), _qdp_ptrs(gauge) if gauge is not None else None, buf, (_i * max(n, 1))(*lengths),
                                (_d * max(n, 1))(*[float(c) for c in coeff]), n, int(max_length if max_length is not None else maxlen),
                                float(eb3), C.byref(q))
    return out if return_mom else None


def update_gauge(gp, dt, gauge=None, mom=None, conj_mom=False, exact=True, make_resident_gauge=False, make_resident_mom=False,
                 return_gauge=True):
    """updateGaugeFieldQuda: U <- exp(dt A) U (exact) or its eighth-order Taylor form.  gauge / mom None: the resident fields.
    Returns the new links, (4, V*18) host QDP order, unless return_gauge is False"""
    V = int(np.prod([gp.X[d] for d in range(4)]))
    out = np.zeros((4, V * 18)) if gauge is None else np.array([np.asarray(gauge[d], dtype=np.float64) for d in range(4)]).reshape(4, V * 18)
    m = None if mom is None else np.ascontiguousarray(mom, dtype=np.float64)
    q = _md_param(gp, use_resident_gauge=gauge is None, use_resident_mom=mom is None, make_resident_gauge=make_resident_gauge,
                  make_resident_mom=make_resident_mom, return_result_gauge=return_gauge)
    lib().updateGaugeFieldQuda(_qdp_ptrs(out), _vp(m), float(dt), int(bool(conj_mom)), int(bool(exact)), C.byref(q))
    return out if return_gauge else None


def mom_action(gp, mom=None, make_resident_mom=False):
    """momActionQuda: sum over links of tr(A^dag A)/2 - 4 of the host momentum (V, 4, 10), None: of the resident momentum"""
    m = None if mom is None else np.ascontiguousarray(mom, dtype=np.float64)
    q = _md_param(gp, use_resident_mom=mom is None, make_resident_mom=make_resident_mom)
    return float(lib().momActionQuda(_vp(m), C.byref(q)))


def _force_mom(gp, mom, overwrite, make_resident_mom, return_mom):
    """(host momentum array, parameters) of a fermion-force call: mom None is the resident momentum, or none at all with overwrite"""
    V = int(np.prod([gp.X[d] for d in range(4)]))
    out = np.zeros((V, 4, 10)) if mom is None else np.ascontiguousarray(mom, dtype=np.float64).reshape(V, 4, 10).copy()
    q = _md_param(gp, overwrite_mom=overwrite, use_resident_gauge=True, use_resident_mom=mom is None and not overwrite,
                  make_resident_mom=make_resident_mom, return_result_mom=return_mom)
    return out, q


def _field_ptrs(fields):
    fields = [np.ascontiguousarray(f, dtype=np.float64) for f in fields]
    return fields, (_p * len(fields))(*[_vp(f) for f in fields])


def ferm_oprod_force(gp, ip, xs, ys, coeff, mom=None, overwrite=False, make_resident_mom=False, return_mom=True):
    """qudaAmdFermionOprodForce: mom <- TA(mom - sum_i coeff[i] U O[xs[i], ys[i]]) on the resident links, O_mu[X, Y](x) =
    tr_spin[(1 - g_mu) X(x + mu) Y^dag(x) + (1 + g_mu) Y(x + mu) X^dag(x)].  xs, ys: full host fields as MatQuda takes them under ip
    (two flavours for the doublet).  mom: (V, 4, 10) host momentum, None: the resident momentum (or, with overwrite, none at all).
    Returns the new momentum unless return_mom is False"""
    n = len(coeff)
    if len(xs) != n or len(ys) != n:
        raise ValueError("one coefficient per pair of fields")
    out, q = _force_mom(gp, mom, overwrite, make_resident_mom, return_mom)
    xs, px = _field_ptrs(xs)
    ys, py = _field_ptrs(ys)
    lib().qudaAmdFermionOprodForce(_vp(out), px, py, (_d * max(n, 1))(*[float(c) for c in coeff]), n, C.byref(q), C.byref(ip))
    return out if return_mom else None


def tm_force(gp, ip, xs, coeff, dt, mom=None, overwrite=False, make_resident_mom=False, return_mom=True):
    """qudaAmdComputeTMForce: mom <- mom + dt sum_i coeff[i] F[xs[i]] on the resident links, F the force of phi^dag (Mh^dag Mh)^-1 phi at
    the single-parity solutions xs[i] of a QUDA_NORMOP_PC_SOLVE under ip (Wilson, twisted mass +-1, the doublet, or twisted clover +-1
    on a clover term built from the resident links with ip.clover_coeff; any matpc type and mass normalisation).  Momentum arguments
    as in ferm_oprod_force"""
    n = len(coeff)
    if len(xs) != n:
        raise ValueError("one coefficient per solution")
    out, q = _force_mom(gp, mom, overwrite, make_resident_mom, return_mom)
    xs, px = _field_ptrs(xs)
    lib().qudaAmdComputeTMForce(_vp(out), float(dt), px, (_d * max(n, 1))(*[float(c) for c in coeff]), n, C.byref(q), C.byref(ip))
    return out if return_mom else None


def _dp(a):
    return a.ctypes.data_as(C.POINTER(_d))


def clover_sigma_oprod(ip, xs, ys, coeff, V):
    """qudaAmdCloverSigmaOprod: T_f(x) = sum_i coeff[i][parity(x)] S_f[xs[i], ys[i]](x), S_f[X, Y]_ba = sum_ss' (sigma_f)_ss' X_s'b conj(Y_sa),
    for full host fields as MatQuda takes them under ip on the resident lattice of V sites.  coeff: (nvector, 2), even and odd.
    Returns the tensor field (V, 6, 3, 3, 2), even sites then odd"""
    n = len(xs)
    c = np.ascontiguousarray(coeff, dtype=np.float64).reshape(n, 2)
    if len(ys) != n:
        raise ValueError("one Y per X")
    out = np.zeros((int(V), 6, 3, 3, 2))
    xs, px = _field_ptrs(xs)
    ys, py = _field_ptrs(ys)
    lib().qudaAmdCloverSigmaOprod(_dp(out), px, py, _dp(c), n, C.byref(ip))
    return out


def clover_sigma_trace(ip, coeff_even, coeff_odd, V):
    """qudaAmdCloverSigmaTrace: T_f(x) = coeff[parity(x)] sum_ss' (sigma_f)_ss' B(x)_(s'b)(sa), B = A (A^2 + a^2)^-1 of the resident fp64 clover
    term.  Returns the tensor field (V, 6, 3, 3, 2)"""
    out = np.zeros((int(V), 6, 3, 3, 2))
    lib().qudaAmdCloverSigmaTrace(_dp(out), float(coeff_even), float(coeff_odd), C.byref(ip))
    return out


def clover_derivative_force(gp, tensor, coeff, mom=None, overwrite=False, make_resident_mom=False, return_mom=True):
    """qudaAmdCloverDerivativeForce: mom <- mom + coeff G[T], G[T] the force of L_T(U) = sum_x sum_f Re tr(T_f(x) F_f(x; U)) on the
    resident links, T = tensor (V, 6, 3, 3, 2).  Momentum arguments as in ferm_oprod_force"""
    out, q = _force_mom(gp, mom, overwrite, make_resident_mom, return_mom)
    t = np.ascontiguousarray(tensor, dtype=np.float64)
    if t.size != out.shape[0] * 108:
        raise ValueError("the tensor field has 108 doubles per site")
    lib().qudaAmdCloverDerivativeForce(_vp(out), _dp(t), float(coeff), C.byref(q))
    return out if return_mom else None


def clover_logdet_force(gp, ip, dt, coeff_even, coeff_odd, mom=None, overwrite=False, make_resident_mom=False, return_mom=True):
    """qudaAmdCloverLogDetForce: mom <- mom + dt (coeff_even F[L_even] + coeff_odd F[L_odd]), L_p = sum over the sites of parity p of
    log det(A^2 + a^2) (trlogA[p] of loadCloverQuda), on a clover term built from the resident links with ip.clover_coeff"""
    out, q = _force_mom(gp, mom, overwrite, make_resident_mom, return_mom)
    lib().qudaAmdCloverLogDetForce(_vp(out), float(dt), float(coeff_even), float(coeff_odd), C.byref(q), C.byref(ip))
    return out if return_mom else None


def ferm_force_kernel_secs():
    """device seconds the kernels of the last fermion-force call took"""
    return float(lib().qudaAmdFermForceLastKernelSecs())


def project_su3(gp, tol, gauge=None, make_resident_gauge=False, return_gauge=True):
    """projectSU3Quda: every link projected onto SU(3); a link further than tol from unitary afterwards is an error.  gauge None:
    the resident links.  Returns the projected links, (4, V*18), unless return_gauge is False"""
    V = int(np.prod([gp.X[d] for d in range(4)]))
    out = np.zeros((4, V * 18)) if gauge is None else np.array([np.asarray(gauge[d], dtype=np.float64) for d in range(4)]).reshape(4, V * 18)
    q = _md_param(gp, use_resident_gauge=gauge is None, make_resident_gauge=make_resident_gauge, return_result_gauge=return_gauge)
    lib().projectSU3Quda(_qdp_ptrs(out), float(tol), C.byref(q))
    return out if return_gauge else None


def gauge_fix_ovr(gp, gauge_dir, n_steps, relax_boost, tolerance, reunit_interval, stop_theta, gauge=None, make_resident_gauge=False,
                  return_gauge=True, transform=False, verbose_interval=0):
    """computeGaugeFixingOVRQuda / qudaAmdGaugeFixOVR: Landau (gauge_dir != 3) or Coulomb (3) gauge fixing by overrelaxation.  gauge
    None: the resident links.  Returns (links, G, info): the fixed links, (4, V*18) host QDP order (None unless return_gauge); with
    transform the accumulated transformation G, (V, 18), even sites then odd, else None; info = {"iterations", "F", "theta", "delta",
    "secs": (load, compute, save)}"""
    V = int(np.prod([gp.X[d] for d in range(4)]))
    out = np.zeros((4, V * 18)) if gauge is None else np.array([np.asarray(gauge[d], dtype=np.float64) for d in range(4)]).reshape(4, V * 18)
    q = _md_param(gp, use_resident_gauge=gauge is None, make_resident_gauge=make_resident_gauge, return_result_gauge=return_gauge)
    G = np.zeros((V, 18)) if transform else None
    info, secs = (_d * 4)(), (_d * 3)()
    lib().qudaAmdGaugeFixOVR(_qdp_ptrs(out), int(gauge_dir), int(n_steps), int(verbose_interval), float(relax_boost), float(tolerance),
                             int(reunit_interval), int(bool(stop_theta)), C.byref(q), secs, _vp(G), info)
    return (out if return_gauge else None, G,
            {"iterations": int(info[0]), "F": float(info[1]), "theta": float(info[2]), "delta": float(info[3]), "secs": tuple(secs)})


def gauge_fix_quality(gauge_dir):
    """qudaAmdGaugeFixQuality: (F, theta) of the resident precise links for gauge_dir 3 (Coulomb) or any other value (Landau)"""
    out = (_d * 2)()
    lib().qudaAmdGaugeFixQuality(int(gauge_dir), out)
    return float(out[0]), float(out[1])


def save_smeared_gauge(local_volume, lexicographic=False):
    out = np.zeros((4, int(local_volume) * 18))
    ptr = (_p * 4)(*[_vp(out[d]) for d in range(4)])
    lib().qudaAmdSaveSmearedGauge(ptr, int(bool(lexicographic)))
    return out


def _lex_links(gauge_lex):
    if gauge_lex is None:
        return None, None
    keep = [np.ascontiguousarray(gauge_lex[d], dtype=np.float64) for d in range(4)]
    return keep, (_p * 4)(*[_vp(a) for a in keep])


def gaussian_smear(vec_lex, gauge_lex, nsmear, alpha):
    """QKXTM_Vector_Kepler::gaussianSmearing on a lexicographic UKQCD host vector (local lattice of the resident gauge field)"""
    vec_lex = np.ascontiguousarray(vec_lex, dtype=np.float64)
    out = np.empty_like(vec_lex)
    keep, links = _lex_links(gauge_lex)
    lib().qudaAmdGaussianSmear(_vp(out), _vp(vec_lex), links, int(nsmear), float(alpha))
    return out


def calc_mg_propagators(gauge_lex, ip, source_position, nsmear, alpha, local_volume):
    """the solve loop of calcMG_threepTwop_EvenOdd: returns (prop_up, prop_dn), each (12, V*24) lexicographic UKQCD vectors"""
    sp = QudaAmdSourceParam()
    for k in range(4):
        sp.sourcePosition[k] = int(source_position[k])
    sp.nsmearGauss, sp.alphaGauss = int(nsmear), float(alpha)
    up = np.zeros((12, int(local_volume) * 24))
    dn = np.zeros((12, int(local_volume) * 24))
    keep, links = _lex_links(gauge_lex)
    lib().qudaAmdCalcMGPropagators(_vp(up), _vp(dn), links, C.byref(ip), C.byref(sp))
    return up, dn


def twop_momenta(Q_sq):
    """qudaAmdTwopMomenta: the momenta |n|^2 <= Q_sq of the two-point functions as an (Nmoms, 3) int array, in the reference's order"""
    n = lib().qudaAmdTwopMomenta(int(Q_sq), None, 0)
    out = np.zeros((n, 3), dtype=np.int32)
    lib().qudaAmdTwopMomenta(int(Q_sq), out.ctypes.data_as(C.POINTER(_i)), n)
    return out


def contract_twop(prop_up, prop_dn, gauge_lex, source_position, Q_sq, nsmear, alpha):
    """qudaAmdContractTwop on two propagators as calc_mg_propagators returns them ((12, V*24) lexicographic UKQCD, local lattice):
    returns (mesons (T, Nmoms, 2, 10), baryons (T, Nmoms, 2, 10, 4, 4)) complex128, time relative to the source"""
    up = np.ascontiguousarray(prop_up, dtype=np.float64)
    dn = np.ascontiguousarray(prop_dn, dtype=np.float64)
    if up.shape != dn.shape or up.shape[0] != 12:
        raise ValueError("prop_up / prop_dn must both be (12, V*24)")
    p = QudaAmdTwopParam()
    for k in range(4):
        p.sourcePosition[k] = int(source_position[k])
    p.Q_sq, p.nsmearGauss, p.alphaGauss = int(Q_sq), int(nsmear), float(alpha)
    T = lib().qudaAmdTwopTimeExtent()
    nm = lib().qudaAmdTwopMomenta(int(Q_sq), None, 0)
    mes = np.zeros((T, nm, 2, 10, 2))
    bar = np.zeros((T, nm, 2, 10, 4, 4, 2))
    keep, links = _lex_links(gauge_lex)
    lib().qudaAmdContractTwop(_vp(mes), _vp(bar), _vp(up), _vp(dn), links, C.byref(p))
    return mes[..., 0] + 1j * mes[..., 1], bar[..., 0] + 1j * bar[..., 1]


def set_twop_output(enable):
    """qudaAmdSetTwopOutput: calcMG_threepTwop_EvenOdd writes the two-point ASCII files"""
    lib().qudaAmdSetTwopOutput(int(bool(enable)))


def loop_momenta(L, Q_sq):
    """qudaAmdLoopMomenta: the momenta |n|^2 <= Q_sq of the quark loops on a lattice of GLOBAL spatial extents L as an (Nmoms, 3) int
    array, in the reference's order (pz outermost, px innermost, components 0 .. L/2-1, -L/2 .. -1); host only"""
    ext = (_i * 3)(*[int(v) for v in L])
    n = lib().qudaAmdLoopMomenta(ext, int(Q_sq), None, 0)
    out = np.zeros((n, 3), dtype=np.int32)
    lib().qudaAmdLoopMomenta(ext, int(Q_sq), out.ctypes.data_as(C.POINTER(_i)), n)
    return out


def contract_loop(solution, ip, Q_sq, L):
    """qudaAmdContractLoop on ONE solution vector ((V*24,) lexicographic UKQCD, local lattice, not rescaled): the 18 blocks
    (Scalar, dOp, Loops[4], LoopsCv[4], LpsDw[4], LpsDwCv[4]) as a complex128 array (18, T, Nmoms, 16), T global, raw sums.
    L: the GLOBAL spatial extents (Lx, Ly, Lz) of the resident lattice (they fix the momentum list)"""
    sol = np.ascontiguousarray(solution, dtype=np.float64)
    nm = len(loop_momenta(L, Q_sq))
    T = lib().qudaAmdTwopTimeExtent()
    out = np.zeros((18, T, nm, 16, 2))
    lib().qudaAmdContractLoop(_vp(out), _vp(sol), C.byref(ip), int(Q_sq))
    return out[..., 0] + 1j * out[..., 1]


def momentum_project(acc, cs, t0, moms, X, gx=(0, 0, 0), L=None):
    """qudaAmdMomentumProject (test hook onto the projection that all contractions share): acc (nblk, Lt, Nm, 16) complex, cs
    (nblk, nt * Vs, 16) complex with Vs = X[0] X[1] X[2] sites per slice, x fastest; returns acc + the projection of cs onto moms (Nm, 3)
    written into the slices [t0, t0 + nt).  X the local extents, gx the global coordinate of the local origin, L the global extents
    (None: X).  Needs init(), no resident field"""
    acc, cs = np.asarray(acc, dtype=np.complex128), np.asarray(cs, dtype=np.complex128)
    m = np.ascontiguousarray(moms, dtype=np.int32).reshape(-1, 3)
    nblk, Lt, Nm = acc.shape[:3]
    Vs = int(X[0]) * int(X[1]) * int(X[2])
    if acc.shape != (nblk, Lt, len(m), 16) or cs.ndim != 3 or cs.shape[0] != nblk or cs.shape[2] != 16 or cs.shape[1] % Vs:
        raise ValueError("acc must be (nblk, Lt, Nm, 16) and cs (nblk, nt * Vs, 16)")
    nt = cs.shape[1] // Vs
    if nt < 1 or t0 < 0 or t0 + nt > Lt:
        raise ValueError("slices [%d, %d) of %d" % (t0, t0 + nt, Lt))
    out = np.ascontiguousarray(np.stack([acc.real, acc.imag], axis=-1))
    h_cs = np.ascontiguousarray(np.stack([cs.real, cs.imag], axis=-1))
    ext = [(_i * 3)(*[int(v) for v in a]) for a in (X, gx, X if L is None else L)]
    lib().qudaAmdMomentumProject(_vp(out), _vp(h_cs), nblk, int(t0), nt, Lt, m.ctypes.data_as(C.POINTER(_i)), Nm, *ext)
    return out[..., 0] + 1j * out[..., 1]


def host_symmetric_eig(a):
    """qudaAmdHostSymmetricEig (cyclic Jacobi, host only): ascending eigenvalues w and the matrix q whose COLUMN i is the eigenvector of
    w[i] of the real symmetric matrix a"""
    a = np.ascontiguousarray(a, dtype=np.float64)
    n = a.shape[0]
    assert a.shape == (n, n)
    w, q = np.zeros(n), np.zeros((n, n))
    lib().qudaAmdHostSymmetricEig(n, _vp(a), _vp(w), _vp(q))
    return w, q


def gcr_back_substitute(alpha, beta, gamma):
    """qudaAmdGcrBackSubstitute (host only): delta[k] of the solution update of restarted GCR from alpha[k], gamma[k] and beta[nK][nK]
    (row-major, the strict upper triangle of its leading k x k block is read), k = len(alpha) <= nK"""
    alpha = np.ascontiguousarray(alpha, dtype=np.complex128)
    beta = np.ascontiguousarray(beta, dtype=np.complex128)
    gamma = np.ascontiguousarray(gamma, dtype=np.float64)
    k, nK = alpha.shape[0], beta.shape[0]
    assert beta.shape == (nK, nK) and gamma.shape == (k,) and 0 < k <= nK
    a, g, delta = np.zeros(nK, dtype=np.complex128), np.ones(nK), np.zeros(k, dtype=np.complex128)
    a[:k], g[:k] = alpha, gamma
    lib().qudaAmdGcrBackSubstitute(k, nK, _vp(a), _vp(beta), _vp(g), _vp(delta))
    return delta


class Deflation:
    """qudaAmdNewDeflation: the nEv lowest eigenpairs of M^dag M of the full operator of `ip` on the resident fields, ascending, kept
    on the device until close().  Host vectors have the layout MatQuda takes for `ip` (even sites then odd, ip.gamma_basis)."""

    def __init__(self, ip, nEv, nKv, PolyDeg, amin, amax, tol, isACC=True, maxRestarts=100):
        ep = QudaAmdEigParam(int(nEv), int(nKv), int(PolyDeg), int(bool(isACC)), int(maxRestarts), float(amin), float(amax), float(tol))
        self._h = lib().qudaAmdNewDeflation(C.byref(ip), C.byref(ep))
        self.nEv = int(nEv)
        ev, res = np.zeros(self.nEv), np.zeros(self.nEv)
        r, mv = _i(0), _i(0)
        n = lib().qudaAmdDeflationInfo(self._h, ev.ctypes.data_as(C.POINTER(_d)), res.ctypes.data_as(C.POINTER(_d)), C.byref(r), C.byref(mv))
        assert n == self.nEv
        self.evals, self.residuals, self.restarts, self.matvecs = ev, res, int(r.value), int(mv.value)
        t = (_d * 4)()
        lib().qudaAmdDeflationTimings(self._h, t)
        self.timings = dict(zip(("filter", "dots", "updates", "rotations"), [float(v) for v in t]))

    def close(self):
        if self._h:
            lib().qudaAmdDestroyDeflation(self._h)
            self._h = None

    def vector(self, i, local_volume):
        out = np.zeros(int(local_volume) * 24)
        lib().qudaAmdDeflationGetVector(self._h, int(i), _vp(out))
        return out

    def project(self, x, n):
        """(1 - U_n U_n^+) x with the first n vectors, on the device"""
        x = np.ascontiguousarray(x, dtype=np.float64)
        out = np.empty_like(x)
        lib().qudaAmdDeflationProject(self._h, int(n), _vp(out), _vp(x))
        return out

    def exact_loop(self, n, Q_sq, L):
        """sum_{i<n} L[v_i] / lambda_i in the layout of contract_loop"""
        nm = len(loop_momenta(L, Q_sq))
        T = lib().qudaAmdTwopTimeExtent()
        out = np.zeros((18, T, nm, 16, 2))
        lib().qudaAmdDeflationExactLoop(self._h, int(n), _vp(out), int(Q_sq))
        return out[..., 0] + 1j * out[..., 1]


def _ext4(X):
    return (_i * 4)(*[int(v) for v in X])


def rotate_basis(V, Q, X):
    """qudaAmdRotateBasis: V (m, V*24) float64 -> V[:k] <- Q^T-combinations, i.e. new V[c] = sum_j Q[j, c] V[j] for c < k; rows k.. unchanged"""
    V = np.array(V, dtype=np.float64, order="C")
    Q = np.ascontiguousarray(Q, dtype=np.float64)
    m, k = Q.shape
    assert V.shape[0] == m
    lib().qudaAmdRotateBasis(_vp(V), m, k, _vp(Q), _ext4(X))
    return V


def block_dot(V, w, X):
    """qudaAmdBlockDot: c[j] = sum conj(v_j) w for the m rows of V ((m, V*24) float64 as V*12 complex numbers)"""
    V = np.ascontiguousarray(V, dtype=np.float64)
    w = np.ascontiguousarray(w, dtype=np.float64)
    c = np.zeros((V.shape[0], 2))
    lib().qudaAmdBlockDot(_vp(c), _vp(V), V.shape[0], _vp(w), _ext4(X))
    return c[:, 0] + 1j * c[:, 1]


def block_axpy(w, c, V, X):
    """qudaAmdBlockAxpy: w - sum_j c[j] v_j"""
    V = np.ascontiguousarray(V, dtype=np.float64)
    w = np.array(w, dtype=np.float64, order="C")
    cc = np.ascontiguousarray(np.stack([np.real(c), np.imag(c)], axis=-1), dtype=np.float64)
    lib().qudaAmdBlockAxpy(_vp(w), _vp(cc), _vp(V), V.shape[0], _ext4(X))
    return w


def last_eigenvalues():
    """qudaAmdLastEigenvalues: the eigenvalues of the last calcMG_loop_wOneD_TSM_wExact call with nEv > 0"""
    n = lib().qudaAmdLastEigenvalues(None, 0)
    out = np.zeros(n)
    lib().qudaAmdLastEigenvalues(out.ctypes.data_as(C.POINTER(_d)), n)
    return out


def set_loop_output(enable):
    """qudaAmdSetLoopOutput: calcMG_loop_wOneD_TSM_EvenOdd contracts its solutions and writes the loop ASCII files"""
    lib().qudaAmdSetLoopOutput(int(bool(enable)))


def _threep_param(source_position, Q_sq, tsink, projector, particle, part, nsmear, alpha):
    p = QudaAmdThreepParam()
    for k in range(4):
        p.sourcePosition[k] = int(source_position[k])
    p.Q_sq, p.tsinkSource, p.projector, p.particle, p.part = int(Q_sq), int(tsink), int(projector), int(particle), int(part)
    p.nsmearGauss, p.alphaGauss = int(nsmear), float(alpha)
    return p


def threep_seq_source(prop_up, prop_dn, gauge_lex, source_position, tsink, projector, particle, part, nsmear, alpha):
    """qudaAmdThreepSeqSource: the twelve sequential sources of the fixed-sink method, (12, V*24) lexicographic UKQCD, as they go to
    the solver, from the unsmeared propagators of calc_mg_propagators.  tsink is relative to the source; particle PROTON / NEUTRON,
    part 1 / 2, projector G4 .. G5G3"""
    up = np.ascontiguousarray(prop_up, dtype=np.float64)
    dn = np.ascontiguousarray(prop_dn, dtype=np.float64)
    if up.shape != dn.shape or up.shape[0] != 12:
        raise ValueError("prop_up / prop_dn must both be (12, V*24)")
    p = _threep_param(source_position, 0, tsink, projector, particle, part, nsmear, alpha)
    out = np.zeros_like(up)
    keep, links = _lex_links(gauge_lex)
    lib().qudaAmdThreepSeqSource(_vp(out), _vp(up), _vp(dn), links, C.byref(p))
    return out


def contract_threep(seq, fwd, gauge_lex, source_position, Q_sq, tsink, particle, part):
    """qudaAmdContractThreep: seq the twelve sequential solutions, fwd the twelve forward columns of the inserted flavour (both
    (12, V*24) lexicographic UKQCD), gauge_lex the links of the derivative with the boundary applied (None: the resident precise
    links).  Returns (local (T, Nmoms, 16), noether (T, Nmoms, 4), oneD (T, Nmoms, 4, 16)) complex128, time relative to the source"""
    y = np.ascontiguousarray(seq, dtype=np.float64)
    f = np.ascontiguousarray(fwd, dtype=np.float64)
    if y.shape != f.shape or y.shape[0] != 12:
        raise ValueError("seq / fwd must both be (12, V*24)")
    p = _threep_param(source_position, Q_sq, tsink, G4, particle, part, 0, 0.0)
    T = lib().qudaAmdTwopTimeExtent()
    nm = lib().qudaAmdTwopMomenta(int(Q_sq), None, 0)
    local, noether, oneD = np.zeros((T, nm, 16, 2)), np.zeros((T, nm, 4, 2)), np.zeros((T, nm, 4, 16, 2))
    keep, links = _lex_links(gauge_lex)
    lib().qudaAmdContractThreep(_vp(local), _vp(noether), _vp(oneD), _vp(y), _vp(f), links, C.byref(p))
    return local[..., 0] + 1j * local[..., 1], noether[..., 0] + 1j * noether[..., 1], oneD[..., 0] + 1j * oneD[..., 1]


def threep_operator(i, s):
    """qudaAmdThreepOperator: the insertion O_i (i = 0 .. 15) for the flavour sign s = +-1 as a 4 x 4 complex matrix; host only"""
    a = (_d * 32)()
    lib().qudaAmdThreepOperator(int(i), int(s), a)
    v = np.array(a[:]).reshape(4, 4, 2)
    return v[..., 0] + 1j * v[..., 1]


def threep_projector(pid, particle):
    """qudaAmdThreepProjector: the projector in the twisted basis, R_p G R_p, as a 4 x 4 complex matrix; host only"""
    a = (_d * 32)()
    lib().qudaAmdThreepProjector(int(pid), int(particle), a)
    v = np.array(a[:]).reshape(4, 4, 2)
    return v[..., 0] + 1j * v[..., 1]


def set_threep_output(enable):
    """qudaAmdSetThreepOutput: calcMG_threepTwop_EvenOdd runs the sequential solves and writes the three-point ASCII files"""
    lib().qudaAmdSetThreepOutput(int(bool(enable)))


def threep_last_timings():
    """qudaAmdThreepLastTimings: seconds of the last calls: dict(source, ghost, stencil, projection)"""
    a = (_d * 4)()
    lib().qudaAmdThreepLastTimings(a)
    return dict(source=a[0], ghost=a[1], stencil=a[2], projection=a[3])


def loop_last_timings():
    """qudaAmdLoopLastTimings: seconds of the last loop contraction: dict(phi, stencil, projection, total)"""
    a = (_d * 4)()
    lib().qudaAmdLoopLastTimings(a)
    return dict(phi=a[0], stencil=a[1], projection=a[2], total=a[3])


class Spinor:
    """Device-resident ColorSpinorField handle (quda_amd_ext.h)."""

    def __init__(self, prec, subset=QUDA_PARITY_SITE_SUBSET, flavor=QUDA_TWIST_PLUS):
        """flavor=QUDA_TWIST_NONDEG_DOUBLET: a two-flavour field, loaded from / saved to host arrays of twice the size"""
        self.h = lib().qudaAmdSpinorCreate(int(prec), int(subset), int(flavor))
        self.prec, self.subset = prec, subset

    def load(self, host, ip):
        lib().qudaAmdSpinorLoad(self.h, _vp(np.ascontiguousarray(host)), C.byref(ip))
        return self

    def save(self, ip, like):
        out = np.empty_like(like)
        lib().qudaAmdSpinorSave(self.h, _vp(out), C.byref(ip))
        return out

    def norm2(self):
        return lib().qudaAmdBlasNorm2(self.h)

    # the fused sweeps of CG (include/blas.h); self is the field called y there
    def axpy_cg_norm(self, a, x):
        """self += a x; returns (|self|^2, (self_new, self_new - self_old))"""
        r = (_d * 2)()
        lib().qudaAmdBlasAxpyCGNorm(float(a), x.h, self.h, r)
        return r[0], r[1]

    def axpy_zpbx(self, a, x, z, b):
        """self += a x; x = z + b x"""
        lib().qudaAmdBlasAxpyZpbx(float(a), x.h, self.h, z.h, float(b))

    def axpy_re_dot(self, a, x):
        """self += a x; returns (x, self)"""
        return lib().qudaAmdBlasAxpyReDot(float(a), x.h, self.h)

    def triple_cg_reduction(self, y, z):
        """(|self|^2, |y|^2, (y, z))"""
        r = (_d * 3)()
        lib().qudaAmdBlasTripleCGReduction(self.h, y.h, z.h, r)
        return r[0], r[1], r[2]

    def raw_info(self):
        """qudaAmdSpinorRawInfo as a dict"""
        a = (C.c_longlong * 20)()
        lib().qudaAmdSpinorRawInfo(self.h, a)
        keys = ("volume", "volumeCB", "stride", "pad", "nSpin", "nColor", "precision", "fieldOrder", "siteSubset", "gammaBasis", "bytes", "norm_bytes",
                "v", "norm", "odd_offset", "odd_norm_offset", "N", "twistFlavor", "x0", "location")
        return dict(zip(keys, [int(v) for v in a]))

    def free(self):
        if self.h:
            lib().qudaAmdSpinorDestroy(self.h)
            self.h = None


def ndeg_twist(out, inp, kappa, mu, epsilon, dagger=0, inverse=0):
    """qudaAmdNdegTwist on resident doublet Spinors: out = (1 + i a g5 tau3 + b tau1) inp with a = 2 kappa mu, b = -2 kappa epsilon, or
    its inverse; dagger flips a; out may be inp"""
    L = lib()
    if not hasattr(L, "qudaAmdNdegTwist"):
        raise RuntimeError("%s does not export qudaAmdNdegTwist: it was built before the non-degenerate doublet" % LIB_PATH)
    L.qudaAmdNdegTwist(out.h, inp.h, float(kappa), float(mu), float(epsilon), int(dagger), int(inverse))
    return out


def raw_device_copy(address, nbytes):
    """bytes of device memory as a uint8 array (layout tests)"""
    out = np.zeros(int(nbytes), dtype=np.uint8)
    lib().qudaAmdRawDeviceCopy(_vp(out), int(address), int(nbytes))
    return out


def gauge_raw_info(which=0):
    a = (C.c_longlong * 12)()
    lib().qudaAmdGaugeRawInfo(int(which), a)
    return dict(zip(("data", "bytes", "stride", "link_bytes", "precision", "reconstruct", "Vh", "tbc_folded", "t_boundary"), [int(v) for v in a][:9]))


def clover_raw_info(which=0):
    a = (C.c_longlong * 12)()
    lib().qudaAmdCloverRawInfo(int(which), a)
    return dict(zip(("A", "Ainv", "norm", "invNorm", "stride", "parity_bytes", "parity_norm_bytes", "precision", "bytes", "Vh", "twisted"), [int(v) for v in a][:11]))


class Dirac:
    """Operator handle: Dirac::create over the resident gauge/clover (quda_amd_ext.h)."""

    def __init__(self, ip, pc=True, which=0):
        self.h = lib().qudaAmdDiracCreate(C.byref(ip), int(pc), int(which))

    def dslash(self, out, inp, parity):
        lib().qudaAmdDiracDslash(self.h, out.h, inp.h, int(parity))

    def dslash_xpay(self, out, inp, parity, x, k):
        lib().qudaAmdDiracDslashXpay(self.h, out.h, inp.h, int(parity), x.h, float(k))

    def M(self, out, inp):
        lib().qudaAmdDiracM(self.h, out.h, inp.h)

    def Mdag(self, out, inp):
        lib().qudaAmdDiracMdag(self.h, out.h, inp.h)

    def MdagM(self, out, inp):
        lib().qudaAmdDiracMdagM(self.h, out.h, inp.h)

    def MdagM_shift(self, out, inp, shift):
        """out = (M^dag M + shift) inp through the DiracMdagM functor of the solvers"""
        lib().qudaAmdDiracMdagMShift(self.h, out.h, inp.h, float(shift))

    def time_MdagM(self, out, inp, niter):
        return lib().qudaAmdTimeMdagM(self.h, out.h, inp.h, int(niter))

    def prepare(self, src_out, x, b, solution_type):
        """Dirac::prepare on resident full fields; the source of the (preconditioned) system is copied into src_out"""
        lib().qudaAmdDiracPrepare(self.h, src_out.h, x.h, b.h, int(solution_type))

    def reconstruct(self, x, b, solution_type):
        lib().qudaAmdDiracReconstruct(self.h, x.h, b.h, int(solution_type))

    def time_dslash(self, out, inp, parity, niter):
        return lib().qudaAmdTimeDslash(self.h, out.h, inp.h, int(parity), int(niter))

    def time_M(self, out, inp, niter):
        return lib().qudaAmdTimeM(self.h, out.h, inp.h, int(niter))

    def free(self):
        if self.h:
            lib().qudaAmdDiracDestroy(self.h)
            self.h = None


def coarse_invert_sites(X, H=None):
    """coarse_invert_kernel / coarse_hat_kernel on the caller's matrices (qudaAmdCoarseInvertSites): X (sites, n, n), H (sites, 8, n, n) or None;
    returns (Xinv, Xinv H_d or None, the kernel's singularity flag)"""
    X = np.ascontiguousarray(X, dtype=np.complex64)
    ns, n = X.shape[0], X.shape[1]
    H = None if H is None else np.ascontiguousarray(H, dtype=np.complex64).reshape(ns, 8, n, n)
    Xinv = np.zeros_like(X)
    hat = None if H is None else np.zeros_like(H)
    fail = _i(-1)
    lib().qudaAmdCoarseInvertSites(int(n), int(ns), _vp(X), _vp(Xinv), _vp(hat), _vp(H), C.byref(fail))
    return Xinv, hat, int(fail.value)


def multigrid_param(ip, n_level=2, geo_block=(4, 4, 4, 4), n_vec=24, nu_pre=2, nu_post=2, cycle=QUDA_MG_CYCLE_RECURSIVE, smoother_tol=0.25,
                    setup_maxiter=500, setup_tol=5e-6, generate_all_levels=True, omega=0.85, smoother_pc=False, coarse_matpc=False):
    """QudaMultigridParam filled the way the reference harness does (tests/multigrid_invert_test.cpp:195-290), with the
    smoother on the full operator (QUDA_DIRECT_SOLVE) or, smoother_pc=True, the reference default QUDA_DIRECT_PC_SOLVE."""
    mp = lib().newQudaMultigridParam()
    mp.invert_param = C.pointer(ip)
    mp.n_level = n_level
    blocks = geo_block if isinstance(geo_block[0], (tuple, list)) else [geo_block] * n_level
    nv = n_vec if isinstance(n_vec, (tuple, list)) else [n_vec] * n_level
    for i in range(n_level):
        for d in range(4):
            mp.geo_block_size[i][d] = int(blocks[i][d])
        for d in range(4, QUDA_MAX_DIM):
            mp.geo_block_size[i][d] = 1
        mp.spin_block_size[i] = 2 if i == 0 else 1
        mp.n_vec[i] = int(nv[i])
        mp.nu_pre[i], mp.nu_post[i] = nu_pre, nu_post
        mp.cycle_type[i] = cycle
        mp.smoother[i] = QUDA_MR_INVERTER
        mp.smoother_tol[i] = smoother_tol
        mp.global_reduction[i] = QUDA_BOOLEAN_YES
        mp.smoother_solve_type[i] = QUDA_DIRECT_PC_SOLVE if smoother_pc else QUDA_DIRECT_SOLVE
        # QUDA_MATPC_SOLUTION: single-parity injection, what the harness pairs with an outer even-odd solve (multigrid_invert_test.cpp:246-252)
        mp.coarse_grid_solution_type[i] = QUDA_MATPC_SOLUTION if coarse_matpc else QUDA_MAT_SOLUTION
        mp.omega[i] = omega
        mp.location[i] = QUDA_CUDA_FIELD_LOCATION
    mp.setup_maxiter, mp.setup_tol = setup_maxiter, setup_tol
    mp.compute_null_vector = QUDA_COMPUTE_NULL_VECTOR_YES
    mp.generate_all_levels = QUDA_BOOLEAN_YES if generate_all_levels else QUDA_BOOLEAN_NO
    mp.run_verify = QUDA_BOOLEAN_NO
    return mp


class Multigrid:
    """newMultigridQuda / destroyMultigridQuda handle"""

    def __init__(self, mp):
        self.mp = mp
        self.h = lib().newMultigridQuda(C.byref(mp))

    def verify(self):
        dev = (_d * 3)()
        lib().qudaAmdMultigridVerify(self.h, dev)
        return [dev[0], dev[1], dev[2]]

    def cycle(self, h_b, ip):
        x = np.zeros_like(h_b)
        lib().qudaAmdMultigridCycle(self.h, _vp(x), _vp(h_b), C.byref(ip))
        return x

    def set_half_storage(self, on=True):
        lib().qudaAmdMultigridSetHalfStorage(self.h, int(bool(on)))

    # ---- introspection (include/quda_amd_ext.h): reference CPU orders, fp32 complex ----
    def levels(self):
        return lib().qudaAmdMultigridLevels(self.h)

    def level_info(self, level):
        a = (_i * 18)()
        lib().qudaAmdMultigridLevelInfo(self.h, level, a)
        v = list(a)
        return dict(Xf=v[0:4], Xc=v[4:8], fineSpin=v[8], fineColor=v[9], Nvec=v[10], geo_bs=v[11:15], spin_bs=v[15], null_method=v[16], null_iters=v[17])

    def refine(self, passes=1, cycles=1):
        """set-up refinement: inverse iteration of the null vectors through the current hierarchy, hierarchy rebuilt; seconds spent"""
        return float(lib().qudaAmdMultigridRefine(self.h, int(passes), int(cycles)))

    def ortho_fallback_blocks(self, level):
        return int(lib().qudaAmdMultigridOrthoFallbackBlocks(self.h, int(level)))

    def null_vector(self, level, k):
        i = self.level_info(level)
        out = np.zeros((int(np.prod(i["Xf"])), i["fineSpin"], i["fineColor"]), dtype=np.complex64)
        lib().qudaAmdMultigridGetNullVector(self.h, level, k, _vp(out))
        return out

    def V(self, level):
        i = self.level_info(level)
        out = np.zeros((int(np.prod(i["Xf"])), i["fineSpin"], i["fineColor"], i["Nvec"]), dtype=np.complex64)
        lib().qudaAmdMultigridGetV(self.h, level, _vp(out))
        return out

    def coarse_links(self, level):
        i = self.level_info(level)
        Vc, n = int(np.prod(i["Xc"])), 2 * i["Nvec"]
        Y = np.zeros((8, Vc, n, n), dtype=np.complex64)
        X = np.zeros((Vc, n, n), dtype=np.complex64)
        lib().qudaAmdMultigridGetCoarseLinks(self.h, level, _vp(Y), _vp(X))
        return Y, X

    def apply_block(self, level, h_in, niter=0):
        """M of `level` on a batch (nrhs, sites, spin, colour) complex64 through the multi-right-hand-side kernels — the MFMA coarse
        operator on a coarse level, the 8/16/24/32-right-hand-side stencil (Wilson / twisted mass / twisted clover) on level 0;
        returns (out, seconds per application if niter > 0)"""
        h_in = np.ascontiguousarray(h_in, dtype=np.complex64)
        out = np.zeros_like(h_in)
        secs = lib().qudaAmdMultigridApplyBlock(self.h, int(level), int(h_in.shape[0]), _vp(out), _vp(h_in), int(niter))
        return out, secs

    def time_apply(self, level, niter=20):
        return lib().qudaAmdMultigridTimeApply(self.h, int(level), int(niter))

    def time_transfer(self, level, what, niter=20):
        """seconds per restriction (what = 'R') or prolongation ('P') between level and level + 1"""
        return lib().qudaAmdMultigridTimeTransfer(self.h, int(level), 1 if what == 'P' else 0, int(niter))

    def apply(self, level, op, h_in):
        """op 'R' (level -> level+1), 'P' (level+1 -> level), 'M' (operator of `level`); fields as (sites, spin, colour) complex64"""
        i = self.level_info(level) if op not in ("M", "K") or level < self.levels() - 1 else None
        if i is None:
            j = self.level_info(level - 1)
            fine_shape = (int(np.prod(j["Xc"])), 2, j["Nvec"])
            coarse_shape = None
        else:
            fine_shape = (int(np.prod(i["Xf"])), i["fineSpin"], i["fineColor"])
            coarse_shape = (int(np.prod(i["Xc"])), 2, i["Nvec"])
        shape_in, shape_out = {"R": (fine_shape, coarse_shape), "P": (coarse_shape, fine_shape), "M": (fine_shape, fine_shape), "K": (fine_shape, fine_shape)}[op]
        h_in = np.ascontiguousarray(h_in, dtype=np.complex64).reshape(shape_in)
        out = np.zeros(shape_out, dtype=np.complex64)
        lib().qudaAmdMultigridApply(self.h, level, {"R": 0, "P": 1, "M": 2, "K": 3}[op], _vp(out), _vp(h_in))
        return out

    TRANSFER_OPS = {"R": 0, "P": 1, "R4": 2, "P4": 3, "R4Block": 4, "P4Block": 5, "P4Block+": 6}

    def apply_transfer(self, level, op, h_in, parity=-1, preload=None):
        """one transfer operator of `level` on host vectors (qudaAmdMultigridApplyTransfer): 'R' / 'P' on one vector, 'R4' / 'P4' and
        'R4Block' on four (leading axis 4), 'P4Block' / 'P4Block+' (accumulate) on four coarse vectors with `preload` = the eight fine
        vectors the block field holds beforehand, returning all eight columns.  parity 0 / 1: single-parity fine fields"""
        i = self.level_info(level)
        fine_shape = (int(np.prod(i["Xf"])), i["fineSpin"], i["fineColor"])
        coarse_shape = (int(np.prod(i["Xc"])), 2, i["Nvec"])
        code = self.TRANSFER_OPS[op]
        n = 1 if code < 2 else 4
        restrict = op.startswith("R")
        h_in = np.ascontiguousarray(h_in, dtype=np.complex64).reshape((n,) + (fine_shape if restrict else coarse_shape))
        if code >= 5:
            h_in = np.concatenate([h_in.reshape(-1), np.ascontiguousarray(preload, dtype=np.complex64).reshape((8,) + fine_shape).reshape(-1)])
        out = np.zeros(((8 if code >= 5 else n),) + (coarse_shape if restrict else fine_shape), dtype=np.complex64)
        lib().qudaAmdMultigridApplyTransfer(self.h, int(level), code, int(parity), _vp(out), _vp(h_in))
        return out[0] if n == 1 else out

    # ---- the even-odd preconditioned coarse operator piece by piece (quda_amd_ext.h) ----
    SITE_LINKS = {"links": 0, "hat": 1, "links16": 2, "hat16": 3}
    PC_OPS = {"M": 0, "prepare": 1, "reconstruct": 2}

    def _coarse_shape(self, level):
        i = self.level_info(level)
        return int(np.prod(i["Xc"])), 2, i["Nvec"]

    def coarse_site_links(self, level, which="links"):
        """(sites, 9, n, n) complex64: the matrices every site of level + 1 multiplies with (m = 2 mu forward, 2 mu + 1 backward, 8 local);
        'links', 'hat' (Xinv H_d, 8 = Xinv), 'links16' / 'hat16': the fp16 mirrors widened"""
        Vc, _, nvec = self._coarse_shape(level)
        out = np.zeros((Vc, 9, 2 * nvec, 2 * nvec), dtype=np.complex64)
        lib().qudaAmdMultigridGetCoarseSiteLinks(self.h, int(level), self.SITE_LINKS[which], _vp(out))
        return out

    def coarse_apply(self, level, which, mmask, h_in, parity=-1):
        """applyCoarse of level + 1 with 'links' or 'hat' and matrix mask mmask; parity 0 / 1: h_in and the result are parity fields (h_in the
        half the call reads: the other parity for hops, the same for mmask == 1 << 8)"""
        Vc, ns, nvec = self._coarse_shape(level)
        shape = (Vc if parity < 0 else Vc // 2, ns, nvec)
        h_in = np.ascontiguousarray(h_in, dtype=np.complex64).reshape(shape)
        out = np.zeros(shape, dtype=np.complex64)
        changed = lib().qudaAmdMultigridCoarseApply(self.h, int(level), self.SITE_LINKS[which], int(mmask), int(parity), _vp(out), _vp(h_in))
        if changed:
            raise RuntimeError("the coarse operator changed %d words of its input field" % changed)
        return out

    def coarse_pc(self, level, impl, op, matpc, x=None, b=None):
        """one Schur piece of the even-odd preconditioned operator of level + 1 with matpc parity `matpc`: op 'M' (x: parity fields), 'prepare'
        (b: full sources), 'reconstruct' (x: the solved parity, b: full sources).  impl 0: DiracCoarsePC on one vector; impl 1: the block-field
        routines on 8 / 16 / 24 vectors (leading axis).  Returns (full fields, nonzero words found where the block cycle relies on zeros)"""
        Vc, ns, nvec = self._coarse_shape(level)
        code = self.PC_OPS[op]
        lead = x if x is not None else b
        single = np.ndim(lead) == 3
        nrhs = 1 if single else int(np.shape(lead)[0])
        parts = []
        if code != 1:
            parts.append(np.ascontiguousarray(x, dtype=np.complex64).reshape(nrhs, Vc // 2, ns, nvec).reshape(-1))
        if code != 0:
            parts.append(np.ascontiguousarray(b, dtype=np.complex64).reshape(nrhs, Vc, ns, nvec).reshape(-1))
        h_in = np.ascontiguousarray(np.concatenate(parts))
        out = np.zeros((nrhs, Vc, ns, nvec), dtype=np.complex64)
        leaked = lib().qudaAmdMultigridCoarsePC(self.h, int(level), int(impl), code, int(matpc), nrhs, _vp(out), _vp(h_in))
        return (out[0] if single else out), int(leaked)

    def fused_stats(self, level):
        """None if `level` does not run its cycle as one persistent kernel (coarse_cycle.h), else the last launch's counters"""
        a = (C.c_longlong * 5)()
        if not lib().qudaAmdMultigridFusedStats(self.h, int(level), a):
            return None
        return dict(barriers=int(a[0]), gcr_iters=int(a[1]), gcr_restarts=int(a[2]), halo_exchanges=int(a[3]), grid=int(a[4]))

    def free(self):
        if self.h:
            lib().destroyMultigridQuda(self.h)
            self.h = None
