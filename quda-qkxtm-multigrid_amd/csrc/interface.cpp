// interface.cpp — the quda.h C ABI.  Thin re-statement of the reference's interface layer
// (lib/interface_quda.cpp:119-145 resident-field globals, :285-520 init, :521-730 loadGaugeQuda,
// :730-930 loadCloverQuda, :1265-1412 setDiracParam/createDirac/massRescale, :1496 dslashQuda,
// :1716 MatQuda, :1796 MatDagMatQuda) on top of the CDNA4 field/operator classes.
#include <cmath>
#include <cstring>
#include <functional>
#include <sys/time.h>

#include "blas.h"
#include "dirac.h"
#include "eig.h"
#include "interface_internal.h"
#include "tune.h"
#include "halo.h"
#include "p2p.h"
#include "quda_amd_ext.h"

namespace quda {

void setVerbosityInternal(QudaVerbosity v, const char *prefix, FILE *f);
void createStreams();
void destroyStreams();
void freeStagingBuffer();
void freeBlockTables();

// resident fields (reference lib/interface_quda.cpp:119-145)
GaugeField *gaugePrecise = nullptr, *gaugeSloppy = nullptr, *gaugePrecondition = nullptr, *gaugeSmeared = nullptr;
MomField *momResident = nullptr;   // the momentum of gauge molecular dynamics (reference lib/interface_quda.cpp:128)
CloverField *cloverPrecise = nullptr, *cloverSloppy = nullptr, *cloverPrecondition = nullptr;
static bool g_initialized = false, g_comms_initialized = false;
static int g_device = -1;
static LatticeGeom g_geom;
static QudaGaugeParam g_gauge_param;

// host copies kept so sloppy/precondition clover fields and MG setup can be (re)built
const LatticeGeom &residentGeom() { return g_geom; }

GaugeField *residentGauge(int which) {
  GaugeField *g = which == 0 ? gaugePrecise : (which == 1 ? gaugeSloppy : gaugePrecondition);
  if (!g) errorQuda("Gauge field not allocated");
  return g;
}
CloverField *residentClover(int which) { return which == 0 ? cloverPrecise : (which == 1 ? cloverSloppy : cloverPrecondition); }

// reference lib/interface_quda.cpp:1265-1340
void setDiracParam(DiracParam &dp, QudaInvertParam *inv, const bool pc) {
  switch (inv->dslash_type) {
    case QUDA_WILSON_DSLASH: dp.type = pc ? QUDA_WILSONPC_DIRAC : QUDA_WILSON_DIRAC; break;
    case QUDA_TWISTED_MASS_DSLASH:
      dp.type = pc ? QUDA_TWISTED_MASSPC_DIRAC : QUDA_TWISTED_MASS_DIRAC;
      if (inv->twist_flavor != QUDA_TWIST_MINUS && inv->twist_flavor != QUDA_TWIST_PLUS && inv->twist_flavor != QUDA_TWIST_NONDEG_DOUBLET)
        errorQuda("twist_flavor %d: the degenerate +-1 flavours and the non-degenerate doublet are on this library's path", inv->twist_flavor);
      if (inv->twist_flavor == QUDA_TWIST_NONDEG_DOUBLET) {
        if (!(inv->epsilon == inv->epsilon)) errorQuda("non-degenerate doublet: parameter epsilon undefined");
        if (inv->inv_type_precondition == QUDA_MG_INVERTER) errorQuda("non-degenerate doublet: a multigrid preconditioner is not available for it");
        double a, b, d;
        ndegTwistCoefficients(inv->kappa, inv->mu, inv->epsilon, true, false, a, b, d);   // stops here if the twist has no inverse
      }
      break;
    case QUDA_TWISTED_CLOVER_DSLASH:
      dp.type = pc ? QUDA_TWISTED_CLOVERPC_DIRAC : QUDA_TWISTED_CLOVER_DIRAC;
      if (inv->twist_flavor == QUDA_TWIST_NONDEG_DOUBLET) errorQuda("twisted clover has no non-degenerate doublet operator (twist_flavor %d)", inv->twist_flavor);
      if (inv->twist_flavor != QUDA_TWIST_MINUS && inv->twist_flavor != QUDA_TWIST_PLUS) errorQuda("twist_flavor %d not supported", inv->twist_flavor);
      break;
    default: errorQuda("Unsupported dslash_type %d (Wilson, twisted-mass and twisted-clover are implemented)", inv->dslash_type);
  }
  dp.matpcType = inv->matpc_type;
  dp.dagger = inv->dagger;
  dp.gauge = gaugePrecise;
  dp.clover = cloverPrecise;
  dp.kappa = inv->kappa;
  dp.mass = inv->mass;
  dp.m5 = inv->m5;
  dp.mu = inv->mu;
  dp.epsilon = inv->twist_flavor == QUDA_TWIST_NONDEG_DOUBLET ? inv->epsilon : 0.0;
  for (int i = 0; i < 4; i++) dp.commDim[i] = 1;
}
void setDiracSloppyParam(DiracParam &dp, QudaInvertParam *inv, const bool pc) {
  setDiracParam(dp, inv, pc);
  dp.gauge = gaugeSloppy ? gaugeSloppy : gaugePrecise;
  dp.clover = cloverSloppy ? cloverSloppy : cloverPrecise;
}
void setDiracPreParam(DiracParam &dp, QudaInvertParam *inv, const bool pc) {
  setDiracParam(dp, inv, pc);
  dp.gauge = gaugePrecondition ? gaugePrecondition : (gaugeSloppy ? gaugeSloppy : gaugePrecise);
  dp.clover = cloverPrecondition ? cloverPrecondition : (cloverSloppy ? cloverSloppy : cloverPrecise);
}

static void checkResident(const QudaInvertParam *inv) {
  if (!g_initialized) errorQuda("QUDA not initialized");
  if (!gaugePrecise) errorQuda("Gauge field not allocated");
  if (!cloverPrecise && inv->dslash_type == QUDA_TWISTED_CLOVER_DSLASH) errorQuda("Clover field not allocated");
  if (inv->dslash_type == QUDA_TWISTED_CLOVER_DSLASH && inv->twist_flavor == QUDA_TWIST_NONDEG_DOUBLET)
    errorQuda("twisted clover has no non-degenerate doublet operator (twist_flavor %d)", inv->twist_flavor);
}

// the twist flavour the fields of a C ABI call carry: only the twisted-mass operator has a doublet, so a QUDA_TWIST_NONDEG_DOUBLET left in the
// parameters of a Wilson call (where twist_flavor means nothing) does not make two-flavour fields
QudaTwistFlavorType fieldTwistFlavor(const QudaInvertParam &inv) {
  return inv.twist_flavor == QUDA_TWIST_NONDEG_DOUBLET && inv.dslash_type != QUDA_TWISTED_MASS_DSLASH ? QUDA_TWIST_NO : inv.twist_flavor;
}

ColorSpinorParam deviceSpinorParam(QudaPrecision prec, QudaSiteSubset subset, QudaTwistFlavorType flavor) {
  ColorSpinorParam p;
  p.location = QUDA_CUDA_FIELD_LOCATION;
  for (int d = 0; d < 4; d++) p.x[d] = g_geom.X[d];
  if (subset == QUDA_PARITY_SITE_SUBSET) p.x[0] /= 2;
  p.siteSubset = subset;
  p.precision = prec;
  p.twistFlavor = flavor;
  if (flavor == QUDA_TWIST_NONDEG_DOUBLET) p.setFlavors(2);
  p.create = QUDA_NULL_FIELD_CREATE;
  return p;
}

}  // namespace quda

QudaTune getTuning();   // include/util_quda.h (global namespace; that header's logging macros clash with qa_core.h's here)
void setTuning(QudaTune tune);

using namespace quda;

// ================================================================================================
extern "C" {

void setVerbosityQuda(QudaVerbosity verbosity, const char prefix[], FILE *outfile) { setVerbosityInternal(verbosity, prefix, outfile); }

void initQudaDevice(int dev) {
  if (g_device >= 0) return;
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n == 0) errorQuda("No HIP devices found — this library has no CPU fallback");
  if (dev < 0) dev = commGrid().rank % n;  // rank-local index (reference :403-408)
  if (dev >= n) errorQuda("Device %d does not exist (%d visible)", dev, n);
  HIP_CHECK(hipSetDevice(dev));
  g_device = dev;
  hipDeviceProp_t prop;
  HIP_CHECK(hipGetDeviceProperties(&prop, dev));
  if (getVerbosity() >= QUDA_SUMMARIZE) printfQuda("QUDA-AMD %d.%d.%d: device %d = %s (%s), %d CUs\n", QUDA_VERSION_MAJOR, QUDA_VERSION_MINOR, QUDA_VERSION_SUBMINOR, dev, prop.name, prop.gcnArchName, prop.multiProcessorCount);
}

void initQudaMemory(void) {
  if (g_initialized) return;
  if (!g_comms_initialized) {
    const int one[4] = {1, 1, 1, 1};
    initCommsGridQuda(4, one, nullptr, nullptr);
  }
  createStreams();
  blas::init();
  loadTuneCache();   // reference initQudaMemory: loadTuneCache() (lib/interface_quda.cpp:468)
  g_initialized = true;
}

void initQuda(int device) {
  if (!g_comms_initialized) {
    const int one[4] = {1, 1, 1, 1};
    initCommsGridQuda(4, one, nullptr, nullptr);
  }
  initQudaDevice(device);
  initQudaMemory();
}

void endQuda(void) {
  if (!g_initialized) return;
  saveTuneCache();   // reference endQuda: saveTuneCache() (lib/interface_quda.cpp:1069)
  tuneCacheClear();
  freeGaugeQuda();
  freeCloverQuda();
  freeStagingBuffer();
  freeBlockTables();
  freeFineBlockDots();
  eigKernelsEnd();
  poolDeviceFlush();
  blas::end();
  commFinalize();
  destroyStreams();
  g_initialized = false;
  g_comms_initialized = false;
  g_device = -1;
}

// reference :285 -> comm_init (lib/comm_mpi.cpp:50); transport here is RCCL, bootstrapped by the launcher (comm.cpp)
void initCommsGridQuda(int nDim, const int *dims, QudaCommsMap func, void *fdata) {
  if (nDim != 4) errorQuda("Number of communication grid dimensions must be 4");
  commInit(dims, func, fdata);
  g_comms_initialized = true;
}

// ---- param constructors / printers (reference lib/check_params.h X-macros) ----
QudaGaugeParam newQudaGaugeParam(void) {
  QudaGaugeParam p;
  memset(&p, 0, sizeof(p));
  p.location = QUDA_CPU_FIELD_LOCATION;
  for (int d = 0; d < 4; d++) p.X[d] = INT_MIN;
  p.anisotropy = NAN; p.tadpole_coeff = NAN; p.scale = 1.0;
  p.type = QUDA_INVALID_LINKS; p.gauge_order = QUDA_INVALID_GAUGE_ORDER; p.t_boundary = QUDA_INVALID_T_BOUNDARY;
  p.cpu_prec = p.cuda_prec = p.cuda_prec_sloppy = p.cuda_prec_precondition = QUDA_INVALID_PRECISION;
  p.reconstruct = p.reconstruct_sloppy = p.reconstruct_precondition = QUDA_RECONSTRUCT_INVALID;
  p.gauge_fix = QUDA_GAUGE_FIXED_INVALID;
  p.ga_pad = INT_MIN;
  p.staggered_phase_type = QUDA_INVALID_STAGGERED_PHASE;
  p.make_resident_gauge = 1; p.return_result_gauge = 1;
  return p;
}

QudaInvertParam newQudaInvertParam(void) {
  QudaInvertParam p;
  memset(&p, 0, sizeof(p));
  p.input_location = p.output_location = QUDA_CPU_FIELD_LOCATION;
  p.dslash_type = QUDA_INVALID_DSLASH; p.inv_type = QUDA_INVALID_INVERTER;
  p.mass = NAN; p.kappa = NAN; p.m5 = NAN; p.Ls = INT_MIN; p.mu = NAN; p.epsilon = NAN;
  p.twist_flavor = QUDA_TWIST_INVALID;
  p.tol = NAN; p.tol_restart = 5e-3; p.tol_hq = 0.0; p.maxiter = INT_MIN; p.reliable_delta = NAN;
  p.use_sloppy_partial_accumulator = 0; p.max_res_increase = 1; p.max_res_increase_total = 10; p.heavy_quark_check = 10;
  p.pipeline = 0; p.num_offset = 0; p.num_src = 1; p.overlap = 0;
  p.solution_type = QUDA_INVALID_SOLUTION; p.solve_type = QUDA_INVALID_SOLVE; p.matpc_type = QUDA_MATPC_INVALID;
  p.dagger = QUDA_DAG_INVALID; p.mass_normalization = QUDA_INVALID_NORMALIZATION;
  p.solver_normalization = QUDA_DEFAULT_NORMALIZATION; p.preserve_source = QUDA_PRESERVE_SOURCE_INVALID;
  p.cpu_prec = p.cuda_prec = p.cuda_prec_sloppy = p.cuda_prec_precondition = QUDA_INVALID_PRECISION;
  p.dirac_order = QUDA_INVALID_DIRAC_ORDER; p.gamma_basis = QUDA_INVALID_GAMMA_BASIS;
  p.clover_location = QUDA_CPU_FIELD_LOCATION;
  p.clover_cpu_prec = p.clover_cuda_prec = p.clover_cuda_prec_sloppy = p.clover_cuda_prec_precondition = QUDA_INVALID_PRECISION;
  p.clover_order = QUDA_INVALID_CLOVER_ORDER; p.use_init_guess = QUDA_USE_INIT_GUESS_INVALID;
  p.clover_coeff = NAN;
  p.verbosity = QUDA_INVALID_VERBOSITY; p.sp_pad = INT_MIN; p.cl_pad = INT_MIN;
  p.tune = QUDA_TUNE_INVALID; p.Nsteps = INT_MIN; p.gcrNkrylov = INT_MIN;
  p.inv_type_precondition = QUDA_INVALID_INVERTER; p.preconditioner = p.preconditionerUP = p.preconditionerDN = nullptr;
  p.dslash_type_precondition = QUDA_INVALID_DSLASH; p.verbosity_precondition = QUDA_INVALID_VERBOSITY;
  p.tol_precondition = NAN; p.maxiter_precondition = INT_MIN; p.omega = NAN; p.precondition_cycle = 1;
  p.schwarz_type = QUDA_INVALID_SCHWARZ; p.residual_type = QUDA_L2_RELATIVE_RESIDUAL;
  p.cuda_prec_ritz = QUDA_SINGLE_PRECISION;
  return p;
}

QudaMultigridParam newQudaMultigridParam(void) {
  QudaMultigridParam p;
  memset(&p, 0, sizeof(p));
  p.invert_param = nullptr;
  p.n_level = INT_MIN;
  for (int i = 0; i < QUDA_MAX_MG_LEVEL; i++) {
    for (int d = 0; d < QUDA_MAX_DIM; d++) p.geo_block_size[i][d] = INT_MIN;
    p.spin_block_size[i] = INT_MIN; p.n_vec[i] = INT_MIN;
    p.smoother[i] = QUDA_INVALID_INVERTER; p.coarse_grid_solution_type[i] = QUDA_INVALID_SOLUTION;
    p.smoother_solve_type[i] = QUDA_INVALID_SOLVE; p.cycle_type[i] = QUDA_MG_CYCLE_INVALID;
    p.nu_pre[i] = INT_MIN; p.nu_post[i] = INT_MIN; p.smoother_tol[i] = NAN; p.omega[i] = NAN;
    p.global_reduction[i] = QUDA_BOOLEAN_INVALID; p.location[i] = QUDA_INVALID_FIELD_LOCATION;
  }
  // the reference leaves these two uninitialised; defaults documented in DESIGN.md
  p.setup_maxiter = 500; p.setup_tol = 5e-6;
  p.compute_null_vector = QUDA_COMPUTE_NULL_VECTOR_INVALID;
  p.generate_all_levels = QUDA_BOOLEAN_INVALID; p.run_verify = QUDA_BOOLEAN_INVALID;
  p.delta_muPR = p.delta_kappaPR = p.delta_cswPR = 1.0;
  p.delta_muCG = p.delta_kappaCG = p.delta_cswCG = 1.0;
  return p;
}

void printQudaGaugeParam(QudaGaugeParam *p) {
  printfQuda("QUDA Gauge Parameters:\n");
  printfQuda("X = %d %d %d %d\nanisotropy = %g\ntype = %d\ngauge_order = %d\nt_boundary = %d\ncpu_prec = %d\ncuda_prec = %d\nreconstruct = %d\n"
             "cuda_prec_sloppy = %d\nreconstruct_sloppy = %d\ncuda_prec_precondition = %d\nreconstruct_precondition = %d\ngauge_fix = %d\nga_pad = %d\ngaugeGiB = %g\n",
             p->X[0], p->X[1], p->X[2], p->X[3], p->anisotropy, p->type, p->gauge_order, p->t_boundary, p->cpu_prec, p->cuda_prec, p->reconstruct,
             p->cuda_prec_sloppy, p->reconstruct_sloppy, p->cuda_prec_precondition, p->reconstruct_precondition, p->gauge_fix, p->ga_pad, p->gaugeGiB);
}
void printQudaInvertParam(QudaInvertParam *p) {
  printfQuda("QUDA Inverter Parameters:\n");
  printfQuda("dslash_type = %d\ninv_type = %d\nkappa = %g\nmu = %g\ntwist_flavor = %d\ntol = %g\nmaxiter = %d\nreliable_delta = %g\nsolution_type = %d\n"
             "solve_type = %d\nmatpc_type = %d\ndagger = %d\nmass_normalization = %d\ncpu_prec = %d\ncuda_prec = %d\ncuda_prec_sloppy = %d\n"
             "cuda_prec_precondition = %d\ndirac_order = %d\ngamma_basis = %d\nclover_cpu_prec = %d\nclover_cuda_prec = %d\nclover_order = %d\n"
             "gcrNkrylov = %d\ninv_type_precondition = %d\nverbosity = %d\niter = %d\nsecs = %g\ngflops = %g\ntrue_res = %g\n",
             p->dslash_type, p->inv_type, p->kappa, p->mu, p->twist_flavor, p->tol, p->maxiter, p->reliable_delta, p->solution_type, p->solve_type,
             p->matpc_type, p->dagger, p->mass_normalization, p->cpu_prec, p->cuda_prec, p->cuda_prec_sloppy, p->cuda_prec_precondition, p->dirac_order,
             p->gamma_basis, p->clover_cpu_prec, p->clover_cuda_prec, p->clover_order, p->gcrNkrylov, p->inv_type_precondition, p->verbosity, p->iter,
             p->secs, p->gflops, p->true_res);
}
void printQudaMultigridParam(QudaMultigridParam *p) {
  printfQuda("QUDA Multigrid Parameters:\nn_level = %d\nsetup_maxiter = %d\nsetup_tol = %g\n", p->n_level, p->setup_maxiter, p->setup_tol);
  for (int i = 0; i < p->n_level && i < QUDA_MAX_MG_LEVEL; i++)
    printfQuda("level %d: geo_block = %d %d %d %d spin_block = %d n_vec = %d smoother = %d solve_type = %d cycle = %d nu_pre = %d nu_post = %d omega = %g tol = %g\n", i,
               p->geo_block_size[i][0], p->geo_block_size[i][1], p->geo_block_size[i][2], p->geo_block_size[i][3], p->spin_block_size[i], p->n_vec[i],
               p->smoother[i], p->smoother_solve_type[i], p->cycle_type[i], p->nu_pre[i], p->nu_post[i], p->omega[i], p->smoother_tol[i]);
}

// reference lib/check_params.h via checkGaugeParam (:531)
static void checkGaugeParam(const QudaGaugeParam *p) {
  for (int d = 0; d < 4; d++) if (p->X[d] <= 0 || p->X[d] % 2) errorQuda("Parameter X[%d] = %d undefined or odd", d, p->X[d]);
  if (!(p->anisotropy == p->anisotropy)) errorQuda("Parameter anisotropy undefined");
  if (p->t_boundary != QUDA_ANTI_PERIODIC_T && p->t_boundary != QUDA_PERIODIC_T) errorQuda("Parameter t_boundary undefined");
  if (p->cpu_prec != QUDA_DOUBLE_PRECISION && p->cpu_prec != QUDA_SINGLE_PRECISION) errorQuda("Parameter cpu_prec = %d undefined", p->cpu_prec);
  if (p->cuda_prec != QUDA_DOUBLE_PRECISION && p->cuda_prec != QUDA_SINGLE_PRECISION && p->cuda_prec != QUDA_HALF_PRECISION) errorQuda("Parameter cuda_prec = %d undefined", p->cuda_prec);
  if (p->reconstruct != QUDA_RECONSTRUCT_NO && p->reconstruct != QUDA_RECONSTRUCT_12 && p->reconstruct != QUDA_RECONSTRUCT_8) errorQuda("Parameter reconstruct = %d: this library implements 18, 12 and 8", p->reconstruct);
  if (p->gauge_order != QUDA_QDP_GAUGE_ORDER) errorQuda("Parameter gauge_order = %d: only QUDA_QDP_GAUGE_ORDER host fields are supported", p->gauge_order);
  if (p->type != QUDA_WILSON_LINKS) errorQuda("Parameter type = %d: only Wilson (SU(3)) links are on this path", p->type);
}

static void freeResidentLinks() {
  delete gaugePrecise; delete gaugeSloppy; delete gaugePrecondition; delete gaugeSmeared;   // reference :1001-1008
  gaugePrecise = gaugeSloppy = gaugePrecondition = gaugeSmeared = nullptr;
}

// the precise, sloppy and preconditioner copies from host QDP links; whatever was resident (a smeared field included) goes
static void loadResidentLinks(void *h_gauge, QudaGaugeParam *param) {
  freeResidentLinks();
  g_geom = LatticeGeom(param->X);
  g_gauge_param = *param;
  void **links = (void **)h_gauge;
  gaugePrecise = new GaugeField(g_geom, param->cuda_prec, param->reconstruct, param->t_boundary, param->anisotropy);
  loadGaugeWithHalo(*gaugePrecise, links, param->cpu_prec);
  double gib = gaugePrecise->GiB();
  auto valid = [](QudaPrecision p) { return p == QUDA_DOUBLE_PRECISION || p == QUDA_SINGLE_PRECISION || p == QUDA_HALF_PRECISION; };
  if (valid(param->cuda_prec_sloppy) && (param->cuda_prec_sloppy != param->cuda_prec || param->reconstruct_sloppy != param->reconstruct)) {
    QudaReconstructType r = (param->reconstruct_sloppy == QUDA_RECONSTRUCT_12 || param->reconstruct_sloppy == QUDA_RECONSTRUCT_8) ? param->reconstruct_sloppy : QUDA_RECONSTRUCT_NO;
    gaugeSloppy = new GaugeField(g_geom, param->cuda_prec_sloppy, r, param->t_boundary, param->anisotropy);
    loadGaugeWithHalo(*gaugeSloppy, links, param->cpu_prec);
    gib += gaugeSloppy->GiB();
  }
  const QudaPrecision sp = gaugeSloppy ? gaugeSloppy->precision : gaugePrecise->precision;
  const QudaReconstructType sr = gaugeSloppy ? gaugeSloppy->reconstruct : gaugePrecise->reconstruct;
  if (valid(param->cuda_prec_precondition) && (param->cuda_prec_precondition != sp || (param->reconstruct_precondition != sr && param->reconstruct_precondition != QUDA_RECONSTRUCT_INVALID))) {
    QudaReconstructType r = (param->reconstruct_precondition == QUDA_RECONSTRUCT_12 || param->reconstruct_precondition == QUDA_RECONSTRUCT_8) ? param->reconstruct_precondition : QUDA_RECONSTRUCT_NO;
    gaugePrecondition = new GaugeField(g_geom, param->cuda_prec_precondition, r, param->t_boundary, param->anisotropy);
    loadGaugeWithHalo(*gaugePrecondition, links, param->cpu_prec);
    gib += gaugePrecondition->GiB();
  }
  param->gaugeGiB = gib;
}

void loadGaugeQuda(void *h_gauge, QudaGaugeParam *param) {
  if (!g_initialized) errorQuda("QUDA not initialized");
  checkGaugeParam(param);
  freeGaugeQuda();
  loadResidentLinks(h_gauge, param);
}

void freeGaugeQuda(void) {
  freeResidentLinks();
  delete momResident;
  momResident = nullptr;
}

// reference lib/interface_quda.cpp:694-728: the resident (precise) links back to the host in the order of param
void saveGaugeQuda(void *h_gauge, QudaGaugeParam *param) {
  if (!g_initialized) errorQuda("QUDA not initialized");
  if (!gaugePrecise) errorQuda("saveGaugeQuda: no resident gauge field");
  if (param->gauge_order != QUDA_QDP_GAUGE_ORDER) errorQuda("gauge_order %d: only QUDA_QDP_GAUGE_ORDER host fields are supported", param->gauge_order);
  saveGaugeQDP(*gaugePrecise, (void *const *)h_gauge, param->cpu_prec);
}

// reference lib/interface_quda.cpp:5510-5563 (lib/gauge_plaq.cu)
void plaqQuda(double plaq[3]) {
  if (!g_initialized) errorQuda("QUDA not initialized");
  if (!gaugePrecise) errorQuda("Cannot compute plaquette as there is no resident gauge field");
  plaquette(*gaugePrecise, plaq);
}

// reference lib/interface_quda.cpp:5565-5640 (lib/gauge_ape.cu): nSteps APE steps on a copy of the resident links; the result
// stays inside the library (gaugeSmeared) until freeGaugeQuda / the next call
void performAPEnStep(unsigned int nSteps, double alpha) {
  if (!g_initialized) errorQuda("QUDA not initialized");
  if (!gaugePrecise) errorQuda("Gauge field must be loaded");
  delete gaugeSmeared;
  gaugeSmeared = apeSmear(*gaugePrecise, nSteps, alpha);
  if (getVerbosity() >= QUDA_VERBOSE) {
    double p0[3], p1[3];
    plaquette(*gaugePrecise, p0); plaquette(*gaugeSmeared, p1);
    printfQuda("Plaquette after 0 APE steps: %le\nPlaquette after %u APE steps: %le\n", p0[0], nSteps, p1[0]);
  }
}

// reference lib/interface_quda.cpp:5640-5713 (lib/gauge_stout.cu): as performAPEnStep with the stout link update; smear_time = 1
// also smears the time links and takes the staples of all six planes
void qudaAmdStoutSmear(unsigned int nSteps, double rho, int smear_time) {
  if (!g_initialized) errorQuda("QUDA not initialized");
  if (!gaugePrecise) errorQuda("Gauge field must be loaded");
  delete gaugeSmeared;
  gaugeSmeared = nullptr;
  gaugeSmeared = stoutSmear(*gaugePrecise, nSteps, rho, smear_time ? 4 : 3);
  if (getVerbosity() >= QUDA_VERBOSE) {
    double p0[3], p1[3];
    plaquette(*gaugePrecise, p0); plaquette(*gaugeSmeared, p1);
    printfQuda("Plaquette after 0 STOUT steps: %le\nPlaquette after %u STOUT steps: %le\n", p0[0], nSteps, p1[0]);
  }
}
void performSTOUTnStep(unsigned int nSteps, double rho) { qudaAmdStoutSmear(nSteps, rho, 0); }

// dst[lexicographic site] = eo[even sites, then odd], realsPerSite reals a site
static void eoToLex(double *dst, const double *eo, const LatticeGeom &g, int realsPerSite) {
  for (long iv = 0; iv < g.V; iv++) {
    long l = iv / g.X[0];
    const int x = (int)(iv % g.X[0]), y = (int)(l % g.X[1]); l /= g.X[1];
    const int z = (int)(l % g.X[2]), t = (int)(l / g.X[2]);
    const int parity = (x + y + z + t) & 1;
    memcpy(dst + iv * realsPerSite, eo + ((size_t)parity * g.Vh + iv / 2) * realsPerSite, realsPerSite * sizeof(double));
  }
}

// reference lib/interface_quda.cpp:5940-5991 (lib/field_strength_tensor.cu, lib/qcharge_quda.cu)
double qudaAmdQCharge(double *h_density, int lexicographic, int which) {
  if (!g_initialized) errorQuda("QUDA not initialized");
  if (which < -1 || which > 1) errorQuda("qudaAmdQCharge: which = %d (-1: smeared field if resident, 0: resident links, 1: smeared field)", which);
  if (which == 1 && !gaugeSmeared) errorQuda("qudaAmdQCharge: no smeared field is resident (performAPEnStep / performSTOUTnStep)");
  const GaugeField *U = (which == 0 || !gaugeSmeared) ? gaugePrecise : gaugeSmeared;
  if (!U) errorQuda("Gauge field must be loaded");
  if (!h_density || !lexicographic) return topologicalCharge(*U, h_density);
  const LatticeGeom &g = U->geom;
  std::vector<double> eo((size_t)g.V);
  const double Q = topologicalCharge(*U, eo.data());
  eoToLex(h_density, eo.data(), g, 1);
  return Q;
}
double qChargeCuda(void) { return qudaAmdQCharge(nullptr, 0, -1); }

void qudaAmdSu3ExpIQ(int n, const double *q, double *out) {
  if (!g_initialized) errorQuda("QUDA not initialized");
  if (n < 0 || (n > 0 && (!q || !out))) errorQuda("qudaAmdSu3ExpIQ: n = %d, q = %p, out = %p", n, (const void *)q, (void *)out);
  su3ExpIQ(n, q, out);
}

void qudaAmdSaveSmearedGauge(void **h_gauge, int lexicographic) {
  if (!gaugeSmeared) errorQuda("qudaAmdSaveSmearedGauge: no smeared field (call performAPEnStep first)");
  if (!lexicographic) { saveGaugeQDP(*gaugeSmeared, (void *const *)h_gauge, QUDA_DOUBLE_PRECISION); return; }
  const LatticeGeom &g = gaugeSmeared->geom;
  HostLinks eo(g.V);
  saveGaugeQDP(*gaugeSmeared, eo.ptr, QUDA_DOUBLE_PRECISION);
  for (int d = 0; d < 4; d++) eoToLex((double *)h_gauge[d], eo.links[d].data(), g, 18);
}

// ---- gauge molecular dynamics (gauge_md.hip).  Host links in QUDA_QDP_GAUGE_ORDER and host momenta in the MILC ten-real layout
// only, both fp64.  A call that makes new links resident rebuilds the precise, sloppy and preconditioner copies through the loader
// and drops the smeared field; a resident clover term and multigrid hierarchy belong to the old links and are the caller's to
// rebuild, as in the reference.  Unlike the reference, a resident field that a call uses without replacing it stays resident. ----
static void checkMdParam(const char *fn, const QudaGaugeParam *p) {
  if (!g_initialized) errorQuda("QUDA not initialized");
  if (p->gauge_order != QUDA_QDP_GAUGE_ORDER)
    errorQuda("%s: gauge_order = %d: only QUDA_QDP_GAUGE_ORDER host links (and MILC-order ten-real momenta) are supported", fn, p->gauge_order);
  if (p->cpu_prec != QUDA_DOUBLE_PRECISION) errorQuda("%s: fp64 host fields only", fn);
}
// the links a call works on: the resident ones, or the host links loaded into a field of the precision and reconstruct of param
static GaugeField *mdLinks(const char *fn, void *h_gauge, QudaGaugeParam *param, bool &owned) {
  owned = false;
  if (param->use_resident_gauge) {
    if (!gaugePrecise) errorQuda("%s: No resident gauge field to use", fn);
    return gaugePrecise;
  }
  checkGaugeParam(param);
  GaugeField *U = new GaugeField(LatticeGeom(param->X), param->cuda_prec, param->reconstruct, param->t_boundary, param->anisotropy);
  loadGaugeWithHalo(*U, (void **)h_gauge, param->cpu_prec);
  owned = true;
  return U;
}
static MomField *mdMomentum(const char *fn, void *h_mom, const QudaGaugeParam *param, const LatticeGeom &geom, bool load, bool &owned) {
  owned = false;
  if (param->use_resident_mom) {
    if (!momResident) errorQuda("%s: No resident momentum field to use", fn);
    if (!(momResident->geom == geom)) errorQuda("%s: the resident momentum differs in geometry from the links", fn);
    return momResident;
  }
  MomField *m = new MomField(geom);
  if (load) m->load(h_mom);
  owned = true;
  return m;
}
static void keepMomentum(MomField *m, bool owned, const QudaGaugeParam *param) {
  if (param->make_resident_mom) {
    if (momResident && momResident != m) delete momResident;
    momResident = m;
  } else if (owned) {
    delete m;
  }
}
// new host QDP links become the resident field, in the precisions of the resident field they replace (else of param)
static void makeLinksResident(HostLinks &links, QudaGaugeParam *param, bool hadResident) {
  QudaGaugeParam gp = hadResident ? g_gauge_param : *param;
  gp.cpu_prec = QUDA_DOUBLE_PRECISION;
  gp.gauge_order = QUDA_QDP_GAUGE_ORDER;
  if (!hadResident) checkGaugeParam(&gp);
  loadResidentLinks(links.ptr, &gp);
  param->gaugeGiB = gp.gaugeGiB;
}

// reference lib/interface_quda.cpp:3799-3935 (lib/gauge_force.cu)
int computeGaugeForceQuda(void *mom, void *sitelink, int ***input_path_buf, int *path_length, double *loop_coeff, int num_paths, int max_length,
                          double dt, QudaGaugeParam *qudaGaugeParam) {
  QudaGaugeParam *param = qudaGaugeParam;
  checkMdParam("computeGaugeForceQuda", param);
  if (max_length > kGaugeForceMaxLength) errorQuda("computeGaugeForceQuda: max_length = %d exceeds the cap of %d links per path", max_length, kGaugeForceMaxLength);
  bool ownU, ownM;
  GaugeField *U;
  if (!param->use_resident_gauge && param->make_resident_gauge) {   // the host links become the resident field first
    checkGaugeParam(param);
    loadResidentLinks(sitelink, param);
    U = gaugePrecise; ownU = false;
  } else {
    U = mdLinks("computeGaugeForceQuda", sitelink, param, ownU);
  }
  MomField *M = mdMomentum("computeGaugeForceQuda", mom, param, U->geom, !param->overwrite_mom, ownM);
  if (param->use_resident_mom && param->overwrite_mom) M->zero();
  gaugeForce(*M, *U, dt, input_path_buf, path_length, loop_coeff, num_paths, max_length);
  if (param->return_result_mom) M->save(mom);
  if (ownU) delete U;
  keepMomentum(M, ownM, param);
  return 0;
}

// reference lib/interface_quda.cpp:5081-5185 (lib/gauge_update_quda.cu)
void updateGaugeFieldQuda(void *gauge, void *momentum, double dt, int conj_mom, int exact, QudaGaugeParam *param) {
  checkMdParam("updateGaugeFieldQuda", param);
  bool ownU, ownM;
  GaugeField *U = mdLinks("updateGaugeFieldQuda", gauge, param, ownU);
  MomField *M = mdMomentum("updateGaugeFieldQuda", momentum, param, U->geom, true, ownM);
  const size_t n = (size_t)U->geom.V * 18;
  HostLinks links(U->geom.V);
  updateGaugeLinks(links.ptr, *U, *M, dt, conj_mom != 0, exact != 0);
  if (ownU) delete U;
  if (param->return_result_gauge) for (int d = 0; d < 4; d++) memcpy(((void **)gauge)[d], links.ptr[d], n * sizeof(double));
  if (param->make_resident_gauge) makeLinksResident(links, param, !ownU);
  keepMomentum(M, ownM, param);
}

// reference lib/interface_quda.cpp:5187-5247
void projectSU3Quda(void *gauge_h, double tol, QudaGaugeParam *param) {
  checkMdParam("projectSU3Quda", param);
  bool ownU;
  GaugeField *U = mdLinks("projectSU3Quda", gauge_h, param, ownU);
  const size_t n = (size_t)U->geom.V * 18;
  HostLinks links(U->geom.V);
  const long failures = projectSU3Links(links.ptr, *U, tol);
  if (ownU) delete U;
  if (failures > 0) errorQuda("Error in the SU(3) unitarization: %ld failures", failures);
  if (param->return_result_gauge) for (int d = 0; d < 4; d++) memcpy(((void **)gauge_h)[d], links.ptr[d], n * sizeof(double));
  if (param->make_resident_gauge) makeLinksResident(links, param, !ownU);
}

// reference lib/interface_quda.cpp:5716-5826 (lib/gauge_fix_ovr.cu).  Unlike the reference, which always reloads the host links and
// leaves them resident, the fields follow the flags of the molecular-dynamics calls above
int qudaAmdGaugeFixOVR(void *gauge, const unsigned int gauge_dir, const unsigned int Nsteps, const unsigned int verbose_interval, const double relax_boost,
                       const double tolerance, const unsigned int reunit_interval, const unsigned int stopWtheta, QudaGaugeParam *param, double *timeinfo,
                       void *h_transform, double info[4]) {
  const char *fn = "computeGaugeFixingOVRQuda";
  checkMdParam(fn, param);
  if (reunit_interval == 0) errorQuda("%s: reunit_interval = 0: the links are projected when iteration %% reunit_interval == reunit_interval - 1", fn);
  if (Nsteps > 0x7fffffffu || reunit_interval > 0x7fffffffu || verbose_interval > 0x7fffffffu) errorQuda("%s: Nsteps, reunit_interval and verbose_interval have to fit an int", fn);
  bool ownU;
  GaugeField *U = mdLinks(fn, gauge, param, ownU);
  const size_t n = (size_t)U->geom.V * 18;
  HostLinks links(U->geom.V);
  double secs[3] = {0, 0, 0};
  const GaugeFixResult res = gaugeFixOVR(links.ptr, (double *)h_transform, *U, gauge_dir == 3 ? 3 : 4, (int)Nsteps, (int)verbose_interval, relax_boost, tolerance,
                                         (int)reunit_interval, stopWtheta != 0, secs);
  if (ownU) delete U;
  if (param->return_result_gauge) for (int d = 0; d < 4; d++) memcpy(((void **)gauge)[d], links.ptr[d], n * sizeof(double));
  if (param->make_resident_gauge) makeLinksResident(links, param, !ownU);
  if (timeinfo) for (int k = 0; k < 3; k++) timeinfo[k] = secs[k];
  if (info) { info[0] = res.iterations; info[1] = res.F; info[2] = res.theta; info[3] = res.delta; }
  return 0;
}
int computeGaugeFixingOVRQuda(void *gauge, const unsigned int gauge_dir, const unsigned int Nsteps, const unsigned int verbose_interval, const double relax_boost,
                              const double tolerance, const unsigned int reunit_interval, const unsigned int stopWtheta, QudaGaugeParam *param, double *timeinfo) {
  return qudaAmdGaugeFixOVR(gauge, gauge_dir, Nsteps, verbose_interval, relax_boost, tolerance, reunit_interval, stopWtheta, param, timeinfo, nullptr, nullptr);
}
void qudaAmdGaugeFixQuality(unsigned gauge_dir, double out[2]) {
  if (!g_initialized) errorQuda("QUDA not initialized");
  if (!gaugePrecise) errorQuda("qudaAmdGaugeFixQuality: No resident gauge field to use");
  gaugeFixQuality(*gaugePrecise, gauge_dir == 3 ? 3 : 4, out);
}

// reference lib/interface_quda.cpp:5310-5370 (lib/momentum.cu)
double momActionQuda(void *momentum, QudaGaugeParam *param) {
  checkMdParam("momActionQuda", param);
  for (int d = 0; d < 4; d++) if (param->X[d] <= 0 || param->X[d] % 2) errorQuda("Parameter X[%d] = %d undefined or odd", d, param->X[d]);
  bool ownM;
  MomField *M = mdMomentum("momActionQuda", momentum, param, LatticeGeom(param->X), true, ownM);
  const double action = momAction(*M);
  keepMomentum(M, ownM, param);
  return action;
}

// ---- fermion force (ferm_force.hip; include/quda_amd_ext.h).  Every refusal comes before any device work ----
static void meetRanksBeforeOperator();
static void checkFermForceParam(const char *fn, int nvector, const QudaGaugeParam *gp, const QudaInvertParam *inv) {
  checkMdParam(fn, gp);
  if (inv->dslash_type != QUDA_WILSON_DSLASH && inv->dslash_type != QUDA_TWISTED_MASS_DSLASH && inv->dslash_type != QUDA_TWISTED_CLOVER_DSLASH)
    errorQuda("%s: dslash_type %d: Wilson, twisted mass and twisted clover only", fn, inv->dslash_type);
  if (inv->dslash_type == QUDA_TWISTED_CLOVER_DSLASH && inv->twist_flavor != QUDA_TWIST_PLUS && inv->twist_flavor != QUDA_TWIST_MINUS)
    errorQuda("%s: twist_flavor %d: twisted clover has the flavours +1 and -1 only (no doublet)", fn, inv->twist_flavor);
  if (inv->cuda_prec != QUDA_DOUBLE_PRECISION) errorQuda("%s: cuda_prec = %d: fp64 spinor fields only", fn, inv->cuda_prec);
  if (inv->solve_type != QUDA_NORMOP_PC_SOLVE && inv->solve_type != QUDA_DIRECT_PC_SOLVE)
    errorQuda("%s: solve_type = %d: the force is that of the even-odd operator (QUDA_NORMOP_PC_SOLVE or QUDA_DIRECT_PC_SOLVE)", fn, inv->solve_type);
  if (nvector < 1) errorQuda("%s: nvector = %d", fn, nvector);
  if (!gaugePrecise) errorQuda("%s: No resident gauge field to use", fn);
  for (int d = 0; d < 4; d++) if (gp->X[d] != g_geom.X[d]) errorQuda("%s: X[%d] = %d differs from the resident links' %d", fn, d, gp->X[d], g_geom.X[d]);
}
// n host fields under inv (parity fields, or full ones) as fp64 device fields
static std::vector<ColorSpinorField *> uploadForceFields(void **h, int n, QudaInvertParam *inv, bool parity) {
  ColorSpinorParam dp = deviceSpinorParam(QUDA_DOUBLE_PRECISION, parity ? QUDA_PARITY_SITE_SUBSET : QUDA_FULL_SITE_SUBSET, fieldTwistFlavor(*inv));
  std::vector<ColorSpinorField *> out(n);
  for (int i = 0; i < n; i++) {
    ColorSpinorParam cpuParam(h[i], *inv, g_geom.X, parity);
    ColorSpinorField host(cpuParam);
    out[i] = new ColorSpinorField(dp);
    *out[i] = host;
  }
  return out;
}
// the resident clover term as the clover force needs it: fp64, with the inverse of this kappa and mu; needCoeff: built from the links
// with the clover_coeff of inv, which the derivative of A = 1 + i c sum sigma F carries
static void checkForceClover(const char *fn, const QudaInvertParam *inv, bool needCoeff) {
  if (!g_initialized) errorQuda("QUDA not initialized");
  if (inv->dslash_type != QUDA_TWISTED_CLOVER_DSLASH) errorQuda("%s: dslash_type %d: twisted clover only", fn, inv->dslash_type);
  if (inv->twist_flavor != QUDA_TWIST_PLUS && inv->twist_flavor != QUDA_TWIST_MINUS) errorQuda("%s: twist_flavor %d: twisted clover has the flavours +1 and -1 only", fn, inv->twist_flavor);
  if (!cloverPrecise) errorQuda("%s: no resident clover term (loadCloverQuda)", fn);
  if (cloverPrecise->precision != QUDA_DOUBLE_PRECISION) errorQuda("%s: the resident clover term is held in precision %d: clover_cuda_prec must be fp64", fn, cloverPrecise->precision);
  const double mu2 = 4.0 * inv->kappa * inv->kappa * inv->mu * inv->mu;
  if (fabs(cloverPrecise->mu2 - mu2) > 1e-14 * (mu2 + cloverPrecise->mu2))
    errorQuda("%s: the resident clover inverse was computed with 4 kappa^2 mu^2 = %.17g, inv_param gives %.17g", fn, cloverPrecise->mu2, mu2);
  if (!needCoeff) return;
  if (cloverPrecise->coeff != cloverPrecise->coeff)
    errorQuda("%s: the resident clover term was loaded from a host field, so its coefficient is unknown: build it from the links (loadCloverQuda(NULL, NULL, inv_param))", fn);
  if (inv->clover_coeff != cloverPrecise->coeff) errorQuda("%s: clover_coeff = %.17g, the resident clover term was built with %.17g", fn, inv->clover_coeff, cloverPrecise->coeff);
}
static void checkForceLattice(const char *fn, const QudaGaugeParam *gp) {
  checkMdParam(fn, gp);
  if (!gaugePrecise) errorQuda("%s: No resident gauge field to use", fn);
  for (int d = 0; d < 4; d++) if (gp->X[d] != g_geom.X[d]) errorQuda("%s: X[%d] = %d differs from the resident links' %d", fn, d, gp->X[d], g_geom.X[d]);
}
static void fermForceCall(const char *fn, void *mom, QudaGaugeParam *param, const std::function<void(MomField &)> &force) {
  bool ownM;
  MomField *M = mdMomentum(fn, mom, param, gaugePrecise->geom, !param->overwrite_mom, ownM);
  if (param->use_resident_mom && param->overwrite_mom) M->zero();
  meetRanksBeforeOperator();
  force(*M);
  if (param->return_result_mom) M->save(mom);
  keepMomentum(M, ownM, param);
}

void qudaAmdFermionOprodForce(void *mom, void **h_x, void **h_y, double *coeff, int nvector, QudaGaugeParam *gauge_param, QudaInvertParam *inv_param) {
  checkFermForceParam("qudaAmdFermionOprodForce", nvector, gauge_param, inv_param);
  fermForceCall("qudaAmdFermionOprodForce", mom, gauge_param, [&](MomField &M) {
    std::vector<ColorSpinorField *> X = uploadForceFields(h_x, nvector, inv_param, false), Y = uploadForceFields(h_y, nvector, inv_param, false);
    fermionOprodForce(M, *gaugePrecise, X, Y, std::vector<double>(coeff, coeff + nvector));
    for (int i = 0; i < nvector; i++) { delete X[i]; delete Y[i]; }
  });
}

void qudaAmdComputeTMForce(void *mom, double dt, void **h_x, double *coeff, int nvector, QudaGaugeParam *gauge_param, QudaInvertParam *inv_param) {
  checkFermForceParam("qudaAmdComputeTMForce", nvector, gauge_param, inv_param);
  if (inv_param->dslash_type == QUDA_TWISTED_CLOVER_DSLASH) {
    checkForceClover("qudaAmdComputeTMForce", inv_param, true);
    checkCloverDerivativeUnpartitioned("qudaAmdComputeTMForce");
  }
  fermForceCall("qudaAmdComputeTMForce", mom, gauge_param, [&](MomField &M) {
    std::vector<ColorSpinorField *> x = uploadForceFields(h_x, nvector, inv_param, true);
    tmForce(M, *gaugePrecise, dt, x, std::vector<double>(coeff, coeff + nvector), inv_param);
    for (int i = 0; i < nvector; i++) delete x[i];
  });
}

double qudaAmdFermForceLastKernelSecs(void) { return fermForceLastKernelSecs(); }

// ---- the clover part of the twisted-clover force and the determinant force (clover_force.hip) ----
void qudaAmdCloverSigmaOprod(double *h_tensor, void **h_x, void **h_y, double *coeff, int nvector, QudaInvertParam *inv_param) {
  const char *fn = "qudaAmdCloverSigmaOprod";
  if (!g_initialized) errorQuda("QUDA not initialized");
  if (!gaugePrecise) errorQuda("%s: No resident gauge field (it fixes the lattice)", fn);
  if (inv_param->cuda_prec != QUDA_DOUBLE_PRECISION) errorQuda("%s: cuda_prec = %d: fp64 spinor fields only", fn, inv_param->cuda_prec);
  if (nvector < 1) errorQuda("%s: nvector = %d", fn, nvector);
  if (inv_param->twist_flavor == QUDA_TWIST_NONDEG_DOUBLET) errorQuda("%s: one-flavour fields only", fn);
  fermForceAddKernelSecs(0, true);
  std::vector<ColorSpinorField *> X = uploadForceFields(h_x, nvector, inv_param, false), Y = uploadForceFields(h_y, nvector, inv_param, false);
  std::vector<SigmaOprodPair> pairs(nvector);
  for (int i = 0; i < nvector; i++) {
    pairs[i].x[0] = &X[i]->Even(); pairs[i].x[1] = &X[i]->Odd(); pairs[i].y[0] = &Y[i]->Even(); pairs[i].y[1] = &Y[i]->Odd();
    for (int q = 0; q < 2; q++) { pairs[i].cr[q] = coeff[2 * i + q]; pairs[i].ci[q] = 0; }
  }
  TensorField T(g_geom);
  cloverSigmaOprod(T, pairs, false);
  T.save(h_tensor);
  for (int i = 0; i < nvector; i++) { delete X[i]; delete Y[i]; }
}

void qudaAmdCloverSigmaTrace(double *h_tensor, double coeff_even, double coeff_odd, QudaInvertParam *inv_param) {
  checkForceClover("qudaAmdCloverSigmaTrace", inv_param, false);
  fermForceAddKernelSecs(0, true);
  const double cr[2] = {coeff_even, coeff_odd}, ci[2] = {0, 0};
  TensorField T(g_geom);
  cloverSigmaTrace(T, *cloverPrecise, cr, ci, false);
  T.save(h_tensor);
}

void qudaAmdCloverDerivativeForce(void *mom, double *h_tensor, double coeff, QudaGaugeParam *gauge_param) {
  checkForceLattice("qudaAmdCloverDerivativeForce", gauge_param);
  checkCloverDerivativeUnpartitioned("qudaAmdCloverDerivativeForce");
  fermForceCall("qudaAmdCloverDerivativeForce", mom, gauge_param, [&](MomField &M) {
    fermForceAddKernelSecs(0, true);
    TensorField T(g_geom);
    T.load(h_tensor);
    cloverDerivativeForce(M, *gaugePrecise, T, coeff);
  });
}

void qudaAmdCloverLogDetForce(void *mom, double dt, double coeff_even, double coeff_odd, QudaGaugeParam *gauge_param, QudaInvertParam *inv_param) {
  checkForceLattice("qudaAmdCloverLogDetForce", gauge_param);
  checkForceClover("qudaAmdCloverLogDetForce", inv_param, true);
  checkCloverDerivativeUnpartitioned("qudaAmdCloverLogDetForce");
  fermForceCall("qudaAmdCloverLogDetForce", mom, gauge_param, [&](MomField &M) {
    fermForceAddKernelSecs(0, true);
    // d log det(A^2 + a^2) = 2 i c sum_f tr(dF_f tr_sigma(B)_f)
    const double cr[2] = {0, 0}, ci[2] = {2.0 * inv_param->clover_coeff * coeff_even, 2.0 * inv_param->clover_coeff * coeff_odd};
    TensorField T(g_geom);
    cloverSigmaTrace(T, *cloverPrecise, cr, ci, false);
    cloverDerivativeForce(M, *gaugePrecise, T, dt);
  });
}

// reference :730-930.  Host order: QUDA_PACKED_CLOVER_ORDER.  If the inverse is not supplied (or
// compute_clover_inverse is set) it is computed on the device; for twisted clover it is (A^2 + 4 kappa^2 mu^2)^-1
// (reference :780-790, lib/clover_invert.cu:56-85).
void loadCloverQuda(void *h_clover, void *h_clovinv, QudaInvertParam *inv) {
  if (!g_initialized) errorQuda("QUDA not initialized");
  if (!gaugePrecise) errorQuda("Cannot call loadCloverQuda with no resident gauge field");
  if (inv->clover_order != QUDA_PACKED_CLOVER_ORDER) errorQuda("clover_order %d: only QUDA_PACKED_CLOVER_ORDER host fields are supported", inv->clover_order);
  if (inv->clover_cpu_prec != QUDA_DOUBLE_PRECISION && inv->clover_cpu_prec != QUDA_SINGLE_PRECISION) errorQuda("Parameter clover_cpu_prec undefined");
  // reference :743-747: with neither field given (or compute_clover set) the clover term is built on the device from the
  // resident links, A = 1 + i clover_coeff sum sigma F (createCloverQuda :3950-4010); what the QKXTM drivers do
  const bool device_calc = (!h_clover && !h_clovinv) || inv->compute_clover;
  if (device_calc && (inv->clover_coeff == 0.0 || inv->clover_coeff != inv->clover_coeff)) errorQuda("called with neither clover term nor inverse and clover coefficient not set");
  if (!device_calc && !h_clover) errorQuda("loadCloverQuda: an inverse without the clover term is not supported (the operators need A itself)");
  freeCloverQuda();
  const bool twisted = inv->dslash_type == QUDA_TWISTED_CLOVER_DSLASH;
  const double mu2 = twisted ? 4.0 * inv->kappa * inv->kappa * inv->mu * inv->mu : 0.0;
  const bool compute_inv = device_calc || !h_clovinv || inv->compute_clover_inverse || inv->return_clover_inverse;
  auto make = [&](QudaPrecision prec) {
    CloverField *c = new CloverField(g_geom, prec);
    if (device_calc) c->computeFromGauge(*gaugePrecise, inv->clover_coeff);
    else c->loadPacked(h_clover, compute_inv ? nullptr : h_clovinv, inv->clover_cpu_prec);
    if (compute_inv) c->computeInverse(mu2, twisted);
    else { c->twisted = twisted; c->mu2 = mu2; }
    return c;
  };
  cloverPrecise = make(inv->clover_cuda_prec);
  double gib = cloverPrecise->GiB();
  auto valid = [](QudaPrecision p) { return p == QUDA_DOUBLE_PRECISION || p == QUDA_SINGLE_PRECISION || p == QUDA_HALF_PRECISION; };
  if (valid(inv->clover_cuda_prec_sloppy) && inv->clover_cuda_prec_sloppy != inv->clover_cuda_prec) { cloverSloppy = make(inv->clover_cuda_prec_sloppy); gib += cloverSloppy->GiB(); }
  const QudaPrecision sp = cloverSloppy ? cloverSloppy->precision : cloverPrecise->precision;
  if (valid(inv->clover_cuda_prec_precondition) && inv->clover_cuda_prec_precondition != sp) { cloverPrecondition = make(inv->clover_cuda_prec_precondition); gib += cloverPrecondition->GiB(); }
  inv->cloverGiB = gib;
  inv->trlogA[0] = cloverPrecise->trlog[0];
  inv->trlogA[1] = cloverPrecise->trlog[1];
  if (h_clover && device_calc && inv->return_clover) cloverPrecise->savePacked(h_clover, inv->clover_cpu_prec);
  if (h_clovinv && compute_inv && inv->return_clover_inverse) {
    // hand the inverse back in double if the device field is 16-bit? no: from the most precise resident copy
    cloverPrecise->savePackedInverse(h_clovinv, inv->clover_cpu_prec);
  }
}

void freeCloverQuda(void) {
  delete cloverPrecise; delete cloverSloppy; delete cloverPrecondition;
  cloverPrecise = cloverSloppy = cloverPrecondition = nullptr;
}

// reference :1496-1570
// The device-side halo waits are bounded (QUDA_AMD_P2P_TIMEOUT_S: a neighbour that never delivers is an error, not a hang), so
// ranks must not ENTER an operator application further apart than that bound.  Inside a solver the global sums keep them in
// step; a stand-alone operator call through the C ABI can follow arbitrary host work (I/O, source construction), hence a
// blocking host-level rendezvous first — tens of microseconds next to the two PCIe transfers of such a call.
static void meetRanksBeforeOperator() {
  if (commGrid().size > 1) commBarrier();
}

void dslashQuda(void *h_out, void *h_in, QudaInvertParam *inv, QudaParity parity) {
  checkResident(inv);
  if (inv->tune == QUDA_TUNE_YES || inv->tune == QUDA_TUNE_NO) setTuning(inv->tune);   // reference dslashQuda: setTuning(inv_param->tune)
  ColorSpinorParam cpuParam(h_in, *inv, g_geom.X, true);
  ColorSpinorField in_h(cpuParam);
  ColorSpinorParam dp = deviceSpinorParam(inv->cuda_prec, QUDA_PARITY_SITE_SUBSET, fieldTwistFlavor(*inv));
  ColorSpinorField in(dp), out(dp);
  in = in_h;
  meetRanksBeforeOperator();
  DiracParam diracParam;
  setDiracParam(diracParam, inv, true);
  Dirac *dirac = Dirac::create(diracParam);
  if (inv->dslash_type == QUDA_TWISTED_CLOVER_DSLASH && inv->dagger) {
    ColorSpinorField tmp1(dp);
    ((DiracTwistedCloverPC *)dirac)->TwistCloverInv(tmp1, in, (parity + 1) % 2);
    dirac->Dslash(out, tmp1, parity);
  } else {
    dirac->Dslash(out, in, parity);
  }
  delete dirac;
  cpuParam.v = h_out;
  ColorSpinorField out_h(cpuParam);
  out_h = out;
}

static void normalizeMat(ColorSpinorField &out, const QudaInvertParam *inv, bool pc, bool squared) {
  const double kappa = inv->kappa;
  double f = 1.0;
  if (pc) {
    if (inv->mass_normalization == QUDA_MASS_NORMALIZATION) f = 0.25 / (kappa * kappa);
    else if (inv->mass_normalization == QUDA_ASYMMETRIC_MASS_NORMALIZATION) f = 0.5 / kappa;
  } else if (inv->mass_normalization == QUDA_MASS_NORMALIZATION || inv->mass_normalization == QUDA_ASYMMETRIC_MASS_NORMALIZATION) {
    f = 0.5 / kappa;
  }
  if (squared) f *= f;
  if (f != 1.0) blas::ax(f, out);
}

static void applyMat(void *h_out, void *h_in, QudaInvertParam *inv, bool dagmat) {
  checkResident(inv);
  if (inv->tune == QUDA_TUNE_YES || inv->tune == QUDA_TUNE_NO) setTuning(inv->tune);
  const bool pc = inv->solution_type == QUDA_MATPC_SOLUTION || inv->solution_type == QUDA_MATPCDAG_MATPC_SOLUTION;
  ColorSpinorParam cpuParam(h_in, *inv, g_geom.X, pc);
  ColorSpinorField in_h(cpuParam);
  ColorSpinorParam dp = deviceSpinorParam(inv->cuda_prec, pc ? QUDA_PARITY_SITE_SUBSET : QUDA_FULL_SITE_SUBSET, fieldTwistFlavor(*inv));
  ColorSpinorField in(dp), out(dp);
  in = in_h;
  meetRanksBeforeOperator();
  DiracParam diracParam;
  setDiracParam(diracParam, inv, pc);
  Dirac *dirac = Dirac::create(diracParam);
  if (dagmat) dirac->MdagM(out, in);
  else dirac->M(out, in);
  delete dirac;
  normalizeMat(out, inv, pc, dagmat);
  cpuParam.v = h_out;
  ColorSpinorField out_h(cpuParam);
  out_h = out;
}

void MatQuda(void *h_out, void *h_in, QudaInvertParam *inv) { applyMat(h_out, h_in, inv, false); }
void MatDagMatQuda(void *h_out, void *h_in, QudaInvertParam *inv) { applyMat(h_out, h_in, inv, true); }

// reference :1650-1714: out = A in (or A^-1 in) on one parity
void cloverQuda(void *h_out, void *h_in, QudaInvertParam *inv, QudaParity *parity, int inverse) {
  if (!g_initialized) errorQuda("QUDA not initialized");
  if (!cloverPrecise) errorQuda("Clover field not allocated");
  ColorSpinorParam cpuParam(h_in, *inv, g_geom.X, true);
  ColorSpinorField in_h(cpuParam);
  ColorSpinorParam dp = deviceSpinorParam(inv->cuda_prec, QUDA_PARITY_SITE_SUBSET, fieldTwistFlavor(*inv));
  ColorSpinorField in(dp), out(dp);
  in = in_h;
  applySite(out, in, SITE_CLOVER, 0.0, 1.0, cloverPrecise, (int)*parity, inverse != 0);
  cpuParam.v = h_out;
  ColorSpinorField out_h(cpuParam);
  out_h = out;
}

void openMagma(void) {}
void closeMagma(void) {}

// ================================================================================================
// quda_amd_ext.h
// ================================================================================================
void *qudaAmdSpinorCreate(QudaPrecision prec, QudaSiteSubset subset, QudaTwistFlavorType flavor) {
  if (!gaugePrecise) errorQuda("load a gauge field first (it defines the local lattice)");
  ColorSpinorParam p = deviceSpinorParam(prec, subset, flavor);
  p.create = QUDA_ZERO_FIELD_CREATE;
  return new ColorSpinorField(p);
}
void qudaAmdSpinorDestroy(void *f) { delete (ColorSpinorField *)f; }
void qudaAmdSpinorLoad(void *f, const void *h_src, const QudaInvertParam *inv) {
  ColorSpinorField *d = (ColorSpinorField *)f;
  ColorSpinorParam cp((void *)h_src, *inv, g_geom.X, d->SiteSubset() == QUDA_PARITY_SITE_SUBSET);
  ColorSpinorField h(cp);
  *d = h;
}
void qudaAmdSpinorSave(const void *f, void *h_dst, const QudaInvertParam *inv) {
  const ColorSpinorField *d = (const ColorSpinorField *)f;
  ColorSpinorParam cp(h_dst, *inv, g_geom.X, d->SiteSubset() == QUDA_PARITY_SITE_SUBSET);
  ColorSpinorField h(cp);
  h = *d;
}
void qudaAmdSpinorCopy(void *dst, const void *src) { copyColorSpinor(*(ColorSpinorField *)dst, *(const ColorSpinorField *)src); }
void qudaAmdSpinorSetTwist(void *f, QudaTwistFlavorType flavor) { ((ColorSpinorField *)f)->changeTwist(flavor); }
// the flavour mixing of the non-degenerate doublet on resident parity (or full) doublets, out may be in:
// direct 1 + i a g5 tau3 + b tau1 with a = 2 kappa mu, b = -2 kappa epsilon, or its inverse; dagger flips a
void qudaAmdNdegTwist(void *out, const void *in, double kappa, double mu, double epsilon, int dagger, int inverse) {
  ColorSpinorField &o = *(ColorSpinorField *)out;
  const ColorSpinorField &i = *(const ColorSpinorField *)in;
  double a, b, d;
  ndegTwistCoefficients(kappa, mu, epsilon, inverse != 0, dagger != 0, a, b, d);
  if (i.SiteSubset() != o.SiteSubset()) errorQuda("site subset mismatch");
  if (i.SiteSubset() == QUDA_FULL_SITE_SUBSET) { applyNdegTwist(o.Even(), i.Even(), a, b, d); applyNdegTwist(o.Odd(), i.Odd(), a, b, d); }
  else applyNdegTwist(o, i, a, b, d);
}

void *qudaAmdDiracCreate(QudaInvertParam *inv, int pc, int which) {
  checkResident(inv);
  DiracParam dp;
  if (which == 0) setDiracParam(dp, inv, pc != 0);
  else if (which == 1) setDiracSloppyParam(dp, inv, pc != 0);
  else setDiracPreParam(dp, inv, pc != 0);
  return Dirac::create(dp);
}
void qudaAmdDiracDestroy(void *d) { delete (Dirac *)d; }
void qudaAmdDiracDslash(void *d, void *out, const void *in, QudaParity parity) { ((Dirac *)d)->Dslash(*(ColorSpinorField *)out, *(const ColorSpinorField *)in, parity); }
void qudaAmdDiracDslashXpay(void *d, void *out, const void *in, QudaParity parity, const void *x, double k) {
  ((Dirac *)d)->DslashXpay(*(ColorSpinorField *)out, *(const ColorSpinorField *)in, parity, *(const ColorSpinorField *)x, k);
}
void qudaAmdDiracM(void *d, void *out, const void *in) { ((Dirac *)d)->M(*(ColorSpinorField *)out, *(const ColorSpinorField *)in); }
void qudaAmdDiracMdag(void *d, void *out, const void *in) { ((Dirac *)d)->Mdag(*(ColorSpinorField *)out, *(const ColorSpinorField *)in); }
void qudaAmdDiracMdagM(void *d, void *out, const void *in) { ((Dirac *)d)->MdagM(*(ColorSpinorField *)out, *(const ColorSpinorField *)in); }
unsigned long long qudaAmdDiracFlops(void *d) { return ((Dirac *)d)->Flops(); }
// Dirac::prepare / reconstruct on resident full fields (reference include/dirac_quda.h:152-164): prepare builds the source of the
// (even-odd preconditioned) system from b — in the half of x the reference uses as scratch — and hands back a copy of it;
// reconstruct completes x from the solved half and b
void qudaAmdDiracPrepare(void *d, void *src_out, void *x, void *b, QudaSolutionType solution_type) {
  ColorSpinorField *src = nullptr, *sol = nullptr;
  ((Dirac *)d)->prepare(src, sol, *(ColorSpinorField *)x, *(ColorSpinorField *)b, solution_type);
  blas::copy(*(ColorSpinorField *)src_out, *src);
}
void qudaAmdDiracReconstruct(void *d, void *x, const void *b, QudaSolutionType solution_type) {
  ((Dirac *)d)->reconstruct(*(ColorSpinorField *)x, *(const ColorSpinorField *)b, solution_type);
}

double qudaAmdTimeDslash(void *d, void *out, const void *in, QudaParity parity, int niter) {
  hipEvent_t e0, e1;
  HIP_CHECK(hipEventCreate(&e0));
  HIP_CHECK(hipEventCreate(&e1));
  HIP_CHECK(hipEventRecord(e0, computeStream()));
  for (int i = 0; i < niter; i++) ((Dirac *)d)->Dslash(*(ColorSpinorField *)out, *(const ColorSpinorField *)in, parity);
  HIP_CHECK(hipEventRecord(e1, computeStream()));
  HIP_CHECK(hipEventSynchronize(e1));
  p2pCheck(__func__);
  float ms = 0;
  HIP_CHECK(hipEventElapsedTime(&ms, e0, e1));
  HIP_CHECK(hipEventDestroy(e0));
  HIP_CHECK(hipEventDestroy(e1));
  return 1e-3 * ms / niter;
}
double qudaAmdTimeM(void *d, void *out, const void *in, int niter) {
  hipEvent_t e0, e1;
  HIP_CHECK(hipEventCreate(&e0));
  HIP_CHECK(hipEventCreate(&e1));
  HIP_CHECK(hipEventRecord(e0, computeStream()));
  for (int i = 0; i < niter; i++) ((Dirac *)d)->M(*(ColorSpinorField *)out, *(const ColorSpinorField *)in);
  HIP_CHECK(hipEventRecord(e1, computeStream()));
  HIP_CHECK(hipEventSynchronize(e1));
  p2pCheck(__func__);
  float ms = 0;
  HIP_CHECK(hipEventElapsedTime(&ms, e0, e1));
  HIP_CHECK(hipEventDestroy(e0));
  HIP_CHECK(hipEventDestroy(e1));
  return 1e-3 * ms / niter;
}

double qudaAmdBlasNorm2(const void *f) { return blas::norm2(*(const ColorSpinorField *)f); }
void qudaAmdBlasCDot(const void *x, const void *y, double r[2]) {
  Complex c = blas::cDotProduct(*(const ColorSpinorField *)x, *(const ColorSpinorField *)y);
  r[0] = c.real(); r[1] = c.imag();
}
void qudaAmdBlasAxpy(double a, const void *x, void *y) { blas::axpy(a, *(const ColorSpinorField *)x, *(ColorSpinorField *)y); }
void qudaAmdBlasAxpyCGNorm(double a, const void *x, void *y, double r[2]) {
  const Complex c = blas::axpyCGNorm(a, *(const ColorSpinorField *)x, *(ColorSpinorField *)y);
  r[0] = c.real(); r[1] = c.imag();
}
void qudaAmdBlasAxpyZpbx(double a, void *x, void *y, const void *z, double b) {
  blas::axpyZpbx(a, *(ColorSpinorField *)x, *(ColorSpinorField *)y, *(const ColorSpinorField *)z, b);
}
void qudaAmdBlasTripleCGReduction(const void *x, const void *y, const void *z, double r[3]) {
  const double3_t t = blas::tripleCGReduction(*(const ColorSpinorField *)x, *(const ColorSpinorField *)y, *(const ColorSpinorField *)z);
  r[0] = t.x; r[1] = t.y; r[2] = t.z;
}
double qudaAmdBlasAxpyReDot(double a, const void *x, void *y) { return blas::axpyReDot(a, *(const ColorSpinorField *)x, *(ColorSpinorField *)y); }
static std::vector<ColorSpinorField *> fieldList(void *f[], int k) {
  std::vector<ColorSpinorField *> v(k > 0 ? k : 0);
  for (int i = 0; i < k; i++) v[i] = (ColorSpinorField *)f[i];
  return v;
}
void qudaAmdBlasMultiShiftUpdate(int k, void *x[], void *p[], const void *r, const double *alpha, const double *beta, const double *zeta) {
  blas::multiShiftUpdate(k, fieldList(x, k), fieldList(p, k), *(const ColorSpinorField *)r, alpha, beta, zeta);
}
int qudaAmdBlasMultiShiftChunk(void) { return blas::multiShiftChunk(); }
// test hooks onto the rest of namespace blas: one dispatcher by name for the single-field functions
int qudaAmdBlasApply(const char *op, const double coeff[4], void *x_, void *y_, void *z_, void *w_, double r[3]) {
  auto is = [&](const char *name) { return !strcmp(op, name); };
  auto field = [&](void *p, const char *which) -> ColorSpinorField & {
    if (!p) errorQuda("qudaAmdBlasApply(%s): operand %s is missing", op, which);
    return *(ColorSpinorField *)p;
  };
  auto X = [&]() -> ColorSpinorField & { return field(x_, "x"); };
  auto Y = [&]() -> ColorSpinorField & { return field(y_, "y"); };
  auto Z = [&]() -> ColorSpinorField & { return field(z_, "z"); };
  auto W = [&]() -> ColorSpinorField & { return field(w_, "w"); };
  const double ra = coeff[0], rb = coeff[1];
  const Complex a(coeff[0], coeff[1]), b(coeff[2], coeff[3]);
  auto put2 = [&](const Complex &c) { r[0] = c.real(); r[1] = c.imag(); return 2; };
  auto put3 = [&](const double3_t &t) { r[0] = t.x; r[1] = t.y; r[2] = t.z; return 3; };
  if (is("norm2")) { r[0] = blas::norm2(X()); return 1; }
  if (is("reDotProduct")) { r[0] = blas::reDotProduct(X(), Y()); return 1; }
  if (is("cDotProduct")) return put2(blas::cDotProduct(X(), Y()));
  if (is("cDotProductNormA")) return put3(blas::cDotProductNormA(X(), Y()));
  if (is("cDotProductNormB")) return put3(blas::cDotProductNormB(X(), Y()));
  if (is("ax")) { blas::ax(ra, X()); return 0; }
  if (is("axpy")) { blas::axpy(ra, X(), Y()); return 0; }
  if (is("xpy")) { blas::xpy(X(), Y()); return 0; }
  if (is("xpay")) { blas::xpay(X(), ra, Y()); return 0; }
  if (is("mxpy")) { blas::mxpy(X(), Y()); return 0; }
  if (is("axpby")) { blas::axpby(ra, X(), rb, Y()); return 0; }
  if (is("xmyNorm")) { r[0] = blas::xmyNorm(X(), Y()); return 1; }
  if (is("axpyNorm")) { r[0] = blas::axpyNorm(ra, X(), Y()); return 1; }
  if (is("caxpy")) { blas::caxpy(a, X(), Y()); return 0; }
  if (is("caxpby")) { blas::caxpby(a, X(), b, Y()); return 0; }
  if (is("xmyz")) { blas::xmyz(X(), Y(), Z()); return 0; }
  if (is("cxpaypbz")) { blas::cxpaypbz(X(), a, Y(), b, Z()); return 0; }
  if (is("caxpyNorm")) { r[0] = blas::caxpyNorm(a, X(), Y()); return 1; }
  if (is("caxpyXmaz")) { blas::caxpyXmaz(a, X(), Y(), Z()); return 0; }
  if (is("caxpyXmazNormX")) { r[0] = blas::caxpyXmazNormX(a, X(), Y(), Z()); return 1; }
  if (is("caxXmaz")) { blas::caxXmaz(a, X(), Y(), Z()); return 0; }
  if (is("caxInit")) { blas::caxInit(a, X(), Y(), Z(), W()); return 0; }
  if (is("cabxpyAx")) { blas::cabxpyAx(ra, b, X(), Y()); return 0; }
  if (is("cabxpyAxNorm")) { r[0] = blas::cabxpyAxNorm(ra, b, X(), Y()); return 1; }
  if (is("caxpyDotzy")) return put2(blas::caxpyDotzy(a, X(), Y(), Z()));
  if (is("caxpbypzYmbw")) { blas::caxpbypzYmbw(a, X(), b, Y(), Z(), W()); return 0; }
  errorQuda("qudaAmdBlasApply: unknown operation %s", op);
  return -1;
}
// both calls in one function: nothing can overwrite the sums in device memory between them
void qudaAmdBlasDevUpdate(const char *op, double omega, const void *p, const void *q, void *x, void *y, void *z, void *w) {
  if (!x || !y || !z || !p || !q) errorQuda("qudaAmdBlasDevUpdate(%s): an operand is missing", op);
  int which = !strcmp(op, "caxpyXmazDev") ? 0 : (!strcmp(op, "caxXmazDev") ? 1 : (!strcmp(op, "caxInitDev") ? 2 : -1));
  if (which < 0) errorQuda("qudaAmdBlasDevUpdate: unknown operation %s", op);
  if (which == 2 && !w) errorQuda("qudaAmdBlasDevUpdate(%s): operand w is missing", op);
  blas::cDotProductNormADev(*(const ColorSpinorField *)p, *(const ColorSpinorField *)q);
  if (which == 0) blas::caxpyXmazDev(omega, *(ColorSpinorField *)x, *(ColorSpinorField *)y, *(const ColorSpinorField *)z);
  else if (which == 1) blas::caxXmazDev(omega, *(ColorSpinorField *)x, *(ColorSpinorField *)y, *(const ColorSpinorField *)z);
  else blas::caxInitDev(omega, *(const ColorSpinorField *)x, *(ColorSpinorField *)y, *(const ColorSpinorField *)z, *(ColorSpinorField *)w);
}
int qudaAmdBlasMultiSupported(const void *f, int k) { return blas::multiSupported(*(const ColorSpinorField *)f, k) ? 1 : 0; }
static std::vector<Complex> complexList(const double *c, int k) {
  std::vector<Complex> v(k > 0 ? k : 1);
  for (int i = 0; i < k; i++) v[i] = Complex(c[2 * i], c[2 * i + 1]);
  return v;
}
void qudaAmdBlasMultiDot(int k, void *f[], const void *y, const void *r, double *beta, double yr[2], double *ynorm) {
  std::vector<Complex> b(k > 0 ? k : 1);
  Complex c;
  blas::multiDot(b.data(), c, *ynorm, fieldList(f, k), k, *(const ColorSpinorField *)y, *(const ColorSpinorField *)r);
  for (int i = 0; i < k; i++) { beta[2 * i] = b[i].real(); beta[2 * i + 1] = b[i].imag(); }
  yr[0] = c.real(); yr[1] = c.imag();
}
void qudaAmdBlasMultiCaxpyResidual(int k, void *f[], const double *c, double scale, void *y, const double a[2], void *r, double sums[2]) {
  blas::multiCaxpyResidual(sums[0], sums[1], complexList(c, k).data(), fieldList(f, k), k, scale, *(ColorSpinorField *)y, Complex(a[0], a[1]), *(ColorSpinorField *)r);
}
void qudaAmdBlasMultiCaxpy(int k, void *f[], const double *c, void *y) {
  blas::multiCaxpy(complexList(c, k).data(), fieldList(f, k), k, *(ColorSpinorField *)y);
}
void qudaAmdBlasHeavyQuarkResidualNorm(const void *x, const void *r, double result[3]) {
  const double3_t t = blas::HeavyQuarkResidualNorm(*(const ColorSpinorField *)x, *(const ColorSpinorField *)r);
  result[0] = t.x; result[1] = t.y; result[2] = t.z;
}
void qudaAmdDiracMdagMShift(void *d, void *out, const void *in, double shift) {
  DiracMdagM m((const Dirac *)d);
  m.shift = shift;
  m(*(ColorSpinorField *)out, *(const ColorSpinorField *)in);
}
// device-event timed loops behind tools/cg_timing.py
extern "C++" template <typename Body> static double timeLoop(int niter, const char *who, Body body) {
  hipEvent_t e0, e1;
  HIP_CHECK(hipEventCreate(&e0));
  HIP_CHECK(hipEventCreate(&e1));
  HIP_CHECK(hipEventRecord(e0, computeStream()));
  for (int i = 0; i < niter; i++) body();
  HIP_CHECK(hipEventRecord(e1, computeStream()));
  HIP_CHECK(hipEventSynchronize(e1));
  p2pCheck(who);
  float ms = 0;
  HIP_CHECK(hipEventElapsedTime(&ms, e0, e1));
  HIP_CHECK(hipEventDestroy(e0));
  HIP_CHECK(hipEventDestroy(e1));
  return 1e-3 * ms / niter;
}
double qudaAmdTimeMdagM(void *d, void *out, const void *in, int niter) {
  return timeLoop(niter, __func__, [&] { ((Dirac *)d)->MdagM(*(ColorSpinorField *)out, *(const ColorSpinorField *)in); });
}
double qudaAmdTimeCGBlas(int fused, void *x_, void *r_, void *p_, void *Ap_, int niter) {
  ColorSpinorField &x = *(ColorSpinorField *)x_, &r = *(ColorSpinorField *)r_, &p = *(ColorSpinorField *)p_, &Ap = *(ColorSpinorField *)Ap_;
  const double alpha = 1e-3, beta = 0.5;   // fixed coefficients: the fields stay bounded over the loop, the traffic is that of an iteration
  if (fused) return timeLoop(niter, __func__, [&] {
    (void)blas::reDotProduct(p, Ap);
    (void)blas::axpyCGNorm(-alpha, Ap, r);
    blas::axpyZpbx(alpha, p, x, r, beta);
  });
  return timeLoop(niter, __func__, [&] {
    (void)blas::reDotProduct(p, Ap);
    blas::axpy(-alpha, Ap, r);
    (void)blas::norm2(r);
    (void)blas::reDotProduct(r, Ap);   // stands for the second sum of axpyCGNorm
    blas::axpy(alpha, p, x);
    blas::xpay(r, beta, p);
  });
}
double qudaAmdTimeMultiShift(int fused, int k, void *x[], void *p[], const void *r_, int niter) {
  const ColorSpinorField &r = *(const ColorSpinorField *)r_;
  const std::vector<ColorSpinorField *> xv = fieldList(x, k), pv = fieldList(p, k);
  std::vector<double> alpha(k > 0 ? k : 1, 1e-3), beta(k > 0 ? k : 1, 0.5), zeta(k > 0 ? k : 1, 0.25);
  if (fused) return timeLoop(niter, __func__, [&] { blas::multiShiftUpdate(k, xv, pv, r, alpha.data(), beta.data(), zeta.data()); });
  return timeLoop(niter, __func__, [&] {
    for (int i = 0; i < k; i++) { blas::axpy(alpha[i], *pv[i], *xv[i]); blas::axpby(zeta[i], r, beta[i], *pv[i]); }
  });
}
// device-event timed y += a x loop: the streaming-bandwidth yardstick printed beside the stencil numbers
double qudaAmdTimeAxpy(double a, const void *x, void *y, int niter) {
  hipEvent_t e0, e1;
  HIP_CHECK(hipEventCreate(&e0));
  HIP_CHECK(hipEventCreate(&e1));
  HIP_CHECK(hipEventRecord(e0, computeStream()));
  for (int i = 0; i < niter; i++) blas::axpy(a, *(const ColorSpinorField *)x, *(ColorSpinorField *)y);
  HIP_CHECK(hipEventRecord(e1, computeStream()));
  HIP_CHECK(hipEventSynchronize(e1));
  p2pCheck(__func__);
  float ms = 0;
  HIP_CHECK(hipEventElapsedTime(&ms, e0, e1));
  HIP_CHECK(hipEventDestroy(e0));
  HIP_CHECK(hipEventDestroy(e1));
  return 1e-3 * ms / niter;
}

static DslashMode pcDslashMode(QudaInvertParam *inv) {
  const bool asym = inv->matpc_type == QUDA_MATPC_EVEN_EVEN_ASYMMETRIC || inv->matpc_type == QUDA_MATPC_ODD_ODD_ASYMMETRIC;
  switch (inv->dslash_type) {
    case QUDA_WILSON_DSLASH: return DSLASH_PLAIN;
    case QUDA_TWISTED_MASS_DSLASH: return (!inv->dagger || asym) ? DSLASH_TWIST_INV : DSLASH_TWIST_INV_DSLASH;
    case QUDA_TWISTED_CLOVER_DSLASH: return (!inv->dagger || asym) ? DSLASH_CLOVER_TWIST_INV : DSLASH_PLAIN;
    default: errorQuda("Unsupported dslash_type %d", inv->dslash_type);
  }
  return DSLASH_PLAIN;
}
long long qudaAmdDslashBytesPerSite(QudaInvertParam *inv, int which, int xpay) {
  GaugeField *g = residentGauge(which);
  return dslashBytesPerSite(g->precision, (int)g->reconstruct, pcDslashMode(inv), xpay != 0);
}
long long qudaAmdDslashFlopsPerSite(QudaInvertParam *inv, int xpay) { return dslashFlopsPerSite(pcDslashMode(inv), xpay != 0); }

void qudaAmdSetPartitionMask(int mask) {
  for (int d = 0; d < 4; d++) commGrid().forced[d] = (mask >> d) & 1;
}
void *qudaAmdComputeStream(void) { return (void *)computeStream(); }
int qudaAmdHaloTransport(void) { return p2pTransport(); }
int qudaAmdHaloWireFormat(void) { return haloWireFormat(); }
// profile post-processing (tools/mg_solve_profile.py): a marker dispatch that brackets a region in the rocprofv3 kernel trace, and the
// launch accounting of qa_core.h
__global__ void qa_profile_marker_kernel(int id, int *sink) { if (sink && id < 0) *sink = id; }
void qudaAmdProfileMarker(int id) { hipLaunchKernelGGL(qa_profile_marker_kernel, dim3(1), dim3(64), 0, computeStream(), id, (int *)nullptr); HIP_CHECK(hipGetLastError()); }
void qudaAmdAccountStart(void) { acctStart(); }
void qudaAmdAccountDump(const char *path) { acctDump(path); }
void qudaAmdCommStats(long long out[8]) { for (int k = 0; k < 8; k++) out[k] = p2pStats()[k]; }
int qudaAmdDescribeHaloError(char *text, int n) { return p2pDescribeError(text, (size_t)n) ? 1 : 0; }
// text written to stdout (and exit status used) if a library error ends the process; nullptr clears (quda_amd_ext.h)
void qudaAmdSetExitLine(const char *text, int status) { setExitLine(text, status); }

void qudaAmdSetDslashTune(const char *key, int value) { setDslashTune(key, value); }

// ---- raw device images (layout contract checks, tests/test_layout_gpu.py) ----
void qudaAmdSpinorRawInfo(const void *field, long long info[20]) {
  const ColorSpinorField &f = *(const ColorSpinorField *)field;
  ColorSpinorField &g = const_cast<ColorSpinorField &>(f);
  const bool full = f.SiteSubset() == QUDA_FULL_SITE_SUBSET;
  info[0] = f.Volume(); info[1] = f.VolumeCB(); info[2] = f.Stride(); info[3] = f.pad; info[4] = f.Nspin(); info[5] = f.Ncolor();
  info[6] = f.Precision(); info[7] = f.fieldOrder; info[8] = f.SiteSubset(); info[9] = f.gammaBasis;
  info[10] = (long long)f.bytes; info[11] = (long long)f.norm_bytes;
  info[12] = (long long)(uintptr_t)f.V(); info[13] = (long long)(uintptr_t)f.Norm();
  info[14] = full ? (long long)((const char *)g.Odd().V() - (const char *)f.V()) : 0;
  info[15] = full && f.Norm() ? (long long)((const char *)g.Odd().Norm() - (const char *)f.Norm()) : 0;
  info[16] = f.Precision() == QUDA_DOUBLE_PRECISION || f.Nspin() != 4 ? 2 : (f.Precision() == QUDA_SINGLE_PRECISION ? 4 : 8);   // reals per plane entry
  info[17] = f.twistFlavor; info[18] = f.x[0]; info[19] = f.Location();
}
void qudaAmdGaugeRawInfo(int which, long long info[12]) {
  const GaugeField *U = residentGauge(which);
  if (!U) errorQuda("no resident gauge field %d", which);
  info[0] = (long long)(uintptr_t)U->data; info[1] = (long long)U->bytes; info[2] = U->stride; info[3] = (long long)U->link_bytes;
  info[4] = U->precision; info[5] = U->reconstruct; info[6] = U->geom.Vh; info[7] = U->tbc_folded ? 1 : 0;
  info[8] = U->t_boundary; info[9] = 0; info[10] = 0; info[11] = 0;
}
void qudaAmdCloverRawInfo(int which, long long info[12]) {
  const CloverField *C = residentClover(which);
  if (!C) errorQuda("no resident clover field %d", which);
  info[0] = (long long)(uintptr_t)C->clover; info[1] = (long long)(uintptr_t)C->cloverInv; info[2] = (long long)(uintptr_t)C->norm; info[3] = (long long)(uintptr_t)C->invNorm;
  info[4] = C->stride; info[5] = (long long)C->parity_bytes; info[6] = (long long)C->parity_norm_bytes; info[7] = C->precision;
  info[8] = (long long)C->bytes; info[9] = C->geom.Vh; info[10] = C->twisted ? 1 : 0; info[11] = 0;
}
void qudaAmdRawDeviceCopy(void *h_dst, long long device_address, size_t bytes) {
  HIP_CHECK(hipDeviceSynchronize());
  HIP_CHECK(hipMemcpy(h_dst, (const void *)(uintptr_t)device_address, bytes, hipMemcpyDeviceToHost));
}
void qudaAmdDeviceSynchronize(void) { HIP_CHECK(hipDeviceSynchronize()); p2pCheck(__func__); }

}  // extern "C"
