// qkxtm.hip — the solve loop of the QKXTM correlator drivers behind the library: source preparation
// (point source, Gaussian smearing with the APE-smeared links), even-odd preconditioned GCR with the resident multigrid
// hierarchies of the two twist flavours, reconstruction, and the propagators handed back in the drivers' own layout.
//
// Reference: calcMG_threepTwop_EvenOdd (lib/interface_quda.cpp:6018-6531; the same loop opens calcMG_loop_wOneD_TSM_*,
// :7093, :8535), QKXTM_Vector_Kepler::gaussianSmearing (lib/qudaQKXTM_Vector_Kepler.cpp:386-421),
// lib/code_pieces_Kepler/Gauss_core_Kepler.h, uploadToCuda / downloadFromCuda (lib/qudaQKXTM_Kepler_kernels.cu:972-1056).
// The contractions and ASCII writers that follow the loop in the reference live in contract.hip (two-point functions), threep.hip
// (three-point functions) and loop.hip; HDF5 output is out of scope.
//
// Everything stays on the device between the point source and the finished propagator:
//  * smearing acts on colour only, so ONE smearing pass per source position serves all twelve spin-colour sources: the
//    point sources of the three colours sit in spin slots 0..2 of a single vector (the reference smears 24 times);
//  * a smearing step is six covariant shifts accumulated in place (applyCovariantShift: the ghost-aware single-direction
//    hop of the multigrid setup without the spin projector), so it runs unchanged on a grid-decomposed lattice;
//  * the QKXTM host layouts are lexicographic in the sites and UKQCD in spin; site reordering and the spin rotation to the
//    device basis happen in the copy kernels.
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "basis.h"
#include "blas.h"
#include "device_io.h"
#include "dslash.h"
#include "interface_internal.h"
#include "lex_index.h"
#include "multigrid.h"
#include "p2p.h"
#include "qkxtm_internal.h"
#include "quda_amd_ext.h"
#include "solver.h"

namespace quda {

// ---- site order / basis: QKXTM host vector (lexicographic sites, UKQCD spin) <-> device full field (even-odd, DeGrand-Rossi) ----

__global__ void __launch_bounds__(256) lex_to_dev_kernel(double *dev, int stride, size_t parityDoubles, const double *lex, int Vh, int Xh, int Y, int Z, int change) {
  const int idx = blockIdx.x * blockDim.x + threadIdx.x, parity = blockIdx.y;
  if (idx >= Vh) return;
  const double *h = lex + lex_of(idx, parity, Xh, Y, Z) * 24;
  double r[24], q[24];
#pragma unroll
  for (int k = 0; k < 24; k++) r[k] = h[k];
  if (change) rotate_basis(q, r, change);
  Planar<double, 24>::store(change ? q : r, dev + parity * parityDoubles, stride, idx, nullptr, idx);
}

__global__ void __launch_bounds__(256) dev_to_lex_kernel(double *lex, const double *dev, int stride, size_t parityDoubles, int Vh, int Xh, int Y, int Z, int change,
                                                         double scale) {
  const int idx = blockIdx.x * blockDim.x + threadIdx.x, parity = blockIdx.y;
  if (idx >= Vh) return;
  double r[24], q[24];
  Planar<double, 24>::load(r, dev + parity * parityDoubles, stride, idx, nullptr, idx);
  if (change) rotate_basis(q, r, change);
  double *h = lex + lex_of(idx, parity, Xh, Y, Z) * 24;
#pragma unroll
  for (int k = 0; k < 24; k++) h[k] = scale * (change ? q[k] : r[k]);
}

// colour point sources in spin slots: psi(site)[slot c][colour c] = 1 for c = 0, 1, 2 (host-basis slots, rotated like any host vector)
__global__ void point_slots_kernel(double *dev, int stride, int idx) {
  double r[24], q[24];
  for (int k = 0; k < 24; k++) r[k] = 0;
  for (int c = 0; c < 3; c++) r[6 * c + 2 * c] = 1.0;
  rotate_basis(q, r, BASIS_UKQCD_TO_DR);
  Planar<double, 24>::store(q, dev, stride, idx, nullptr, idx);
}

// out = e_{spin s0} (x) [colour vector held in spin slot `slot` of in], both in the device basis of host-basis slots
__global__ void __launch_bounds__(256) spread_slot_kernel(double *out, const double *in, int stride, size_t parityDoubles, int Vh, int s0, int slot) {
  const int idx = blockIdx.x * blockDim.x + threadIdx.x, parity = blockIdx.y;
  if (idx >= Vh) return;
  double r[24], q[24];
  Planar<double, 24>::load(r, in + parity * parityDoubles, stride, idx, nullptr, idx);
  rotate_basis(q, r, BASIS_DR_TO_UKQCD);
#pragma unroll
  for (int k = 0; k < 24; k++) r[k] = 0;
#pragma unroll
  for (int k = 0; k < 6; k++) r[6 * s0 + k] = q[6 * slot + k];
  rotate_basis(q, r, BASIS_UKQCD_TO_DR);
  Planar<double, 24>::store(q, out + parity * parityDoubles, stride, idx, nullptr, idx);
}

static void checkFullDouble(const ColorSpinorField &f) {
  if (f.Location() != QUDA_CUDA_FIELD_LOCATION || f.Precision() != QUDA_DOUBLE_PRECISION || f.SiteSubset() != QUDA_FULL_SITE_SUBSET || f.Nspin() != 4 || f.Ncolor() != 3)
    errorQuda("expected a full fp64 device spinor");
}

void lexToDevice(ColorSpinorField &dst, const double *h_lex, const LatticeGeom &g, bool ukqcd) {
  checkFullDouble(dst);
  const size_t bytes = (size_t)g.V * 24 * sizeof(double);
  double *stage = (double *)stagingBuffer(bytes);
  HIP_CHECK(hipMemcpyAsync(stage, h_lex, bytes, hipMemcpyHostToDevice, computeStream()));
  deviceLexToField(dst, stage, g, ukqcd);
}

void deviceLexToField(ColorSpinorField &dst, const double *d_lex, const LatticeGeom &g, bool ukqcd) {
  checkFullDouble(dst);
  hipLaunchKernelGGL(lex_to_dev_kernel, dim3((g.Vh + 255) / 256, 2), dim3(256), 0, computeStream(), (double *)dst.V(), dst.Stride(), parityDoubles(dst), d_lex, g.Vh, g.Xh,
                     g.X[1], g.X[2], ukqcd ? BASIS_UKQCD_TO_DR : BASIS_NONE);
  HIP_CHECK(hipGetLastError());
  HIP_CHECK(hipStreamSynchronize(computeStream()));
}

void deviceToLex(double *h_lex, const ColorSpinorField &src, const LatticeGeom &g, bool ukqcd, double scale) {
  checkFullDouble(src);
  const size_t bytes = (size_t)g.V * 24 * sizeof(double);
  double *stage = (double *)stagingBuffer(bytes);
  hipLaunchKernelGGL(dev_to_lex_kernel, dim3((g.Vh + 255) / 256, 2), dim3(256), 0, computeStream(), stage, (const double *)src.V(), src.Stride(), parityDoubles(src), g.Vh, g.Xh,
                     g.X[1], g.X[2], ukqcd ? BASIS_DR_TO_UKQCD : BASIS_NONE, scale);
  HIP_CHECK(hipGetLastError());
  HIP_CHECK(hipMemcpyAsync(h_lex, stage, bytes, hipMemcpyDeviceToHost, computeStream()));
  HIP_CHECK(hipStreamSynchronize(computeStream()));
  p2pCheck("deviceToLex");
}

// ---- the smearing links: QKXTM host layout gauge[dir][lexicographic site][3][3][2] (lib/qudaQKXTM_Gauge_Kepler.cpp:73-89) ----
GaugeField *loadLexGauge(void **gauge_lex, const LatticeGeom &g) {
  // reorder to the QDP host order (even sites then odd) the loader takes; host loop, once per call
  std::vector<std::vector<double>> eo(4, std::vector<double>((size_t)g.V * 18));
  void *ptr[4];
  for (int d = 0; d < 4; d++) {
    const double *src = (const double *)gauge_lex[d];
    if (!src) errorQuda("gauge_APE[%d] is NULL", d);
    for (long iv = 0; iv < g.V; iv++) {
      long l = iv / g.X[0];
      const int x = (int)(iv % g.X[0]), y = (int)(l % g.X[1]); l /= g.X[1];
      const int z = (int)(l % g.X[2]), t = (int)(l / g.X[2]);
      const int parity = (x + y + z + t) & 1;
      memcpy(&eo[d][((size_t)parity * g.Vh + iv / 2) * 18], src + iv * 18, 18 * sizeof(double));
    }
    ptr[d] = eo[d].data();
  }
  GaugeField *U = new GaugeField(g, QUDA_DOUBLE_PRECISION, QUDA_RECONSTRUCT_NO, QUDA_PERIODIC_T, 1.0);
  loadGaugeWithHalo(*U, ptr, QUDA_DOUBLE_PRECISION);
  return U;
}

// v <- smear^n(v):  psi' = (psi + alpha sum_{i<3} [U_i(x) psi(x+i) + U_i(x-i)^dag psi(x-i)]) / (1 + 6 alpha)   (Gauss_core_Kepler.h)
void gaussianSmear(ColorSpinorField &v, const GaugeField &U, double alpha, int nsmear) {
  checkFullDouble(v);
  ColorSpinorField tmp(v);
  ColorSpinorField *src = &v, *dst = &tmp;
  const double normalize = 1.0 / (1.0 + 6.0 * alpha);
  for (int it = 0; it < nsmear; it++) {
    for (int parity = 0; parity < 2; parity++) {
      ColorSpinorField &o = parity ? dst->Odd() : dst->Even();
      const ColorSpinorField &same = parity ? src->Odd() : src->Even();
      const ColorSpinorField &other = parity ? src->Even() : src->Odd();
      for (int dir = 0; dir < 6; dir++)
        applyCovariantShift(o, other, U, parity, dir, alpha * normalize, dir == 0 ? &same : &o, dir == 0 ? normalize : 1.0);
    }
    std::swap(src, dst);
  }
  if (src != &v) blas::copy(v, *src);
}

static void checkCalcParam(const QudaInvertParam *param, const char *fname) {
  // reference :6041-6054
  if (param->twist_flavor == QUDA_TWIST_NONDEG_DOUBLET) errorQuda("%s: the QKXTM drivers are not available for the non-degenerate doublet", fname);
  if (param->solve_type != QUDA_DIRECT_PC_SOLVE) errorQuda("%s: This function works only with Direct solve and even odd preconditioning", fname);
  if (param->inv_type != QUDA_GCR_INVERTER) errorQuda("%s: This function works only with GCR method", fname);
  if (param->gamma_basis != QUDA_UKQCD_GAMMA_BASIS) errorQuda("%s: This function works only with ukqcd gamma basis", fname);
  if (param->dirac_order != QUDA_DIRAC_ORDER) errorQuda("%s: This function works only with colors inside the spins", fname);
  if (param->matpc_type != QUDA_MATPC_EVEN_EVEN && param->matpc_type != QUDA_MATPC_ODD_ODD) errorQuda("%s: matpc_type %d not supported (symmetric even-even / odd-odd only)", fname, param->matpc_type);
  if (param->solution_type != QUDA_MAT_SOLUTION) errorQuda("%s: solution_type %d not supported (the drivers ask for QUDA_MAT_SOLUTION)", fname, param->solution_type);
  if (param->dslash_type != QUDA_TWISTED_MASS_DSLASH && param->dslash_type != QUDA_TWISTED_CLOVER_DSLASH) errorQuda("%s: twisted-mass / twisted-clover operators only", fname);
  if (param->inv_type_precondition == QUDA_MG_INVERTER && (!param->preconditionerUP || !param->preconditionerDN))
    errorQuda("%s: preconditionerUP / preconditionerDN not set (one multigrid hierarchy per twist flavour)", fname);
}

// Do n sources fit through one lockstep solve (block_solver.cpp)?  A source takes three full fields and 2 + 2 gcrNkrylov sloppy parity
// fields; all of them within 0.6 of the free device memory.  QUDA_AMD_QKXTM_LOCKSTEP=0 answers no.
static bool lockstepFits(int n, const QudaInvertParam *param, const LatticeGeom &g) {
  static int env = -1;
  if (env < 0) { const char *e = getenv("QUDA_AMD_QKXTM_LOCKSTEP"); env = e ? atoi(e) : 1; }
  if (!env) return false;
  size_t freeB = 0, totalB = 0;
  HIP_CHECK(hipMemGetInfo(&freeB, &totalB));
  const double full = (double)g.V * 24 * (int)param->cuda_prec, parS = 0.5 * (double)g.V * 24 * (int)param->cuda_prec_sloppy;
  return n * (3.0 * full + (2.0 + 2.0 * param->gcrNkrylov) * parS) <= 0.6 * (double)freeB;
}

}  // namespace quda

using namespace quda;

extern "C" {

void qudaAmdGaussianSmear(void *h_out, const void *h_in, void **gauge_APE, int nsmear, double alpha) {
  if (!gaugePrecise) errorQuda("Gauge field not allocated");   // the lattice geometry comes from the resident field, as in the reference
  if (nsmear < 0) errorQuda("nsmear = %d", nsmear);
  const LatticeGeom &g = residentGeom();
  if (!gauge_APE && !gaugeSmeared) errorQuda("qudaAmdGaussianSmear: gauge_APE is NULL and no smeared field is resident (performAPEnStep)");
  GaugeField *U = gauge_APE ? loadLexGauge(gauge_APE, g) : gaugeSmeared;
  ColorSpinorParam cp = deviceSpinorParam(QUDA_DOUBLE_PRECISION, QUDA_FULL_SITE_SUBSET, QUDA_TWIST_NO);
  cp.create = QUDA_ZERO_FIELD_CREATE;
  ColorSpinorField v(cp);
  lexToDevice(v, (const double *)h_in, g, true);
  gaussianSmear(v, *U, alpha, nsmear);
  deviceToLex((double *)h_out, v, g, true, 1.0);
  if (gauge_APE) delete U;
}

}  // extern "C"

namespace quda {
// the solve loop itself; every finished propagator (isc = spin * 3 + colour of the source, flavour +1 up / -1 down) is handed to
// `each` as a lexicographic UKQCD host vector of V * 24 doubles that is only valid during the call
void calcMGPropagatorsEach(void **gauge_APE, QudaInvertParam *param, const QudaAmdSourceParam *src, const char *fname,
                           void (*each)(void *ctx, int isc, int flavor, const double *h_prop, size_t nreal), void *ctx,
                           void (*eachDevice)(void *ctx, int isc, int flavor, ColorSpinorField &x, double scale) = nullptr) {
  if (!gaugePrecise) errorQuda("%s: Gauge field not allocated", fname);
  if (!cloverPrecise && param->dslash_type == QUDA_TWISTED_CLOVER_DSLASH) errorQuda("%s: Clover field not allocated", fname);
  if (!src) errorQuda("%s: source description is NULL", fname);
  checkCalcParam(param, fname);
  const bool flag_eo = param->matpc_type == QUDA_MATPC_EVEN_EVEN;
  const LatticeGeom &g = residentGeom();
  const CommGrid &cg = commGrid();
  for (int d = 0; d < 4; d++)
    if (src->sourcePosition[d] < 0 || src->sourcePosition[d] >= g.X[d] * cg.dims[d]) errorQuda("%s: source position %d out of range in dimension %d", fname, src->sourcePosition[d], d);
  if (src->nsmearGauss < 0) errorQuda("%s: nsmearGauss = %d", fname, src->nsmearGauss);
  param->secs = 0; param->gflops = 0; param->iter = 0;

  if (src->nsmearGauss > 0 && !gauge_APE && !gaugeSmeared) errorQuda("%s: gauge_APE is NULL and no smeared field is resident (performAPEnStep)", fname);
  GaugeField *Uape = (src->nsmearGauss > 0) ? (gauge_APE ? loadLexGauge(gauge_APE, g) : gaugeSmeared) : nullptr;

  // reference createDirac :6291-6300, once, before the loop: the twist flavour travels with the fields
  const bool pc_solve = true;
  DiracParam dp, dpSloppy, dpPre;
  setDiracParam(dp, param, pc_solve);
  setDiracSloppyParam(dpSloppy, param, pc_solve);
  setDiracPreParam(dpPre, param, pc_solve);
  Dirac *d = Dirac::create(dp), *dSloppy = Dirac::create(dpSloppy), *dPre = Dirac::create(dpPre);
  Dirac &dirac = *d;
  DiracM m(dirac), mSloppy(*dSloppy), mPre(*dPre);

  ColorSpinorParam cp64 = deviceSpinorParam(QUDA_DOUBLE_PRECISION, QUDA_FULL_SITE_SUBSET, QUDA_TWIST_PLUS);
  cp64.create = QUDA_ZERO_FIELD_CREATE;
  ColorSpinorField phi(cp64), source(cp64), result(cp64);
  ColorSpinorParam cp = deviceSpinorParam(param->cuda_prec, QUDA_FULL_SITE_SUBSET, QUDA_TWIST_PLUS);
  cp.create = QUDA_ZERO_FIELD_CREATE;
  ColorSpinorField *b = new ColorSpinorField(cp), *x = new ColorSpinorField(cp);

  // the three colour point sources in spin slots 0..2, on the rank that owns the site (reference :6404-6421), smeared once
  int my_src[4];
  bool mine = true;
  for (int k = 0; k < 4; k++) { my_src[k] = src->sourcePosition[k] - cg.coords[k] * g.X[k]; mine = mine && my_src[k] >= 0 && my_src[k] < g.X[k]; }
  if (mine) {
    const long iv = (((long)my_src[3] * g.X[2] + my_src[2]) * g.X[1] + my_src[1]) * g.X[0] + my_src[0];
    const int parity = (my_src[0] + my_src[1] + my_src[2] + my_src[3]) & 1;
    ColorSpinorField &half = parity ? phi.Odd() : phi.Even();
    hipLaunchKernelGGL(point_slots_kernel, dim3(1), dim3(1), 0, computeStream(), (double *)half.V(), half.Stride(), (int)(iv / 2));
    HIP_CHECK(hipGetLastError());
  }
  if (Uape) gaussianSmear(phi, *Uape, src->alphaGauss, src->nsmearGauss);

  const size_t vec = (size_t)g.V * 24;
  std::vector<double> h_one(vec);
  double secs = 0, gflops = 0;
  int iters = 0;
  const bool rescale = param->mass_normalization == QUDA_MASS_NORMALIZATION || param->mass_normalization == QUDA_ASYMMETRIC_MASS_NORMALIZATION;
  // The twelve spin-colour sources of a flavour through ONE lockstep solve (block_solver.cpp; DESIGN 3 "Several sources in lockstep") when the
  // solver is multigrid-preconditioned GCR without an initial guess and the fields fit: the hierarchy's cycle runs once per iteration for all of
  // them.  QUDA_AMD_QKXTM_LOCKSTEP=0 keeps the reference's order of 24 separate solves.
  const bool lockstep = param->inv_type == QUDA_GCR_INVERTER && param->inv_type_precondition == QUDA_MG_INVERTER && param->preconditionerUP && param->preconditionerDN &&
                        param->use_init_guess != QUDA_USE_INIT_GUESS_YES && lockstepFits(12, param, g);
  if (lockstep) {
    std::vector<ColorSpinorField *> bs(12), xs(12), ins(12), outs(12);
    for (int isc = 0; isc < 12; isc++) { bs[isc] = new ColorSpinorField(cp); xs[isc] = new ColorSpinorField(cp); }
    for (int fl = 0; fl < 2; fl++) {
      const QudaTwistFlavorType flavor = fl == 0 ? QUDA_TWIST_PLUS : QUDA_TWIST_MINUS;   // up, then down (:6401, :6470)
      param->twist_flavor = flavor;
      param->preconditioner = fl == 0 ? param->preconditionerUP : param->preconditionerDN;
      for (int isc = 0; isc < 12; isc++) {
        hipLaunchKernelGGL(spread_slot_kernel, dim3((g.Vh + 255) / 256, 2), dim3(256), 0, computeStream(), (double *)source.V(), (const double *)phi.V(), source.Stride(),
                           parityDoubles(source), g.Vh, isc / 3, isc % 3);
        HIP_CHECK(hipGetLastError());
        bs[isc]->changeTwist(flavor); xs[isc]->changeTwist(flavor);
        *bs[isc] = source;
        blas::zero(*xs[isc]);
        dirac.prepare(ins[isc], outs[isc], *xs[isc], *bs[isc], param->solution_type);
        ins[isc]->changeTwist(flavor); outs[isc]->changeTwist(flavor);
      }
      param->secs = 0; param->gflops = 0; param->iter = 0;
      SolverParam sp(*param);
      MG *K = static_cast<multigrid_solver *>(param->preconditioner)->mg;
      const MultiSrcSolve res = solveMultiSrcGCR(outs, ins, m, mSloppy, K, sp, dSloppy);
      secs += res.secs; iters += 12 * res.iter;
      double worst = 0;
      for (int isc = 0; isc < 12; isc++) worst = std::max(worst, sqrt(res.r2[isc] / res.b2[isc]));
      param->true_res = worst;
      for (int isc = 0; isc < 12; isc++) {
        dirac.reconstruct(*xs[isc], *bs[isc], param->solution_type);
        result = *xs[isc];
        if (eachDevice) eachDevice(ctx, isc, fl == 0 ? +1 : -1, result, rescale ? 2.0 * param->kappa : 1.0);
        deviceToLex(h_one.data(), result, g, true, rescale ? 2.0 * param->kappa : 1.0);
        each(ctx, isc, fl == 0 ? +1 : -1, h_one.data(), vec);
      }
    }
    for (int isc = 0; isc < 12; isc++) { delete bs[isc]; delete xs[isc]; }
  }
  for (int isc = 0; isc < 12 && !lockstep; isc++) {
    hipLaunchKernelGGL(spread_slot_kernel, dim3((g.Vh + 255) / 256, 2), dim3(256), 0, computeStream(), (double *)source.V(), (const double *)phi.V(), source.Stride(),
                       parityDoubles(source), g.Vh, isc / 3, isc % 3);
    HIP_CHECK(hipGetLastError());
    for (int fl = 0; fl < 2; fl++) {
      const QudaTwistFlavorType flavor = fl == 0 ? QUDA_TWIST_PLUS : QUDA_TWIST_MINUS;   // up, then down (:6401, :6470)
      param->twist_flavor = flavor;
      b->changeTwist(flavor); x->changeTwist(flavor);
      *b = source;
      ColorSpinorField *in = nullptr, *out = nullptr;
      dirac.prepare(in, out, *x, *b, param->solution_type);
      param->preconditioner = fl == 0 ? param->preconditionerUP : param->preconditionerDN;
      // counters: SolverParam starts from the values in *param and updateInvertParam adds them back (reference
      // include/invert_quda.h:262-300), which in the reference's loop doubles the running totals at every solve; summed
      // properly here
      param->secs = 0; param->gflops = 0; param->iter = 0;
      SolverParam sp(*param);
      Solver *solve = Solver::create(sp, m, mSloppy, mPre);
      // the smeared source on the solve parity is the initial guess (:6442-6445; used when use_init_guess says so)
      *out = flag_eo ? source.Even() : source.Odd();
      out->changeTwist(flavor);
      (*solve)(*out, *in);
      sp.updateInvertParam(*param);
      secs += param->secs; gflops += param->gflops; iters += param->iter;
      dirac.reconstruct(*x, *b, param->solution_type);
      delete solve;
      result = *x;
      if (eachDevice) eachDevice(ctx, isc, fl == 0 ? +1 : -1, result, rescale ? 2.0 * param->kappa : 1.0);
      deviceToLex(h_one.data(), result, g, true, rescale ? 2.0 * param->kappa : 1.0);
      each(ctx, isc, fl == 0 ? +1 : -1, h_one.data(), vec);
    }
  }
  param->secs = secs; param->gflops = gflops; param->iter = iters;
  delete b; delete x;
  delete d; delete dSloppy; delete dPre;
  if (gauge_APE) delete Uape;
}

// Twelve given sources of ONE twist flavour (+1 up, -1 down; full fp64 device fields in the device basis) through the path of the forward
// solves above: one lockstep solve where the solver is multigrid-preconditioned GCR and lockstepFits allows it, one by one otherwise.
// Every reconstructed solution is handed to `done` unscaled, with the factor of the normalisation.  param->secs / gflops / iter are
// those of these twelve solves.
void solveTwelveEach(QudaInvertParam *param, int flavorSign, ColorSpinorField *const sources[12], const char *fname,
                     void (*done)(void *ctx, int isc, ColorSpinorField &result, double scale), void *ctx) {
  checkCalcParam(param, fname);
  const bool flag_eo = param->matpc_type == QUDA_MATPC_EVEN_EVEN;
  const LatticeGeom &g = residentGeom();
  const QudaTwistFlavorType flavor = flavorSign > 0 ? QUDA_TWIST_PLUS : QUDA_TWIST_MINUS;
  param->twist_flavor = flavor;
  param->preconditioner = flavorSign > 0 ? param->preconditionerUP : param->preconditionerDN;
  const bool pc_solve = true;
  DiracParam dp, dpSloppy, dpPre;
  setDiracParam(dp, param, pc_solve);
  setDiracSloppyParam(dpSloppy, param, pc_solve);
  setDiracPreParam(dpPre, param, pc_solve);
  Dirac *d = Dirac::create(dp), *dSloppy = Dirac::create(dpSloppy), *dPre = Dirac::create(dpPre);
  Dirac &dirac = *d;
  DiracM m(dirac), mSloppy(*dSloppy), mPre(*dPre);
  ColorSpinorParam cp64 = deviceSpinorParam(QUDA_DOUBLE_PRECISION, QUDA_FULL_SITE_SUBSET, flavor);
  cp64.create = QUDA_ZERO_FIELD_CREATE;
  ColorSpinorField result(cp64);
  ColorSpinorParam cp = deviceSpinorParam(param->cuda_prec, QUDA_FULL_SITE_SUBSET, flavor);
  cp.create = QUDA_ZERO_FIELD_CREATE;
  const double scale = (param->mass_normalization == QUDA_MASS_NORMALIZATION || param->mass_normalization == QUDA_ASYMMETRIC_MASS_NORMALIZATION) ? 2.0 * param->kappa : 1.0;
  double secs = 0, gflops = 0;
  int iters = 0;
  const bool lockstep = param->inv_type == QUDA_GCR_INVERTER && param->inv_type_precondition == QUDA_MG_INVERTER && param->preconditionerUP && param->preconditionerDN &&
                        param->use_init_guess != QUDA_USE_INIT_GUESS_YES && lockstepFits(12, param, g);
  if (lockstep) {
    std::vector<ColorSpinorField *> bs(12), xs(12), ins(12), outs(12);
    for (int isc = 0; isc < 12; isc++) {
      bs[isc] = new ColorSpinorField(cp); xs[isc] = new ColorSpinorField(cp);
      *bs[isc] = *sources[isc];
      bs[isc]->changeTwist(flavor); xs[isc]->changeTwist(flavor);
      blas::zero(*xs[isc]);
      dirac.prepare(ins[isc], outs[isc], *xs[isc], *bs[isc], param->solution_type);
      ins[isc]->changeTwist(flavor); outs[isc]->changeTwist(flavor);
    }
    param->secs = 0; param->gflops = 0; param->iter = 0;
    SolverParam sp(*param);
    MG *K = static_cast<multigrid_solver *>(param->preconditioner)->mg;
    const MultiSrcSolve res = solveMultiSrcGCR(outs, ins, m, mSloppy, K, sp, dSloppy);
    secs += res.secs; iters += 12 * res.iter;
    double worst = 0;
    for (int isc = 0; isc < 12; isc++) worst = std::max(worst, sqrt(res.r2[isc] / res.b2[isc]));
    param->true_res = worst;
    for (int isc = 0; isc < 12; isc++) {
      dirac.reconstruct(*xs[isc], *bs[isc], param->solution_type);
      result = *xs[isc];
      done(ctx, isc, result, scale);
      delete bs[isc]; delete xs[isc];
    }
  } else {
    ColorSpinorField b(cp), x(cp);
    for (int isc = 0; isc < 12; isc++) {
      b = *sources[isc];
      b.changeTwist(flavor); x.changeTwist(flavor);
      ColorSpinorField *in = nullptr, *out = nullptr;
      dirac.prepare(in, out, x, b, param->solution_type);
      param->secs = 0; param->gflops = 0; param->iter = 0;
      SolverParam sp(*param);
      Solver *solve = Solver::create(sp, m, mSloppy, mPre);
      *out = flag_eo ? sources[isc]->Even() : sources[isc]->Odd();   // the source on the solve parity is the initial guess, as for the forward solves
      out->changeTwist(flavor);
      (*solve)(*out, *in);
      sp.updateInvertParam(*param);
      secs += param->secs; gflops += param->gflops; iters += param->iter;
      dirac.reconstruct(x, b, param->solution_type);
      delete solve;
      result = x;
      done(ctx, isc, result, scale);
    }
  }
  param->secs = secs; param->gflops = gflops; param->iter = iters;
  delete d; delete dSloppy; delete dPre;
}
}  // namespace quda

extern "C" {

void qudaAmdCalcMGPropagators(void *h_prop_up, void *h_prop_dn, void **gauge_APE, QudaInvertParam *param, const QudaAmdSourceParam *src) {
  if (!h_prop_up || !h_prop_dn) errorQuda("qudaAmdCalcMGPropagators: propagator buffers are NULL");
  struct Out { double *up, *dn; } out = {(double *)h_prop_up, (double *)h_prop_dn};
  calcMGPropagatorsEach(gauge_APE, param, src, "qudaAmdCalcMGPropagators",
                        [](void *c, int isc, int flavor, const double *h, size_t n) { Out *o = (Out *)c; memcpy((flavor > 0 ? o->up : o->dn) + (size_t)isc * n, h, n * sizeof(double)); }, &out);
}

}

// ================================================================================================
// the reference's entry-point names (include/qudaQKXTM_Kepler.h): solve loops only, solutions go to the registered sink
// ================================================================================================
#include "qudaQKXTM_Kepler.h"

namespace quda {

static QudaAmdSolutionSink g_sink = nullptr;
static void *g_sinkCtx = nullptr;

static void toSink(const char *kind, int index, int flavor, const double *h_source, const double *h_solution, size_t nreal) {
  if (g_sink) { g_sink(g_sinkCtx, kind, index, flavor, h_source, h_solution, nreal); return; }
  double n2 = 0;
  for (size_t i = 0; i < nreal; i++) n2 += h_solution[i] * h_solution[i];
  comm_allreduce(&n2, 1);
  printfQuda("%s %d (flavour %+d): |solution|^2 = %.12e (no sink registered: dropped)\n", kind, index, flavor, n2);
}

// Z4 noise on every spin-colour component of every local site (reference getStochasticRandomSource<Float>,
// lib/qudaQKXTM_Kepler_utils.cpp:149-180: 1, -1, i, -i with equal probability; UNITY: all ones).  The reference draws from GSL's
// ranlux seeded with seed + rank * seed; GSL is not a dependency here: a counter-based generator keyed by (seed, rank, source
// number, component) — the same stream for a given decomposition, independent of how many sources came before.
static void stochasticSource(double *h, size_t ncomplex, unsigned long seed, int isrc, SOURCE_T type) {
  const unsigned long long key = (unsigned long long)seed * 0x9E3779B97F4A7C15ull + (unsigned long long)commGrid().rank * 0xD1B54A32D192ED03ull + (unsigned long long)isrc * 0x94D049BB133111EBull;
  for (size_t i = 0; i < ncomplex; i++) {
    if (type == UNITY) { h[2 * i] = 1.0; h[2 * i + 1] = 0.0; continue; }
    const int r = z4Draw(key, i);
    h[2 * i] = r == 0 ? 1.0 : (r == 1 ? -1.0 : 0.0);
    h[2 * i + 1] = r == 2 ? 1.0 : (r == 3 ? -1.0 : 0.0);
  }
}

// the loop of calcMG_loop_wOneD_TSM_EvenOdd (reference lib/interface_quda.cpp:8535-9430).  writeLoops (the loop output switched on,
// qudaAmdSetLoopOutput): every solution is contracted from the device-resident field after the reconstruction (loop.hip), the sums
// over the noise vectors are cumulative and a snapshot goes to the reference's ASCII files whenever (is + 1) % Ndump == 0.
// defl (calcMG_loop_wOneD_TSM_wExact, reference :7940-8420): one set of accumulators per deflation step; before the contraction the
// solution is projected off the first steps[s] eigenvectors, the sink still receives the solution itself
static void loopSolves(QudaInvertParam *param, const qudaQKXTM_loopInfo &loopInfo, const qudaQKXTMinfo_Kepler &info, const char *fname, bool writeLoops,
                       Deflation *defl = nullptr, const std::vector<int> &steps = std::vector<int>()) {
  if (!gaugePrecise) errorQuda("%s: Gauge field not allocated", fname);
  if (!cloverPrecise && param->dslash_type == QUDA_TWISTED_CLOVER_DSLASH) errorQuda("%s: Clover field not allocated", fname);
  if (param->twist_flavor == QUDA_TWIST_NONDEG_DOUBLET) errorQuda("%s: the QKXTM drivers are not available for the non-degenerate doublet", fname);
  if (param->solve_type != QUDA_DIRECT_PC_SOLVE) errorQuda("%s: This function works only with Direct solve and even odd preconditioning", fname);
  if (param->gamma_basis != QUDA_UKQCD_GAMMA_BASIS) errorQuda("%s: This function works only with ukqcd gamma basis", fname);
  if (param->dirac_order != QUDA_DIRAC_ORDER) errorQuda("%s: This function works only with colors inside the spins", fname);
  if (param->solution_type != QUDA_MAT_SOLUTION) errorQuda("%s: solution_type %d not supported (QUDA_MAT_SOLUTION)", fname, param->solution_type);
  if (info.isEven && param->matpc_type != QUDA_MATPC_EVEN_EVEN) errorQuda("%s: Inconsistency between operator types!", fname);        // :8560
  if (!info.isEven && param->matpc_type != QUDA_MATPC_ODD_ODD) errorQuda("%s: Inconsistency between operator types!", fname);

  // truncated-solver-method stopping criterion (:8595-8625): iterations if given, else tolerance; both given -> iterations
  const bool useTSM = loopInfo.useTSM;
  long TSM_maxiter = 0;
  double TSM_tol = 0.0;
  if (loopInfo.TSM_tol == 0 && loopInfo.TSM_maxiter != 0) TSM_maxiter = loopInfo.TSM_maxiter;
  else if (loopInfo.TSM_tol != 0 && loopInfo.TSM_maxiter == 0) TSM_tol = loopInfo.TSM_tol;
  else if (useTSM && loopInfo.TSM_tol != 0 && loopInfo.TSM_maxiter != 0) {
    warningQuda("Both max-iter = %ld and tolerance = %lf defined as criterions for the TSM. Proceeding with max-iter = %ld criterion.", loopInfo.TSM_maxiter, loopInfo.TSM_tol, loopInfo.TSM_maxiter);
    TSM_maxiter = loopInfo.TSM_maxiter;
  } else if (useTSM) errorQuda("%s: the truncated solver method needs TSM_tol or TSM_maxiter", fname);

  const LatticeGeom &g = residentGeom();
  const size_t vec = (size_t)g.V * 24;
  param->secs = 0; param->gflops = 0; param->iter = 0;
  const bool pc_solve = true;
  DiracParam dp, dpSloppy, dpPre;
  setDiracParam(dp, param, pc_solve);
  setDiracSloppyParam(dpSloppy, param, pc_solve);
  setDiracPreParam(dpPre, param, pc_solve);
  Dirac *d = Dirac::create(dp), *dSloppy = Dirac::create(dpSloppy), *dPre = Dirac::create(dpPre);
  Dirac &dirac = *d;
  DiracM m(dirac), mSloppy(*dSloppy), mPre(*dPre);
  ColorSpinorParam cp64 = deviceSpinorParam(QUDA_DOUBLE_PRECISION, QUDA_FULL_SITE_SUBSET, param->twist_flavor);
  cp64.create = QUDA_ZERO_FIELD_CREATE;
  ColorSpinorField stage(cp64);
  ColorSpinorParam cp = deviceSpinorParam(param->cuda_prec, QUDA_FULL_SITE_SUBSET, param->twist_flavor);
  cp.create = QUDA_ZERO_FIELD_CREATE;
  ColorSpinorField b(cp), x(cp);
  std::vector<double> h_src(vec), h_sol(vec);
  const bool rescale = param->mass_normalization == QUDA_MASS_NORMALIZATION || param->mass_normalization == QUDA_ASYMMETRIC_MASS_NORMALIZATION;
  double secs = 0, gflops = 0;
  int iters = 0;

  // loop output: accumulator 0 the production run (then the high-precision solves of the bias run), 1 the low-precision solves of the bias run
  std::vector<LoopAccum *> acc[2];
  std::vector<std::string> pref[2];
  const size_t nAcc = defl ? steps.size() : 1;
  auto prefixOf = [&](size_t s) {   // :8050 with deflation, :9060 without
    if (defl) return std::string(loopInfo.loop_fname) + (useTSM ? "_stoch_TSM_NeV" : "_stoch_NeV") + std::to_string(steps[s]);
    return std::string(loopInfo.loop_fname) + (useTSM ? "_stoch_TSM_MG" : "_stoch_MG");
  };
  ColorSpinorField *deflated = nullptr;
  const char *tsmTag = nullptr;
  int Ndump = 0;
  if (writeLoops) {
    if (param->dslash_type != QUDA_TWISTED_MASS_DSLASH && param->dslash_type != QUDA_TWISTED_CLOVER_DSLASH)
      errorQuda("%s: the one-end trick works only for twisted-mass and twisted-clover fermions", fname);
    if (loopInfo.HighMomForm) errorQuda("%s: the high-momenta form is written only as HDF5, which this library does not link; set HighMomForm = false", fname);
    if (loopInfo.FileFormat == HDF5_FORM) warningQuda("%s: HDF5 is not linked into this library; writing the loops in ASCII format", fname);
    if (info.Q_sq < 0) errorQuda("%s: Q_sq = %d", fname, info.Q_sq);
    for (size_t s = 0; s < nAcc; s++) {
      acc[0].push_back(loopAccumCreate(info.Q_sq));
      if (useTSM) acc[1].push_back(loopAccumCreate(info.Q_sq));
      pref[0].push_back(prefixOf(s));
      pref[1].push_back(std::string());
    }
    if (defl) deflated = new ColorSpinorField(cp64);
    int L[3];
    for (int k = 0; k < 3; k++) L[k] = g.X[k] * commGrid().dims[k];
    const int Nmoms = qudaAmdLoopMomenta(L, info.Q_sq, nullptr, 0);
    if (loopInfo.Nmoms != 0 && loopInfo.Nmoms != Nmoms) errorQuda("%s: loopInfo.Nmoms = %d, but Q_sq = %d holds %d momenta", fname, loopInfo.Nmoms, info.Q_sq, Nmoms);
    Ndump = useTSM ? loopInfo.TSM_NdumpLP : loopInfo.Ndump;
    if (Ndump <= 0 || (useTSM && loopInfo.TSM_NHP > 0 && loopInfo.TSM_NdumpHP <= 0)) errorQuda("%s: the dump interval must be positive", fname);
    tsmTag = useTSM ? "NLP" : nullptr;
  }
  // `stage` holds the reconstructed solution in the solver's normalisation (the reference contracts it without the 2 kappa rescale)
  auto absorb = [&](int which, int index) {
    for (size_t s = 0; s < acc[which].size(); s++) {
      ColorSpinorField *v = &stage;
      if (defl) {
        blas::copy(*deflated, stage);
        deflationProject(defl, steps[s], *deflated);
        v = deflated;
      }
      loopContractAdd(*acc[which][s], *v, param);
      if ((index + 1) % Ndump == 0) loopWriteAscii(*acc[which][s], pref[which][s].c_str(), tsmTag, index + 1);
    }
  };

  auto solve = [&](bool lowPrecision, const char *kind, int index, int which) {
    lexToDevice(stage, h_src.data(), g, true);
    b = stage;
    blas::zero(x);
    ColorSpinorField *in = nullptr, *out = nullptr;
    dirac.prepare(in, out, x, b, param->solution_type);
    const double tol0 = param->tol;
    const int maxiter0 = param->maxiter;
    if (lowPrecision) { if (TSM_maxiter == 0) param->tol = TSM_tol; else param->maxiter = (int)TSM_maxiter; }   // :9025-9030
    param->secs = 0; param->gflops = 0; param->iter = 0;
    SolverParam sp(*param);
    Solver *s = Solver::create(sp, m, mSloppy, mPre);
    (*s)(*out, *in);
    sp.updateInvertParam(*param);
    delete s;
    param->tol = tol0; param->maxiter = maxiter0;
    secs += param->secs; gflops += param->gflops; iters += param->iter;
    dirac.reconstruct(x, b, param->solution_type);
    stage = x;
    absorb(which, index);
    deviceToLex(h_sol.data(), stage, g, true, rescale ? 2.0 * param->kappa : 1.0);
    toSink(kind, index, (int)param->twist_flavor, h_src.data(), h_sol.data(), vec);
  };

  // Groups of stochastic sources through ONE lockstep solve (block_solver.cpp) when the solver is multigrid-preconditioned GCR without an initial
  // guess: the hierarchy's cycle runs once per iteration for the whole group.  The sources of a group are drawn exactly as one by one (the
  // generator is keyed by the source number); QUDA_AMD_QKXTM_LOCKSTEP=0 keeps the reference's one-by-one order.
  int group = 1;
  if (param->inv_type == QUDA_GCR_INVERTER && param->inv_type_precondition == QUDA_MG_INVERTER && param->preconditioner && param->use_init_guess != QUDA_USE_INIT_GUESS_YES)
    for (group = 12; group > 1 && !lockstepFits(group, param, g); group /= 2) {}
  auto solveGroup = [&](bool lowPrecision, const char *kind, int first, int n) {
    std::vector<std::vector<double>> h_srcs(n, std::vector<double>(vec));
    std::vector<ColorSpinorField *> bs(n), xs(n), ins(n), outs(n);
    for (int j = 0; j < n; j++) {
      stochasticSource(h_srcs[j].data(), (size_t)g.V * 12, loopInfo.seed, first + j, info.source_type);
      lexToDevice(stage, h_srcs[j].data(), g, true);
      bs[j] = new ColorSpinorField(cp); xs[j] = new ColorSpinorField(cp);
      *bs[j] = stage;
      blas::zero(*xs[j]);
      dirac.prepare(ins[j], outs[j], *xs[j], *bs[j], param->solution_type);
      ins[j]->changeTwist(param->twist_flavor); outs[j]->changeTwist(param->twist_flavor);
    }
    const double tol0 = param->tol;
    const int maxiter0 = param->maxiter;
    if (lowPrecision) { if (TSM_maxiter == 0) param->tol = TSM_tol; else param->maxiter = (int)TSM_maxiter; }
    param->secs = 0; param->gflops = 0; param->iter = 0;
    SolverParam sp(*param);
    MG *K = static_cast<multigrid_solver *>(param->preconditioner)->mg;
    const MultiSrcSolve res = solveMultiSrcGCR(outs, ins, m, mSloppy, K, sp, dSloppy);
    param->tol = tol0; param->maxiter = maxiter0;
    secs += res.secs; iters += n * res.iter;
    for (int j = 0; j < n; j++) {
      dirac.reconstruct(*xs[j], *bs[j], param->solution_type);
      stage = *xs[j];
      absorb(0, first + j);
      deviceToLex(h_sol.data(), stage, g, true, rescale ? 2.0 * param->kappa : 1.0);
      toSink(kind, first + j, (int)param->twist_flavor, h_srcs[j].data(), h_sol.data(), vec);
      delete bs[j]; delete xs[j];
    }
  };

  // production sources: low-precision solves under the truncated solver method, full solves otherwise (:9000-9050)
  const int Nrun = useTSM ? loopInfo.TSM_NLP : loopInfo.Nstoch;
  for (int is = 0; is < Nrun;) {
    const int n = std::min(group, Nrun - is);
    if (n >= 2) { solveGroup(useTSM, useTSM ? "loop_LP" : "loop_stoch", is, n); is += n; continue; }
    stochasticSource(h_src.data(), (size_t)g.V * 12, loopInfo.seed, is, info.source_type);
    solve(useTSM, useTSM ? "loop_LP" : "loop_stoch", is, 0);
    is++;
  }
  // bias correction of the truncated solver method: TSM_NHP fresh sources solved to both precisions (:9170-9230)
  if (useTSM) {
    if (writeLoops) {   // :9164-9410: fresh accumulators, the high- and the low-precision sums side by side, both dumped every TSM_NdumpHP
      for (size_t s = 0; s < nAcc; s++) {
        acc[0][s]->zero();
        pref[0][s] = prefixOf(s) + "_HighPrec";
        pref[1][s] = prefixOf(s) + "_LowPrec";
      }
      tsmTag = "NHP";
      Ndump = loopInfo.TSM_NdumpHP;
    }
    for (int is = 0; is < loopInfo.TSM_NHP; is++) {
      stochasticSource(h_src.data(), (size_t)g.V * 12, loopInfo.seed, Nrun + is, info.source_type);
      solve(false, "loop_HP", is, 0);
      solve(true, "loop_HP_LP", is, 1);
    }
  }
  for (int which = 0; which < 2; which++)
    for (LoopAccum *a : acc[which]) delete a;
  delete deflated;
  param->secs = secs; param->gflops = gflops; param->iter = iters;
  delete d; delete dSloppy; delete dPre;
}

}  // namespace quda

extern "C" void qudaAmdSetSolutionSink(QudaAmdSolutionSink sink, void *ctx) { quda::g_sink = sink; quda::g_sinkCtx = ctx; }

void calcMG_threepTwop_EvenOdd(void **gaugeSmeared, void **gauge, QudaGaugeParam *gauge_param, QudaInvertParam *param, quda::qudaQKXTMinfo_Kepler info,
                               char *filename_twop, char *filename_threep, quda::WHICHPARTICLE NUCLEON) {
  (void)gauge_param;
  const char *fname = "calcMG_threepTwop_EvenOdd";
  if (info.Nsources < 0 || info.Nsources > MAX_NSOURCES) errorQuda("%s: Nsources = %d", fname, info.Nsources);
  // two-point output (qudaAmdSetTwopOutput): contractions from the device-resident solutions, the reference's ASCII files;
  // three-point output (qudaAmdSetThreepOutput): the fixed-sink sequential solves and contractions of the sources with run3pt_src != 0
  const bool twop = quda::twopOutputEnabled(), threep = quda::threepOutputEnabled();
  if (twop || threep) {
    if (info.CorrSpace == quda::POSITION_SPACE)
      errorQuda("%s: position-space correlators are written only as HDF5, which this library does not link; use CorrSpace = MOMENTUM_SPACE", fname);
    if (info.HighMomForm) errorQuda("%s: the high-momenta form is written only as HDF5, which this library does not link; set HighMomForm = false", fname);
    if (info.CorrFileFormat == quda::HDF5_FORM) warningQuda("%s: HDF5 is not linked into this library; writing the correlation functions in ASCII format", fname);
    if (twop && !filename_twop) errorQuda("%s: filename_twop is NULL", fname);
    if (info.Q_sq < 0) errorQuda("%s: Q_sq = %d", fname, info.Q_sq);
  }
  static const char *const projName[MAX_PROJS] = {"G4", "G5G123", "G5G1", "G5G2", "G5G3"};
  quda::GaugeField *Uder = nullptr;   // the links of the derivative operators and the conserved current
  if (threep) {
    if (!filename_threep) errorQuda("%s: filename_threep is NULL", fname);
    if (NUCLEON != quda::PROTON && NUCLEON != quda::NEUTRON) errorQuda("%s: NUCLEON = %d (proton and neutron only)", fname, (int)NUCLEON);
    if (info.Ntsink < 0 || info.Ntsink > MAX_TSINK) errorQuda("%s: Ntsink = %d", fname, info.Ntsink);
    for (int its = 0; its < info.Ntsink; its++) {
      if (info.Nproj[its] < 0 || info.Nproj[its] > MAX_PROJS) errorQuda("%s: Nproj[%d] = %d", fname, its, info.Nproj[its]);
      for (int ip = 0; ip < info.Nproj[its]; ip++)
        if (info.proj_list[its][ip] < 0 || info.proj_list[its][ip] >= MAX_PROJS) errorQuda("%s: proj_list[%d][%d] = %d", fname, its, ip, info.proj_list[its][ip]);
    }
    bool any = false;
    for (int isource = 0; isource < info.Nsources; isource++) any = any || info.run3pt_src[isource] != 0;
    if (any) Uder = gauge ? quda::loadLexGauge(gauge, quda::residentGeom()) : gaugePrecise;
  }
  double secs = 0, gflops = 0;
  int iters = 0;
  for (int isource = 0; isource < info.Nsources; isource++) {
    QudaAmdSourceParam src;
    for (int k = 0; k < 4; k++) src.sourcePosition[k] = info.sourcePosition[isource][k];
    src.nsmearGauss = info.nsmearGauss;
    src.alphaGauss = info.alphaGauss;
    const bool do3 = threep && info.run3pt_src[isource] != 0;
    struct Ctx {
      int base;
      quda::TwopProps *props;    // the two-point stage rotates these in place
      quda::TwopProps *sprops;   // sink-smeared, unrotated: what the sequential source is built from
      quda::ColorSpinorField **fwd;   // [2][12]: the unsmeared forward columns in the UKQCD basis, what the three-point contraction reads
      quda::ColorSpinorField *work;
      quda::GaugeField *U;
      int nsmear;
      double alpha;
    } ctx = {12 * isource, nullptr, nullptr, nullptr, nullptr, nullptr, info.nsmearGauss, info.alphaGauss};
    const quda::LatticeGeom &g = quda::residentGeom();
    std::vector<quda::ColorSpinorField *> fwd;
    if (twop || do3) {
      if (info.nsmearGauss > 0 && !gaugeSmeared && !quda::gaugeSmeared) errorQuda("%s: gaugeSmeared is NULL and no smeared field is resident (performAPEnStep)", fname);
      ctx.U = info.nsmearGauss > 0 ? (gaugeSmeared ? quda::loadLexGauge(gaugeSmeared, g) : quda::gaugeSmeared) : nullptr;
      if (twop) ctx.props = quda::twopPropsCreate(g);
      quda::ColorSpinorParam cp = quda::deviceSpinorParam(QUDA_DOUBLE_PRECISION, QUDA_FULL_SITE_SUBSET, QUDA_TWIST_NO);
      cp.create = QUDA_ZERO_FIELD_CREATE;
      ctx.work = new quda::ColorSpinorField(cp);
      if (do3) {
        ctx.sprops = quda::twopPropsCreate(g);
        for (int k = 0; k < 24; k++) fwd.push_back(new quda::ColorSpinorField(cp));
        ctx.fwd = fwd.data();
      }
    }
    quda::calcMGPropagatorsEach(
        gaugeSmeared, param, &src, fname,
        [](void *c, int isc, int flavor, const double *h, size_t n) { quda::toSink(flavor > 0 ? "prop_up" : "prop_dn", ((Ctx *)c)->base + isc, flavor, nullptr, h, n); }, &ctx,
        (twop || do3) ? +[](void *c, int isc, int flavor, quda::ColorSpinorField &x, double scale) {
          Ctx *o = (Ctx *)c;
          const int fl = flavor > 0 ? 0 : 1;
          if (o->fwd) quda::threepToUkqcd(*o->fwd[fl * 12 + isc], x, scale);   // before the sink smearing, from the solution itself
          quda::blas::copy(*o->work, x);   // the solution itself still goes to the sink unsmeared
          bool smeared = false;
          if (o->props) { quda::twopAbsorbColumn(*o->props, fl, isc, *o->work, quda::residentGeom(), o->U, o->nsmear, o->alpha, true, scale); smeared = true; }
          if (o->sprops) quda::twopAbsorbColumn(*o->sprops, fl, isc, *o->work, quda::residentGeom(), smeared ? nullptr : o->U, o->nsmear, o->alpha, true, scale);
        } : nullptr);
    secs += param->secs; gflops += param->gflops; iters += param->iter;
    const int T = g.X[3] * quda::commGrid().dims[3];
    const int Nm = (twop || do3) ? qudaAmdTwopMomenta(info.Q_sq, nullptr, 0) : 0;
    if (twop) {
      std::vector<double> mes((size_t)T * Nm * 2 * 10 * 2), bar((size_t)T * Nm * 2 * 10 * 16 * 2);
      quda::twopContract(*ctx.props, g, src.sourcePosition, info.Q_sq, mes.data(), bar.data());
      quda::twopWriteAscii(filename_twop, src.sourcePosition, info.Q_sq, T, mes.data(), bar.data());
      quda::twopPropsDestroy(ctx.props);
    }
    if (do3) {
      // fixed-sink stage (reference :6560-6950): for every sink separation, projector and part the sequential source, twelve solves
      // with the twist opposite to the inserted flavour, the contraction with the forward propagator of that flavour, three files
      quda::ColorSpinorParam cp = quda::deviceSpinorParam(QUDA_DOUBLE_PRECISION, QUDA_FULL_SITE_SUBSET, QUDA_TWIST_NO);
      cp.create = QUDA_ZERO_FIELD_CREATE;
      quda::ColorSpinorField *seqSrc[12], *seqSol[12];
      for (int k = 0; k < 12; k++) { seqSrc[k] = new quda::ColorSpinorField(cp); seqSol[k] = new quda::ColorSpinorField(cp); }
      const size_t vec = (size_t)g.V * 24;
      std::vector<double> h_src(vec), h_sol(vec), loc((size_t)T * Nm * 16 * 2), noe((size_t)T * Nm * 4 * 2), oneD((size_t)T * Nm * 64 * 2);
      QudaAmdThreepParam tp;
      for (int k = 0; k < 4; k++) tp.sourcePosition[k] = src.sourcePosition[k];
      tp.Q_sq = info.Q_sq; tp.particle = (int)NUCLEON; tp.nsmearGauss = info.nsmearGauss; tp.alphaGauss = info.alphaGauss;
      for (int its = 0; its < info.Ntsink; its++)
        for (int ip = 0; ip < info.Nproj[its]; ip++)
          for (int part = 1; part <= 2; part++) {
            tp.tsinkSource = info.tsinkSource[its]; tp.projector = info.proj_list[its][ip]; tp.part = part;
            if (tp.tsinkSource < 0 || tp.tsinkSource >= T) errorQuda("%s: tsinkSource[%d] = %d", fname, its, tp.tsinkSource);
            quda::threepSeqSourceDevice(seqSrc, *ctx.sprops, ctx.U, &tp);
            const int s = quda::threepInsertedFlavor(tp.particle, part);
            struct SeqCtx {
              const char *kind;
              int base, flavor;
              quda::ColorSpinorField **src, **sol;
              double *h_src, *h_sol;
              size_t vec;
            } sc = {part == 1 ? "seq_part1" : "seq_part2", ((isource * info.Ntsink + its) * info.Nproj[its] + ip) * 12, -s, seqSrc, seqSol, h_src.data(), h_sol.data(), vec};
            quda::solveTwelveEach(param, -s, seqSrc, fname, [](void *c, int isc, quda::ColorSpinorField &x, double scale) {
              SeqCtx *o = (SeqCtx *)c;
              const quda::LatticeGeom &gg = quda::residentGeom();
              quda::threepToUkqcd(*o->sol[isc], x, scale);
              quda::deviceToLex(o->h_src, *o->src[isc], gg, true, 1.0);
              quda::deviceToLex(o->h_sol, x, gg, true, scale);
              quda::toSink(o->kind, o->base + isc, o->flavor, o->h_src, o->h_sol, o->vec);
            }, &sc);
            secs += param->secs; gflops += param->gflops; iters += param->iter;
            quda::threepContract(loc.data(), noe.data(), oneD.data(), seqSol, ctx.fwd + (s > 0 ? 0 : 12), *Uder, &tp);
            const char *pname = info.thrp_proj_type[tp.projector] ? info.thrp_proj_type[tp.projector] : projName[tp.projector];
            const std::string out = std::string(filename_threep) + "_tsink" + std::to_string(tp.tsinkSource) + "_proj" + pname;
            quda::threepWriteAscii(out.c_str(), &tp, T, loc.data(), noe.data(), oneD.data());
          }
      for (int k = 0; k < 12; k++) { delete seqSrc[k]; delete seqSol[k]; }
      quda::twopPropsDestroy(ctx.sprops);
      for (quda::ColorSpinorField *f : fwd) delete f;
    }
    if (twop || do3) {
      delete ctx.work;
      if (ctx.U && gaugeSmeared) delete ctx.U;
    }
  }
  if (Uder && gauge) delete Uder;
  param->secs = secs; param->gflops = gflops; param->iter = iters;
}

void calcMG_loop_wOneD_TSM_EvenOdd(void **gaugeToPlaquette, QudaInvertParam *param, QudaGaugeParam *gauge_param, quda::qudaQKXTM_loopInfo loopInfo,
                                   quda::qudaQKXTMinfo_Kepler info) {
  (void)gaugeToPlaquette; (void)gauge_param;   // plaquette check and covariant derivatives of the contraction stage
  quda::loopSolves(param, loopInfo, info, "calcMG_loop_wOneD_TSM_EvenOdd", quda::loopOutputEnabled());
}

static std::vector<double> g_lastEvals;
extern "C" int qudaAmdLastEigenvalues(double *evals, int n) {
  if (evals) for (int i = 0; i < n && i < (int)g_lastEvals.size(); i++) evals[i] = g_lastEvals[i];
  return (int)g_lastEvals.size();
}

void calcMG_loop_wOneD_TSM_wExact(void **gaugeToPlaquette, QudaInvertParam *EVparam, QudaInvertParam *param, QudaGaugeParam *gauge_param,
                                  quda::qudaQKXTM_arpackInfo arpackInfo, quda::qudaQKXTM_loopInfo loopInfo, quda::qudaQKXTMinfo_Kepler info) {
  (void)gaugeToPlaquette; (void)gauge_param;
  const char *fname = "calcMG_loop_wOneD_TSM_wExact";
  if (arpackInfo.nEv == 0) {   // the undeflated loop: the solves run, no file is written
    if (quda::loopOutputEnabled()) {
      static bool warned = false;
      if (!warned) warningQuda("%s: nEv = 0, there is no exact part of the loops; the solves run, no loop files are written", fname);
      warned = true;
    }
    quda::loopSolves(param, loopInfo, info, fname, false);
    return;
  }
  // reference :7118-7126, then what its exact-loop and projection functions and this eigensolver require
  if (!EVparam) errorQuda("%s: EVparam is NULL", fname);
  if (EVparam->matpc_type != QUDA_MATPC_EVEN_EVEN_ASYMMETRIC && EVparam->matpc_type != QUDA_MATPC_ODD_ODD_ASYMMETRIC)
    errorQuda("%s: EVparam->matpc_type: only asymmetric operators are supported in deflation", fname);
  if (arpackInfo.isEven != (EVparam->matpc_type == QUDA_MATPC_EVEN_EVEN_ASYMMETRIC)) errorQuda("%s: EVparam->matpc_type: inconsistency between operator types (arpackInfo.isEven)", fname);
  if (!arpackInfo.isFullOp) errorQuda("%s: arpackInfo.isFullOp must be set: the exact part and the projection work with the full operator", fname);
  if (arpackInfo.nEv < 0) errorQuda("%s: arpackInfo.nEv = %d", fname, arpackInfo.nEv);
  if (arpackInfo.spectrumPart != quda::SR) errorQuda("%s: arpackInfo.spectrumPart = %d, only SR (the smallest eigenvalues) is supported", fname, (int)arpackInfo.spectrumPart);
  if (arpackInfo.nKv <= arpackInfo.nEv) errorQuda("%s: arpackInfo.nKv = %d must exceed nEv = %d", fname, arpackInfo.nKv, arpackInfo.nEv);
  if (loopInfo.nSteps_defl < 1 || loopInfo.nSteps_defl > MAX_DEFLSTEPS) errorQuda("%s: loopInfo.nSteps_defl = %d (1 .. %d)", fname, loopInfo.nSteps_defl, MAX_DEFLSTEPS);
  std::vector<int> steps(loopInfo.deflStep, loopInfo.deflStep + loopInfo.nSteps_defl);
  for (size_t s = 0; s < steps.size(); s++)
    if (steps[s] < 1 || steps[s] > arpackInfo.nEv || (s > 0 && steps[s] <= steps[s - 1]))
      errorQuda("%s: loopInfo.deflStep[%d] = %d (ascending, 1 .. nEv = %d)", fname, (int)s, steps[s], arpackInfo.nEv);
  const bool output = quda::loopOutputEnabled();
  if (output) {
    if (loopInfo.HighMomForm) errorQuda("%s: the high-momenta form is written only as HDF5, which this library does not link; set HighMomForm = false", fname);
    if (info.Q_sq < 0) errorQuda("%s: Q_sq = %d", fname, info.Q_sq);
  }
  if (arpackInfo.arpack_logfile[0]) printfQuda("%s: arpack_logfile is ignored (the eigensolver of this library is not ARPACK)\n", fname);

  QudaAmdEigParam ep;
  ep.nEv = arpackInfo.nEv; ep.nKv = arpackInfo.nKv; ep.PolyDeg = arpackInfo.PolyDeg; ep.isACC = arpackInfo.isACC ? 1 : 0; ep.maxRestarts = arpackInfo.maxIterArpack;
  ep.amin = arpackInfo.amin; ep.amax = arpackInfo.amax; ep.tol = arpackInfo.tolArpack;
  quda::Deflation *defl = quda::deflationCreate(param, &ep);
  const int nEv = quda::deflationSize(defl);
  g_lastEvals.assign(quda::deflationEigenvalues(defl), quda::deflationEigenvalues(defl) + nEv);
  {
    const quda::LatticeGeom &g = quda::residentGeom();
    const size_t vec = (size_t)g.V * 24;
    std::vector<double> h(vec);
    for (int i = 0; i < nEv; i++) {
      quda::deviceToLex(h.data(), quda::deflationVector(defl, i), g, true, 1.0);
      quda::toSink("eigvec", i, (int)param->twist_flavor, nullptr, h.data(), vec);
    }
  }
  if (output) {   // reference :7643-7743: the exact part for every deflation step, one print, no dump number in the name
    quda::LoopAccum *A = quda::loopAccumCreate(info.Q_sq);
    int done = 0;
    for (int n : steps) {
      quda::deflationExactLoopAdd(defl, *A, done, n);
      done = n;
      const std::string pref = std::string(loopInfo.loop_fname) + "_exact_NeV" + std::to_string(n);
      quda::loopWriteAscii(*A, pref.c_str(), nullptr, -1);
    }
    delete A;
  }
  quda::loopSolves(param, loopInfo, info, fname, output, defl, steps);
  quda::deflationDestroy(defl);
}
