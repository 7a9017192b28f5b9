// block_solver.cpp — several right-hand sides through MG-preconditioned GCR in lockstep (invertMultiSrcQuda).
//
// The reference declares the entry point (include/quda.h:647, QudaInvertParam::num_src) and carries a multi-source fifth dimension through
// its coarse-grid kernel (lib/dslash_coarse.cu:278, :294-333), but its invertMultiSrcQuda "is just a copy of invertQuda and cannot work"
// (lib/interface_quda.cpp:2546-2549).  The consumer is there all the same: calcMG_threepTwop_EvenOdd solves twelve spin-colour sources per
// flavour with one operator and one hierarchy (lib/interface_quda.cpp:6018-6531).  Here the sources go through the solver TOGETHER:
//   * outer solver: restarted flexible GCR per source with a shared Krylov index (reference lib/inv_gcr_quda.cpp:235-516 per source; a source
//     that has converged simply stops being updated), mixed precision and true-residual restarts as the single-source GCR of solver.cpp,
//     whose Krylov step and solution update it shares (solver.h gcrKrylovStep / gcrUpdateSolution);
//   * preconditioner: ONE multigrid cycle for all sources (MG::cycleBlock, block_mg_cycle.cpp): smoothing, restriction and prolongation on
//     the fine level per source or on block fields (block_fine_smoother.cpp), and everything below the fine level on block fields
//     (block_coarse_cycle.cpp).
#include <cmath>
#include <cstdio>
#include <cstring>

#include "block_cycle.h"
#include "gcr_core.h"
#include "interface_internal.h"

void setTuning(QudaTune tune);   // include/util_quda.h

namespace quda {

void massRescale(ColorSpinorField &b, QudaInvertParam &param);   // solve_interface.cpp

static long long g_msStats[4] = {0, 0, 0, 0};   // qudaAmdMultiSrcStats
void multiSrcCount(MultiSrcStat which) { g_msStats[which]++; }

// ================================================================================================
// lockstep GCR (reference lib/inv_gcr_quda.cpp:235-516 per source; host form solver.cpp GCR::operator())
// ================================================================================================
static MultiSrcSolve blockGCR(std::vector<ColorSpinorField *> &x, std::vector<ColorSpinorField *> &b, DiracMatrix &mat, DiracMatrix &matSloppy, MG *K, SolverParam &param, const Dirac *sloppyPC,
                              const Dirac *sloppyFull = nullptr) {
  const int ns = (int)x.size(), nK = param.Nkrylov;
  MultiSrcSolve res;
  res.r2.assign(ns, 0.0); res.b2.assign(ns, 0.0);
  const bool mixed = param.precision_sloppy != x[0]->Precision();
  const QudaPrecision ps = param.precision_sloppy;
  std::vector<ColorSpinorField *> r(ns), y(ns), xS(ns), rS(ns);
  std::vector<std::vector<ColorSpinorField *>> p(ns), Ap(ns);
  for (int i = 0; i < ns; i++) {
    r[i] = like(*x[i], x[i]->Precision(), true); y[i] = like(*x[i], x[i]->Precision(), true);
    xS[i] = mixed ? like(*x[i], ps, true) : x[i]; rS[i] = mixed ? like(*x[i], ps, true) : r[i];
    p[i].assign(nK, nullptr); Ap[i].assign(nK, nullptr);   // the Krylov space grows with the iteration count (12 sources x 40 fields otherwise)
    for (ColorSpinorField *f : {r[i], y[i], xS[i], rS[i]}) f->twistFlavor = b[i]->twistFlavor;
  }
  auto grow = [&](int k) {   // direction k of every source: written in full before it is read, so not cleared
    for (int i = 0; i < ns; i++) {
      if (p[i][k]) continue;
      p[i][k] = like(*x[i], ps, false); Ap[i][k] = like(*x[i], ps, false);
      p[i][k]->twistFlavor = Ap[i][k]->twistFlavor = b[i]->twistFlavor;
    }
  };
  std::vector<GcrCoeffs> coeffs(ns, GcrCoeffs(nK));
  std::vector<double> stop(ns), r2(ns), r2_old(ns);
  std::vector<char> open(ns, 1);
  blas::setGlobalReduction(param.global_reduction);
  const double t0 = wallTime();
  for (int i = 0; i < ns; i++) {
    res.b2[i] = blas::norm2(*b[i]);
    if (res.b2[i] == 0.0) errorQuda("Source %d has zero norm", i);
    blas::copy(*r[i], *b[i]);
    r2[i] = r2_old[i] = res.b2[i];
    blas::zero(*x[i]);
    if (mixed) { blas::zero(*xS[i]); blas::copy(*rS[i], *r[i]); }
    stop[i] = Solver::stopping(param.tol, res.b2[i], param.residual_type);
  }
  // test hook (tests/test_multisrc_gpu.py): "i:f" loosens the tolerance of source i by the factor f, so that it converges — and stops being
  // updated — iterations before the others; with one operator and one preconditioner the sources otherwise finish together
  if (const char *e = getenv("QUDA_AMD_MULTISRC_TEST_LOOSE")) {
    int i = -1;
    double f = 1.0;
    if (sscanf(e, "%d:%lf", &i, &f) == 2 && i >= 0 && i < ns && f >= 1.0) stop[i] *= f * f;
  }
  auto anyOpen = [&]() { for (int i = 0; i < ns; i++) if (open[i]) return true; return false; };
  int k = 0, total = 0;
  std::vector<ColorSpinorField *> pk(ns), rk(ns);
  while (anyOpen() && total < param.maxiter) {
    // p_k = K r for every open source: one block cycle
    grow(k);
    for (int i = 0; i < ns; i++) { pk[i] = p[i][k]; rk[i] = rS[i]; }
    bool done = false;
    if (K) {
      if (sloppyPC || sloppyFull) K->blockWantImage(ns, true);
      done = K->cycleBlock(pk, rk, open);
    }
    // A p_k for all sources while p_k is still on the smoother's block fields (even-odd outer solve on the smoother's operator)
    bool applied = false;
    if (done && sloppyPC) {
      std::vector<ColorSpinorField *> apk(ns);
      for (int i = 0; i < ns; i++) apk[i] = Ap[i][k];
      applied = K->blockApplyLast(apk, *sloppyPC, open);
    } else if (done && sloppyFull) {
      std::vector<ColorSpinorField *> apk(ns);
      for (int i = 0; i < ns; i++) apk[i] = Ap[i][k];
      applied = K->blockImageFull(apk, rk, *sloppyFull, open);
    }
    for (int i = 0; i < ns; i++) {
      if (!open[i]) continue;
      if (!done) { if (K) (*K)(*p[i][k], *rS[i]); else blas::copy(*p[i][k], *rS[i]); }
      blas::setGlobalReduction(param.global_reduction);
      if (!applied) matSloppy(*Ap[i][k], *p[i][k]);
      // the Krylov step of solver.cpp's GCR against the source's own directions, with the cDotProduct + caxpy chain and WITHOUT the measured-norm
      // guard: handing a per-source `blockedOk` flag in here, reset at the restart below, is all that applying it takes
      r2[i] = gcrKrylovStep(coeffs[i], Ap[i], k, *rS[i], GcrChain::Sequential, nullptr);
    }
    k++; total++;
    // reliable update / restart for ALL sources when the Krylov space is full or every open source has reached its sloppy target
    bool allSloppy = true, anyDelta = false;
    for (int i = 0; i < ns; i++) if (open[i]) { allSloppy = allSloppy && r2[i] < stop[i]; anyDelta = anyDelta || sqrt(r2[i] / r2_old[i]) < param.delta; }
    if (k == nK || total == param.maxiter || allSloppy || anyDelta) {
      for (int i = 0; i < ns; i++) {
        if (!open[i]) continue;
        gcrUpdateSolution(*xS[i], coeffs[i], k, p[i]);
        if (mixed) blas::copy(*x[i], *xS[i]);
        blas::xpy(*x[i], *y[i]);
        mat(*r[i], *y[i]);
        r2[i] = blas::xmyNorm(*b[i], *r[i]);
        if (r2[i] <= stop[i]) {
          open[i] = 0;
        } else {
          if (mixed) blas::copy(*rS[i], *r[i]);
          blas::zero(*xS[i]);
          if (!mixed) blas::zero(*x[i]);
        }
        r2_old[i] = r2[i];
      }
      k = 0;
    }
  }
  for (int i = 0; i < ns; i++) { blas::copy(*x[i], *y[i]); res.r2[i] = r2[i]; }
  res.iter = total;
  res.secs = wallTime() - t0;
  for (int i = 0; i < ns; i++) {
    delete r[i]; delete y[i];
    if (mixed) { delete xS[i]; delete rS[i]; }
    for (int kk = 0; kk < nK; kk++) { delete p[i][kk]; delete Ap[i][kk]; }   // nullptr beyond the directions used
  }
  blas::setGlobalReduction(true);
  return res;
}

MultiSrcSolve solveMultiSrcGCR(std::vector<ColorSpinorField *> &x, std::vector<ColorSpinorField *> &b, DiracMatrix &mat, DiracMatrix &matSloppy, MG *K, SolverParam &param, const Dirac *sloppyPC) {
  const MultiSrcSolve res = blockGCR(x, b, mat, matSloppy, K, param, sloppyPC);
  multiSrcCount(MS_SOLVES);
  return res;
}

}  // namespace quda

using namespace quda;

extern "C" {

void qudaAmdMultiSrcStats(long long out[4]) { for (int i = 0; i < 4; i++) out[i] = g_msStats[i]; }

// reference include/quda.h:647 (lib/interface_quda.cpp:2546: "currently that code is just a copy of invertQuda and cannot work"): param->num_src
// sources _hp_b[i] -> solutions _hp_x[i], one operator, one preconditioner.  GCR (optionally MG-preconditioned) direct solves; iter / secs
// are those of the lockstep solve, true_res the worst source's.
void invertMultiSrcQuda(void **_hp_x, void **_hp_b, QudaInvertParam *param) {
  if (!gaugePrecise) errorQuda("Gauge field not allocated");
  if (param->twist_flavor == QUDA_TWIST_NONDEG_DOUBLET) errorQuda("invertMultiSrcQuda: the multi-source solver is not available for the non-degenerate doublet");
  if (param->tune == QUDA_TUNE_YES || param->tune == QUDA_TUNE_NO) setTuning(param->tune);
  if (!cloverPrecise && param->dslash_type == QUDA_TWISTED_CLOVER_DSLASH) errorQuda("Clover field not allocated");
  const int ns = param->num_src;
  if (ns < 1 || ns > kMaxBlockRhs) errorQuda("num_src = %d outside 1 .. %d", ns, kMaxBlockRhs);
  const bool pc_solution = param->solution_type == QUDA_MATPC_SOLUTION;
  const bool pc_solve = param->solve_type == QUDA_DIRECT_PC_SOLVE;
  if (param->solve_type != QUDA_DIRECT_SOLVE && param->solve_type != QUDA_DIRECT_PC_SOLVE) errorQuda("invertMultiSrcQuda: direct solves only");
  if (param->solution_type != QUDA_MAT_SOLUTION && param->solution_type != QUDA_MATPC_SOLUTION) errorQuda("invertMultiSrcQuda: MAT / MATPC solutions only");
  if (param->inv_type != QUDA_GCR_INVERTER) errorQuda("invertMultiSrcQuda: the lockstep solver is GCR (inv_type %d)", param->inv_type);
  if (pc_solution && !pc_solve) errorQuda("Preconditioned (PC) solution_type requires a PC solve_type");
  param->secs = 0; param->gflops = 0; param->iter = 0;

  DiracParam dp, dpSloppy, dpPre;
  setDiracParam(dp, param, pc_solve);
  setDiracSloppyParam(dpSloppy, param, pc_solve);
  setDiracPreParam(dpPre, param, pc_solve);
  Dirac *d = Dirac::create(dp), *dSloppy = Dirac::create(dpSloppy), *dPre = Dirac::create(dpPre);
  const LatticeGeom &geom = residentGeom();
  std::vector<ColorSpinorField *> b(ns), x(ns), in(ns), out(ns);
  std::vector<double> nb(ns);
  for (int i = 0; i < ns; i++) {
    ColorSpinorParam cpuParam(_hp_b[i], *param, geom.X, pc_solution);
    ColorSpinorField h_b(cpuParam);
    ColorSpinorParam cp = deviceSpinorParam(param->cuda_prec, pc_solution ? QUDA_PARITY_SITE_SUBSET : QUDA_FULL_SITE_SUBSET, param->twist_flavor);
    cp.create = QUDA_ZERO_FIELD_CREATE;
    b[i] = new ColorSpinorField(cp); x[i] = new ColorSpinorField(cp);
    *b[i] = h_b;
    nb[i] = blas::norm2(*b[i]);
    if (nb[i] == 0.0) errorQuda("Source %d has zero norm", i);
    if (param->solver_normalization == QUDA_SOURCE_NORMALIZATION) blas::ax(1.0 / sqrt(nb[i]), *b[i]);
    massRescale(*b[i], *param);
    d->prepare(in[i], out[i], *x[i], *b[i], param->solution_type);
  }
  {
    DiracM m(*d), mSloppy(*dSloppy);
    SolverParam sp(*param);
    MG *K = nullptr;
    if (param->inv_type_precondition == QUDA_MG_INVERTER) {
      if (!param->preconditioner) errorQuda("GCR with multigrid preconditioner: param.preconditioner is NULL");
      K = static_cast<multigrid_solver *>(param->preconditioner)->mg;
    } else if (param->inv_type_precondition != QUDA_INVALID_INVERTER) {
      errorQuda("invertMultiSrcQuda: preconditioner %d not supported (none or QUDA_MG_INVERTER)", param->inv_type_precondition);
    }
    const MultiSrcSolve res = blockGCR(out, in, m, mSloppy, K, sp, pc_solve ? dSloppy : nullptr, pc_solve ? nullptr : dSloppy);
    multiSrcCount(MS_SOLVES);
    param->iter = res.iter;
    param->secs = res.secs;
    double worst = 0;
    for (int i = 0; i < ns; i++) worst = std::max(worst, sqrt(res.r2[i] / res.b2[i]));
    param->true_res = worst;
    // the hierarchy keeps its multi-source work space (solvers, residuals, block fields of the coarse levels) for the next call with the same
    // number of sources — a propagator is 12 of these calls' worth; released with the hierarchy or when num_src changes
  }
  for (int i = 0; i < ns; i++) {
    d->reconstruct(*x[i], *b[i], param->solution_type);
    if (param->solver_normalization == QUDA_SOURCE_NORMALIZATION) blas::ax(sqrt(nb[i]), *x[i]);
    ColorSpinorParam cpuParam(_hp_x[i], *param, geom.X, pc_solution);
    ColorSpinorField h_x(cpuParam);
    h_x = *x[i];
    delete b[i]; delete x[i];
  }
  delete d; delete dSloppy; delete dPre;
}

}
