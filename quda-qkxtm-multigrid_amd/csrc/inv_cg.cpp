// inv_cg.cpp — CG and multi-shift CG on Hermitian positive definite operators (M^dag M, optionally shifted).  Recurrences restated from the
// reference (lib/inv_cg_quda.cpp:40-360, plain CG; lib/inv_multi_cg_quda.cpp:115-527); outside the operator an iteration is three fused
// sweeps of blas.hip (axpyReDot / reDotProduct, axpyCGNorm, axpyZpbx or the multi-shift update).
//
// What differs from the reference:
//   * every sweep works on fields of ONE precision, so in mixed precision the iterated solution is always a sloppy field that a precise y
//     accumulates at the reliable updates (the reference does that only with use_sloppy_partial_accumulator and otherwise updates the
//     precise x from the sloppy p);
//   * with equal precisions there are no reliable updates at all: nothing is more reliable than the iteration itself, and a residual
//     replacement would only cost an operator application;
//   * use_init_guess is honoured (the reference's CG always starts from whatever x holds);
//   * the stopping rule is the L2 residual; QUDA_HEAVY_QUARK_RESIDUAL only adds the final heavy-quark residual to the report;
//   * multi-shift: the shifted updates run in the same iteration as the base update (the reference defers them into the next stencil
//     application to hide communication) and in one sweep for all active shifts, base system included; beta falls back to
//     r2 / r2_old where (r_new, r_new - r_old) comes out negative, as the single-shift CG does.
#include <cmath>

#include "solver.h"

namespace quda {

static void needL2(const SolverParam &param, const char *name) {
  if (!(param.residual_type & (QUDA_L2_RELATIVE_RESIDUAL | QUDA_L2_ABSOLUTE_RESIDUAL)))
    errorQuda("%s stops on the L2 residual: residual_type %d has no L2 bit (the heavy-quark residual alone is not a stopping criterion here)", name, (int)param.residual_type);
}

// ================================================================================================
// CG
// ================================================================================================
CG::CG(DiracMatrix &mat_, DiracMatrix &matSloppy_, SolverParam &p) : Solver(p), mat(mat_), matSloppy(matSloppy_) {}

void CG::operator()(ColorSpinorField &x, ColorSpinorField &b) {
  needL2(param, "CG");
  const double t0 = wallTime();
  const double b2 = blas::norm2(b);
  if (b2 == 0) {
    warningQuda("inverting on zero-field source");
    blas::copy(x, b);
    param.true_res = 0.0; param.true_res_hq = 0.0;
    return;
  }
  const bool mixed = param.precision_sloppy != x.Precision();
  const bool guess = param.use_init_guess == QUDA_USE_INIT_GUESS_YES;
  ColorSpinorField *rp = like(x, x.Precision(), false);
  ColorSpinorField *yp = mixed ? like(x, x.Precision(), true) : nullptr;
  ColorSpinorField *App = like(x, param.precision_sloppy, false), *pp = like(x, param.precision_sloppy, false);
  ColorSpinorField *rsp = mixed ? like(x, param.precision_sloppy, false) : nullptr;
  ColorSpinorField *xsp = mixed ? like(x, param.precision_sloppy, true) : nullptr;
  ColorSpinorField &r = *rp, &Ap = *App, &p = *pp;
  ColorSpinorField &rSloppy = mixed ? *rsp : r, &xSloppy = mixed ? *xsp : x;

  double r2;
  if (guess) {
    mat(r, x);
    r2 = blas::xmyNorm(b, r);            // r = b - A x
    if (mixed) blas::copy(*yp, x);       // y carries the guess, the sloppy x starts from zero
  } else {
    blas::copy(r, b);
    r2 = b2;
    blas::zero(x);
  }
  if (mixed) blas::copy(rSloppy, r);
  blas::copy(p, rSloppy);

  const double stop = stopping(param.tol, b2, param.residual_type);
  const double delta = mixed ? param.delta : 0.0;   // reliable updates in mixed precision only
  const int maxResIncrease = param.max_res_increase, maxResIncreaseTotal = param.max_res_increase_total;
  int resIncrease = 0, resIncreaseTotal = 0, rUpdate = 0, k = 0;
  double r2_old = r2, alpha = 0, beta = 0;
  double rNorm = sqrt(r2), r0Norm = rNorm, maxrx = rNorm, maxrr = rNorm;
  blas::flops = 0;
  PrintStats("CG", k, r2, b2, 0.0);

  while (r2 > stop && k < param.maxiter) {
    matSloppy(Ap, p);
    r2_old = r2;
    const double pAp = blas::reDotProduct(p, Ap);
    alpha = r2 / pAp;
    const Complex cg_norm = blas::axpyCGNorm(-alpha, Ap, rSloppy);   // r -= alpha A p ; (|r|^2, (r_new, r_new - r_old))
    r2 = cg_norm.real();
    const double sigma = cg_norm.imag() >= 0.0 ? cg_norm.imag() : r2;

    rNorm = sqrt(r2);
    if (rNorm > maxrx) maxrx = rNorm;
    if (rNorm > maxrr) maxrr = rNorm;
    int updateX = (rNorm < delta * r0Norm && r0Norm <= maxrx) ? 1 : 0;
    const int updateR = ((rNorm < delta * maxrr && r0Norm <= maxrr) || updateX) ? 1 : 0;
    // the iterated residual has met the tolerance: confirm it with the precise operator before stopping
    if (mixed && r2 <= stop && param.delta >= param.tol) updateX = 1;

    if (!(updateR || updateX)) {
      beta = sigma / r2_old;
      blas::axpyZpbx(alpha, p, xSloppy, rSloppy, beta);   // x += alpha p ; p = r + beta p
    } else {
      blas::axpy(alpha, p, xSloppy);
      blas::copy(x, xSloppy);
      blas::xpy(x, *yp);
      mat(r, *yp);
      r2 = blas::xmyNorm(b, r);
      blas::copy(rSloppy, r);
      blas::zero(xSloppy);
      if (sqrt(r2) > r0Norm && updateX) {
        resIncrease++;
        resIncreaseTotal++;
        warningQuda("CG: new reliable residual norm %e is greater than previous reliable residual norm %e (total #inc %i)", sqrt(r2), r0Norm, resIncreaseTotal);
        if (resIncrease > maxResIncrease || resIncreaseTotal > maxResIncreaseTotal) {
          warningQuda("CG: solver exiting due to too many true residual norm increases");
          k++;
          break;
        }
      } else {
        resIncrease = 0;
      }
      rNorm = sqrt(r2); maxrr = rNorm; maxrx = rNorm; r0Norm = rNorm;
      rUpdate++;
      // explicitly restore the orthogonality of the gradient vector
      const double rp_ = blas::reDotProduct(rSloppy, p) / r2;
      blas::axpy(-rp_, rSloppy, p);
      beta = r2 / r2_old;
      blas::xpay(rSloppy, beta, p);
    }
    k++;
    PrintStats("CG", k, r2, b2, 0.0);
  }
  if (mixed) { blas::copy(x, xSloppy); blas::xpy(*yp, x); }

  param.secs += wallTime() - t0;
  param.gflops += (blas::flops + mat.flops() + matSloppy.flops()) * 1e-9;
  param.iter += k;
  if (k == param.maxiter) warningQuda("Exceeded maximum iterations %d", param.maxiter);
  if (getVerbosity() >= QUDA_VERBOSE) printfQuda("CG: Reliable updates = %d\n", rUpdate);

  mat(r, x);
  param.true_res = sqrt(blas::xmyNorm(b, r) / b2);
  param.true_res_hq = (param.residual_type & QUDA_HEAVY_QUARK_RESIDUAL) ? sqrt(blas::HeavyQuarkResidualNorm(x, r).z) : 0.0;
  PrintSummary("CG", k, r2, b2);
  blas::flops = 0;
  delete rp; delete yp; delete App; delete pp; delete rsp; delete xsp;
}

// ================================================================================================
// multi-shift CG
// ================================================================================================
MultiShiftCG::MultiShiftCG(DiracMatrix &mat_, DiracMatrix &matSloppy_, SolverParam &p) : param(p), mat(mat_), matSloppy(matSloppy_) {}

// reference lib/inv_multi_cg_quda.cpp:128-155
static void updateAlphaZeta(double *alpha, double *zeta, double *zeta_old, const double *r2, const double *beta, const double pAp, const double *offset,
                            const int nShift, const int j_low) {
  double alpha_old[QUDA_MAX_MULTI_SHIFT];
  for (int j = 0; j < nShift; j++) alpha_old[j] = alpha[j];
  alpha[0] = r2[0] / pAp;
  zeta[0] = 1.0;
  for (int j = 1; j < nShift; j++) {
    const double c0 = zeta[j] * zeta_old[j] * alpha_old[j_low];
    const double c1 = alpha[j_low] * beta[j_low] * (zeta_old[j] - zeta[j]);
    const double c2 = zeta_old[j] * alpha_old[j_low] * (1.0 + (offset[j] - offset[0]) * alpha[j_low]);
    zeta_old[j] = zeta[j];
    zeta[j] = (c1 + c2 != 0.0) ? c0 / (c1 + c2) : 0.0;
    alpha[j] = (zeta[j] != 0.0) ? alpha[j_low] * zeta[j] / zeta_old[j] : 0.0;
  }
}

void MultiShiftCG::operator()(std::vector<ColorSpinorField *> &x, ColorSpinorField &b) {
  needL2(param, "MultiShiftCG");
  const int num_offset = param.num_offset;
  const double *offset = param.offset;
  if (num_offset == 0) return;
  if (num_offset < 0 || num_offset > QUDA_MAX_MULTI_SHIFT || (int)x.size() < num_offset) errorQuda("MultiShiftCG: %d shifts, %zu solution fields", num_offset, x.size());
  const double t0 = wallTime();
  const double b2 = blas::norm2(b);
  if (b2 == 0) {
    warningQuda("inverting on zero-field source");
    for (int i = 0; i < num_offset; i++) { blas::copy(*x[i], b); param.true_res_offset[i] = 0.0; param.iter_res_offset[i] = 0.0; }
    return;
  }
  const QudaPrecision prec = x[0]->Precision();
  const bool mixed = param.precision_sloppy != prec;
  const double prec_tol = pow(10., (-2 * (int)b.Precision() + 1));   // the limit of precision possible

  double zeta[QUDA_MAX_MULTI_SHIFT], zeta_old[QUDA_MAX_MULTI_SHIFT], alpha[QUDA_MAX_MULTI_SHIFT], beta[QUDA_MAX_MULTI_SHIFT];
  const int j_low = 0;
  int num_offset_now = num_offset;
  for (int i = 0; i < num_offset; i++) { zeta[i] = zeta_old[i] = 1.0; beta[i] = 0.0; alpha[i] = 1.0; }

  // reliable updates (of the base system) where a lower sloppy precision calls for them
  bool reliable = false;
  if (mixed) for (int j = 0; j < num_offset; j++) if (param.tol_offset[j] < param.delta) reliable = true;

  ColorSpinorField *rp = like(b, prec, false);
  blas::copy(*rp, b);
  ColorSpinorField *rsp = mixed ? like(b, param.precision_sloppy, false) : nullptr;
  ColorSpinorField &r = *rp, &rSloppy = mixed ? *rsp : r;
  if (mixed) blas::copy(rSloppy, r);
  std::vector<ColorSpinorField *> xs(num_offset), p(num_offset), y;
  if (reliable) { y.resize(num_offset); for (int i = 0; i < num_offset; i++) y[i] = like(b, prec, true); }
  for (int i = 0; i < num_offset; i++) {
    if (mixed) xs[i] = like(b, param.precision_sloppy, true);
    else { xs[i] = x[i]; blas::zero(*xs[i]); }
    p[i] = like(b, param.precision_sloppy, false);
    blas::copy(*p[i], rSloppy);
  }
  ColorSpinorField *App = like(b, param.precision_sloppy, false);
  ColorSpinorField &Ap = *App;

  double stop[QUDA_MAX_MULTI_SHIFT], r2[QUDA_MAX_MULTI_SHIFT];
  for (int i = 0; i < num_offset; i++) { r2[i] = b2; stop[i] = Solver::stopping(param.tol_offset[i], b2, param.residual_type); }
  double r2_old;
  double rNorm = sqrt(r2[0]), r0Norm = rNorm, maxrx = rNorm, maxrr = rNorm;
  const double delta = param.delta;
  const int maxResIncrease = param.max_res_increase, maxResIncreaseTotal = param.max_res_increase_total;
  int resIncrease = 0, resIncreaseTotal = 0, k = 0, rUpdate = 0;
  blas::flops = 0;
  if (getVerbosity() >= QUDA_VERBOSE) printfQuda("MultiShift CG: %d iterations, <r,r> = %e, |r|/|b| = %e\n", k, r2[0], sqrt(r2[0] / b2));

  while (r2[0] > stop[0] && k < param.maxiter) {
    matSloppy(Ap, *p[0]);
    const double pAp = blas::axpyReDot(offset[0], *p[0], Ap);   // A p + offset_0 p ; (p, (A + offset_0) p)
    updateAlphaZeta(alpha, zeta, zeta_old, r2, beta, pAp, offset, num_offset_now, j_low);
    r2_old = r2[0];
    const Complex cg_norm = blas::axpyCGNorm(-alpha[j_low], Ap, rSloppy);
    r2[0] = cg_norm.real();
    const double zn = cg_norm.imag() >= 0.0 ? cg_norm.imag() : r2[0];

    // reliable update conditions: the base system sets them (reference :340-350)
    rNorm = sqrt(r2[0]);
    if (rNorm > maxrx) maxrx = rNorm;
    if (rNorm > maxrr) maxrr = rNorm;
    const int updateX = (rNorm < delta * r0Norm && r0Norm <= maxrx) ? 1 : 0;
    const int updateR = ((rNorm < delta * maxrr && r0Norm <= maxrr) || updateX) ? 1 : 0;

    if (!(updateR || updateX) || !reliable) {
      beta[0] = zn / r2_old;
      for (int j = 1; j < num_offset_now; j++) beta[j] = beta[j_low] * zeta[j] * alpha[j] / (zeta_old[j] * alpha[j_low]);
      // x_j += alpha_j p_j ; p_j = zeta_j r + beta_j p_j for every active shift, the base system (zeta_0 = 1) included: r is read once
      blas::multiShiftUpdate(num_offset_now, xs, p, rSloppy, alpha, beta, zeta);
    } else {
      for (int j = 0; j < num_offset_now; j++) {
        blas::axpy(alpha[j], *p[j], *xs[j]);
        blas::copy(*x[j], *xs[j]);
        blas::xpy(*x[j], *y[j]);
      }
      mat(r, *y[0]);
      blas::axpy(offset[0], *y[0], r);
      r2[0] = blas::xmyNorm(b, r);
      for (int j = 1; j < num_offset_now; j++) r2[j] = zeta[j] * zeta[j] * r2[0];
      for (int j = 0; j < num_offset_now; j++) blas::zero(*xs[j]);
      blas::copy(rSloppy, r);
      if (sqrt(r2[0]) > r0Norm) {
        resIncrease++;
        resIncreaseTotal++;
        warningQuda("MultiShiftCG: updated residual %e is greater than previous residual %e (total #inc %i)", sqrt(r2[0]), r0Norm, resIncreaseTotal);
        if (resIncrease > maxResIncrease || resIncreaseTotal > maxResIncreaseTotal) {
          warningQuda("MultiShiftCG: solver exiting due to too many true residual norm increases");
          k++;
          break;
        }
      } else {
        resIncrease = 0;
      }
      // explicitly restore the orthogonality of the gradient vectors, then the new directions
      for (int j = 0; j < num_offset_now; j++) {
        const double rp_ = blas::reDotProduct(rSloppy, *p[j]) / r2[0];
        blas::axpy(-rp_, rSloppy, *p[j]);
      }
      beta[0] = r2[0] / r2_old;
      blas::xpay(rSloppy, beta[0], *p[0]);
      for (int j = 1; j < num_offset_now; j++) {
        beta[j] = beta[j_low] * zeta[j] * alpha[j] / (zeta_old[j] * alpha[j_low]);
        blas::axpby(zeta[j], rSloppy, beta[j], *p[j]);
      }
      rNorm = sqrt(r2[0]); maxrr = rNorm; maxrx = rNorm; r0Norm = rNorm;
      rUpdate++;
    }

    // shifts that have converged leave the iteration (they are the last ones: the offsets ascend)
    int converged = 0;
    for (int j = 1; j < num_offset_now; j++) {
      if (zeta[j] == 0.0) {
        converged++;
      } else {
        r2[j] = zeta[j] * zeta[j] * r2[0];
        if (r2[j] < stop[j] || sqrt(r2[j] / b2) < prec_tol) converged++;
      }
    }
    num_offset_now -= converged;
    k++;
    if (getVerbosity() >= QUDA_VERBOSE) printfQuda("MultiShift CG: %d iterations, <r,r> = %e, |r|/|b| = %e, %d shifts active\n", k, r2[0], sqrt(r2[0] / b2), num_offset_now);
  }

  for (int i = 0; i < num_offset; i++) {
    if (mixed) blas::copy(*x[i], *xs[i]);
    if (reliable) blas::xpy(*y[i], *x[i]);
  }
  param.secs += wallTime() - t0;
  param.gflops += (blas::flops + mat.flops() + matSloppy.flops()) * 1e-9;
  param.iter += k;
  if (k == param.maxiter) warningQuda("Exceeded maximum iterations %d", param.maxiter);
  if (getVerbosity() >= QUDA_VERBOSE) printfQuda("MultiShift CG: Reliable updates = %d\n", rUpdate);

  for (int i = 0; i < num_offset; i++) {
    mat(r, *x[i]);
    blas::axpy(offset[i], *x[i], r);
    param.true_res_offset[i] = sqrt(blas::xmyNorm(b, r) / b2);
    param.iter_res_offset[i] = sqrt(r2[i] / b2);
  }
  if (getVerbosity() >= QUDA_SUMMARIZE) {
    printfQuda("MultiShift CG: Converged after %d iterations\n", k);
    for (int i = 0; i < num_offset; i++) printfQuda(" shift=%d, relative residual: iterated = %e, true = %e\n", i, param.iter_res_offset[i], param.true_res_offset[i]);
  }
  blas::flops = 0;
  delete rp; delete rsp; delete App;
  for (int i = 0; i < num_offset; i++) { delete p[i]; if (mixed) delete xs[i]; if (reliable) delete y[i]; }
}

}  // namespace quda
