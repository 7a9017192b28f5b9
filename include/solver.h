// solver.h — Krylov layer of the MG-GCR path: GCR (outer solver, K-cycle coarse solver), MR (smoother),
// BiCGstab (null-vector setup).  Interface mirrors the reference (include/invert_quda.h:15-331: SolverParam,
// Solver::create, operator()(x, b)); algorithms restated from lib/inv_gcr_quda.cpp:53-516,
// lib/inv_mr_quda.cpp:40-200, lib/inv_bicgstab_quda.cpp:40-354, lib/solver.cpp:13-150.  CG and multi-shift CG on Hermitian positive
// definite operators (M^dag M): lib/inv_cg_quda.cpp:40-360, lib/inv_multi_cg_quda.cpp:115-527.
#pragma once

#include <memory>
#include <vector>

#include "blas.h"
#include "dirac.h"

namespace quda {

struct GcrCoeffs;   // csrc/gcr_core.h: alpha, beta, gamma of one Krylov cycle and their back substitution

double wallTime();   // seconds (gettimeofday)
// a device field of the shape and twist flavour of x in precision prec, cleared or left as allocated
ColorSpinorField *like(const ColorSpinorField &x, QudaPrecision prec, bool zero);

struct SolverParam {
  QudaInverterType inv_type = QUDA_GCR_INVERTER;
  QudaInverterType inv_type_precondition = QUDA_INVALID_INVERTER;
  void *preconditioner = nullptr;  // multigrid_solver* when inv_type_precondition == QUDA_MG_INVERTER
  QudaResidualType residual_type = QUDA_L2_RELATIVE_RESIDUAL;
  QudaUseInitGuess use_init_guess = QUDA_USE_INIT_GUESS_NO;
  QudaComputeNullVector compute_null_vector = QUDA_COMPUTE_NULL_VECTOR_NO;
  double delta = 1e-4;  // reliable-update threshold
  bool use_sloppy_partial_accumulator = false;
  int max_res_increase = 1, max_res_increase_total = 10, heavy_quark_check = 10, pipeline = 0;
  double tol = 1e-10, tol_restart = 5e-3, tol_hq = 0;
  double true_res = 0, true_res_hq = 0;
  int maxiter = 1000, iter = 0;
  QudaPrecision precision = QUDA_DOUBLE_PRECISION, precision_sloppy = QUDA_DOUBLE_PRECISION, precision_precondition = QUDA_DOUBLE_PRECISION;
  QudaPreserveSource preserve_source = QUDA_PRESERVE_SOURCE_YES;
  int Nkrylov = 20;
  int precondition_cycle = 1;
  double tol_precondition = 1e-1;
  int maxiter_precondition = 10;
  double omega = 1.0;
  QudaSchwarzType schwarz_type = QUDA_ADDITIVE_SCHWARZ;
  double secs = 0, gflops = 0;
  QudaVerbosity verbosity_precondition = QUDA_SILENT;
  bool is_preconditioner = false;
  bool global_reduction = true;
  bool compute_true_res = true;
  // multi-shift solves (reference include/invert_quda.h:108-130)
  int num_offset = 0;
  double offset[QUDA_MAX_MULTI_SHIFT] = {}, tol_offset[QUDA_MAX_MULTI_SHIFT] = {}, true_res_offset[QUDA_MAX_MULTI_SHIFT] = {},
         iter_res_offset[QUDA_MAX_MULTI_SHIFT] = {};
  SolverParam() {}
  explicit SolverParam(const QudaInvertParam &p);   // reference include/invert_quda.h:197-255
  void updateInvertParam(QudaInvertParam &p) const; // reference :262-300
  void updateMultiShiftParam(QudaInvertParam &p) const;   // true_res_offset[], iter_res_offset[] of a multi-shift solve (reference :278-290)
};

class Solver {
 protected:
  SolverParam &param;
 public:
  explicit Solver(SolverParam &p) : param(p) {}
  virtual ~Solver() {}
  virtual void operator()(ColorSpinorField &out, ColorSpinorField &in) = 0;
  virtual unsigned long long flops() const { return 0; }
  // b - A x of the system the last call worked on, in the solver's work precision, if the solver keeps it (MR); else nullptr
  virtual const ColorSpinorField *lastResidual() const { return nullptr; }
  // used as a preconditioner x = K b: A x for the x of the LAST call, if the solver can give it without applying A (a multigrid cycle that ends in
  // an MR smoother on A's own even-odd system holds b - A x: multigrid.cpp); false: not available, the caller applies A
  virtual bool imageOfLast(ColorSpinorField &, const ColorSpinorField &, const DiracMatrix &) { return false; }
  static Solver *create(SolverParam &param, DiracMatrix &mat, DiracMatrix &matSloppy, DiracMatrix &matPrecon);  // reference lib/solver.cpp:13
  static double stopping(double tol, double b2, QudaResidualType type);
  bool convergence(double r2, double hq2, double r2_tol, double hq_tol) const;
  void PrintStats(const char *name, int k, double r2, double b2, double hq2) const;
  void PrintSummary(const char *name, int k, double r2, double b2) const;
};

class MR : public Solver {
  const DiracMatrix &mat, &matSloppy;
  ColorSpinorField *rp, *Arp, *tmpp, *yp;
  bool residualValid;
 public:
  MR(DiracMatrix &mat, DiracMatrix &matSloppy, SolverParam &param);
  ~MR() override;
  void operator()(ColorSpinorField &out, ColorSpinorField &in) override;
  const ColorSpinorField *lastResidual() const override { return residualValid ? rp : nullptr; }
};

class BiCGstab : public Solver {
  DiracMatrix &mat, &matSloppy, &matPrecon;
  ColorSpinorField *yp, *rp, *pp, *vp, *tp, *r0p, *xsp, *rsp;
 public:
  BiCGstab(DiracMatrix &mat, DiracMatrix &matSloppy, DiracMatrix &matPrecon, SolverParam &param);
  ~BiCGstab() override;
  void operator()(ColorSpinorField &out, ColorSpinorField &in) override;
};

class GCR : public Solver {
  const DiracMatrix &mat, &matSloppy, &matPrecon;
  Solver *K;
  bool ownK;
  SolverParam Kparam;
  int nKrylov;
  std::unique_ptr<GcrCoeffs> coeffs;
  bool init;
  ColorSpinorField *rp, *yp, *x_sloppy, *r_sloppy, *p_pre, *r_pre, *rM;
  std::vector<ColorSpinorField *> p, Ap;
 public:
  GCR(DiracMatrix &mat, DiracMatrix &matSloppy, DiracMatrix &matPrecon, SolverParam &param);
  GCR(DiracMatrix &mat, Solver &K, DiracMatrix &matSloppy, DiracMatrix &matPrecon, SolverParam &param);
  ~GCR() override;
  void operator()(ColorSpinorField &out, ColorSpinorField &in) override;
};

// CG on a Hermitian positive definite operator (mat = matSloppy in another precision).  Equal precisions: the textbook recurrence in that
// precision.  Lower sloppy precision: x, r, p, Ap of the iteration are sloppy fields, a precise y accumulates x and the true residual
// replaces the iterated one whenever the latter has dropped by param.delta since the last such reliable update.
class CG : public Solver {
  const DiracMatrix &mat, &matSloppy;
 public:
  CG(DiracMatrix &mat, DiracMatrix &matSloppy, SolverParam &param);
  void operator()(ColorSpinorField &out, ColorSpinorField &in) override;
};

// (A + offset_i) x_i = b for param.num_offset ascending offsets with the Krylov space of the smallest one; fills param.true_res_offset[],
// param.iter_res_offset[] (precise operator / recurrence).  Not a Solver: it has as many solutions as shifts (reference MultiShiftSolver).
class MultiShiftCG {
  SolverParam &param;
  const DiracMatrix &mat, &matSloppy;
 public:
  MultiShiftCG(DiracMatrix &mat, DiracMatrix &matSloppy, SolverParam &param);
  void operator()(std::vector<ColorSpinorField *> &x, ColorSpinorField &b);
};

void fillInnerSolveParam(SolverParam &inner, const SolverParam &outer);  // reference lib/inv_gcr_quda.cpp:17-50

// One Krylov step of GCR on fields, shared by GCR::operator() and the lockstep multi-source GCR (block_solver.cpp): Ap[k] is orthogonalised
// against Ap[0 .. k) and normalised, r -= alpha_k Ap[k]; column k of beta, gamma[k] and alpha[k] go into c; returns |r|^2.  The blocked two-sweep
// form runs where blas::multiSupported allows it and the inferred norm keeps two digits, else the one-direction-at-a-time chain in the form
// `chain` (the two forms reduce in different kernels, so a caller's results depend on its choice in the last bits).  blockedOk: the
// measured-norm guard — read before the blocked form is tried, cleared (with Ap[k], gamma, alpha put right) when the measured |Ap_k|^2 is
// off; the caller sets it again at its restart.  nullptr: no guard, the blocked form is always tried.
enum class GcrChain { Pipelined, Sequential };   // caxpyDotzy pipeline (reference :103-121) / cDotProduct + caxpy (reference :86-101)
double gcrKrylovStep(GcrCoeffs &c, std::vector<ColorSpinorField *> &Ap, int k, ColorSpinorField &r, GcrChain chain, bool *blockedOk);
// x += sum_{a < k} delta_a p_a with delta from c.backSubstitute (reference :125-157)
void gcrUpdateSolution(ColorSpinorField &x, const GcrCoeffs &c, int k, std::vector<ColorSpinorField *> &p);

}  // namespace quda
