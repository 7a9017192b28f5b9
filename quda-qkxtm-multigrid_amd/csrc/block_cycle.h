// block_cycle.h — the layers of the multigrid cycle for several sources at once (invertMultiSrcQuda), internal to the library:
//   block_coarse_cycle.cpp    BlockCoarseCycle: everything below the fine level on block fields
//   block_fine_smoother.cpp   BlockFineSmoother: MR on the fine level for groups of 8 or 4 sources
//   block_mg_cycle.cpp        MGBlockState and the MG::block* members: the cycle that joins the two
//   block_solver.cpp          the lockstep GCR around that cycle, the entry point and the statistics
#pragma once

#include <vector>

#include "block.h"
#include "multigrid.h"

namespace quda {

// ================================================================================================
// the cycle below the fine level on block fields
// ================================================================================================
struct BlockLevel {
  const CoarseGauge *Y = nullptr, *H = nullptr;   // links (slot 8 = X) and preconditioned links Xinv Y (slot 8 = Xinv)
  const Transfer *T = nullptr;                    // to the next coarser level (nullptr on the coarsest)
  int p = 0;                                      // parity of the even-odd preconditioned system
  int nuPre = 0, nuPost = 0;
  double omega = 1.0;
  BlockField *b = nullptr, *x = nullptr, *bt = nullptr, *r = nullptr, *Ar = nullptr, *t = nullptr, *w1 = nullptr, *w2 = nullptr;
  std::vector<ColorSpinorField *> fine, coarse;   // per right-hand side staging fields of the transfer to the next level
  // K-cycle (QUDA_MG_CYCLE_RECURSIVE on the level above): this level's system is solved by a flexible GCR around its own cycle (reference
  // lib/multigrid.cpp:230-260: coarse solver = GCR(10), at most 11 iterations, to the smoother tolerance of this level) — source kb, work fields
  bool kSolve = false;
  int kKrylov = 10, kMaxiter = 11;
  double kTol = 0.25;
  BlockField *kb = nullptr, *ky = nullptr, *kr = nullptr;
  std::vector<BlockField *> KP, KAP;
};

class BlockCoarseCycle {
 public:
  int nl = 0, nb = 0;   // levels, right-hand sides of the block (a multiple of 8)
  int nReal = 0;        // columns that carry a source (the rest pad the block: their staging fields are zero from their creation and stay so)
  std::vector<BlockLevel> L;
  // coarsest-grid GCR
  int nKrylov = 20, maxiter = 1000;
  double tol = 0.25;
  std::vector<BlockField *> P, AP;
  BlockField *y = nullptr;
  std::vector<MG *> parents;   // MG object of every level of the sub-hierarchy (creation only)
  long applies = 0, gcrIters = 0, kIters = 0;

  ~BlockCoarseCycle();
  static void zeroParity(BlockField &f, int par);
  // out_p = in_p - Yhat_pq Yhat_qp in_p   (in: other parity zero; out: other parity zero)   reference DiracCoarsePC::M, lib/dirac_coarse.cpp:332-350
  void matpc(BlockLevel &l, BlockField &out, BlockField &in);
  // Schur prepare (reference DiracCoarsePC::prepare, :296-330): bt_p = Xinv (b_p - D_pq Xinv b_q)
  void prepare(BlockLevel &l);
  // x_q = Xinv (b_q - D_qp x_p)   (reference DiracCoarsePC::reconstruct, :352-372); x_q is overwritten
  void reconstruct(BlockLevel &l);
  // the solve of level lev as the level above wants it: its cycle, or (K-cycle above) the GCR around it; source in source(lev), solution in L[lev].x
  BlockField &source(int lev) { return L[lev].kSolve ? *L[lev].kb : *L[lev].b; }
  void solve(int lev) { if (L[lev].kSolve) kgcr(lev); else cycle(lev); }

 private:
  static void copyParity(BlockField &dst, const BlockField &src, int par);
  void apply(BlockField &out, BlockField &in, const CoarseGauge &G, int parity = -1) { applyCoarseBlock(out, in, G, parity); applies++; }
  void mr(BlockLevel &l, int nu, bool guess);
  template <typename Op, typename Prec>
  int gcrLockstep(BlockField &b, BlockField &yv, BlockField &r, std::vector<BlockField *> &Pv, std::vector<BlockField *> &APv, int nK, int maxit, double tl, Op op, Prec prec);
  void gcr(BlockLevel &l);
  void kgcr(int lev);
  void cycle(int lev);
};

// nullptr: the sub-hierarchy below `top` does not qualify (a K-cycle below the first coarse level is fine; an operator the MFMA kernel does not take is not)
BlockCoarseCycle *blockCoarseCreate(MG &top, int nb, const MGParam *parent);

// ================================================================================================
// the smoother of the fine level for all sources: MR on the even-odd preconditioned operator, on block fields
// ================================================================================================
struct FineGroup {
  int first = 0, n = 0, nrhs = 0;   // sources [first, first + n) are the first n columns of blocks with nrhs columns
  BlockField *B = nullptr, *X = nullptr, *R = nullptr, *AR = nullptr, *T = nullptr, *W2 = nullptr;
  double *d_sums = nullptr, *d_sums7 = nullptr;
};

class BlockFineSmoother {
 public:
  const GaugeField *U = nullptr;
  double kappa = 0, a = 0, binv = 1, omega = 1, mu = 0;
  QudaDiracType type = QUDA_INVALID_DIRAC;
  QudaMatPCType matpcType = QUDA_MATPC_INVALID;
  int par = 0;                         // parity of the preconditioned system
  int nuPre = 0, nuPost = 0;
  bool globalSums = false;             // the MR sums cross ranks
  bool twoStep = true;                 // QUDA_AMD_MULTISRC_MR_PAIRS=0: one update per step
  float *tmat[2] = {nullptr, nullptr};   // twisted clover: dense (A + i a g5)^-1 per parity
  size_t tmatBytes = 0;
  std::vector<FineGroup> groups;

  ~BlockFineSmoother();
  // out = in - kappa^2 A^-1 D_pq A^-1 D_qp in     (reference DiracTwistedMassPC::M / DiracTwistedCloverPC::M, symmetric preconditioning)
  // dots: 0 none; 3: (out, in), |out|^2 -> g.d_sums; 2: the seven sums with a = `dotA` -> g.d_sums7 (rank-local device sums; sums across ranks go the mode-3 way only)
  void matpc(FineGroup &g, BlockField &out, BlockField &in, int dots, const GaugeField *links = nullptr, const BlockField *dotA = nullptr);
  // nu MR steps on (X, R); fresh: X is not defined yet and the residual is `first` (the source itself), not R
  void mr(FineGroup &g, int nu, BlockField *first, bool needResidual);
  // R = B - M X
  void residual(FineGroup &g);
};

// nullptr: this fine level keeps the per-source smoother (asymmetric preconditioning, a smoother other than MR, 16-bit smoothing, links the
// multi-right-hand-side stencil does not read, QUDA_AMD_MULTISRC_BLOCK_SMOOTHER=0)
BlockFineSmoother *blockFineCreate(const Dirac &dirac, const SolverParam &pre, const SolverParam &post, int flavor, int nsrc);

// ================================================================================================
// the multigrid cycle for several sources at once (level 0: per source; below: block fields)
// ================================================================================================
struct MGBlockState {
  int nsrc = 0, nb = 0;
  std::vector<Solver *> pre, post;
  std::vector<SolverParam *> prePar, postPar;
  std::vector<ColorSpinorField *> r, rc, xc, btilde;
  BlockCoarseCycle *coarse = nullptr;
  BlockFineSmoother *fine = nullptr;   // nullptr: the per-source smoothers above
  bool solutionOnBlocks = false;       // the last cycle left its solutions in fine->groups[].X (blockApplyLast)
  bool wantImage = false;              // the caller will ask for A x of the cycle's solutions: the post-smoother keeps its last residual
  bool residualOnBlocks = false;       // ... and did: fine->groups[].R = b - A x
  ~MGBlockState();
};

// the counters behind qudaAmdMultiSrcStats (quda_amd_ext.h), owned by block_solver.cpp
enum MultiSrcStat { MS_CYCLES = 0, MS_BLOCK_SMOOTHED = 1, MS_QUAD_TRANSFERS = 2, MS_SOLVES = 3 };
void multiSrcCount(MultiSrcStat which);

}  // namespace quda
