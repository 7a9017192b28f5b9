// block_fine_smoother.cpp — the smoother of the fine level for all sources: MR on the even-odd preconditioned operator, on block fields.
//
// The per-source smoother streams the gauge links once per source and step (384 - 576 B per site against 192 B of spinor), and every step is a
// chain of five launches per source.  Here groups of 8 (or 4) sources share one pass over the links (fine_block_kernel: dslash.h
// applyFineBlockParity), the two sums of the MR step come out of the second launch's epilogue where `A r` and `r` already sit in registers
// (mode 3), and the coefficient never leaves the device (fineBlockDotsFinishDev -> blockblas::mrUpdateDev) — the same arithmetic as MR of
// solver.cpp with device-side scalars (fp32 fields, fp64 sums, rank-local), reference lib/inv_mr_quda.cpp:40-200.
#include "block_cycle.h"
#include "env.h"

namespace quda {

BlockFineSmoother::~BlockFineSmoother() {
  for (FineGroup &g : groups) {
    for (BlockField *f : {g.B, g.X, g.R, g.AR, g.T, g.W2}) delete f;
    if (g.d_sums) poolDeviceFree(g.d_sums, 0);
    if (g.d_sums7) poolDeviceFree(g.d_sums7, 0);
  }
  for (int p = 0; p < 2; p++) if (tmat[p]) poolDeviceFree(tmat[p], tmatBytes);
}

static float2 *ghostOf(BlockField &f) { return f.nGhost ? f.v + f.elems() : nullptr; }

void BlockFineSmoother::matpc(FineGroup &g, BlockField &out, BlockField &in, int dots, const GaugeField *links, const BlockField *dotA) {
  const FineBlockDots d = {dots == 2 ? dotA->v : nullptr, dots == 2 ? 2 : 3};
  const int p = par, q = 1 - par;
  const GaugeField &W = links ? *links : *U;
  if (tmat[0]) {
    applyFineBlockParity(g.T->v, nullptr, in.v, in.nrhs, W, q, 0.0, 0.0, 1.0, 0.0, tmat[q], 1, ghostOf(in));
    applyFineBlockParity(out.v, in.v, g.T->v, in.nrhs, W, p, 1.0, 0.0, -kappa * kappa, 0.0, tmat[p], 1, ghostOf(*g.T), dots ? &d : nullptr);
  } else {
    applyFineBlockParity(g.T->v, nullptr, in.v, in.nrhs, W, q, 0.0, 0.0, binv, -a, nullptr, 0, ghostOf(in));
    applyFineBlockParity(out.v, in.v, g.T->v, in.nrhs, W, p, 1.0, 0.0, -kappa * kappa * binv, -a, nullptr, 0, ghostOf(*g.T), dots ? &d : nullptr);
  }
  if (!dots) return;
  if (dots == 2) { fineBlockDotsFinishDev(g.d_sums7, in.nrhs, 2); return; }
  if (!globalSums) { fineBlockDotsFinishDev(g.d_sums, in.nrhs, 3); return; }
  // sums over all ranks (smoother with global_reduction on a grid-decomposed lattice): through the host, one round trip per step and group
  double sums[3 * 8];
  fineBlockDotsFinish(sums, in.nrhs, 3);
  HIP_CHECK(hipMemcpyAsync(g.d_sums, sums, 3 * in.nrhs * sizeof(double), hipMemcpyHostToDevice, computeStream()));
  HIP_CHECK(hipStreamSynchronize(computeStream()));
}

void BlockFineSmoother::mr(FineGroup &g, int nu, BlockField *first, bool needResidual) {
  int k = 0;
  // pairs of steps as one update (blockblas::mr2UpdateDev: w1 = A r, w2 = A w1, both coefficients from the epilogue sums) while two or more are left
  while (twoStep && !globalSums && k + 1 < nu) {
    BlockField &rin = (k == 0 && first) ? *first : *g.R;
    matpc(g, *g.AR, rin, 3);
    matpc(g, *g.W2, *g.AR, 2, nullptr, &rin);
    blockblas::mr2UpdateDev(*g.X, *g.R, rin, *g.AR, *g.W2, g.d_sums, g.d_sums7, omega, k == 0 && first, needResidual || k + 2 < nu);
    k += 2;
  }
  for (; k < nu; k++) {
    BlockField &rin = (k == 0 && first) ? *first : *g.R;
    matpc(g, *g.AR, rin, 3);
    blockblas::mrUpdateDev(*g.X, *g.R, rin, *g.AR, g.d_sums, omega, k == 0 && first, needResidual || k + 1 < nu);
  }
}

void BlockFineSmoother::residual(FineGroup &g) {
  matpc(g, *g.AR, *g.X, 0);
  std::vector<Complex> zero(g.nrhs, Complex(0.0, 0.0)), mone(g.nrhs, Complex(-1.0, 0.0));
  blockblas::cxpaypbz(*g.B, zero.data(), *g.B, mone.data(), *g.AR);   // AR = B - AR
  std::swap(g.R, g.AR);
}

BlockFineSmoother *blockFineCreate(const Dirac &dirac, const SolverParam &pre, const SolverParam &post, int flavor, int nsrc) {
  static const bool on = envInt("QUDA_AMD_MULTISRC_BLOCK_SMOOTHER", 1) != 0;   // read once
  if (!on) return nullptr;
  const QudaDiracType ty = dirac.getDiracType();
  if (ty != QUDA_TWISTED_MASSPC_DIRAC && ty != QUDA_WILSONPC_DIRAC && ty != QUDA_TWISTED_CLOVERPC_DIRAC) return nullptr;
  const QudaMatPCType mt = dirac.getMatPCType();
  if (mt != QUDA_MATPC_EVEN_EVEN && mt != QUDA_MATPC_ODD_ODD) return nullptr;
  if (pre.inv_type != QUDA_MR_INVERTER || post.inv_type != QUDA_MR_INVERTER) return nullptr;
  if (pre.precision_sloppy != QUDA_SINGLE_PRECISION || post.precision_sloppy != QUDA_SINGLE_PRECISION) return nullptr;
  const GaugeField *U = dirac.Gauge();
  if (!U || !fineBlockSupported(*U, 8) || !fineBlockSupported(*U, 4) || !fineBlockDotsSupported(8) || !fineBlockDotsSupported(4)) return nullptr;
  const bool tmc = ty == QUDA_TWISTED_CLOVERPC_DIRAC;
  if (tmc && !(dirac.Clover() && dirac.Clover()->precision == QUDA_SINGLE_PRECISION)) return nullptr;
  BlockFineSmoother *f = new BlockFineSmoother;
  f->U = U;
  f->kappa = dirac.Kappa(); f->mu = dirac.Mu(); f->type = ty; f->matpcType = mt;
  f->a = ty == QUDA_WILSONPC_DIRAC ? 0.0 : 2.0 * dirac.Kappa() * (double)flavor * dirac.Mu();
  f->binv = 1.0 / (1.0 + f->a * f->a);
  f->omega = pre.omega;
  f->par = mt == QUDA_MATPC_ODD_ODD ? 1 : 0;
  f->nuPre = pre.maxiter; f->nuPost = post.maxiter;
  f->globalSums = pre.global_reduction && commReductionsNeeded();
  f->twoStep = envInt("QUDA_AMD_MULTISRC_MR_PAIRS", 1) != 0;   // read at every creation
  const int Vh = U->geom.Vh;
  if (tmc) {
    f->tmatBytes = (size_t)Vh * 144 * sizeof(float);
    for (int p = 0; p < 2; p++) {
      f->tmat[p] = (float *)poolDeviceMalloc(f->tmatBytes);
      cloverTwistDense(f->tmat[p], *dirac.Clover(), p, f->a, true);
    }
  }
  const int nGhost = blockGhost(U->geom.X, true).nGhost;
  for (int first = 0; first < nsrc;) {
    FineGroup g;
    const int left = nsrc - first;
    g.first = first; g.n = left >= 8 ? 8 : left; g.nrhs = g.n > 4 ? 8 : 4;
    g.B = new BlockField(Vh, 12, g.nrhs, nGhost); g.X = new BlockField(Vh, 12, g.nrhs, nGhost); g.R = new BlockField(Vh, 12, g.nrhs, nGhost);
    g.AR = new BlockField(Vh, 12, g.nrhs, nGhost); g.T = new BlockField(Vh, 12, g.nrhs, nGhost); g.W2 = new BlockField(Vh, 12, g.nrhs, nGhost);
    g.d_sums = (double *)poolDeviceMalloc(3 * 8 * sizeof(double));
    g.d_sums7 = (double *)poolDeviceMalloc(7 * 8 * sizeof(double));
    f->groups.push_back(g);
    first += g.n;
  }
  return f;
}

}  // namespace quda
