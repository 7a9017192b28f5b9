// block_coarse_cycle.cpp — the multigrid cycle below the fine level for several right-hand sides on BLOCK FIELDS (block.h: site-major, right-hand
// side fastest): the coarse operators read their dense link matrices once for all sources and run on the matrix cores (coarse_block_kernel,
// v_mfma_f32_16x16x4_f32).
// The even-odd preconditioned coarse operator on block fields needs no kernel of its own: the full block operator applied to a field whose
// other parity is zero IS the parity-restricted hop (sites of one parity only have neighbours of the other), at 2.25 x the necessary flops —
// which the matrix cores have to spare — and the local terms Xinv come out of the same application (slot 8 of the preconditioned links).
#include <cmath>

#include "block_cycle.h"
#include "gcr_core.h"

namespace quda {

BlockCoarseCycle::~BlockCoarseCycle() {
  for (BlockLevel &l : L) {
    for (BlockField *f : {l.b, l.x, l.bt, l.r, l.Ar, l.t, l.w1, l.w2, l.kb, l.ky, l.kr}) delete f;
    for (BlockField *f : l.KP) delete f;
    for (BlockField *f : l.KAP) delete f;
    for (ColorSpinorField *f : l.fine) delete f;
    for (ColorSpinorField *f : l.coarse) delete f;
  }
  for (BlockField *f : P) delete f;
  for (BlockField *f : AP) delete f;
  delete y;
}

void BlockCoarseCycle::zeroParity(BlockField &f, int par) {
  const size_t half = (size_t)f.Vh * f.ncomp * f.nrhs;
  HIP_CHECK(hipMemsetAsync(f.v + (size_t)par * half, 0, half * sizeof(float2), computeStream()));
}
void BlockCoarseCycle::copyParity(BlockField &dst, const BlockField &src, int par) {
  const size_t half = (size_t)src.Vh * src.ncomp * src.nrhs;
  HIP_CHECK(hipMemcpyAsync(dst.v + (size_t)par * half, src.v + (size_t)par * half, half * sizeof(float2), hipMemcpyDeviceToDevice, computeStream()));
}

// (the two hops are computed on the output parity only: l.t is written on parity q alone; its other half, which the second application multiplies
// with Xinv, is cleared here and not trusted to have stayed zero since its creation)
void BlockCoarseCycle::matpc(BlockLevel &l, BlockField &out, BlockField &in) {
  zeroParity(*l.t, l.p);
  apply(*l.t, in, *l.H, 1 - l.p);
  apply(out, *l.t, *l.H, l.p);
  zeroParity(out, 1 - l.p);
  blockblas::xmy(in, out);
}
void BlockCoarseCycle::prepare(BlockLevel &l) {
  const int p = l.p, q = 1 - p;
  blockblas::copy(*l.w1, *l.b);
  zeroParity(*l.w1, p);
  apply(*l.w2, *l.w1, *l.H, q);       // parity q: Xinv b_q
  zeroParity(*l.w2, p);
  apply(*l.w1, *l.w2, *l.Y, p);       // parity p: D_pq (Xinv b_q)
  blockblas::xmy(*l.b, *l.w1);        // b - ...
  zeroParity(*l.w1, q);
  apply(*l.bt, *l.w1, *l.H, p);       // parity p: Xinv ( . )
  zeroParity(*l.bt, q);
}
void BlockCoarseCycle::reconstruct(BlockLevel &l) {
  const int p = l.p, q = 1 - p;
  zeroParity(*l.x, q);
  apply(*l.w1, *l.x, *l.Y, q);        // parity q: D_qp x_p
  blockblas::xmy(*l.b, *l.w1);
  zeroParity(*l.w1, p);
  apply(*l.w2, *l.w1, *l.H, q);       // parity q: Xinv ( . )
  copyParity(*l.x, *l.w2, q);
}
// MR on the preconditioned system, per right-hand side alpha (reference lib/inv_mr_quda.cpp:40-200)
void BlockCoarseCycle::mr(BlockLevel &l, int nu, bool guess) {
  std::vector<Complex> dot(nb), al(nb), mal(nb);
  std::vector<double> nrm(nb);
  if (guess) {
    blockblas::copy(*l.w1, *l.x);
    zeroParity(*l.w1, 1 - l.p);
    matpc(l, *l.r, *l.w1);
    blockblas::xmy(*l.bt, *l.r);        // r = bt - Mhat x_p
  } else {
    zeroParity(*l.x, l.p);
    blockblas::copy(*l.r, *l.bt);
  }
  for (int it = 0; it < nu; it++) {
    matpc(l, *l.Ar, *l.r);
    blockblas::cDotNormA(dot.data(), nrm.data(), *l.Ar, *l.r);
    for (int i = 0; i < nb; i++) { al[i] = nrm[i] > 0.0 ? l.omega * dot[i] / nrm[i] : Complex(0.0); mal[i] = -al[i]; }
    blockblas::caxpy(al.data(), *l.r, *l.x);     // x_p += alpha r   (r is zero on the other parity)
    blockblas::caxpy(mal.data(), *l.Ar, *l.r);   // r -= alpha Ar
  }
}
// restarted flexible GCR(nK) per right-hand side in lockstep (reference lib/inv_gcr_quda.cpp:235-516): y = A^-1 b to |r| <= tol |b|, p_k = K r
// (prec == nullptr: p_k = r).  r is work space; op / prec are (out, in)
template <typename Op, typename Prec>
int BlockCoarseCycle::gcrLockstep(BlockField &b, BlockField &yv, BlockField &r, std::vector<BlockField *> &Pv, std::vector<BlockField *> &APv, int nK, int maxit, double tl, Op op, Prec prec) {
  std::vector<double> b2(nb), r2(nb), stop(nb), nrm(nb);
  std::vector<Complex> dot(nb), c(nb);
  blockblas::norm2(b2.data(), b);
  blockblas::copy(r, b);
  blockblas::zero(yv);
  bool any = false;
  for (int i = 0; i < nb; i++) { stop[i] = tl * tl * b2[i]; r2[i] = b2[i]; any = any || b2[i] > 0.0; }
  std::vector<GcrCoeffs> co(nb, GcrCoeffs(nK));   // per right-hand side
  auto open = [&]() { for (int i = 0; i < nb; i++) if (r2[i] > stop[i]) return true; return false; };
  int k = 0, total = 0;
  while (any && open() && total < maxit) {
    prec(*Pv[k], r);
    op(*APv[k], *Pv[k]);
    for (int j = 0; j < k; j++) {
      blockblas::cDot(dot.data(), *APv[j], *APv[k]);
      for (int i = 0; i < nb; i++) { co[i].b(j, k) = dot[i]; c[i] = -dot[i]; }
      blockblas::caxpy(c.data(), *APv[j], *APv[k]);
    }
    blockblas::cDotNormA(dot.data(), nrm.data(), *APv[k], r);
    for (int i = 0; i < nb; i++) {
      const double g = co[i].gamma[k] = sqrt(nrm[i]);   // 0 on a padding column: its coefficients stay zero (GcrCoeffs::backSubstitute)
      co[i].alpha[k] = g > 0.0 ? dot[i] / g : Complex(0.0);
      c[i] = g > 0.0 ? Complex(1.0 / g - 1.0) : Complex(0.0);   // AP_k *= 1 / gamma  (y += c x with x = y)
    }
    blockblas::caxpy(c.data(), *APv[k], *APv[k]);
    for (int i = 0; i < nb; i++) c[i] = -co[i].alpha[k];
    blockblas::caxpy(c.data(), *APv[k], r);
    blockblas::norm2(r2.data(), r);
    k++; total++;
    if (k == nK || total == maxit || !open()) {
      // solution update by back substitution per right-hand side, then the true residual
      std::vector<std::vector<Complex>> delta(k, std::vector<Complex>(nb));
      std::vector<Complex> d(k);
      for (int i = 0; i < nb; i++) {
        co[i].backSubstitute(k, d.data());
        for (int a = 0; a < k; a++) delta[a][i] = d[a];
      }
      for (int a = 0; a < k; a++) blockblas::caxpy(delta[a].data(), *Pv[a], yv);
      if (total < maxit) {   // true residual of the restart (it decides whether the iteration goes on)
        op(r, yv);
        blockblas::xmy(b, r);
        blockblas::norm2(r2.data(), r);
      }
      k = 0;
    }
  }
  return total;
}
// coarsest grid: GCR(nKrylov) on Mhat x_p = bt
void BlockCoarseCycle::gcr(BlockLevel &l) {
  gcrIters += gcrLockstep(*l.bt, *y, *l.r, P, AP, nKrylov, maxiter, tol, [&](BlockField &out, BlockField &in) { matpc(l, out, in); },
                          [&](BlockField &out, BlockField &in) { blockblas::copy(out, in); });
  // x_p = y (other parity of x is rebuilt by reconstruct)
  copyParity(*l.x, *y, l.p);
}
// K-cycle: level lev's full system M x = kb by GCR around its own cycle; the solution lands in l.x like a cycle's
void BlockCoarseCycle::kgcr(int lev) {
  BlockLevel &l = L[lev];
  kIters += gcrLockstep(*l.kb, *l.ky, *l.kr, l.KP, l.KAP, l.kKrylov, l.kMaxiter, l.kTol, [&](BlockField &out, BlockField &in) { apply(out, in, *l.Y); },
                        [&](BlockField &out, BlockField &in) { blockblas::copy(*l.b, in); cycle(lev); blockblas::copy(out, *l.x); });
  blockblas::copy(*l.x, *l.ky);
}

// x = cycle(b) on level lev of the sub-hierarchy; on level 0 the fields L[0].b / L[0].x are filled / read by the caller
void BlockCoarseCycle::cycle(int lev) {
  BlockLevel &l = L[lev];
  if (lev == nl - 1) {
    prepare(l);
    gcr(l);
    reconstruct(l);
    return;
  }
  prepare(l);
  mr(l, l.nuPre, false);
  BlockField *full = l.r;
  if (l.nuPre > 0) {
    // the full residual behind the even-odd pre-smoother is X_pp r~ on the solved parity and zero on the other (MG::imageOfLast): the operator on
    // MR's residual (zero on the other parity), output parity p only — one half application instead of reconstruct + full operator (four halves)
    apply(*l.w1, *l.r, *l.Y, l.p);
    zeroParity(*l.w1, 1 - l.p);
    full = l.w1;
  } else {
    reconstruct(l);
    apply(*l.r, *l.x, *l.Y);            // r = b - M x on every site
    blockblas::xmy(*l.b, *l.r);
  }
  // restrict / prolongate per right-hand side with the single-vector kernels of the level (aggregates of the coarse levels are tiny)
  BlockLevel &c = L[lev + 1];
  blockUnpack(l.fine, *full);
  for (int i = 0; i < nReal; i++) l.T->R(*l.coarse[i], *l.fine[i]);
  blockPack(source(lev + 1), l.coarse);
  solve(lev + 1);
  blockUnpack(l.coarse, *c.x);
  for (int i = 0; i < nReal; i++) l.T->P(*l.fine[i], *l.coarse[i]);
  blockPack(*l.w1, l.fine);
  std::vector<Complex> one(nb, Complex(1.0, 0.0));
  blockblas::caxpy(one.data(), *l.w1, *l.x);
  mr(l, l.nuPost, true);
  reconstruct(l);
}

BlockCoarseCycle *blockCoarseCreate(MG &top, int nb, const MGParam *parent) {
  const MGParam &tp = top.params();
  if (tp.level < 1) return nullptr;
  BlockCoarseCycle *bc = new BlockCoarseCycle;
  bc->nl = tp.Nlevel - tp.level;
  bc->nb = nb;
  bc->L.resize(bc->nl);
  MG *m = &top;
  for (int l = 0; l < bc->nl; l++, m = m->getCoarse()) {
    if (!m) { delete bc; return nullptr; }
    const MGParam &p = m->params();
    const bool coarsest = p.level == p.Nlevel - 1;
    const DiracCoarse *dc = dynamic_cast<const DiracCoarse *>(p.matResidual.Expose());
    const DiracCoarsePC *ds = dynamic_cast<const DiracCoarsePC *>(p.matSmooth.Expose());
    if (!dc || !ds || !m->smootherIsPC() || !blockCoarseSupported(dc->Links(), nb)) { delete bc; return nullptr; }
    BlockLevel &L = bc->L[l];
    {
      // the level above runs a K-cycle and this level is not the coarsest: GCR around this level's cycle (parameters of MG's coarse solver, multigrid.cpp)
      const MGParam *pp = l == 0 ? parent : &bc->parents[l - 1]->params();
      L.kSolve = !coarsest && pp && pp->cycle_type != QUDA_MG_CYCLE_VCYCLE;
      L.kTol = p.mg_global.smoother_tol[p.level];
    }
    bc->parents.push_back(m);
    L.Y = &dc->Links(); L.H = &ds->HatLinks();
    const QudaMatPCType pc = ds->getMatPCType();
    L.p = (pc == QUDA_MATPC_ODD_ODD) ? 1 : 0;
    L.nuPre = p.nu_pre; L.nuPost = p.nu_post; L.omega = p.omega;
    const int nGhost = blockGhost(L.Y->Xc, false).nGhost;
    for (BlockField **f : {&L.b, &L.x, &L.bt, &L.r, &L.Ar, &L.t, &L.w1, &L.w2}) { *f = new BlockField(L.Y->nSites, L.Y->n, nb, nGhost); blockblas::zero(**f); }
    if (L.kSolve) {
      for (BlockField **f : {&L.kb, &L.ky, &L.kr}) { *f = new BlockField(L.Y->nSites, L.Y->n, nb, nGhost); blockblas::zero(**f); }
      for (int k = 0; k < L.kKrylov; k++) {
        L.KP.push_back(new BlockField(L.Y->nSites, L.Y->n, nb, nGhost)); L.KAP.push_back(new BlockField(L.Y->nSites, L.Y->n, nb, nGhost));
        blockblas::zero(*L.KP.back()); blockblas::zero(*L.KAP.back());
      }
    }
    if (!coarsest) {
      L.T = m->getTransfer();
      if (!L.T) { delete bc; return nullptr; }
      for (int i = 0; i < nb; i++) { L.fine.push_back(L.T->createFineField()); L.coarse.push_back(L.T->createCoarseField()); }
    } else {
      const SolverParam *sp = m->preSmootherParam();
      bc->nKrylov = sp->Nkrylov; bc->maxiter = sp->maxiter; bc->tol = sp->tol;
      for (int k = 0; k < bc->nKrylov; k++) {
        bc->P.push_back(new BlockField(L.Y->nSites, L.Y->n, nb, nGhost)); bc->AP.push_back(new BlockField(L.Y->nSites, L.Y->n, nb, nGhost));
        blockblas::zero(*bc->P.back()); blockblas::zero(*bc->AP.back());
      }
      bc->y = new BlockField(L.Y->nSites, L.Y->n, nb, nGhost);
      blockblas::zero(*bc->y);
    }
  }
  return bc;
}

// One Schur piece of the cycle above on host-supplied fields (block.h; qudaAmdMultigridCoarsePC impl 1): a one-level BlockCoarseCycle on the links
// Y / H with matpc parity p, every work field preloaded with nonzero words on both parities (the input of matpc keeps its contract: other parity
// zero).  Returns the number of nonzero words found afterwards in the half of l.t that the second application of matpc multiplies with Xinv.
int blockCoarseSchurPiece(const CoarseGauge &Y, const CoarseGauge &H, int p, int op, int nrhs, const std::vector<ColorSpinorField *> &out,
                          const std::vector<ColorSpinorField *> &in, const std::vector<ColorSpinorField *> &b) {
  if (p < 0 || p > 1 || op < 0 || op > 2) errorQuda("Schur piece: matpc parity %d, op %d", p, op);
  if (!blockCoarseSupported(Y, nrhs)) errorQuda("block coarse operator not available for n = %d, nrhs = %d", Y.n, nrhs);
  BlockCoarseCycle bc;
  bc.nl = 1; bc.nb = bc.nReal = nrhs;
  bc.L.resize(1);
  BlockLevel &l = bc.L[0];
  l.Y = &Y; l.H = &H; l.p = p;
  const int nGhost = blockGhost(Y.Xc, false).nGhost;
  for (BlockField **f : {&l.b, &l.x, &l.bt, &l.r, &l.Ar, &l.t, &l.w1, &l.w2}) { *f = new BlockField(Y.nSites, Y.n, nrhs, nGhost); blockblas::zero(**f); }
  const size_t half = (size_t)l.t->Vh * l.t->ncomp * l.t->nrhs;
  auto dirty = [&](BlockField &f, int par) { HIP_CHECK(hipMemsetAsync(f.v + (size_t)par * half, 0x3f, half * sizeof(float2), computeStream())); };   // 0x3f3f3f3f = 0.747
  for (BlockField *f : {l.bt, l.Ar, l.t, l.w1, l.w2}) { dirty(*f, 0); dirty(*f, 1); }
  if (op == 0) {          // Mhat: in (parity p, the other half zero) -> out, with MR's operands
    blockPack(*l.r, in);
    BlockCoarseCycle::zeroParity(*l.r, 1 - p);
    bc.matpc(l, *l.Ar, *l.r);
    blockUnpack(out, *l.Ar);
  } else if (op == 1) {   // b -> bt
    blockPack(*l.b, b);
    bc.prepare(l);
    blockUnpack(out, *l.bt);
  } else {                // x_p, b -> x
    blockPack(*l.b, b);
    blockPack(*l.x, in);
    dirty(*l.x, 1 - p);
    bc.reconstruct(l);
    blockUnpack(out, *l.x);
  }
  std::vector<float2> th(half);
  HIP_CHECK(hipMemcpyAsync(th.data(), l.t->v + (size_t)p * half, half * sizeof(float2), hipMemcpyDeviceToHost, computeStream()));
  HIP_CHECK(hipStreamSynchronize(computeStream()));   // also: the work fields return to the pool at the end of this scope
  int nonzero = 0;
  if (op == 0) for (const float2 &w : th) nonzero += (w.x != 0.f) + (w.y != 0.f);   // prepare and reconstruct do not use l.t
  return nonzero;
}

}  // namespace quda
