// block_mg_cycle.cpp — ONE multigrid cycle for all sources of a lockstep solve (MG::cycleBlock): smoothing, restriction and prolongation on the
// fine level per source with the kernels of the single-source cycle or, where the fine level allows it, on block fields (BlockFineSmoother,
// four-source transfers), and everything below the fine level on block fields (BlockCoarseCycle).
#include "block_cycle.h"
#include "env.h"

namespace quda {

MGBlockState::~MGBlockState() {
  delete fine;
  for (Solver *s : pre) delete s;
  for (Solver *s : post) delete s;
  for (SolverParam *s : prePar) delete s;
  for (SolverParam *s : postPar) delete s;
  for (ColorSpinorField *f : r) delete f;
  for (ColorSpinorField *f : rc) delete f;
  for (ColorSpinorField *f : xc) delete f;
  for (ColorSpinorField *f : btilde) delete f;
  delete coarse;
}

// switches, each read once.  QUDA_AMD_MULTISRC_QUAD=0: restrict / prolong the sources one at a time (the comparison leg of tools/multisrc_timing.py);
// _DIRECT=0: the quads go through fields (unpack, R4 / P4, pack) instead of their block columns; _BLOCK_OUTER=0: blockApplyLast declines;
// _IMAGE_FROM_RESIDUAL=0: A x of the last cycle from two block stencil launches instead of the post-smoother's residual
static bool blockQuadTransfer() { static const bool on = envInt("QUDA_AMD_MULTISRC_QUAD", 1) != 0; return on; }
static bool blockDirectTransfer() { static const bool on = envInt("QUDA_AMD_MULTISRC_DIRECT", 1) != 0; return on; }
static bool blockOuter() { static const bool on = envInt("QUDA_AMD_MULTISRC_BLOCK_OUTER", 1) != 0; return on; }
static int imageFromResidual() { static const int on = envInt("QUDA_AMD_MULTISRC_IMAGE_FROM_RESIDUAL", 1); return on; }

void MG::blockRelease() { delete blockState; blockState = nullptr; }

bool MG::blockPrepare(int nsrc) {
  if (blockState && blockState->nsrc == nsrc) return true;
  blockRelease();
  if (mgp.level != 0 || mgp.level == mgp.Nlevel - 1 || !pcSmooth || !coarse) return false;
  const int nb = (nsrc + 7) / 8 * 8;
  if (nb > kMaxBlockRhs) return false;
  MGBlockState *st = new MGBlockState;
  st->nsrc = nsrc; st->nb = nb;
  // nullptr (a K-cycle below the first coarse level, an operator the MFMA kernel does not take): the coarse solves run source by source through
  // the hierarchy's own coarse solver, the fine level keeps its block smoother and four-source transfers
  st->coarse = blockCoarseCreate(*coarse, nb, &mgp);
  if (st->coarse) st->coarse->nReal = nsrc;
  for (int i = 0; i < nsrc; i++) {
    st->prePar.push_back(new SolverParam(*param_presmooth));
    st->postPar.push_back(new SolverParam(*param_postsmooth));
    st->pre.push_back(Solver::create(*st->prePar.back(), mgp.matSmooth, mgp.matSmooth, mgp.matSmooth));
    st->post.push_back(Solver::create(*st->postPar.back(), mgp.matSmooth, mgp.matSmooth, mgp.matSmooth));
    ColorSpinorParam cp = r->param();
    cp.create = QUDA_ZERO_FIELD_CREATE;
    st->r.push_back(new ColorSpinorField(cp));
    ColorSpinorParam bp = r->Even().param();
    bp.create = QUDA_ZERO_FIELD_CREATE;
    st->btilde.push_back(new ColorSpinorField(bp));
  }
  for (int i = 0; i < nb; i++) { st->rc.push_back(transfer->createCoarseField()); st->xc.push_back(transfer->createCoarseField()); }
  st->fine = blockFineCreate(*mgp.matSmooth.Expose(), *param_presmooth, *param_postsmooth, (int)mgp.fineFlavor, nsrc);
  blockState = st;
  return true;
}

// ================================================================================================
// the parity cycle of MG::cycleParity for all sources, stage by stage
// ================================================================================================
// what one call of MG::cycleParityBlock works on: its arguments, the pieces of the hierarchy the stages need, and the plan
struct ParityBlockCycle {
  std::vector<ColorSpinorField *> &x, &b;
  const std::vector<char> &active;
  Transfer &transfer;
  DiracMatrix &matSmooth;
  const Dirac &dirac;      // the smoother's operator
  Solver *coarseSolver;    // of the hierarchy, source by source (no BlockCoarseCycle)
  int nuPre;
  bool odd;                // parity of the even-odd system
  bool localTerm;          // the full residual is wanted behind a symmetrically preconditioned smoother: A_pp on the parity residual
  bool blockSmooth;        // smoothing of all sources on block fields (BlockFineSmoother), else source by source
  bool quad;               // four-source transfers
  bool blockDirect;        // ... from / onto the smoother's block columns
  std::vector<char> quadAt, inQuad;             // a quad starts at source i / source i is in one
  std::vector<const ColorSpinorField *> rin;    // what is restricted for source i (not for the sources of a direct quad)
  ColorSpinorField &parityOf(ColorSpinorField &f) const { return odd ? f.Odd() : f.Even(); }
};

static FineGroup *groupOfQuad(MGBlockState &st, int i, int &col0) {
  for (FineGroup &g : st.fine->groups) if (i >= g.first && i + 3 < g.first + g.n) { col0 = i - g.first; return &g; }
  return nullptr;
}

// quads of active sources for the four-source transfers; with the block smoother a quad sits inside one smoother group and (unless the local term has
// to be applied to the residual first) is restricted from / prolongated onto its block columns directly.  fieldsKnown: rin is set (per-source path)
static void planQuads(MGBlockState &st, ParityBlockCycle &c, bool fieldsKnown) {
  for (int i = 0; c.quad && i + 4 <= st.nsrc;) {
    bool ok = true;
    int col0;
    for (int s = 0; s < 4; s++) ok = ok && c.active[i + s] && (!fieldsKnown || c.rin[i + s]->Precision() == QUDA_SINGLE_PRECISION);
    if (ok && c.blockSmooth && !groupOfQuad(st, i, col0)) ok = false;
    if (ok) { c.quadAt[i] = 1; for (int s = 0; s < 4; s++) c.inQuad[i + s] = 1; i += 4; } else i++;
  }
}

// x_i = K b_i starts here for source i: the fields of the cycle take the source's flavour; returns the parity of st.r[i] the cycle works on
static ColorSpinorField &adoptFlavor(MGBlockState &st, ParityBlockCycle &c, int i) {
  c.x[i]->twistFlavor = c.b[i]->twistFlavor;
  ColorSpinorField &rp = c.parityOf(*st.r[i]);
  st.r[i]->twistFlavor = rp.twistFlavor = c.b[i]->twistFlavor;
  return rp;
}

// block path: sources onto the groups' B, nuPre MR steps, residuals back into fields for every source outside a direct quad
static void preSmoothBlocks(MGBlockState &st, ParityBlockCycle &c) {
  BlockFineSmoother &F = *st.fine;
  for (FineGroup &g : F.groups) {
    const ColorSpinorField *src[8];
    ColorSpinorField *dst[8];
    bool anyField = false;
    for (int j = 0; j < g.n; j++) {
      const int i = g.first + j;
      src[j] = c.active[i] ? c.b[i] : nullptr;
      dst[j] = nullptr;
      if (!c.active[i]) continue;
      ColorSpinorField &rp = adoptFlavor(st, c, i);
      if (!(c.blockDirect && c.inQuad[i])) { dst[j] = &rp; anyField = true; }
    }
    blockPackParity(*g.B, src, g.n);
    if (F.nuPre > 0) {
      F.mr(g, F.nuPre, g.B, true);
      if (anyField) blockUnpackParity(dst, g.n, *g.R);
    }
    for (int j = 0; j < g.n; j++) {
      const int i = g.first + j;
      if (!c.active[i] || (c.blockDirect && c.inQuad[i])) continue;
      if (F.nuPre > 0) {
        if (c.localTerm) c.dirac.localTermParity(*dst[j], *dst[j], c.odd ? 1 : 0);
        c.rin[i] = dst[j];
      } else if (c.localTerm) {
        c.dirac.localTermParity(*dst[j], *c.b[i], c.odd ? 1 : 0);
        c.rin[i] = dst[j];
      } else {
        c.rin[i] = c.b[i];
      }
    }
  }
}

// per-source path: the hierarchy's own kind of smoother, one per source; the residual is MR's where it keeps one, else b - A x
static void preSmoothPerSource(MGBlockState &st, ParityBlockCycle &c) {
  for (int i = 0; i < st.nsrc; i++) {
    if (!c.active[i]) continue;
    ColorSpinorField &rp = adoptFlavor(st, c, i);
    (*st.pre[i])(*c.x[i], *c.b[i]);
    const ColorSpinorField *res = c.nuPre > 0 ? st.pre[i]->lastResidual() : nullptr;
    if (res && res->Precision() == QUDA_SINGLE_PRECISION && !c.localTerm) {
      c.rin[i] = res;
    } else if (res) {
      if (c.localTerm && res->Precision() == QUDA_SINGLE_PRECISION) c.dirac.localTermParity(rp, *res, c.odd ? 1 : 0);
      else { blas::copy(rp, *res); if (c.localTerm) c.dirac.localTermParity(rp, rp, c.odd ? 1 : 0); }
      c.rin[i] = &rp;
    } else {
      c.matSmooth(rp, *c.x[i]);
      blas::axpby(1.0, *c.b[i], -1.0, rp);
      if (c.localTerm) c.dirac.localTermParity(rp, rp, c.odd ? 1 : 0);
      c.rin[i] = &rp;
    }
  }
}

// V (2304 B per fine site) is the traffic of the restrictor and the prolongator: groups of four active sources share one pass over it
static void restrictSources(MGBlockState &st, ParityBlockCycle &c) {
  for (int i = 0; i < st.nb;) {
    if (i < st.nsrc && c.quadAt[i]) {
      ColorSpinorField *c4[4] = {st.rc[i], st.rc[i + 1], st.rc[i + 2], st.rc[i + 3]};
      if (c.blockDirect) {
        int col0;
        FineGroup *g = groupOfQuad(st, i, col0);
        c.transfer.R4Block(c4, (st.fine->nuPre > 0 ? g->R : g->B)->v, g->nrhs, col0);
      } else {
        const ColorSpinorField *f4[4] = {c.rin[i], c.rin[i + 1], c.rin[i + 2], c.rin[i + 3]};
        c.transfer.R4(c4, f4);
      }
      multiSrcCount(MS_QUAD_TRANSFERS);
      i += 4;
      continue;
    }
    if (i < st.nsrc && c.active[i]) c.transfer.R(*st.rc[i], *c.rin[i]);
    else blas::zero(*st.rc[i]);
    i++;
  }
}

static void coarseSolve(MGBlockState &st, ParityBlockCycle &c) {
  if (st.coarse) {
    // everything below the fine level for all sources at once, on the matrix cores
    blockPack(st.coarse->source(0), st.rc);
    st.coarse->solve(0);
    blockUnpack(st.xc, *st.coarse->L[0].x);
  } else {
    for (int i = 0; i < st.nsrc; i++) {
      if (!c.active[i]) continue;
      blas::zero(*st.xc[i]);
      (*c.coarseSolver)(*st.xc[i], *st.rc[i]);
    }
  }
}

// prolongation through fields: the sources outside the direct quads.  Per-source path: the correction is added to x_i here; block path: it stays
// in the cycle's parity of st.r[i] for postSmoothBlocks, which also prolongates the direct quads straight onto their columns
static void prolongThroughFields(MGBlockState &st, ParityBlockCycle &c) {
  for (int i = 0; i < st.nsrc;) {
    if (c.quadAt[i]) {
      if (!c.blockDirect) {
        ColorSpinorField *f4[4];
        const ColorSpinorField *c4[4] = {st.xc[i], st.xc[i + 1], st.xc[i + 2], st.xc[i + 3]};
        for (int s = 0; s < 4; s++) f4[s] = &c.parityOf(*st.r[i + s]);
        c.transfer.P4(f4, c4);
        multiSrcCount(MS_QUAD_TRANSFERS);
        if (!c.blockSmooth) for (int s = 0; s < 4; s++) blas::xpy(*f4[s], *c.x[i + s]);
      }
      i += 4;
      continue;
    }
    if (c.active[i]) {
      ColorSpinorField &rp = c.parityOf(*st.r[i]);
      c.transfer.P(rp, *st.xc[i]);
      if (!c.blockSmooth) blas::xpy(rp, *c.x[i]);
    }
    i++;
  }
}

// block path: X (+)= P e, nuPost MR steps from the explicitly computed residual, solutions back into the x_i
static void postSmoothBlocks(MGBlockState &st, ParityBlockCycle &c) {
  BlockFineSmoother &F = *st.fine;
  for (FineGroup &g : F.groups) {
    const ColorSpinorField *corr[8];
    ColorSpinorField *dst[8];
    bool viaFields = false;
    for (int j = 0; j < g.n; j++) {
      const int i = g.first + j;
      const bool direct = c.blockDirect && c.inQuad[i];
      corr[j] = c.active[i] && !direct ? &c.parityOf(*st.r[i]) : nullptr;
      dst[j] = c.active[i] ? c.x[i] : nullptr;
      viaFields = viaFields || (c.active[i] && !direct);
    }
    // X (+)= P e: corrections that went through fields are packed onto X (columns without one get zeros, or stay as they are when X already
    // holds the pre-smoothed solution); ... the quads are prolongated straight onto their columns
    if (viaFields || F.nuPre == 0) blockPackParity(*g.X, corr, g.n, F.nuPre > 0);   // (after pre-smoothing the idle and padding columns of X are zero already)
    for (int j = 0; j + 3 < g.n; j++) {
      const int i = g.first + j;
      if (!c.blockDirect || !c.quadAt[i]) continue;
      const ColorSpinorField *c4[4] = {st.xc[i], st.xc[i + 1], st.xc[i + 2], st.xc[i + 3]};
      c.transfer.P4Block(g.X->v, g.nrhs, j, true, c4);
      multiSrcCount(MS_QUAD_TRANSFERS);
    }
    if (F.nuPost > 0) {
      F.residual(g);
      F.mr(g, F.nuPost, nullptr, st.wantImage);
    }
    blockUnpackParity(dst, g.n, *g.X);
  }
}

static void postSmoothPerSource(MGBlockState &st, ParityBlockCycle &c) {
  for (int i = 0; i < st.nsrc; i++) if (c.active[i]) (*st.post[i])(*c.x[i], *c.b[i]);
}

// x_i = K b_i (single-parity fields)
void MG::cycleParityBlock(std::vector<ColorSpinorField *> &x, std::vector<ColorSpinorField *> &b, const std::vector<char> &active, bool fullResidual) {
  MGBlockState &st = *blockState;
  const int nsrc = st.nsrc;
  const Dirac &dirac = *mgp.matSmooth.Expose();
  const QudaMatPCType mt = dirac.getMatPCType();
  const bool odd = mt == QUDA_MATPC_ODD_ODD || mt == QUDA_MATPC_ODD_ODD_ASYMMETRIC;
  const bool symmetric = mt == QUDA_MATPC_EVEN_EVEN || mt == QUDA_MATPC_ODD_ODD;
  ParityBlockCycle c = {x, b, active, *transfer, mgp.matSmooth, dirac, coarse_solver, mgp.nu_pre, odd, fullResidual && symmetric};
  c.blockSmooth = st.fine != nullptr;
  for (int i = 0; i < nsrc && c.blockSmooth; i++)
    if (active[i] && (b[i]->Precision() != QUDA_SINGLE_PRECISION || x[i]->Precision() != QUDA_SINGLE_PRECISION || (int)b[i]->twistFlavor != (int)mgp.fineFlavor)) c.blockSmooth = false;
  c.quad = transfer->canQuad() && blockQuadTransfer();
  c.blockDirect = c.blockSmooth && c.quad && !c.localTerm && blockDirectTransfer();
  c.quadAt.assign(nsrc + 4, 0); c.inQuad.assign(nsrc + 4, 0);
  c.rin.assign(nsrc, nullptr);
  multiSrcCount(MS_CYCLES);
  if (c.blockSmooth) multiSrcCount(MS_BLOCK_SMOOTHED);
  st.solutionOnBlocks = c.blockSmooth;
  st.residualOnBlocks = c.blockSmooth && st.wantImage && st.fine->nuPost > 0;

  const QudaParity parity = odd ? QUDA_ODD_PARITY : QUDA_EVEN_PARITY;
  if (c.blockSmooth) {
    planQuads(st, c, false);
    preSmoothBlocks(st, c);
    transfer->setSiteSubset(QUDA_PARITY_SITE_SUBSET, parity);
    restrictSources(st, c);
    coarseSolve(st, c);
    prolongThroughFields(st, c);
    postSmoothBlocks(st, c);
    transfer->setSiteSubset(QUDA_FULL_SITE_SUBSET, QUDA_INVALID_PARITY);
  } else {
    preSmoothPerSource(st, c);
    transfer->setSiteSubset(QUDA_PARITY_SITE_SUBSET, parity);
    planQuads(st, c, true);
    restrictSources(st, c);
    coarseSolve(st, c);
    prolongThroughFields(st, c);
    transfer->setSiteSubset(QUDA_FULL_SITE_SUBSET, QUDA_INVALID_PARITY);
    postSmoothPerSource(st, c);
  }
  blas::setGlobalReduction(true);
}

void MG::blockWantImage(int nsrc, bool on) { if (blockPrepare(nsrc)) blockState->wantImage = on; }

bool MG::blockApplyLast(std::vector<ColorSpinorField *> &out, const Dirac &pc, const std::vector<char> &active) {
  if (!blockState || !blockState->fine || !blockState->solutionOnBlocks) return false;
  BlockFineSmoother &F = *blockState->fine;
  if (!blockOuter()) return false;
  const GaugeField *W = pc.Gauge();
  if (pc.getDiracType() != F.type || pc.getMatPCType() != F.matpcType || pc.Kappa() != F.kappa || pc.Mu() != F.mu || !W || !fineBlockSupported(*W, 8) || !fineBlockSupported(*W, 4)) return false;
  if (F.tmat[0] && !(pc.Clover() && pc.Clover()->precision == QUDA_SINGLE_PRECISION)) return false;
  if ((int)out.size() != blockState->nsrc) return false;
  for (size_t i = 0; i < out.size(); i++)
    if (active[i] && (out[i]->Precision() != QUDA_SINGLE_PRECISION || out[i]->SiteSubset() != QUDA_PARITY_SITE_SUBSET)) return false;
  // the post-smoother's last residual r = b - A x is at hand (MR keeps it with the solution): A x = b - r, one sweep instead of two stencil launches
  // (the same operator in exact arithmetic; in fp32 the recursion of two MR steps from an explicitly computed residual is as good as the product)
  const int viaResidual = imageFromResidual();
  for (FineGroup &g : F.groups) {
    ColorSpinorField *dst[8];
    for (int j = 0; j < g.n; j++) dst[j] = active[g.first + j] ? out[g.first + j] : nullptr;
    if (blockState->residualOnBlocks && viaResidual) {   // (sloppy and preconditioner links hold the same matrices, to the rounding of their storage)
      blockblas::xmy(*g.B, *g.R);    // R <- b - r
      blockUnpackParity(dst, g.n, *g.R);
    } else {
      F.matpc(g, *g.AR, *g.X, 0, W);
      blockUnpackParity(dst, g.n, *g.AR);
    }
  }
  return true;
}

// Full-system outer solve: M x_i for the reconstructed solutions of the last cycleBlock, from the post-smoother's residuals on the block fields —
// (M x)_q = b_q, (M x)_p = b_p - A_pp r~ (symmetric preconditioning; see MG::imageOfLast): unpack r~ into scratch fields, local term, subtract.
bool MG::blockImageFull(std::vector<ColorSpinorField *> &out, std::vector<ColorSpinorField *> &b, const Dirac &full, const std::vector<char> &active) {
  if (!blockState || !blockState->fine || !blockState->residualOnBlocks) return false;
  if (!imageFromResidual()) return false;
  BlockFineSmoother &F = *blockState->fine;
  MGBlockState &st = *blockState;
  const Dirac &S = *mgp.matSmooth.Expose();
  const QudaDiracType at = full.getDiracType();
  const bool pair = (F.type == QUDA_WILSONPC_DIRAC && at == QUDA_WILSON_DIRAC) || (F.type == QUDA_TWISTED_MASSPC_DIRAC && at == QUDA_TWISTED_MASS_DIRAC) ||
                    (F.type == QUDA_TWISTED_CLOVERPC_DIRAC && at == QUDA_TWISTED_CLOVER_DIRAC);
  if (!pair || full.Kappa() != F.kappa || full.Mu() != F.mu || (int)out.size() != st.nsrc) return false;
  for (size_t i = 0; i < out.size(); i++)
    if (active[i] && (out[i]->Precision() != QUDA_SINGLE_PRECISION || out[i]->SiteSubset() != QUDA_FULL_SITE_SUBSET || b[i]->Precision() != QUDA_SINGLE_PRECISION)) return false;
  const int par = F.par;
  for (FineGroup &g : F.groups) {
    ColorSpinorField *dst[8];
    for (int j = 0; j < g.n; j++) {
      const int i = g.first + j;
      dst[j] = active[i] ? (par ? &st.r[i]->Odd() : &st.r[i]->Even()) : nullptr;
      if (dst[j]) dst[j]->twistFlavor = b[i]->twistFlavor;
    }
    blockUnpackParity(dst, g.n, *g.R);
    for (int j = 0; j < g.n; j++) {
      const int i = g.first + j;
      if (!active[i]) continue;
      S.localTermParity(*dst[j], *dst[j], par);     // symmetric preconditioning only (the block smoother's condition)
      blas::copy(*out[i], *b[i]);
      blas::mxpy(*dst[j], par ? out[i]->Odd() : out[i]->Even());
    }
  }
  return true;
}

// x_i = K b_i for all sources (full fields: Schur prepare, parity cycle, reconstruct, as MG::operator(); parity fields: the parity cycle)
bool MG::cycleBlock(std::vector<ColorSpinorField *> &x, std::vector<ColorSpinorField *> &b, const std::vector<char> &active) {
  const int nsrc = (int)x.size();
  if (!blockPrepare(nsrc)) return false;
  if (b[0]->SiteSubset() != QUDA_FULL_SITE_SUBSET) { cycleParityBlock(x, b, active, false); return true; }
  MGBlockState &st = *blockState;
  const Dirac &dirac = *mgp.matSmooth.Expose();
  const bool matpc = mgp.mg_global.coarse_grid_solution_type[0] == QUDA_MATPC_SOLUTION;
  std::vector<ColorSpinorField *> in(nsrc, nullptr), out(nsrc, nullptr);
  for (int i = 0; i < nsrc; i++) {
    if (!active[i]) continue;
    st.r[i]->twistFlavor = x[i]->twistFlavor = b[i]->twistFlavor;
    // (no copies: prepare() reads b and leaves the prepared source in the parity of x that reconstruct() fills last — MG::cycleUnfused)
    ColorSpinorField *pin = nullptr, *pout = nullptr;
    dirac.prepare(pin, pout, *x[i], *b[i], QUDA_MAT_SOLUTION);
    pin->twistFlavor = b[i]->twistFlavor;
    in[i] = pin; out[i] = pout;
  }
  for (int i = 0; i < nsrc; i++) if (!active[i]) { in[i] = st.btilde[i]; out[i] = st.btilde[i]; }
  cycleParityBlock(out, in, active, !matpc);
  st.solutionOnBlocks = false;   // the outer solver's direction is the reconstructed full field
  for (int i = 0; i < nsrc; i++) if (active[i]) dirac.reconstruct(*x[i], *b[i], QUDA_MAT_SOLUTION);
  return true;
}

}  // namespace quda
