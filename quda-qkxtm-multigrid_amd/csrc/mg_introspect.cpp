// mg_introspect.cpp — read-only access to the pieces of a multigrid hierarchy for parity tests and FFI callers: what a
// C++ test of the reference reaches through multigrid_solver->mg (null vectors B, the packed block-orthonormal V,
// the coarse link fields Y / X, and R, P, M of every level; reference include/multigrid.h:108-330, include/transfer.h).
// Host layouts are the reference's CPU orders: vectors site-major (parity*Vh + x_cb, spin, colour, re/im) fp32
// (QUDA_SPACE_SPIN_COLOR_FIELD_ORDER, DeGrand-Rossi basis on level 0); V as (site, spin, colour, vector);
// coarse links as QDP-ordered Y[dim 0-3 backward | 4-7 forward][site][row][col] with the operator's -kappa folded in.
// At the end: the even-odd preconditioned coarse operator piece by piece (qudaAmdMultigridGetCoarseSiteLinks, qudaAmdMultigridCoarseApply,
// qudaAmdMultigridCoarsePC, qudaAmdCoarseInvertSites), which the library itself reaches only from inside a solve.
#include <hip/hip_runtime.h>

#include <cstring>
#include <vector>

#include "interface_internal.h"
#include "block.h"
#include "coarse_cycle.h"
#include "dslash.h"
#include "multigrid.h"
#include "quda_amd_ext.h"

using namespace quda;

static MG *levelOf(void *mg_instance, int level) {
  if (!mg_instance) errorQuda("null multigrid handle");
  MG *m = static_cast<multigrid_solver *>(mg_instance)->mg;
  for (int l = 0; l < level && m; l++) m = m->getCoarse();
  if (!m) errorQuda("multigrid level %d does not exist", level);
  return m;
}

static ColorSpinorField hostView(const ColorSpinorField &dev, void *ptr) {
  ColorSpinorParam p = dev.param();
  p.location = QUDA_CPU_FIELD_LOCATION;
  p.precision = QUDA_SINGLE_PRECISION;
  p.fieldOrder = QUDA_SPACE_SPIN_COLOR_FIELD_ORDER;
  p.gammaBasis = QUDA_DEGRAND_ROSSI_GAMMA_BASIS;
  p.create = QUDA_REFERENCE_FIELD_CREATE;
  p.pad = 0;
  p.v = ptr;
  return ColorSpinorField(p);
}

extern "C" {

void qudaAmdMultigridSetHalfStorage(void *mg_instance, int on) { multigridSetHalfStorage(*static_cast<multigrid_solver *>(mg_instance), on != 0); }

int qudaAmdMultigridLevels(void *mg_instance) {
  int n = 0;
  for (MG *m = static_cast<multigrid_solver *>(mg_instance)->mg; m; m = m->getCoarse()) n++;
  return n;
}

// info[18] = Xf[4], Xc[4], fineSpin, fineColor, Nvec, geo_bs[4], spin_bs, 0, 0  (of the transfer level -> level+1)
void qudaAmdMultigridLevelInfo(void *mg_instance, int level, int info[18]) {
  const MG *lv = levelOf(mg_instance, level);
  const Transfer *T = lv->getTransfer();
  if (!T) errorQuda("level %d is the coarsest level: no transfer", level);
  memset(info, 0, 18 * sizeof(int));
  for (int d = 0; d < 4; d++) { info[d] = T->Xf[d]; info[4 + d] = T->Xc[d]; info[11 + d] = T->geo_bs[d]; }
  info[8] = T->fineSpin; info[9] = T->fineColor; info[10] = T->Nvec; info[15] = T->spin_bs;
  info[16] = lv->nullVectorMethod; info[17] = lv->nullVectorIterations;
}

// set-up refinement (multigrid.h multigrid_solver::refine): `passes` inverse-iteration passes of `cycles` multigrid cycles per null vector,
// the hierarchy rebuilt after each; returns the seconds it took
double qudaAmdMultigridRefine(void *mg_instance, int passes, int cycles) {
  multigrid_solver *s = static_cast<multigrid_solver *>(mg_instance);
  if (!s) errorQuda("null multigrid instance");
  const double before = s->mg_param_copy.secs;
  s->refine(passes, cycles);
  return s->mg_param_copy.secs - before;
}

// (aggregate, chirality) blocks of the level's transfer operator that the fp32 CholeskyQR2 orthonormalisation handed to Gram-Schmidt
int qudaAmdMultigridOrthoFallbackBlocks(void *mg_instance, int level) {
  const Transfer *T = levelOf(mg_instance, level)->getTransfer();
  if (!T) errorQuda("level %d is the coarsest level: no transfer", level);
  return T->lastGsFallbackBlocks;
}

void qudaAmdMultigridGetNullVector(void *mg_instance, int level, int k, float *h_out) {
  const std::vector<ColorSpinorField *> &B = levelOf(mg_instance, level)->nullVectors();
  if (k < 0 || k >= (int)B.size()) errorQuda("null vector %d of %zu", k, B.size());
  ColorSpinorField h = hostView(*B[k], h_out);
  h = *B[k];
}

void qudaAmdMultigridGetV(void *mg_instance, int level, float *h_out) {
  const Transfer *T = levelOf(mg_instance, level)->getTransfer();
  if (!T) errorQuda("level %d is the coarsest level: no transfer", level);
  const int K = T->fineSpin * T->fineColor, N = T->Nvec, bv = T->blockVol;
  std::vector<float> v(T->vBytes() / sizeof(float));
  std::vector<int> b2f(T->fineVol);
  HIP_CHECK(hipStreamSynchronize(computeStream()));
  HIP_CHECK(hipMemcpy(v.data(), T->V, T->vBytes(), hipMemcpyDeviceToHost));
  HIP_CHECK(hipMemcpy(b2f.data(), T->block_to_fine, T->fineVol * sizeof(int), hipMemcpyDeviceToHost));
  for (long A = 0; A < T->nAgg; A++)
    for (int b = 0; b < bv; b++) {
      const long f = b2f[A * bv + b];
      for (int k = 0; k < K; k++)
        for (int j = 0; j < N; j++) {
          const size_t src = ((((size_t)A * K + k) * (N / 2) + j / 2) * bv + b) * 4 + (j & 1) * 2;
          const size_t dst = (((size_t)f * K + k) * N + j) * 2;
          h_out[dst] = v[src]; h_out[dst + 1] = v[src + 1];
        }
    }
}

// Y[8][Vc][n][n], X[Vc][n][n] complex fp32 of the operator on level+1, reference index convention (include/
// gauge_field_order.h QDP order; dims 0-3 = the link applied daggered from the backward neighbour, 4-7 forward)
void qudaAmdMultigridGetCoarseLinks(void *mg_instance, int level, float *h_Y, float *h_X) {
  const DiracCoarse *D = levelOf(mg_instance, level)->getCoarseDirac();
  if (!D) errorQuda("level %d has no coarse operator", level);
  const CoarseGauge &G = D->Links();
  const int n = G.n;
  const long Vc = G.nSites, Vh = Vc / 2;
  std::vector<float> g(G.bytes / sizeof(float));
  HIP_CHECK(hipStreamSynchronize(computeStream()));
  HIP_CHECK(hipMemcpy(g.data(), G.data, G.bytes, hipMemcpyDeviceToHost));
  auto elem = [&](long A, int m, int r, int c) { return &g[((((size_t)A * 9 + m) * (n / 2) + c / 2) * n + r) * 4 + (c & 1) * 2]; };
  for (long A = 0; A < Vc; A++) {
    const int par = A >= Vh;
    long l = A - par * Vh;
    const int Xh = G.Xc[0] / 2;
    const int xh = (int)(l % Xh); l /= Xh;
    const int y = (int)(l % G.Xc[1]); l /= G.Xc[1];
    const int z = (int)(l % G.Xc[2]), t = (int)(l / G.Xc[2]);
    const int c[4] = {2 * xh + ((y + z + t + par) & 1), y, z, t};
    for (int r = 0; r < n; r++)
      for (int q = 0; q < n; q++) {
        const float *x = elem(A, 8, r, q);
        float *o = h_X + (((size_t)A * n + r) * n + q) * 2;
        o[0] = x[0]; o[1] = x[1];
      }
    for (int mu = 0; mu < 4; mu++) {
      // forward link: stored at its own site
      for (int r = 0; r < n; r++)
        for (int q = 0; q < n; q++) {
          const float *f = elem(A, 2 * mu, r, q);
          float *o = h_Y + ((((size_t)(mu + 4) * Vc + A) * n + r) * n + q) * 2;
          o[0] = f[0]; o[1] = f[1];
        }
      // backward link of site A + mu is Y_mu(A)^dagger
      int cn[4] = {c[0], c[1], c[2], c[3]};
      cn[mu] = (c[mu] + 1) % G.Xc[mu];
      const int npar = (cn[0] + cn[1] + cn[2] + cn[3]) & 1;
      const long An = npar * Vh + ((((long)cn[3] * G.Xc[2] + cn[2]) * G.Xc[1] + cn[1]) * G.Xc[0] + cn[0]) / 2;
      for (int r = 0; r < n; r++)
        for (int q = 0; q < n; q++) {
          const float *bk = elem(An, 2 * mu + 1, q, r);
          float *o = h_Y + ((((size_t)mu * Vc + A) * n + r) * n + q) * 2;
          o[0] = bk[0]; o[1] = -bk[1];
        }
    }
  }
}

// op 0: R (level -> level+1), 1: P (level+1 -> level), 2: M of level (the operator the cycle takes residuals with)
void qudaAmdMultigridApply(void *mg_instance, int level, int op, float *h_out, const float *h_in) {
  MG *m = levelOf(mg_instance, level);
  const Transfer *T = m->getTransfer();
  if (op < 2 && !T) errorQuda("level %d is the coarsest level: no transfer", level);
  ColorSpinorField *fin = nullptr, *fout = nullptr;
  const ColorSpinorField &proto = *m->nullVectors()[0];
  auto fine = [&]() { ColorSpinorParam p = proto.param(); p.create = QUDA_ZERO_FIELD_CREATE; return new ColorSpinorField(p); };
  switch (op) {
    case 0: fin = fine(); fout = T->createCoarseField(); break;
    case 1: fin = T->createCoarseField(); fout = fine(); break;
    case 2: case 3: fin = fine(); fout = fine(); break;
    default: errorQuda("unknown op %d", op);
  }
  ColorSpinorField hin = hostView(*fin, const_cast<float *>(h_in)), hout = hostView(*fout, h_out);
  *fin = hin;
  fin->twistFlavor = fout->twistFlavor = proto.twistFlavor;
  if (op == 0) T->R(*fout, *fin);
  else if (op == 1) T->P(*fout, *fin);
  else if (op == 3) (*m)(*fout, *fin);   // one multigrid cycle of this level (MG::operator(): the fused persistent kernel where it qualifies)
  else m->residualMatrix()(*fout, *fin);
  hout = *fout;
  delete fin; delete fout;
}

// The transfer operators of `level` one by one (quda_amd_ext.h lists the ops): the quad and block-column variants and the single-parity route,
// which the library itself reaches only from inside a solve.  parity 0 / 1: the transfer is set to that parity subset for the call, the fine
// operands are the parity views of full device fields (the other half of an input stays loaded and must be ignored, the other half of an
// output stays zero).
void qudaAmdMultigridApplyTransfer(void *mg_instance, int level, int op, int parity, float *h_out, const float *h_in) {
  MG *m = levelOf(mg_instance, level);
  Transfer *T = const_cast<Transfer *>(m->getTransfer());
  if (!T) errorQuda("level %d is the coarsest level: no transfer", level);
  if (op < 0 || op > 6) errorQuda("unknown transfer op %d", op);
  if (parity < -1 || parity > 1) errorQuda("parity %d (-1: full fields, 0 / 1)", parity);
  const bool block = op >= 4, isR = op == 0 || op == 2 || op == 4;
  if (block && parity < 0) errorQuda("the block-column transfers work on one parity");
  const int nsrc = op < 2 ? 1 : 4, col0 = 4, nrhs = 8;
  const int nfine = block ? nrhs : nsrc;   // fine fields on the device: the block ops fill / return all eight columns
  const ColorSpinorField &proto = *m->nullVectors()[0];
  std::vector<ColorSpinorField *> fine(nfine), coarse(nsrc);
  for (auto &f : fine) { ColorSpinorParam p = proto.param(); p.create = QUDA_ZERO_FIELD_CREATE; f = new ColorSpinorField(p); }
  for (auto &c : coarse) c = T->createCoarseField();
  const size_t flen = (size_t)proto.Volume() * proto.Nspin() * proto.Ncolor() * 2, clen = (size_t)T->nAgg * 2 * T->Nvec * 2;
  // host -> device.  Restrictors: nsrc fine vectors.  Prolongators: nsrc coarse vectors, for the block op followed by the eight fine
  // vectors the block field is preloaded with.
  for (int s = 0; s < nsrc; s++) {
    ColorSpinorField &d = isR ? *fine[block ? col0 + s : s] : *coarse[s];
    d = hostView(d, const_cast<float *>(h_in) + s * (isR ? flen : clen));
  }
  if (block && isR) for (int s = 0; s < 4; s++) blas::copy(*fine[s], *fine[col0 + 3 - s]);   // columns 0..3: the sources in reverse order
  if (block && !isR) for (int i = 0; i < nrhs; i++) *fine[i] = hostView(*fine[i], const_cast<float *>(h_in) + 4 * clen + i * flen);
  const QudaSiteSubset subset0 = T->site_subset;
  const QudaParity parity0 = T->subset_parity;
  if (parity >= 0) T->setSiteSubset(QUDA_PARITY_SITE_SUBSET, parity ? QUDA_ODD_PARITY : QUDA_EVEN_PARITY);
  std::vector<ColorSpinorField *> f(nfine);
  for (int i = 0; i < nfine; i++) f[i] = parity < 0 ? fine[i] : (parity ? &fine[i]->Odd() : &fine[i]->Even());
  if (op == 0) T->R(*coarse[0], *f[0]);
  else if (op == 1) T->P(*f[0], *coarse[0]);
  else if (op == 2) T->R4(coarse.data(), f.data());
  else if (op == 3) T->P4(f.data(), coarse.data());
  else {
    BlockField b(proto.VolumeCB(), 12, nrhs);
    blockPackParity(b, f.data(), nrhs);
    if (isR) T->R4Block(coarse.data(), b.v, nrhs, col0);
    else { T->P4Block(b.v, nrhs, col0, op == 6, coarse.data()); blockUnpackParity(f.data(), nrhs, b); }
    HIP_CHECK(hipStreamSynchronize(computeStream()));   // b returns to the pool at the end of this scope
  }
  T->setSiteSubset(subset0, parity0);
  if (!isR && parity >= 0 && block)   // only the parity views came back from the block: the other half reports as zero
    for (int i = 0; i < nrhs; i++) blas::zero(parity ? fine[i]->Even() : fine[i]->Odd());
  const int nout = isR ? nsrc : nfine;
  for (int s = 0; s < nout; s++) {
    ColorSpinorField &d = isR ? *coarse[s] : *fine[s];
    ColorSpinorField h = hostView(d, h_out + s * (isR ? clen : flen));
    h = d;
  }
  for (auto p : fine) delete p;
  for (auto p : coarse) delete p;
}

// the cycle below a coarse level as one persistent kernel (coarse_cycle.h): process-wide switch and the statistics of the last launch of `level`
void qudaAmdMultigridSetFused(int on) { coarseCycleSetEnabled(on); }
int qudaAmdMultigridFusedStats(void *mg_instance, int level, long long out[5]) {
  MG *m = levelOf(mg_instance, level);
  coarseCycleStats(m->fusedCycle(), out);
  return m->fusedCycle() ? 1 : 0;
}

// M of a COARSE level applied to nrhs host vectors at once through the multi-right-hand-side MFMA kernel (block.h): h_in / h_out
// hold nrhs vectors back to back, each in the host layout of qudaAmdMultigridApply.  niter > 0: the application is repeated
// niter times between device events on the compute stream and the seconds per application are returned (else 0).
double qudaAmdMultigridApplyBlock(void *mg_instance, int level, int nrhs, float *h_out, const float *h_in, int niter) {
  MG *m = levelOf(mg_instance, level);
  const Dirac *dg = m->residualMatrix().Expose();
  const DiracCoarse *dc = dynamic_cast<const DiracCoarse *>(dg);
  const QudaDiracType ty = dg->getDiracType();
  const bool fine = ty == QUDA_WILSON_DIRAC || ty == QUDA_TWISTED_MASS_DIRAC || ty == QUDA_TWISTED_CLOVER_DIRAC;
  if (!fine && (!dc || ty != QUDA_COARSE_DIRAC)) errorQuda("level %d does not carry a full fine or coarse operator", level);
  if (!fine && !blockCoarseSupported(dc->Links(), nrhs)) errorQuda("block coarse operator not available for n = %d, nrhs = %d on this lattice", dc->Links().n, nrhs);
  if (fine && !fineBlockSupported(*dg->Gauge(), nrhs)) errorQuda("block fine operator not available for nrhs = %d on this lattice", nrhs);
  const ColorSpinorField &proto = *m->nullVectors()[0];
  std::vector<ColorSpinorField *> f(nrhs);
  const size_t len = (size_t)proto.Volume() * proto.Nspin() * proto.Ncolor() * 2;
  for (int i = 0; i < nrhs; i++) {
    ColorSpinorParam p = proto.param(); p.create = QUDA_ZERO_FIELD_CREATE;
    f[i] = new ColorSpinorField(p);
    ColorSpinorField hin = hostView(*f[i], const_cast<float *>(h_in) + i * len);
    *f[i] = hin;
  }
  const int nSites = fine ? proto.Volume() : dc->Links().nSites, ncomp = fine ? 12 : dc->Links().n;
  const int nGhost = fine ? 2 * blockGhost(dg->Gauge()->geom.X, true).nGhost : blockGhost(dc->Links().Xc, false).nGhost;
  BlockField in(nSites, ncomp, nrhs, nGhost), out(nSites, ncomp, nrhs);
  blockPack(in, f);
  // level 0: the multi-right-hand-side stencil of the null-vector solves (dslash.h applyFineBlockM), twisted clover with its dense
  // site matrices A + i a g5
  float *tmat[2] = {nullptr, nullptr};
  const size_t tmatBytes = (size_t)proto.VolumeCB() * 144 * sizeof(float);
  double a = 0.0;
  if (fine) {
    a = ty == QUDA_WILSON_DIRAC ? 0.0 : 2.0 * dg->Kappa() * (double)proto.TwistFlavor() * dg->Mu();
    if (ty == QUDA_TWISTED_CLOVER_DIRAC)
      for (int p = 0; p < 2; p++) { tmat[p] = (float *)poolDeviceMalloc(tmatBytes); cloverTwistDense(tmat[p], *dg->Clover(), p, a, false); }
  }
  auto apply = [&]() {
    if (fine) applyFineBlockM(out.v, in.v, nrhs, *dg->Gauge(), dg->Kappa(), a, tmat[0] ? tmat : nullptr);
    else applyCoarseBlock(out, in, dc->Links());
  };
  apply();
  double secs = 0;
  if (niter > 0) {
    hipEvent_t e0, e1;
    HIP_CHECK(hipEventCreate(&e0)); HIP_CHECK(hipEventCreate(&e1));
    HIP_CHECK(hipEventRecord(e0, computeStream()));
    for (int k = 0; k < niter; k++) apply();
    HIP_CHECK(hipEventRecord(e1, computeStream()));
    HIP_CHECK(hipEventSynchronize(e1));
    float ms = 0;
    HIP_CHECK(hipEventElapsedTime(&ms, e0, e1));
    HIP_CHECK(hipEventDestroy(e0)); HIP_CHECK(hipEventDestroy(e1));
    secs = 1e-3 * ms / niter;
  }
  blockUnpack(f, out);
  HIP_CHECK(hipStreamSynchronize(computeStream()));
  for (int p = 0; p < 2; p++) if (tmat[p]) poolDeviceFree(tmat[p], tmatBytes);
  for (int i = 0; i < nrhs; i++) {
    ColorSpinorField hout = hostView(*f[i], h_out + i * len);
    hout = *f[i];
    delete f[i];
  }
  return secs;
}
// seconds per application of the level's restrictor (what = 0) or prolongator (1), HIP events on the compute stream
double qudaAmdMultigridTimeTransfer(void *mg_instance, int level, int what, int niter) {
  MG *m = levelOf(mg_instance, level);
  const Transfer *T = m->getTransfer();
  if (!T) errorQuda("level %d has no transfer operator", level);
  ColorSpinorField *fine = T->createFineField(), *coarse = T->createCoarseField();
  blas::copy(*fine, *m->nullVectors()[0]);
  T->R(*coarse, *fine);
  T->P(*fine, *coarse);
  hipEvent_t e0, e1;
  HIP_CHECK(hipEventCreate(&e0)); HIP_CHECK(hipEventCreate(&e1));
  HIP_CHECK(hipEventRecord(e0, computeStream()));
  for (int k = 0; k < niter; k++) { if (what) T->P(*fine, *coarse); else T->R(*coarse, *fine); }
  HIP_CHECK(hipEventRecord(e1, computeStream()));
  HIP_CHECK(hipEventSynchronize(e1));
  float ms = 0;
  HIP_CHECK(hipEventElapsedTime(&ms, e0, e1));
  HIP_CHECK(hipEventDestroy(e0)); HIP_CHECK(hipEventDestroy(e1));
  delete fine; delete coarse;
  return 1e-3 * ms / niter;
}
// the single-right-hand-side coarse operator of the same level, timed the same way (seconds per application)
double qudaAmdMultigridTimeApply(void *mg_instance, int level, int niter) {
  MG *m = levelOf(mg_instance, level);
  const ColorSpinorField &proto = *m->nullVectors()[0];
  ColorSpinorParam p = proto.param(); p.create = QUDA_ZERO_FIELD_CREATE;
  ColorSpinorField a(p), b(p);
  blas::copy(a, proto);
  a.twistFlavor = b.twistFlavor = proto.twistFlavor;
  m->residualMatrix()(b, a);
  hipEvent_t e0, e1;
  HIP_CHECK(hipEventCreate(&e0)); HIP_CHECK(hipEventCreate(&e1));
  HIP_CHECK(hipEventRecord(e0, computeStream()));
  for (int k = 0; k < niter; k++) m->residualMatrix()(b, a);
  HIP_CHECK(hipEventRecord(e1, computeStream()));
  HIP_CHECK(hipEventSynchronize(e1));
  float ms = 0;
  HIP_CHECK(hipEventElapsedTime(&ms, e0, e1));
  HIP_CHECK(hipEventDestroy(e0)); HIP_CHECK(hipEventDestroy(e1));
  return 1e-3 * ms / niter;
}

}

// ---- the even-odd preconditioned coarse operator piece by piece (quda_amd_ext.h; tests/test_coarse_pc_gpu.py) ----
// device layout of a link set (coarse.h): [site][matrix][column pair][row] float4 <-> host [site][matrix][row][col] complex
static size_t linkWord(int n, size_t A, int m, int r, int c) { return ((((size_t)A * 9 + m) * (n / 2) + c / 2) * n + r) * 4 + (c & 1) * 2; }

static const DiracCoarse *coarseOperatorOf(void *mg_instance, int level) {
  const DiracCoarse *D = levelOf(mg_instance, level)->getCoarseDirac();
  if (!D) errorQuda("level %d has no coarse operator below it", level);
  return D;
}
// host vectors travel as full fields; a parity half is the contiguous range [parity * half, (parity + 1) * half) of one
static void loadFull(ColorSpinorField &d, const float *h) { d = hostView(d, const_cast<float *>(h)); }
static void saveFull(float *h, const ColorSpinorField &d) { ColorSpinorField v = hostView(d, h); v = d; }
static void loadHalf(ColorSpinorField &d, const float *h_half, int parity, size_t half) {
  std::vector<float> full(2 * half, 0.f);
  memcpy(full.data() + parity * half, h_half, half * sizeof(float));
  loadFull(d, full.data());
}
static ColorSpinorField &parityOf(ColorSpinorField &f, int parity) { return parity ? f.Odd() : f.Even(); }

extern "C" {

void qudaAmdMultigridGetCoarseSiteLinks(void *mg_instance, int level, int which, float *h_out) {
  const DiracCoarse *D = coarseOperatorOf(mg_instance, level);
  if (which < 0 || which > 3) errorQuda("link set %d (0 links, 1 preconditioned links, 2 / 3 their fp16 mirrors)", which);
  const CoarseGauge &G = (which & 1) ? D->HatLinks() : D->Links();
  const int n = G.n;
  const size_t words = G.bytes / sizeof(float);
  std::vector<float> g(words);
  HIP_CHECK(hipStreamSynchronize(computeStream()));
  if (which < 2) {
    HIP_CHECK(hipMemcpy(g.data(), G.data, G.bytes, hipMemcpyDeviceToHost));
  } else {
    if (!G.data_h) errorQuda("the %s have no fp16 mirror (qudaAmdMultigridSetHalfStorage makes it)", (which & 1) ? "preconditioned links" : "links");
    std::vector<_Float16> h(words);
    HIP_CHECK(hipMemcpy(h.data(), G.data_h, words * sizeof(_Float16), hipMemcpyDeviceToHost));
    for (size_t i = 0; i < words; i++) g[i] = (float)h[i];
  }
  for (size_t A = 0; A < (size_t)G.nSites; A++)
    for (int m = 0; m < 9; m++)
      for (int r = 0; r < n; r++)
        for (int c = 0; c < n; c++) {
          const float *w = &g[linkWord(n, A, m, r, c)];
          float *o = h_out + ((((size_t)A * 9 + m) * n + r) * n + c) * 2;
          o[0] = w[0]; o[1] = w[1];
        }
}

int qudaAmdMultigridCoarseApply(void *mg_instance, int level, int which, int mmask, int parity, float *h_out, const float *h_in) {
  const DiracCoarse *D = coarseOperatorOf(mg_instance, level);
  const Transfer *T = levelOf(mg_instance, level)->getTransfer();
  if (which < 0 || which > 1) errorQuda("link set %d (0 links, 1 preconditioned links)", which);
  if (parity < -1 || parity > 1) errorQuda("parity %d (-1: full fields, 0 / 1)", parity);
  if (mmask <= 0 || mmask > 0x1ff) errorQuda("matrix mask 0x%x", mmask);
  const CoarseGauge &G = which ? D->HatLinks() : D->Links();
  ColorSpinorField *in = T->createCoarseField(), *out = T->createCoarseField();
  const size_t half = (size_t)G.nSites / 2 * G.n * 2;
  const int inPar = parity < 0 ? -1 : (mmask == (1 << 8) ? parity : 1 - parity);   // the local term reads its own parity, hops the other one
  std::vector<float> full(2 * half);
  if (parity < 0) {
    loadFull(*in, h_in);
    applyCoarse(*out, *in, G, mmask, -1);
    saveFull(h_out, *out);
  } else {
    loadHalf(*in, h_in, inPar, half);
    applyCoarse(parityOf(*out, parity), parityOf(*in, inPar), G, mmask, parity);
    saveFull(full.data(), *out);
    memcpy(h_out, full.data() + parity * half, half * sizeof(float));
  }
  // the input as the device holds it afterwards against what was loaded, word by word
  saveFull(full.data(), *in);
  int changed = 0;
  for (size_t i = 0; i < 2 * half; i++) {
    const bool loaded = inPar < 0 || (int)(i / half) == inPar;
    const float was = loaded ? h_in[inPar < 0 ? i : i - inPar * half] : 0.f;
    changed += memcmp(&was, &full[i], sizeof(float)) != 0;
  }
  delete in; delete out;
  return changed;
}

int qudaAmdMultigridCoarsePC(void *mg_instance, int level, int impl, int op, int parity, int nrhs, float *h_out, const float *h_in) {
  MG *fineLevel = levelOf(mg_instance, level);
  const DiracCoarse *D = coarseOperatorOf(mg_instance, level);
  const Transfer *T = fineLevel->getTransfer();
  if (impl < 0 || impl > 1 || op < 0 || op > 2 || parity < 0 || parity > 1) errorQuda("impl %d (0, 1), op %d (0..2), matpc parity %d (0, 1)", impl, op, parity);
  if (impl == 0 && nrhs != 1) errorQuda("DiracCoarsePC works on one vector, not %d", nrhs);
  const size_t half = (size_t)D->Links().nSites / 2 * D->Links().n * 2, full = 2 * half;
  std::vector<ColorSpinorField *> x(nrhs), b(nrhs), out(nrhs);
  for (int i = 0; i < nrhs; i++) {
    x[i] = T->createCoarseField(); b[i] = T->createCoarseField(); out[i] = T->createCoarseField();
    if (op == 0) loadHalf(*x[i], h_in + i * half, parity, half);
    if (op == 1) loadFull(*b[i], h_in + i * full);
    if (op == 2) { loadHalf(*x[i], h_in + i * half, parity, half); loadFull(*b[i], h_in + nrhs * half + i * full); }
  }
  int leaked = 0;
  if (impl == 1) {
    leaked = blockCoarseSchurPiece(D->Links(), D->HatLinks(), parity, op, nrhs, out, x, b);
  } else {
    // the level's own smoother operator where it is preconditioned on this parity, else one made for the call that shares the links
    const QudaMatPCType want = parity ? QUDA_MATPC_ODD_ODD : QUDA_MATPC_EVEN_EVEN;
    const MG *coarseLevel = fineLevel->getCoarse();
    const DiracCoarsePC *pc = coarseLevel ? dynamic_cast<const DiracCoarsePC *>(coarseLevel->params().matSmooth.Expose()) : nullptr;
    DiracCoarsePC *mine = nullptr;
    if (!pc || pc->getMatPCType() != want) {
      DiracParam dp;
      dp.type = QUDA_COARSEPC_DIRAC;
      dp.kappa = 1.0;
      dp.dagger = QUDA_DAG_NO;
      dp.matpcType = want;
      pc = mine = new DiracCoarsePC(*D, dp);
    }
    if (op == 0) {
      pc->M(parityOf(*out[0], parity), parityOf(*x[0], parity));
    } else if (op == 1) {
      ColorSpinorField *src = nullptr, *sol = nullptr;
      pc->prepare(src, sol, *x[0], *b[0], QUDA_MAT_SOLUTION);
      if (sol != &parityOf(*x[0], parity)) errorQuda("prepare: the solution does not live on parity %d", parity);
      blas::copy(parityOf(*out[0], parity), *src);
    } else {
      pc->reconstruct(*x[0], *b[0], QUDA_MAT_SOLUTION);
      blas::copy(*out[0], *x[0]);
    }
    HIP_CHECK(hipStreamSynchronize(computeStream()));
    delete mine;
  }
  for (int i = 0; i < nrhs; i++) {
    saveFull(h_out + i * full, *out[i]);
    delete x[i]; delete b[i]; delete out[i];
  }
  return leaked;
}

void qudaAmdCoarseInvertSites(int n, int nsites, const float *h_X, float *h_Xinv, float *h_hat, const float *h_H, int *fail) {
  if (n < 2 || n > 64 || (n & 1) || nsites < 1) errorQuda("batched inverse of %d matrices of order %d (even, at most 64)", nsites, n);
  const int xc[4] = {nsites, 1, 1, 1};
  CoarseGauge G(xc, n), hat(xc, n);
  std::vector<float> g(G.bytes / sizeof(float), 0.f);
  for (size_t A = 0; A < (size_t)nsites; A++)
    for (int m = 0; m < 9; m++) {
      const float *src = m == 8 ? h_X + A * n * n * 2 : (h_H ? h_H + (A * 8 + m) * n * n * 2 : nullptr);
      if (!src) continue;
      for (int r = 0; r < n; r++)
        for (int c = 0; c < n; c++) { float *w = &g[linkWord(n, A, m, r, c)]; w[0] = src[((size_t)r * n + c) * 2]; w[1] = src[((size_t)r * n + c) * 2 + 1]; }
    }
  HIP_CHECK(hipMemcpyAsync(G.data, g.data(), G.bytes, hipMemcpyHostToDevice, computeStream()));
  const int f = coarseInvertHat(hat, G);
  if (fail) *fail = f;
  HIP_CHECK(hipMemcpy(g.data(), hat.data, hat.bytes, hipMemcpyDeviceToHost));
  for (size_t A = 0; A < (size_t)nsites; A++)
    for (int m = 0; m < 9; m++) {
      float *dst = m == 8 ? h_Xinv + A * n * n * 2 : (h_hat ? h_hat + (A * 8 + m) * n * n * 2 : nullptr);
      if (!dst) continue;
      for (int r = 0; r < n; r++)
        for (int c = 0; c < n; c++) { const float *w = &g[linkWord(n, A, m, r, c)]; dst[((size_t)r * n + c) * 2] = w[0]; dst[((size_t)r * n + c) * 2 + 1] = w[1]; }
    }
}

}
