// block_hooks.cpp — test hooks (quda_amd_ext.h qudaAmdBlock*) onto the multi-right-hand-side path: block fields free of any lattice,
// namespace blockblas by name, the minimal-residual updates with their sums as inputs, the four pack functions and one parity launch of the
// multi-right-hand-side fine stencil with its epilogue sums (include/block.h, include/dslash.h).  tests/test_block_kernels_gpu.py compares
// them with the longdouble references of tests/block_ref.py.  The same launch with dense clover-twist site matrices, and those matrices
// themselves: tests/test_fine_stencil_gpu.py against the fp64 reference of tests/fine_stencil_ref.py.
#include <hip/hip_runtime.h>

#include <cstring>
#include <vector>

#include "interface_internal.h"
#include "block.h"
#include "dslash.h"
#include "quda_amd_ext.h"

using namespace quda;

static BlockField &blk(void *p, const char *hook, const char *which) {
  if (!p) errorQuda("%s: operand %s is missing", hook, which);
  return *(BlockField *)p;
}
static size_t imageFloats(const BlockField &f) { return 2 * (f.elems() + (size_t)f.nGhost * f.ncomp * f.nrhs); }
static void complexArray(Complex *dst, const double *src, int n) {
  for (int i = 0; i < n; i++) dst[i] = src ? Complex(src[2 * i], src[2 * i + 1]) : Complex(0.0);
}

extern "C" {

void *qudaAmdBlockFieldCreate(int nSites, int ncomp, int nrhs, int nGhost) {
  if (nSites < 1 || ncomp < 1 || nGhost < 0) errorQuda("block field of %d sites x %d components, %d ghost panels", nSites, ncomp, nGhost);
  return new BlockField(nSites, ncomp, nrhs, nGhost);
}
void qudaAmdBlockFieldDestroy(void *f) {
  HIP_CHECK(hipStreamSynchronize(computeStream()));   // the buffer returns to the pool: nothing on the stream may still use it
  delete (BlockField *)f;
}
void qudaAmdBlockFieldLoad(void *f_, const float *h_src) {
  BlockField &f = blk(f_, __func__, "field");
  HIP_CHECK(hipMemcpyAsync(f.v, h_src, imageFloats(f) * sizeof(float), hipMemcpyHostToDevice, computeStream()));
  HIP_CHECK(hipStreamSynchronize(computeStream()));
}
void qudaAmdBlockFieldSave(const void *f_, float *h_dst) {
  const BlockField &f = blk(const_cast<void *>(f_), __func__, "field");
  HIP_CHECK(hipMemcpyAsync(h_dst, f.v, imageFloats(f) * sizeof(float), hipMemcpyDeviceToHost, computeStream()));
  HIP_CHECK(hipStreamSynchronize(computeStream()));
}

int qudaAmdBlockBlasApply(const char *op, const double *a_, const double *b_, const double *c_, void *x_, void *y_, void *z_, void *w_, void *u_, double *res) {
  auto is = [&](const char *name) { return !strcmp(op, name); };
  auto X = [&]() -> BlockField & { return blk(x_, op, "x"); };
  auto Y = [&]() -> BlockField & { return blk(y_, op, "y"); };
  auto Z = [&]() -> BlockField & { return blk(z_, op, "z"); };
  auto W = [&]() -> BlockField & { return blk(w_, op, "w"); };
  auto U = [&]() -> BlockField & { return blk(u_, op, "u"); };
  const int n = X().nrhs;
  Complex a[kMaxBlockRhs], b[kMaxBlockRhs], c[kMaxBlockRhs], d0[kMaxBlockRhs], d1[kMaxBlockRhs], d2[kMaxBlockRhs];
  double r0[kMaxBlockRhs];
  complexArray(a, a_, n); complexArray(b, b_, n); complexArray(c, c_, n);
  auto put = [&](int k, const Complex *v) { for (int i = 0; i < n; i++) { res[k * n + i] = v[i].real(); res[(k + 1) * n + i] = v[i].imag(); } };
  auto putReal = [&](int k, const double *v) { for (int i = 0; i < n; i++) res[k * n + i] = v[i]; };
  if (is("norm2")) { blockblas::norm2(r0, X()); putReal(0, r0); return 1; }
  if (is("cDot")) { blockblas::cDot(d0, X(), Y()); put(0, d0); return 2; }
  if (is("caxpy")) { blockblas::caxpy(a, X(), Y()); return 0; }
  if (is("cDotNormA")) { blockblas::cDotNormA(d0, r0, X(), Y()); put(0, d0); putReal(2, r0); return 3; }
  if (is("bicgstabUpdate")) { blockblas::bicgstabUpdate(d0, r0, a, X(), b, Y(), Z(), W(), U()); put(0, d0); putReal(2, r0); return 3; }
  if (is("cxpaypbz")) { blockblas::cxpaypbz(X(), a, Y(), b, Z()); return 0; }
  if (is("bicgstabDots")) { blockblas::bicgstabDots(d0, r0, d1, d2, X(), Y(), U()); put(0, d0); putReal(2, r0); put(3, d1); put(5, d2); return 7; }
  if (is("bicgstabFused")) { blockblas::bicgstabFused(r0, a, b, c, X(), Y(), Z(), W(), U()); putReal(0, r0); return 1; }
  if (is("xmy")) { blockblas::xmy(X(), Y()); return 0; }
  if (is("negate")) { blockblas::negate(X()); return 0; }
  if (is("copy")) { blockblas::copy(Y(), X()); return 0; }
  if (is("zero")) { blockblas::zero(X()); return 0; }
  errorQuda("qudaAmdBlockBlasApply: unknown operation %s", op);
  return -1;
}

void qudaAmdBlockMrUpdate(int steps, double omega, int fresh, int needResidual, const double *s3, const double *s7, void *x_, void *r_, void *rin_, void *w1_, void *w2_) {
  if (steps != 1 && steps != 2) errorQuda("qudaAmdBlockMrUpdate: %d steps (1 or 2)", steps);
  BlockField &x = blk(x_, __func__, "x"), &r = blk(r_, __func__, "r"), &rin = blk(rin_, __func__, "rin"), &w1 = blk(w1_, __func__, "w1");
  const int n = x.nrhs;
  if (!s3 || (steps == 2 && !s7)) errorQuda("qudaAmdBlockMrUpdate: sums missing");
  double *d = nullptr;
  HIP_CHECK(qaMalloc(&d, (size_t)10 * kMaxBlockRhs * sizeof(double)));
  HIP_CHECK(hipMemcpyAsync(d, s3, (size_t)3 * n * sizeof(double), hipMemcpyHostToDevice, computeStream()));
  if (steps == 2) HIP_CHECK(hipMemcpyAsync(d + 3 * kMaxBlockRhs, s7, (size_t)7 * n * sizeof(double), hipMemcpyHostToDevice, computeStream()));
  if (steps == 1) blockblas::mrUpdateDev(x, r, rin, w1, d, omega, fresh != 0, needResidual != 0);
  else blockblas::mr2UpdateDev(x, r, rin, w1, blk(w2_, __func__, "w2"), d, d + 3 * kMaxBlockRhs, omega, fresh != 0, needResidual != 0);
  HIP_CHECK(hipStreamSynchronize(computeStream()));
  HIP_CHECK(hipFree(d));
}

static std::vector<ColorSpinorField *> spinorList(void *f[], int n) {
  std::vector<ColorSpinorField *> v(n > 0 ? n : 0);
  for (int i = 0; i < n; i++) v[i] = (ColorSpinorField *)f[i];
  return v;
}
void qudaAmdBlockPack(void *block, void *spinors[], int n, int parity) { blockPack(blk(block, __func__, "block"), spinorList(spinors, n), parity); }
void qudaAmdBlockUnpack(void *block, void *spinors[], int n, int parity) { blockUnpack(spinorList(spinors, n), blk(block, __func__, "block"), parity); }
void qudaAmdBlockPackParity(void *block, void *spinors[], int n, int accumulate) {
  const std::vector<ColorSpinorField *> v = spinorList(spinors, n);
  blockPackParity(blk(block, __func__, "block"), v.data(), n, accumulate != 0);
}
void qudaAmdBlockUnpackParity(void *block, void *spinors[], int n) {
  const std::vector<ColorSpinorField *> v = spinorList(spinors, n);
  blockUnpackParity(v.data(), n, blk(block, __func__, "block"));
}

int qudaAmdBlockGhostPanels(int parityField) {
  if (!gaugePrecise) errorQuda("load a gauge field first (it defines the local lattice)");
  return blockGhost(gaugePrecise->geom.X, parityField != 0).nGhost;
}

void qudaAmdBlockFineApply(void *out_, void *in_same_, void *in_other_, void *dotA_, int parity, double s0, double a0, double k1, double a1, int mode, int deviceSums, double *sums) {
  if (!gaugePrecise) errorQuda("load a gauge field first");
  const GaugeField &U = *gaugePrecise;
  BlockField &out = blk(out_, __func__, "out"), &other = blk(in_other_, __func__, "in_other");
  BlockField *same = (BlockField *)in_same_, *dotA = (BlockField *)dotA_;
  const int n = out.nrhs, Vh = U.geom.Vh;
  for (const BlockField *f : {(const BlockField *)&out, (const BlockField *)&other, (const BlockField *)same, (const BlockField *)dotA})
    if (f && (f->nSites != Vh || f->ncomp != 12 || f->nrhs != n)) errorQuda("qudaAmdBlockFineApply: single-parity fields of %d sites x 12 components x %d right-hand sides", Vh, n);
  if (out.v == other.v || (same && out.v == same->v)) errorQuda("qudaAmdBlockFineApply: out must not alias an input");
  const BlockGhost gh = blockGhost(U.geom.X, true);
  if (gh.mask && other.nGhost < gh.nGhost) errorQuda("qudaAmdBlockFineApply: in_other has %d ghost panels, %d needed", other.nGhost, gh.nGhost);
  if (mode && mode != 3 && !dotA) errorQuda("qudaAmdBlockFineApply: mode %d needs dotA", mode);
  const FineBlockDots dots = {dotA ? dotA->v : nullptr, mode};
  applyFineBlockParity(out.v, same ? same->v : nullptr, other.v, n, U, parity, s0, a0, k1, a1, nullptr, 0, gh.mask ? other.v + other.elems() : nullptr, mode ? &dots : nullptr);
  if (!mode) { HIP_CHECK(hipStreamSynchronize(computeStream())); return; }
  const int nval = (mode == 1 ? 2 : (mode == 3 ? 3 : 7)) * n;
  if (!deviceSums) { fineBlockDotsFinish(sums, n, mode); return; }
  double *d = nullptr;
  HIP_CHECK(qaMalloc(&d, (size_t)nval * sizeof(double)));
  fineBlockDotsFinishDev(d, n, mode);
  HIP_CHECK(hipMemcpyAsync(sums, d, (size_t)nval * sizeof(double), hipMemcpyDeviceToHost, computeStream()));
  HIP_CHECK(hipStreamSynchronize(computeStream()));
  HIP_CHECK(hipFree(d));
}

static const CloverField &denseSource(const char *hook) {
  if (!cloverPrecise) errorQuda("%s: load a clover field first", hook);
  if (cloverPrecise->precision != QUDA_SINGLE_PRECISION) errorQuda("%s: the resident clover field must be fp32 (clover_cuda_prec = 4)", hook);
  return *cloverPrecise;
}
static size_t denseFloats(const CloverField &C) { return (size_t)C.geom.Vh * 2 * 72; }

void qudaAmdCloverTwistDense(int parity, double a, int inverse, float *h_out) {
  const CloverField &C = denseSource(__func__);
  if (parity != 0 && parity != 1) errorQuda("qudaAmdCloverTwistDense: parity %d", parity);
  float *d = nullptr;
  HIP_CHECK(qaMalloc(&d, denseFloats(C) * sizeof(float)));
  cloverTwistDense(d, C, parity, a, inverse != 0);
  HIP_CHECK(hipMemcpyAsync(h_out, d, denseFloats(C) * sizeof(float), hipMemcpyDeviceToHost, computeStream()));
  HIP_CHECK(hipStreamSynchronize(computeStream()));
  HIP_CHECK(hipFree(d));
}

int qudaAmdBlockFineApplySite(void *out_, void *in_same_, void *in_other_, int parity, double s0, double a0, double k1, double a1, int tmode, double a, int inverse) {
  if (!gaugePrecise) errorQuda("load a gauge field first");
  const GaugeField &U = *gaugePrecise;
  BlockField &out = blk(out_, __func__, "out"), &other = blk(in_other_, __func__, "in_other");
  BlockField *same = (BlockField *)in_same_;
  const int n = out.nrhs, Vh = U.geom.Vh;
  for (const BlockField *f : {(const BlockField *)&out, (const BlockField *)&other, (const BlockField *)same})
    if (f && (f->nSites != Vh || f->ncomp != 12 || f->nrhs != n)) errorQuda("qudaAmdBlockFineApplySite: single-parity fields of %d sites x 12 components x %d right-hand sides", Vh, n);
  if (out.v == other.v || (same && out.v == same->v)) errorQuda("qudaAmdBlockFineApplySite: out must not alias an input");
  if (tmode < 0 || tmode > 2) errorQuda("qudaAmdBlockFineApplySite: site-matrix mode %d (0 none, 1 on the hop sum, 2 on in_same)", tmode);
  const BlockGhost gh = blockGhost(U.geom.X, true);
  if (gh.mask && other.nGhost < gh.nGhost) errorQuda("qudaAmdBlockFineApplySite: in_other has %d ghost panels, %d needed", other.nGhost, gh.nGhost);
  float *tmat = nullptr;
  if (tmode) {
    const CloverField &C = denseSource(__func__);
    if (C.geom.Vh != Vh) errorQuda("qudaAmdBlockFineApplySite: clover field of %d sites per parity, links of %d", C.geom.Vh, Vh);
    HIP_CHECK(qaMalloc(&tmat, denseFloats(C) * sizeof(float)));
    cloverTwistDense(tmat, C, parity, a, inverse != 0);
  }
  applyFineBlockParity(out.v, same ? same->v : nullptr, other.v, n, U, parity, s0, a0, k1, a1, tmat, tmode, gh.mask ? other.v + other.elems() : nullptr);
  HIP_CHECK(hipStreamSynchronize(computeStream()));
  if (tmat) HIP_CHECK(hipFree(tmat));
  return fineBlockOrderTiled(U.geom, n) ? 1 : 0;
}

}  // extern "C"
