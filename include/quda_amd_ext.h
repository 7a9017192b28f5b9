/*
 * quda_amd_ext.h — C-ABI handles onto the C++ surface of the library (resident fields and operator
 * objects), for callers that cannot bind C++ classes (ctypes / cgo / JNI style FFI) and for the
 * benchmark, which — like the reference's tests/dslash_test.cpp with transfer=0 (:455-616) — times
 * Dirac::Dslash on fields that stay in HBM.
 *
 * Each function is a thin wrapper over the C++ method it cites:
 *   qudaAmdSpinor*      -> cudaColorSpinorField ctor / operator= (reference include/color_spinor_field.h:458-640,
 *                          lib/cuda_color_spinor_field.cu:513-590)
 *   qudaAmdDirac*       -> Dirac::create, Dslash, DslashXpay, M, Mdag, MdagM, prepare/reconstruct
 *                          (reference include/dirac_quda.h:88-164, :449-617; lib/interface_quda.cpp:1265, :1386)
 *   qudaAmdBlas*        -> blas::norm2 / cDotProduct / axpy (reference include/blas_quda.h:33-144)
 * Plain pointers and PODs only; errors follow quda.h (message + exit(1)).
 */
#ifndef QUDA_AMD_EXT_H
#define QUDA_AMD_EXT_H

#include <stddef.h>
#include "quda.h"

#ifdef __cplusplus
extern "C" {
#endif

/* device-resident spinor field on the local lattice loaded by loadGaugeQuda.
 * site_subset: QUDA_PARITY_SITE_SUBSET (1) or QUDA_FULL_SITE_SUBSET (2). */
void *qudaAmdSpinorCreate(QudaPrecision prec, QudaSiteSubset site_subset, QudaTwistFlavorType flavor);
void qudaAmdSpinorDestroy(void *field);
/* host <-> device with reorder, precision and gamma-basis change; host layout described by inv_param
 * (cpu_prec, dirac_order, gamma_basis) exactly as for dslashQuda */
void qudaAmdSpinorLoad(void *field, const void *h_src, const QudaInvertParam *inv_param);
void qudaAmdSpinorSave(const void *field, void *h_dst, const QudaInvertParam *inv_param);
void qudaAmdSpinorCopy(void *dst, const void *src);   /* device-device, any precision pair */
void qudaAmdSpinorSetTwist(void *field, QudaTwistFlavorType flavor);
/* flavour mixing of the non-degenerate twisted-mass doublet on resident doublet fields (created with QUDA_TWIST_NONDEG_DOUBLET: two flavours,
   [flavour 1][flavour 2] per parity); out may be in.  direct: 1 + i a g5 tau3 + b tau1 with a = 2 kappa mu, b = -2 kappa epsilon; inverse != 0:
   its inverse; dagger != 0 flips the sign of a */
void qudaAmdNdegTwist(void *out, const void *in, double kappa, double mu, double epsilon, int dagger, int inverse);

/* operator object built from the resident gauge/clover fields.
 * pc != 0: even-odd preconditioned type (Dirac::create of *PC_DIRAC); which: 0 precise, 1 sloppy, 2 precondition */
void *qudaAmdDiracCreate(QudaInvertParam *inv_param, int pc, int which);
void qudaAmdDiracDestroy(void *dirac);
void qudaAmdDiracDslash(void *dirac, void *out, const void *in, QudaParity parity);
void qudaAmdDiracDslashXpay(void *dirac, void *out, const void *in, QudaParity parity, const void *x, double k);
void qudaAmdDiracM(void *dirac, void *out, const void *in);
void qudaAmdDiracMdag(void *dirac, void *out, const void *in);
void qudaAmdDiracMdagM(void *dirac, void *out, const void *in);
unsigned long long qudaAmdDiracFlops(void *dirac);
/* Dirac::prepare / reconstruct (include/dirac_quda.h:152-164) on resident FULL fields x, b: prepare leaves the source of the
 * preconditioned system in src_out (a parity field; a full field for un-preconditioned operators), reconstruct completes x */
void qudaAmdDiracPrepare(void *dirac, void *src_out, void *x, void *b, QudaSolutionType solution_type);
void qudaAmdDiracReconstruct(void *dirac, void *x, const void *b, QudaSolutionType solution_type);

/* niter back-to-back Dslash applications bracketed by device events on the compute stream;
 * returns seconds per application (reference tests/dslash_test.cpp:455-616). */
double qudaAmdTimeDslash(void *dirac, void *out, const void *in, QudaParity parity, int niter);
double qudaAmdTimeM(void *dirac, void *out, const void *in, int niter);

double qudaAmdBlasNorm2(const void *field);
void qudaAmdBlasCDot(const void *x, const void *y, double result[2]);
void qudaAmdBlasAxpy(double a, const void *x, void *y);
double qudaAmdTimeAxpy(double a, const void *x, void *y, int niter);   /* seconds per y += a x, device-event timed */
/* the fused sweeps of CG and multi-shift CG (include/blas.h) on qudaAmdSpinor handles of one precision and geometry:
 *   AxpyCGNorm          y += a x ; result = (|y|^2, (y_new, y_new - y_old))
 *   AxpyZpbx            y += a x ; x = z + b x
 *   TripleCGReduction   result = (|x|^2, |y|^2, (y, z))
 *   AxpyReDot           y += a x ; returns (x, y)
 *   MultiShiftUpdate    x[i] += alpha[i] p[i] ; p[i] = zeta[i] r + beta[i] p[i] for i < k, r read once per sweep of at most
 *                       qudaAmdBlasMultiShiftChunk() shifts */
void qudaAmdBlasAxpyCGNorm(double a, const void *x, void *y, double result[2]);
void qudaAmdBlasAxpyZpbx(double a, void *x, void *y, const void *z, double b);
void qudaAmdBlasTripleCGReduction(const void *x, const void *y, const void *z, double result[3]);
double qudaAmdBlasAxpyReDot(double a, const void *x, void *y);
void qudaAmdBlasMultiShiftUpdate(int k, void *x[], void *p[], const void *r, const double *alpha, const double *beta, const double *zeta);
int qudaAmdBlasMultiShiftChunk(void);
/* test hooks onto the rest of namespace blas (include/blas.h), all on qudaAmdSpinor handles of one precision and geometry.
 * qudaAmdBlasApply calls the function named op (its name in blas.h: "caxpyXmazNormX", ...) on the operands it takes (the others may be
 * null), writes the sums it returns to result — a dot product as (re, im), the NormA / NormB forms as (re, im, norm) — and returns
 * their number.  coeff: a complex a is (coeff[0], coeff[1]) and a complex b (coeff[2], coeff[3]); two real coefficients a, b (axpby) are
 * coeff[0], coeff[1]; cabxpyAx / cabxpyAxNorm take the real a from coeff[0] and the complex b from (coeff[2], coeff[3]).  Operands are
 * named as in blas.h; the operations are norm2, reDotProduct, cDotProduct, cDotProductNormA, cDotProductNormB, ax, axpy, xpy, xpay, mxpy,
 * axpby, xmyNorm, axpyNorm, caxpy, caxpby, xmyz, cxpaypbz, caxpyNorm, caxpyXmaz, caxpyXmazNormX, caxXmaz, caxInit, cabxpyAx,
 * cabxpyAxNorm, caxpyDotzy, caxpbypzYmbw */
int qudaAmdBlasApply(const char *op, const double coeff[4], void *x, void *y, void *z, void *w, double result[3]);
/* the device-scalar sequence of the MR smoother: cDotProductNormADev(p, q) immediately followed by the update named op — "caxpyXmazDev",
 * "caxXmazDev" (x, y, z) or "caxInitDev" (x, y, z, w) — which takes alpha = omega (p, q) / |p|^2 from device memory (0 where |p|^2 = 0) */
void qudaAmdBlasDevUpdate(const char *op, double omega, const void *p, const void *q, void *x, void *y, void *z, void *w);
/* the multi-field kernels of the blocked GCR orthogonalisation, k fields f[i]; complex arrays as (re, im) pairs:
 *   MultiSupported       1 if k fields of field's precision can go through them
 *   MultiDot             beta[i] = (f_i, y) for i < k, yr = (y, r), *ynorm = |y|^2
 *   MultiCaxpyResidual   y <- scale (y + sum_i c_i f_i) ; r <- r - a y ; sums = (|r|^2, |y|^2)
 *   MultiCaxpy           y <- y + sum_i c_i f_i */
int qudaAmdBlasMultiSupported(const void *field, int k);
void qudaAmdBlasMultiDot(int k, void *f[], const void *y, const void *r, double *beta, double yr[2], double *ynorm);
void qudaAmdBlasMultiCaxpyResidual(int k, void *f[], const double *c, double scale, void *y, const double a[2], void *r, double sums[2]);
void qudaAmdBlasMultiCaxpy(int k, void *f[], const double *c, void *y);
/* result = (|x|^2, |r|^2, mean over sites of |r(site)|^2 / |x(site)|^2, a site with x = 0 counting 1) */
void qudaAmdBlasHeavyQuarkResidualNorm(const void *x, const void *r, double result[3]);
/* ---- test hooks onto the multi-right-hand-side ("block") path (include/block.h, csrc/block_hooks.cpp) ----
 * A block field handle is a BlockField of nSites panels of ncomp x nrhs complex numbers (nrhs <= 32) plus nGhost ghost panels; it needs
 * no lattice.  Load / Save copy the raw device image, (nSites + nGhost) * ncomp * nrhs float2 in device order: rhs-fastest,
 * float2 index (site * ncomp + j) * nrhs + i, or for ncomp == 12 pair-major, ((site * 6 + j / 2) * nrhs + i) * 2 + j % 2 (block.h). */
void *qudaAmdBlockFieldCreate(int nSites, int ncomp, int nrhs, int nGhost);
void qudaAmdBlockFieldDestroy(void *field);
void qudaAmdBlockFieldLoad(void *field, const float *h_src);
void qudaAmdBlockFieldSave(const void *field, float *h_dst);
/* qudaAmdBlockBlasApply calls the function of namespace blockblas named op (its name in block.h) on block field handles of one shape.
 * a, b, c: nrhs complex coefficients each as (re, im) pairs, or NULL.  The operands of block.h go to the slots x, y, z, w, u as follows
 * (slots an operation does not take may be NULL):
 *   norm2(x)  cDot(x, y)  caxpy(a; x, y)  xmy(x, y)  negate(x)  zero(x)  copy(dst = y, src = x)
 *   cDotNormA(t = x, r = y)
 *   bicgstabUpdate(alpha = a, omega = b; p = x, r = y, solution x = z, t = w, r0 = u)
 *   cxpaypbz(a, b; r = x, v = y, p = z)
 *   bicgstabDots(t = x, s = y, r0 = u)
 *   bicgstabFused(alpha = a, omega = b, beta = c; p = x, r = y, solution x = z, t = w, v = u)
 * result[k * nrhs + i] is sum k of right-hand side i in the order block.h lists them, a complex one as two sums (re, im): cDot 2, cDotNormA 3
 * (dot, norm), bicgstabUpdate 3 (rho, r2), bicgstabDots 7 (ts, tt, r0s, r0t), norm2 and bicgstabFused 1.  Returns the sums per right-hand side. */
int qudaAmdBlockBlasApply(const char *op, const double *a, const double *b, const double *c, void *x, void *y, void *z, void *w, void *u, double *result);
/* the minimal-residual updates with their sums as INPUTS: s3[3 nrhs] = [Re (w1, r) | Im (w1, r) | |w1|^2] and, for steps = 2,
 * s7[7 nrhs] = [Re, Im (w2, w1) | |w2|^2 | Re, Im (r, w1) | Re, Im (r, w2)] are copied to device memory, then steps = 1 calls
 * blockblas::mrUpdateDev(x, r, rin, Ar = w1) and steps = 2 blockblas::mr2UpdateDev(x, r, rin, w1, w2) (12-component fields, 4 or 8 right-hand sides) */
void qudaAmdBlockMrUpdate(int steps, double omega, int fresh, int needResidual, const double *s3, const double *s7, void *x, void *r, void *rin, void *w1, void *w2);
/* blockPack / blockUnpack between n >= nrhs full fp32 qudaAmdSpinor fields and a block (parity -1: both halves, nSites = volume; 0 / 1: that
 * half, nSites = volumeCB), and blockPackParity / blockUnpackParity between n <= nrhs single-parity fp32 fields and a 12-component block of
 * volumeCB sites: a NULL entry is a column of zeros on pack and is left alone on unpack; accumulate != 0: block += fields */
void qudaAmdBlockPack(void *block, void *spinors[], int n, int parity);
void qudaAmdBlockUnpack(void *block, void *spinors[], int n, int parity);
void qudaAmdBlockPackParity(void *block, void *spinors[], int n, int accumulate);
void qudaAmdBlockUnpackParity(void *block, void *spinors[], int n);
/* ghost panels a block field needs behind its local ones to be the hop input of the fine stencil under the current partition:
 * blockGhost(X, parityField).nGhost of the resident lattice (0 on an unpartitioned one) */
int qudaAmdBlockGhostPanels(int parityField);
/* one launch of applyFineBlockParity on the resident precise links (fp32: cuda_prec = 4), single-parity 12-component block fields:
 * out = s0 (1 + i a0 g5) in_same + k1 (1 + i a1 g5) [8 hops of in_other] on the sites of `parity`; in_same may be NULL with s0 = 0; on a
 * partitioned lattice in_other must carry qudaAmdBlockGhostPanels(1) ghost panels (they are filled here).  mode 0: no inner products.
 * mode 1, 2, 3 (dslash.h FineBlockDots, a = dotA; NULL for mode 3): the epilogue sums, finished by fineBlockDotsFinish (deviceSums = 0) or
 * by fineBlockDotsFinishDev into device memory and copied back (deviceSums != 0), in sums[k * nrhs + i] */
void qudaAmdBlockFineApply(void *out, void *in_same, void *in_other, void *dotA, int parity, double s0, double a0, double k1, double a1, int mode, int deviceSums, double *sums);
/* cloverTwistDense on the resident precise clover field (fp32: clover_cuda_prec = 4): the dense site matrices A + i a s (s = +1 upper, -1
 * lower chirality) of one parity, or their inverses (inverse != 0), copied to h_out[site][chirality][6][6] complex fp32 */
void qudaAmdCloverTwistDense(int parity, double a, int inverse, float *h_out);
/* the same parity launch as qudaAmdBlockFineApply (no inner products) with the dense site matrices of the OUTPUT parity, built here by
 * cloverTwistDense(a, inverse) and freed after a stream synchronise: tmode 1 puts them on the hop sum in place of (1 + i a1 g5), tmode 2 on
 * in_same in place of (1 + i a0 g5), tmode 0 launches without them (a, inverse unused).  Ghost panels as for qudaAmdBlockFineApply.
 * Returns a flag word: bit 0 is set if the launch walked its work-groups in the XCD plane-tiled order (fineBlockOrderTiled), clear: linear */
int qudaAmdBlockFineApplySite(void *out, void *in_same, void *in_other, int parity, double s0, double a0, double k1, double a1, int tmode, double a, int inverse);
/* out = (M^dag M + shift) in through the DiracMdagM functor the solvers use; shift = 0 launches exactly what qudaAmdDiracMdagM does */
void qudaAmdDiracMdagMShift(void *dirac, void *out, const void *in, double shift);
/* device-event timed loops for tools/cg_timing.py, seconds per pass:
 *   TimeMdagM          out = M^dag M in
 *   TimeCGBlas         the vector work of ONE CG iteration on four fields; fused != 0: reDotProduct, axpyCGNorm, axpyZpbx (three sweeps);
 *                      fused == 0: the same update from reDotProduct, axpy, norm2, reDotProduct, axpy, xpay (the calls it replaces)
 *   TimeMultiShift     fused != 0: MultiShiftUpdate of k shifts; fused == 0: per shift axpy then axpby (the calls it replaces) */
double qudaAmdTimeMdagM(void *dirac, void *out, const void *in, int niter);
double qudaAmdTimeCGBlas(int fused, void *x, void *r, void *p, void *Ap, int niter);
double qudaAmdTimeMultiShift(int fused, int k, void *x[], void *p[], const void *r, int niter);

/* algorithmic work model of the stencil kernel behind Dirac::Dslash */
long long qudaAmdDslashBytesPerSite(QudaInvertParam *inv_param, int which, int xpay);
long long qudaAmdDslashFlopsPerSite(QudaInvertParam *inv_param, int xpay);

/* multigrid introspection: the reference's MG::verify() identities (lib/multigrid.cpp:372-486) and one preconditioner
 * application K b on host vectors (full fields, layout described by inv_param as for MatQuda) */
void qudaAmdMultigridVerify(void *mg_instance, double dev[3]);
void qudaAmdMultigridCycle(void *mg_instance, void *h_x, void *h_b, QudaInvertParam *inv_param);

/* Read-only access to a hierarchy built by newMultigridQuda — what a C++ test of the reference reaches through
 * multigrid_solver->mg (include/multigrid.h:108-330: B, transfer, diracCoarse).  Host layouts are the reference's CPU
 * orders, fp32: vectors site-major (parity*Vh + x_cb, spin, colour, re/im), DeGrand-Rossi basis on level 0; V as
 * (site, spin, colour, vector) (lib/transfer_util.cu:15-36); coarse links as QDP-ordered
 * Y[dim 0-3 backward | 4-7 forward][site][row][col] and X[site][row][col] (lib/dslash_coarse.cu:50-64) with the
 * operator's -kappa already multiplied into Y.  `level` names the finer of the two levels a transfer connects. */
/* opt-in half-precision cycle: R, P and the coarse operators stream fp16 mirrors of the null-vector matrix V and of the
 * coarse links, and the level-0 even-odd smoother iterates in 16-bit storage (work fields + a 16-bit copy of the links made
 * on the device; twisted-mass / Wilson only).  Setup, verify, residuals, the accessors below and the outer solve keep their
 * precision.  The V / link switch is process-wide; `on` also creates the mirrors of this hierarchy.  Env QUDA_AMD_MG_HALF=1
 * does the same at newMultigridQuda. */
void qudaAmdMultigridSetHalfStorage(void *mg_instance, int on);
int qudaAmdMultigridLevels(void *mg_instance);
/* set-up refinement: every level-0 null vector is replaced by (one multigrid cycle)^cycles applied to it and the hierarchy is rebuilt, `passes`
 * times (an inverse iteration through the hierarchy; for problems at a critical kappa, where the first BiCGstab set-up stops at its cap).
 * The QudaMultigridParam the hierarchy was created from need not be alive any more.  Returns the seconds spent. */
double qudaAmdMultigridRefine(void *mg_instance, int passes, int cycles);
int qudaAmdMultigridOrthoFallbackBlocks(void *mg_instance, int level); /* blocks the fp32 CholeskyQR2 block orthonormalisation handed to Gram-Schmidt (ill-conditioned) */
void qudaAmdMultigridLevelInfo(void *mg_instance, int level, int info[18]); /* Xf[4] Xc[4] fineSpin fineColor Nvec geo_bs[4] spin_bs null_vector_method (0 sequential solves / loaded, 1 lockstep on the multi-rhs fine stencil, 2 lockstep on the MFMA coarse operator) lockstep_iterations */
void qudaAmdMultigridGetNullVector(void *mg_instance, int level, int k, float *h_out);
void qudaAmdMultigridGetV(void *mg_instance, int level, float *h_out);
void qudaAmdMultigridGetCoarseLinks(void *mg_instance, int level, float *h_Y, float *h_X);
/* op 0: R (level -> level+1; lib/restrictor.cu), 1: P (level+1 -> level; lib/prolongator.cu), 2: M of `level`,
 * 3: one multigrid cycle of `level`, x = K b (MG::operator(), lib/multigrid.cpp:488-604) */
void qudaAmdMultigridApply(void *mg_instance, int level, int op, float *h_out, const float *h_in);
/* The transfer operators of `level` one by one, on host vectors in the layout of qudaAmdMultigridApply; several vectors lie back to back.
 * parity -1: full fine fields.  parity 0 / 1: Transfer::setSiteSubset(QUDA_PARITY_SITE_SUBSET, parity) for the call (the previous subset
 * is restored), single-parity fine fields: the other parity of a fine input is ignored, that of a fine result is reported as zeros.
 *   op 0  R        1 fine -> 1 coarse                     op 1  P        1 coarse -> 1 fine
 *   op 2  R4       4 fine -> 4 coarse                     op 3  P4       4 coarse -> 4 fine
 *   op 4  R4Block  4 fine -> 4 coarse; the sources go through blockPackParity into columns 4..7 of an 8-column parity block field whose
 *                  columns 0..3 hold the same sources in reverse order (parity >= 0 only)
 *   op 5  P4Block  accumulate = 0, op 6: accumulate = 1.  h_in: 4 coarse vectors, then the 8 fine vectors the 8-column parity block
 *                  field is preloaded with; the prolongation goes to columns 4..7; h_out: all 8 columns as fine vectors (parity >= 0 only) */
void qudaAmdMultigridApplyTransfer(void *mg_instance, int level, int op, int parity, float *h_out, const float *h_in);
/* The even-odd preconditioned coarse operator piece by piece (tests/test_coarse_pc_gpu.py against tests/coarse_ref.py).  `level` names the finer
 * level, as for qudaAmdMultigridGetCoarseLinks: the operator lives on level + 1.  Vectors in the layout of qudaAmdMultigridApply; a parity field
 * is the half [parity * Vh, (parity + 1) * Vh) of one; several vectors lie back to back.
 * GetCoarseSiteLinks: the nine matrices every coarse site multiplies with, in the device's own bidirectional meaning (include/coarse.h),
 *   h_out[site][m][row][col] complex fp32, m = 2 mu forward hop, 2 mu + 1 backward hop, 8 local.  which 0: the links (8 = X), 1: the
 *   preconditioned links Xinv H_d (8 = Xinv), 2 / 3: the same read back from the fp16 mirror and widened (an error if there is no mirror).
 *   GetCoarseLinks folds the backward links into the reference's dagger convention, which the preconditioned links do not obey.
 * CoarseApply: applyCoarse itself on the links (which 0) or the preconditioned links (1) with matrix mask mmask (bit m = matrix m).  parity -1:
 *   full fields.  parity 0 / 1: parity fields, h_out the half of that parity, h_in the half the call reads — the other parity for hops, the
 *   same parity for mmask == 1 << 8.  The fp16 mirror is read when half storage is on.  Returns the number of words of the device's input
 *   field (both parities) that differ afterwards from what was loaded: 0 unless the operator wrote into its input.
 * CoarsePC: the Schur pieces with matpc = parity on nrhs vectors.  op 0: Mhat, h_in nrhs parity fields; op 1: prepare for a MAT solution, h_in
 *   nrhs full sources b, the preconditioned source comes back on `parity`; op 2: reconstruct, h_in nrhs solved parity fields x then nrhs full b.
 *   h_out: nrhs FULL fields in every case (what the routine leaves on the other parity is part of the answer).  impl 0: DiracCoarsePC, nrhs = 1
 *   (the level's smoother operator where its matpc fits, else one made for the call that shares the links).  impl 1: BlockCoarseCycle::matpc /
 *   prepare / reconstruct of csrc/block_coarse_cycle.cpp on the MFMA kernel, nrhs in {8, 16, 24}, every work field preloaded with nonzero words on both
 *   parities.  Returns (impl 1) the nonzero words left in the half of matpc's temporary that its second application multiplies with Xinv,
 *   else 0.
 * qudaAmdCoarseInvertSites: coarse_invert_kernel and coarse_hat_kernel on matrices of the caller (no hierarchy): h_X[site][row][col], h_H[site]
 *   [d = 0..7][row][col] (NULL: zeros) -> h_Xinv, h_hat (NULL: not returned); *fail = the kernel's flag (1: an identically zero pivot column
 *   somewhere) where DiracCoarse::HatLinks stops with an error.  n even, at most 64. */
void qudaAmdMultigridGetCoarseSiteLinks(void *mg_instance, int level, int which, float *h_out);
int qudaAmdMultigridCoarseApply(void *mg_instance, int level, int which, int mmask, int parity, float *h_out, const float *h_in);
int qudaAmdMultigridCoarsePC(void *mg_instance, int level, int impl, int op, int parity, int nrhs, float *h_out, const float *h_in);
void qudaAmdCoarseInvertSites(int n, int nsites, const float *h_X, float *h_Xinv, float *h_hat, const float *h_H, int *fail);
/* The operator of a COARSE level applied to nrhs (8, 16, 24 or 32) host vectors at once through the multi-right-hand-side kernel
 * on the matrix cores (v_mfma_f32_16x16x4_f32; the reference's multi-source coarse Dslash, lib/dslash_coarse.cu:294-333): the
 * vectors lie back to back in h_in / h_out, each in the layout of qudaAmdMultigridApply.  niter > 0 additionally times niter
 * back-to-back applications with device events and returns the seconds per application (0 otherwise).
 * qudaAmdMultigridTimeApply times the single-vector operator of a level the same way. */
double qudaAmdMultigridApplyBlock(void *mg_instance, int level, int nrhs, float *h_out, const float *h_in, int niter);
/* errorQuda ends the process (reference convention, include/util_quda.h:51-61).  A caller holding finished results can leave a text
 * here that is written to stdout first, and the exit status to use; text = NULL restores the default (nothing, status 1). */
/* this process' transport counters since initQuda: fine-grid exchanges through peer stores / staged (RCCL), the same for the coarse
 * grids, global sums inside the reduction kernel / through the collective library, fall-backs to the staged transport, block exchanges */
void qudaAmdCommStats(long long out[8]);
/* text of the device error record of a halo wait that ran out (dimension, direction, buffer, exchange number, expected and last-seen
 * flag, interpretation); returns 0 if none is recorded */
int qudaAmdDescribeHaloError(char *text, int n);
/* profile post-processing: a one-wave marker dispatch (kernel qa_profile_marker_kernel) that brackets a region of the rocprofv3 kernel
 * trace, and the launch accounting — between Start and Dump every instrumented launch is recorded with its ALGORITHMIC bytes */
void qudaAmdProfileMarker(int id);
void qudaAmdAccountStart(void);
void qudaAmdAccountDump(const char *path);
/* Nvec colour-spinor fields in the SciDAC / QIO single-file container the reference's read_spinor_field / write_spinor_field use
 * (lib/qio_field.cpp:198-328; LIME records scidac-private-file-xml ... scidac-binary-data, scidac-checksum).  V[i]: host field of the local
 * lattice X[4], even-odd site order, 2 nSpin nColor reals per site in `precision`; the file holds fp32.  Every rank moves its own rows. */
void qudaAmdWriteSpinorFields(const char *filename, void *V[], QudaPrecision precision, const int *X, int nColor, int nSpin, int Nvec);
void qudaAmdReadSpinorFields(const char *filename, void *V[], QudaPrecision precision, const int *X, int nColor, int nSpin, int Nvec);
void qudaAmdSetExitLine(const char *text, int status);
double qudaAmdMultigridTimeApply(void *mg_instance, int level, int niter);
/* The cycle from a coarse level down (smoothers, residual, R, coarsest-grid GCR, P) as ONE persistent kernel (include/coarse_cycle.h) where
 * the sub-hierarchy qualifies; on by default (QUDA_AMD_MG_FUSED=0 / SetFused(0): the kernel-per-operation path).  FusedStats: returns 1 if
 * `level` owns such a kernel and fills out[] with the last launch's device-wide barriers, coarsest-grid GCR iterations, its restarts,
 * halo exchanges and the grid size. */
void qudaAmdMultigridSetFused(int on);
/* Launch-parameter cache (include/tune.h; reference lib/tune.cpp:213-355): tunecache.tsv under QUDA_RESOURCE_PATH in the reference's text
 * format.  Load re-reads the file and returns the number of entries; Store / Lookup address one entry by the reference's key triple,
 * param = block.x y z, grid.x y z, shared_bytes, aux.x y z w; Sweeps = sweeps this process has run (0 when everything came from the file). */
int qudaAmdTuneCacheLoad(void);
void qudaAmdTuneCacheSave(void);
void qudaAmdTuneCacheStore(const char *volume, const char *name, const char *aux, const int param[11], float time, const char *comment);
int qudaAmdTuneCacheLookup(const char *volume, const char *name, const char *aux, int param[11], float *time);
long qudaAmdTuneSweeps(void);
int qudaAmdMultigridFusedStats(void *mg_instance, int level, long long out[5]);
/* counters of invertMultiSrcQuda since start-up: [0] multigrid cycles run for all sources at once (coarse levels on block fields), [1] those of
 * them whose fine-level smoothing also ran on block fields (multi-right-hand-side stencil; QUDA_AMD_MULTISRC_BLOCK_SMOOTHER=0 switches it off),
 * [2] four-source restrictor / prolongator launches (QUDA_AMD_MULTISRC_QUAD=0), [3] lockstep solves */
void qudaAmdMultiSrcStats(long long out[4]);
/* seconds per application of the restrictor (what = 0) or prolongator (what = 1) between `level` and `level + 1` */
double qudaAmdMultigridTimeTransfer(void *mg_instance, int level, int what, int niter);

/* ---- the solve loop of the QKXTM correlator drivers ----
 * calcMG_threepTwop_EvenOdd / calcMG_loop_wOneD_TSM_* (lib/interface_quda.cpp:6018-6531, :7093, :8535) open with the same
 * loop: for every spin-colour component of a point source, Gaussian-smear it with the APE-smeared links, solve for the up
 * quark (twist +, inv_param->preconditionerUP) and the down quark (twist -, preconditionerDN) with even-odd preconditioned
 * GCR, reconstruct, rescale by 2 kappa under mass normalisation.  The reference then contracts and writes its files; these
 * entry points hand the propagators back, and the contractions below compute the correlators on the device: two-point functions
 * (qudaAmdContractTwop, qudaAmdSetTwopOutput), nucleon three-point functions by the fixed-sink method (qudaAmdThreepSeqSource,
 * qudaAmdContractThreep, qudaAmdSetThreepOutput) and quark loops (qudaAmdContractLoop, qudaAmdSetLoopOutput).  HDF5 output is not
 * part of the library.
 * Host layouts are the QKXTM ones: sites lexicographic x fastest (LOCAL lattice of the calling rank), vectors
 * iv*24 + (spin*3 + colour)*2 + re/im in the UKQCD basis (lib/qudaQKXTM_Vector_Kepler.cpp:72-81), smearing links
 * gauge_APE[dir][iv*18 + (row*3 + col)*2 + re/im] (lib/qudaQKXTM_Gauge_Kepler.cpp:73-89, what mapEvenOddToNormalGauge
 * leaves in the driver, qkxtm/CalcMG_2pt3pt_EvenOdd.cpp:684-686); fp64. */
typedef struct QudaAmdSourceParam_s {
  int sourcePosition[4];   /* GLOBAL (x, y, z, t): qudaQKXTMinfo_Kepler::sourcePosition[i] (include/qudaQKXTM_Kepler_utils.h:51) */
  int nsmearGauss;         /* qudaQKXTMinfo_Kepler::nsmearGauss (:46); 0: point source, gauge_APE may be NULL */
  double alphaGauss;       /* qudaQKXTMinfo_Kepler::alphaGauss (:48) */
} QudaAmdSourceParam;
/* The smeared field that performAPEnStep leaves inside the library (the reference keeps it in the file-scope gaugeSmeared and has
 * no accessor): host copy, fp64, either in QDP order (lexicographic = 0: even sites then odd, as loadGaugeQuda takes it) or in
 * the QKXTM lexicographic order gauge_APE uses (lexicographic = 1).  The two functions below also accept gauge_APE = NULL and
 * then smear with that resident field — what the drivers' read-smeared-configuration step supplies otherwise. */
void qudaAmdSaveSmearedGauge(void **h_gauge, int lexicographic);
/* Stout smearing (Morningstar and Peardon, hep-lat/0311018) of the resident links into the library's smeared field, which replaces
 * an earlier one.  smear_time = 0 is performSTOUTnStep: the spatial links from the staples of the three spatial planes, time links
 * copied.  smear_time = 1 smears all four directions with the staples of all six planes - what a measurement of the topological
 * charge wants.  fp64 arithmetic whatever the precision of the resident links. */
void qudaAmdStoutSmear(unsigned int nSteps, double rho, int smear_time);
/* Topological charge Q = sum_x q(x), q(x) = [Re tr(F10 F32) + Re tr(F30 F21) - Re tr(F20 F31)] / (4 pi^2) with the clover-leaf
 * F_mu_nu = (Q_mu_nu - Q_mu_nu^dag)/8.  which = -1: the smeared field if one is resident, else the resident links (qChargeCuda);
 * 0: the resident links; 1: the smeared field (an error if there is none).  h_density (may be NULL) receives q(x) of the calling
 * rank's local lattice, V doubles: even sites then odd (lexicographic = 0) or lexicographic, x fastest (1).  Returns the global Q,
 * summed in a fixed order: two calls on the same field return the same bits. */
double qudaAmdQCharge(double *h_density, int lexicographic, int which);
/* Test hook: out[k] = exp(i q[k]) for n traceless Hermitian 3x3 matrices, 18 doubles each (row-major, re/im), evaluated on the
 * device by the function the stout kernel calls (Cayley-Hamilton form). */
void qudaAmdSu3ExpIQ(int n, const double *q, double *out);
/* Gauge fixing by overrelaxation: computeGaugeFixingOVRQuda (quda.h) with two more results.  h_transform (may be NULL): the accumulated
 * transformation G of the calling rank's local lattice, V x 18 doubles (row-major, re/im), even sites then odd, with
 * U^fixed_mu(x) = G(x) U_mu(x) G(x + mu)^dag for the input links without their anti-periodic sign.  info (may be NULL): {iterations done,
 * F, theta, the last |F - F_prev|}; F = sum_x sum_{mu<D} Re tr U_mu(x) / (3 D V) and theta = sum_x tr(Delta Delta^dag) / (3 V) as evaluated
 * after the last iteration, D = 3 for gauge_dir == 3 (Coulomb) and 4 otherwise (Landau), V the global volume.
 * qudaAmdGaugeFixQuality: out = {F, theta} of the resident precise links, summed in a fixed order (the same field gives the same bits). */
int qudaAmdGaugeFixOVR(void *gauge, const unsigned int gauge_dir, const unsigned int Nsteps, const unsigned int verbose_interval, const double relax_boost,
                       const double tolerance, const unsigned int reunit_interval, const unsigned int stopWtheta, QudaGaugeParam *param, double *timeinfo,
                       void *h_transform, double info[4]);
void qudaAmdGaugeFixQuality(unsigned gauge_dir, double out[2]);
/* Fermion force of molecular dynamics for the actions this library solves (Wilson, degenerate twisted mass, the non-degenerate
 * doublet, twisted clover); the reference's only Wilson-type fermion force, computeCloverForceQuda, belongs to the Wilson-clover action
 * with the MILC / Chroma gamma5 conventions and is not provided under that name.  Conventions
 * of the gauge force: U' = A U, momenta as ten reals per link [site (even, odd)][mu][10], TA(M) = (M - M^dag)/2 - tr(M - M^dag)/6.
 * Both calls work on the resident links (an error if there are none), take fp64 host momenta under gauge_param with
 * QUDA_QDP_GAUGE_ORDER, honour overwrite_mom, use_resident_mom, make_resident_mom and return_result_mom as computeGaugeForceQuda
 * does, and run under any partition (twisted clover in qudaAmdComputeTMForce: unpartitioned lattices only, see below).  Refused:
 * cuda_prec other than fp64, solve_type other than QUDA_NORMOP_PC_SOLVE / QUDA_DIRECT_PC_SOLVE, the doublet with a clover term.
 *
 * qudaAmdFermionOprodForce: mom_mu(x) <- TA(mom_mu(x) - sum_i coeff[i] U_mu(x) O_mu[X_i, Y_i](x)) with
 *   O_mu[X, Y](x) = tr_spin[(1 - g_mu) X(x + mu) Y^dag(x) + (1 + g_mu) Y(x + mu) X^dag(x)]
 * for nvector pairs of full host fields h_x[i], h_y[i] in the layout, basis and precision MatQuda takes under inv_param (two flavours
 * when twist_flavor is the doublet, summed over).  U is the link as the stencil sees it, anti-periodic sign included.
 *
 * qudaAmdComputeTMForce: mom <- mom + dt sum_i coeff[i] F[x_i], F the force of phi^dag (Mh^dag Mh)^-1 phi, for the single-parity
 * solutions h_x[i] = (Mh^dag Mh + shift_i)^-1 phi that a QUDA_NORMOP_PC_SOLVE returns under inv_param (the shifts drop out of the force).
 * Mh is the even-odd operator of inv_param: dslash_type Wilson or twisted mass, twist +-1 or the doublet with epsilon, the four
 * matpc_type (Wilson: the two symmetric ones), every mass_normalization.  X_i and Y_i are built on the device.
 * With dslash_type QUDA_TWISTED_CLOVER_DSLASH (twist +-1, any mu including 0: Wilson clover) Mh is the twisted-clover operator on the
 * resident clover term and the call adds the derivative of that term as well: one sigma outer product and one derivative launch (below)
 * after the hop kernel.  The clover term must have been built from the resident links by loadCloverQuda(NULL, NULL, inv_param) in fp64
 * (clover_cuda_prec) with the kappa, mu and clover_coeff of inv_param; the caller rebuilds it after every link update.  Refused
 * before any device work: no resident clover term, one loaded from a host field (its coefficient is unknown), a clover_coeff, kappa or
 * mu that differ from those it was built with, a clover term held in another precision than fp64, any partitioned direction. */
void qudaAmdFermionOprodForce(void *mom, void **h_x, void **h_y, double *coeff, int nvector, QudaGaugeParam *gauge_param, QudaInvertParam *inv_param);
void qudaAmdComputeTMForce(void *mom, double dt, void **h_x, double *coeff, int nvector, QudaGaugeParam *gauge_param, QudaInvertParam *inv_param);
/* seconds the kernels of the last of these calls, or of the clover-force calls below, took on the device (tools/ferm_force_timing.py,
 * tools/clover_force_timing.py) */
double qudaAmdFermForceLastKernelSecs(void);
/* The clover part of the twisted-clover force and the force of the clover determinant.  Conventions as above; in addition
 * F_mu_nu = (Q_mu_nu - Q_mu_nu^dag)/8 of the four clover leaves, no trace removed, plane index f = mu (mu - 1)/2 + nu for nu < mu (F10,
 * F20, F21, F30, F31, F32); the clover term is A = 1 + i c sum_f sigma_f (x) F_f with c = clover_coeff and sigma_mu_nu = (i/2)[g_mu, g_nu];
 * a = 2 kappa mu twist_flavor and R = A + i a g5, so that R^dag R = A^2 + a^2, whose inverse is the resident clover inverse.  A tensor
 * field holds six 3x3 complex colour matrices per site: h_tensor[site (even, odd)][f][3][3][re, im], 108 doubles per site.  "The force
 * F[S] of S" is what a call adds to the momentum per unit dt: d/d eps S(exp(eps Theta) U) = sum_links Re tr(Theta_mu(x) F_mu(x)) for every
 * traceless anti-Hermitian Theta.
 *
 * qudaAmdCloverSigmaOprod: h_tensor_f(x) = sum_i coeff[2 i + parity(x)] S_f[X_i, Y_i](x) with
 *   S_f[X, Y](x)_ba = sum_ss' (sigma_f)_ss' X(x)_s'b conj(Y(x)_sa),        so that Y^dag(x) dA(x) X(x) = i c sum_f tr(dF_f(x) S_f(x)),
 * for nvector pairs of full one-flavour host fields as MatQuda takes them under inv_param.  Overwrites h_tensor.  Site-local: any
 * partition.  Refused: cuda_prec other than fp64, the doublet, no resident links (they fix the lattice).
 *
 * qudaAmdCloverSigmaTrace: h_tensor_f(x) = coeff[parity(x)] sum_ss' (sigma_f)_ss' B(x)_(s'b)(sa) with B = A (A^2 + a^2)^-1 from the
 * resident fp64 clover term and its inverse, a from the kappa, mu and twist_flavor of inv_param (which must be those the inverse was
 * computed with).  d log det(A^2 + a^2) = 2 i c sum_f tr(dF_f [this with coeff 1]).  Overwrites h_tensor.  Site-local: any partition.
 * Refused: no resident clover term, one not held in fp64, kappa and mu that differ from those of the resident inverse.
 *
 * qudaAmdCloverDerivativeForce: mom <- mom + coeff G[T] for the tensor field T = h_tensor (general complex; only (T - T^dag)/2 counts),
 * G[T] the force of L_T(U) = sum_x sum_f Re tr(T_f(x) F_f(x; U)) on the resident links, in every precision and reconstruction the gauge
 * force takes, fp64 arithmetic.  Momentum flags as above.  Unpartitioned lattices only: refused before any device work, with a message
 * that names the partitioned directions.
 *
 * qudaAmdCloverLogDetForce: mom <- mom + dt (coeff_even F[L_even] + coeff_odd F[L_odd]) with L_p = sum over the sites of parity p of
 * log det(A(x)^2 + a^2), the quantity loadCloverQuda reports in trlogA[p].  Even-odd preconditioning leaves the determinant of the
 * eliminated parity outside the pseudofermion action: a pair of flavours +-mu under asymmetric preconditioning has the weight
 * det(A^2 + a^2) of that parity, S = -L_p, so the caller passes -1 for the parity that was eliminated (the odd one for the EVEN_EVEN
 * types) and 0 for the other; symmetric preconditioning divides by R on both parities, -1 for both.  Requirements and refusals on the
 * clover term and the partition as for twisted clover in qudaAmdComputeTMForce. */
void qudaAmdCloverSigmaOprod(double *h_tensor, void **h_x, void **h_y, double *coeff /* [nvector][2]: even, odd */, int nvector, QudaInvertParam *inv_param);
void qudaAmdCloverSigmaTrace(double *h_tensor, double coeff_even, double coeff_odd, QudaInvertParam *inv_param);
void qudaAmdCloverDerivativeForce(void *mom, double *h_tensor, double coeff, QudaGaugeParam *gauge_param);
void qudaAmdCloverLogDetForce(void *mom, double dt, double coeff_even, double coeff_odd, QudaGaugeParam *gauge_param, QudaInvertParam *inv_param);
/* h_out = smear^nsmear(h_in) (QKXTM_Vector_Kepler::gaussianSmearing, lib/qudaQKXTM_Vector_Kepler.cpp:386-421); the lattice is
 * that of the resident gauge field */
void qudaAmdGaussianSmear(void *h_out, const void *h_in, void **gauge_APE, int nsmear, double alpha);
/* h_prop_up / h_prop_dn: 12 vectors each (index isc = spin*3 + colour of the source, as the reference's loop), V*24 doubles per
 * vector.  inv_param as the reference requires it (:6041-6054): QUDA_DIRECT_PC_SOLVE, QUDA_GCR_INVERTER, UKQCD basis,
 * QUDA_DIRAC_ORDER, symmetric even-even / odd-odd preconditioning, QUDA_MAT_SOLUTION; iter / secs / gflops are summed over
 * the 24 solves; twist_flavor and preconditioner are left at their last values (minus / DN), as in the reference. */
void qudaAmdCalcMGPropagators(void *h_prop_up, void *h_prop_dn, void **gauge_APE, QudaInvertParam *inv_param, const QudaAmdSourceParam *source);

/* Sink for the solutions of the QKXTM entry points of qudaQKXTM_Kepler.h (calcMG_threepTwop_EvenOdd, calcMG_loop_wOneD_TSM_*):
 * called once per finished solve with host vectors in the QKXTM layout (lexicographic sites of the LOCAL lattice, UKQCD spin,
 * V * 24 doubles; h_source may be NULL) that are valid only during the call.  This is where a driver runs the contractions the
 * reference does inside those functions.  No sink registered: the solutions are dropped after their norm has been printed. */
typedef void (*QudaAmdSolutionSink)(void *ctx, const char *kind, int index, int twist_flavor, const double *h_source, const double *h_solution, size_t nreal);
void qudaAmdSetSolutionSink(QudaAmdSolutionSink sink, void *ctx);

/* ---- two-point correlators of the QKXTM drivers (reference lib/interface_quda.cpp:6960-7030) ----
 * Mesons (channel order pseudoscalar, scalar, g5g1, g5g2, g5g3, g5g4, g1, g2, g3, g4) and baryons (nucl_nucl, nucl_roper,
 * roper_nucl, roper_roper, deltapp_deltamm_11/22/33, deltap_deltaz_11/22/33) of the up / down propagators of one source, after
 * Gaussian smearing at the sink, the rotation (1 +- i g5)/sqrt2 to the physical basis (+ up, - down) and the projection
 * sum_x e^{-2 pi i n.(x - x0)/L} onto every momentum |n|^2 <= Q_sq.  Flavour index 0 / 1: the up / down propagator for the mesons,
 * proton (uud) / neutron (ddu) for the baryons.  Time runs from the source (it = 0 is the source time slice: global slice
 * (it + t0) mod T); the baryons carry the sign -1 where it + t0 >= T, as the reference's ASCII writer applies it. */
typedef struct QudaAmdTwopParam_s {
  int sourcePosition[4];   /* GLOBAL (x, y, z, t) */
  int Q_sq;                /* momenta n with |n|^2 <= Q_sq, in the order of qudaAmdTwopMomenta */
  int nsmearGauss;         /* sink smearing steps; 0: none, gauge_APE may be NULL */
  double alphaGauss;
} QudaAmdTwopParam;
/* the momentum list: shells iQ = 0 .. Q_sq, inside a shell nx, ny, nz each from +iQ down to -iQ (lib/qudaQKXTM_Kepler_kernels.cu:96-114);
 * returns Nmoms and, if moms is not NULL, fills moms[Nmoms][3] (max_moms entries available) */
int qudaAmdTwopMomenta(int Q_sq, int *moms, int max_moms);
/* global time extent T of the resident lattice (the first dimension of the outputs below) */
int qudaAmdTwopTimeExtent(void);
/* h_prop_up / h_prop_dn: 12 vectors each exactly as qudaAmdCalcMGPropagators returns them (LOCAL lattice, lexicographic, UKQCD);
 * gauge_APE: smearing links as for qudaAmdGaussianSmear (NULL: the resident smeared field, or none with nsmearGauss = 0).
 * h_mesons [T][Nmoms][2][10][re, im], h_baryons [T][Nmoms][2][10][4 gamma][4 gamma'][re, im], fp64, T global; every rank
 * receives the full result (summed over the ranks' time slices and spatial sub-volumes).  Either output may be NULL. */
void qudaAmdContractTwop(double *h_mesons, double *h_baryons, const void *h_prop_up, const void *h_prop_dn, void **gauge_APE, const QudaAmdTwopParam *p);
/* off by default.  On: calcMG_threepTwop_EvenOdd contracts every source from the device-resident solutions (sink smearing with
 * info.nsmearGauss / alphaGauss, momenta info.Q_sq) after its 24 solves and rank 0 writes the reference's ASCII files
 * <filename_twop>.mesons.SS.xx.yy.zz.tt.dat and <filename_twop>.baryons.SS.xx.yy.zz.tt.dat; the solution sink is still called as
 * before.  CorrSpace = POSITION_SPACE and HighMomForm need HDF5 and are errors; CorrFileFormat = HDF5_FORM warns and writes ASCII. */
void qudaAmdSetTwopOutput(int enable);

/* ---- disconnected quark loops of the QKXTM drivers (reference lib/qudaQKXTM_Loops_Kepler.cpp:300-497) ----
 * One-end-trick contractions with one covariant derivative of ONE solution vector x, phi = g5 D_W x (the kappa-normalised Wilson
 * or Wilson-clover operator at mu = 0 on the resident fields), C[u, v][4a + b] = sum_c conj(u[(a + 2) mod 4, c]) v[b, c] in the UKQCD
 * basis, F / B the forward / backward covariant shifts on the resident precise links.  18 blocks of 16 complex numbers:
 *   0 Scalar -C[x,x];  1 dOp +C[x,phi];  2+mu Loops -(C[x,Fx] + C[Bx,x] - C[Fx,x] - C[x,Bx]);  6+mu LoopsCv -(the four added);
 *   10+mu LpsDw +(C[x,F phi] + C[Bx,phi] - C[Fx,phi] - C[x,B phi]);  14+mu LpsDwCv +(the four added);
 * each projected with sum_x e^{-2 pi i n.x/L} (global coordinates, no source offset) onto the momenta of qudaAmdLoopMomenta. */
/* the momentum list of the loops (createLoopMomenta, lib/qudaQKXTM_Kepler_utils.cpp:255-298; NOT the two-point list): pz outermost,
 * px innermost, every component 0 .. L/2-1, -L/2 .. -1 over the GLOBAL extent L, kept where |n|^2 <= Q_sq.  Host only; returns
 * Nmoms and, if moms is not NULL, fills moms[Nmoms][3] (max_moms entries available) */
int qudaAmdLoopMomenta(const int L[3], int Q_sq, int *moms, int max_moms);
/* h_solution: V*24 doubles, LOCAL lattice, lexicographic UKQCD (the layout the solution sink receives), NOT rescaled by 2 kappa;
 * param: dslash_type (twisted mass or twisted clover; anything else is an error) and kappa are read; the resident precise links
 * (and clover term) must be fp64.  out[18][T global][Nmoms][16][re, im]: raw sums of this one vector (no factor 0.25); every rank
 * receives the full result.  QUDA_AMD_LOOP_FUSED=0 in the environment selects the unfused chain of covariant shifts and pairwise
 * contractions in the reference's call order instead of the fused stencil kernel. */
void qudaAmdContractLoop(double *out, const void *h_solution, QudaInvertParam *param, int Q_sq);
/* off by default.  On: calcMG_loop_wOneD_TSM_EvenOdd contracts every solution from the device-resident field, accumulates over the
 * noise vectors in momentum space (momenta info.Q_sq) and rank 0 writes the reference's ASCII files at every dump (writeLoops_ASCII:
 * <loop_fname>_stoch_MG_<type>.loop.<NNNN>.<nT>_<r>, under the truncated solver method <loop_fname>_stoch_TSM_MG_NLP<NNNN>_<type>.loop.<nT>_<r>
 * and the _HighPrec / _LowPrec pair of the bias run); the solution sink is still called as before.  loopInfo.HighMomForm needs HDF5
 * and is an error; FileFormat = HDF5_FORM warns and writes ASCII. */
void qudaAmdSetLoopOutput(int enable);
/* seconds of the last loop contraction on this rank (device events): phi, stencil (or the unfused chain), projection, all of it */
void qudaAmdLoopLastTimings(double secs[4]);

/* ---- the momentum projection that the two-point, loop and three-point contractions share (csrc/momproj.hip) ---- */
/* test hook: h_acc[nblk][Lt][Nm][16][re,im] (host, in and out) += the projection of h_cs[nblk][nt * Vs][16][re,im] (host), Vs = X[0] X[1] X[2],
   x fastest, for the local slices [t0, t0 + nt): uploads both, runs momentumProject once, downloads h_acc.  moms[Nm][3] (host), X the
   local spatial extents, gx the global coordinate of the local origin (of any sign), L the global extents:
     h_acc[k][t0 + tl][m][e] += sum_s exp(-2 pi i sum_d moms[m][d] (x_d(s) + gx[d]) / L[d]) h_cs[k][tl * Vs + s][e]
   in the fixed summation order stated at momentumProject (csrc/qkxtm_internal.h).  Needs initQuda, no resident field. */
void qudaAmdMomentumProject(double *h_acc, const double *h_cs, int nblk, int t0, int nt, int Lt, const int *moms, int Nm,
                            const int X[3], const int gx[3], const int L[3]);

/* ---- exact deflation of the quark loops (reference QKXTM_Deflation_Kepler, lib/qudaQKXTM_Deflation_Kepler.cpp; ARPACK is replaced by a
 * thick-restart Lanczos process on the device) ----
 * A = M^dag M of the FULL (not even-odd) twisted-mass or twisted-clover operator made from `param` (dslash_type, kappa, mu,
 * twist_flavor; cuda_prec must be fp64), in the normalisation of the operator the solver inverts (no mass normalisation applied).
 * isACC != 0: the Lanczos process runs on the reference's Chebyshev filter p(A) of degree PolyDeg that is small on [amin, amax] and
 * takes its largest Ritz values; isACC = 0: it runs on A and takes the smallest.  nKv basis vectors (nEv < nKv <= 256) stay on the
 * device, every step orthogonalises against all of them (classical Gram-Schmidt, twice); at nKv vectors a Ritz pair counts as
 * converged when |beta_m s_(m,i)| <= tol |theta_i|; otherwise the basis is compressed to nEv + (nKv - nEv) / 2 Ritz vectors plus the
 * residual vector, at most maxRestarts times.  The start vector is Z4 noise keyed by the global site index.  For every returned
 * vector lambda_i = Re (v_i, A v_i) and the residual |A v_i - lambda_i v_i| with A itself; the pairs are sorted by ASCENDING lambda
 * (the reference keeps ARPACK's order), so the first n vectors are the n lowest modes.  nKv + 4 full fp64 fields must fit into the
 * free device memory. */
typedef struct { int nEv, nKv, PolyDeg, isACC, maxRestarts; double amin, amax, tol; } QudaAmdEigParam;
/* runs the eigensolver on the resident fields and keeps the nEv eigenvectors U on the device */
void *qudaAmdNewDeflation(QudaInvertParam *param, const QudaAmdEigParam *eig);
void qudaAmdDestroyDeflation(void *defl);
/* returns nEv; evals[nEv], residuals[nEv], the number of restarts and of applications of A (any of them may be NULL) */
int qudaAmdDeflationInfo(void *defl, double *evals, double *residuals, int *restarts, int *matvecs);
/* seconds the eigensolver spent on this rank (device events): filter (operator applications and recurrence), dots, updates, basis
 * rotations.  QUDA_AMD_EIG_PANEL=0 in the environment runs the eigensolver on blas::multiDot / multiCaxpy in chunks of 20 fields
 * and rotates with k multiCaxpy sweeps into spare fields instead of the panel kernels (tools/eig_timing.py compares the two). */
void qudaAmdDeflationTimings(void *defl, double secs[4]);
/* eigenvector i in the host layout and basis that MatQuda takes for the `param` of qudaAmdNewDeflation with a full-field solution
 * type (cpu_prec, gamma_basis, dirac_order; even sites then odd) */
void qudaAmdDeflationGetVector(void *defl, int i, void *h_vec);
/* h_out = (1 - U_n U_n^+) h_in with the first n vectors, on the device (the reference: zgemv on the host); layout of
 * qudaAmdDeflationGetVector */
void qudaAmdDeflationProject(void *defl, int n, void *h_out, const void *h_in);
/* the exact part of the loops, out = sum_{i<n} L[v_i] / lambda_i, L the 18 blocks of qudaAmdContractLoop with v_i in place of the
 * solution (the reference's +1/lambda on the generalised and -1/lambda on the standard blocks, lib/qudaQKXTM_Loops_Kepler.cpp:178-281,
 * sit in the blocks' definitions); out[18][T global][Nmoms][16][re, im] as qudaAmdContractLoop */
void qudaAmdDeflationExactLoop(void *defl, int n, double *out, int Q_sq);
/* dense real symmetric eigenproblem on the host (cyclic Jacobi; what the eigensolver diagonalises its projected matrix with):
 * a[n][n] row-major (the upper triangle is read), w[n] ascending, q[n][n] row-major with COLUMN i the eigenvector of w[i] */
void qudaAmdHostSymmetricEig(int n, const double *a, double *w, double *q);
/* the back substitution of the restarted GCRs (csrc/gcr_core.h; host only): delta_a = (alpha_a - sum_{a < j < k} beta_aj delta_j) / gamma_a for
 * a = k-1 .. 0, and delta_a = 0 where gamma_a == 0.  Complex values as interleaved doubles: alpha[nK], beta[nK][nK] row-major (leading
 * dimension nK, the strict upper triangle is read), gamma[nK] real, delta[k]; k <= nK */
void qudaAmdGcrBackSubstitute(int k, int nK, const double *alpha, const double *beta, const double *gamma, double *delta);
/* test hooks onto the eigensolver's kernels; h_V: m <= 256 vectors of V * 24 doubles (V = X[0] X[1] X[2] X[3], even) seen as V * 12
 * complex numbers or V * 24 real rows; no resident field is needed.
 * qudaAmdRotateBasis: V[:, 0..k) <- V[:, 0..m) Q in place, Q real m x k row-major, the columns k .. m-1 are left alone (fp64 matrix cores);
 * qudaAmdBlockDot: c[j] = (v_j, w) = sum conj(v_j) w as c[m][re, im], one launch;  qudaAmdBlockAxpy: w -= sum_j c[j] v_j */
void qudaAmdRotateBasis(void *h_V, int m, int k, const double *Q, const int X[4]);
void qudaAmdBlockDot(double *c, const void *h_V, int m, const void *h_w, const int X[4]);
void qudaAmdBlockAxpy(void *h_w, const double *c, const void *h_V, int m, const int X[4]);
/* calcMG_loop_wOneD_TSM_wExact with arpackInfo.nEv > 0 (isFullOp, spectrumPart = SR, nKv > nEv, deflStep ascending and <= nEv): the
 * eigensolver above with nEv, nKv, PolyDeg, isACC, amin, amax, tolArpack, maxIterArpack (arpack_logfile is ignored with a notice);
 * every eigenvector goes to the solution sink as kind "eigvec", index i (lexicographic UKQCD, no source), before the solves.  With
 * the loop output on, rank 0 writes for every deflStep n the exact part <loop_fname>_exact_NeV<n>_<type>.loop.<nT>_<r>, and the
 * stochastic part is contracted from the solutions projected with the first n vectors:
 * <loop_fname>_stoch_NeV<n>_<type>.loop.<NNNN>.<nT>_<r>, under the truncated solver method <loop_fname>_stoch_TSM_NeV<n>_NLP<NNNN>_... and
 * the _HighPrec / _LowPrec pair.  The sink receives the UNPROJECTED solutions.  qudaAmdLastEigenvalues copies up to n eigenvalues of
 * the last such call and returns how many there are. */
int qudaAmdLastEigenvalues(double *evals, int n);

/* ---- nucleon three-point functions by the fixed-sink sequential method (reference lib/interface_quda.cpp:6560-6950) ----
 * UKQCD basis, fp64.  s = +1 where the operator is inserted on the up quark, -1 on the down quark: proton part 1 up, part 2 down;
 * neutron part 1 down, part 2 up.  Projectors (enum WHICHPROJECTOR of qudaQKXTM_Kepler_utils.h): G4 = (1 + g4)/4,
 * G5Gk = (1 + g4) i g5 gk / 4, G5G123 their sum over k; the code uses G_tm = R_p G R_p, R_p = (1 + p i g5)/sqrt2, p = +1 proton,
 * -1 neutron.
 * Sequential source: U3 / D3 the up / down propagators, sink-smeared and not rotated; N[x; k, n] the nucleon Wick sum (diquark
 * C g5 at source and sink, direct minus exchange term; the neutron with up and down exchanged), f(x) = sum_kn G_tm[n][k] N[x; k, n].
 * Part 1 is the derivative of f with respect to the propagator of the flavour that occurs twice (both slots), part 2 with respect
 * to the other; component (nu, c) of the source for column (nu', c') is sigma = df/dP[x; nu, nu'; c, c'].  The solver gets
 * g5 conj(sigma) on the sink time slice (tsinkSource + t0) mod T, Gaussian-smeared, zero elsewhere.
 * Contraction: y_(pi, b) the twelve sequential solutions, q[x; kappa, pi; a, b] = conj((g5 y_(pi, b))[x; kappa, a]), F the forward
 * propagator of the inserted flavour, per site
 *   S0[kappa][lambda] = sum q[x] F[x],  A_mu = sum q[x] U_mu(x) F[x + mu],  B_mu = sum q[x] U_mu(x - mu)^+ F[x - mu],
 *   C_mu = sum q[x + mu] U_mu(x)^+ F[x],  D_mu = sum q[x - mu] U_mu(x - mu) F[x]     (sums over pi, b and the colours),
 *   local[i] = tr O_i^T S0,  oneD[mu][i] = tr O_i^T ((A + D) - (B + C))_mu / 4,
 *   noether[mu] = (tr (1 + g_mu)^T (B + C)_mu - tr (1 - g_mu)^T (A + D)_mu) / 4,
 * O_i = s i g5, g1 .. g4, s i 1, g5g1 .. g5g4, s g5g1g2, s g5g1g3, s g5g2g3, s g5g4g1, s g5g4g2, s g5g4g3 (tr X^T Y = sum X[k][l] Y[k][l]),
 * projected with sum_x e^{+2 pi i n.(x - x0)/L} (the sign opposite to the two-point functions) onto the momenta of
 * qudaAmdTwopMomenta.  Time runs from the source (it = 0: global slice (it + t0) mod T); everything carries -1 when
 * tsinkSource + t0 >= T. */
typedef struct QudaAmdThreepParam_s {
  int sourcePosition[4];   /* GLOBAL (x, y, z, t) */
  int Q_sq;                /* momenta of the contraction */
  int tsinkSource;         /* sink time slice relative to the source */
  int projector;           /* enum WHICHPROJECTOR */
  int particle;            /* enum WHICHPARTICLE: PROTON or NEUTRON */
  int part;                /* 1 or 2 */
  int nsmearGauss;         /* smearing of the propagators at the sink and of the sequential source; 0: none, gauge_APE may be NULL */
  double alphaGauss;
} QudaAmdThreepParam;
/* h_prop_up / h_prop_dn: the 12 + 12 unsmeared columns as qudaAmdCalcMGPropagators returns them; h_out: the twelve vectors as
 * they go to the solver (V * 24 doubles each, LOCAL lattice, lexicographic UKQCD).  A rank that does not own the sink slice gets zeros. */
void qudaAmdThreepSeqSource(void *h_out, const void *h_prop_up, const void *h_prop_dn, void **gauge_APE, const QudaAmdThreepParam *p);
/* h_seq: the twelve sequential solutions as the solver returns them (solved with the twist opposite to the inserted flavour);
 * h_fwd: the twelve forward columns of the inserted flavour; gauge: the links of the derivative in the QKXTM lexicographic layout
 * with the boundary condition already applied, or NULL for the resident precise links (fp64).  h_local [T][Nmoms][16],
 * h_noether [T][Nmoms][4], h_oneD [T][Nmoms][4][16] complex, T global; any of them may be NULL; every rank receives the full result. */
void qudaAmdContractThreep(double *h_local, double *h_noether, double *h_oneD, const void *h_seq, const void *h_fwd, void **gauge, const QudaAmdThreepParam *p);
/* host-only queries of the spin tables, row-major 4 x 4 complex: O_i for the flavour sign s = +-1; G_tm of a projector and particle */
void qudaAmdThreepOperator(int i, int s, double out[32]);
void qudaAmdThreepProjector(int pid, int particle, double out[32]);
/* off by default.  On: calcMG_threepTwop_EvenOdd runs, for every source with info.run3pt_src != 0, every sink separation
 * info.tsinkSource[its < Ntsink], every projector info.proj_list[its][ip < Nproj[its]] and both parts: the sequential source from the
 * device-resident forward solutions, twelve solves through the path of the forward solves (lockstep where it fits, one by one
 * otherwise and with QUDA_AMD_QKXTM_LOCKSTEP=0) with the twist opposite to the inserted flavour, the contraction, and rank 0 writes the
 * reference's three ASCII files <filename_threep>_tsink<t>_proj<info.thrp_proj_type[P]>.<proton|neutron>.<up|down>.
 * <ultra_local|noether|oneD>.SS.xx.yy.zz.tt.dat (writeThrp_ASCII; a NULL thrp_proj_type entry falls back to the enumerator's name).
 * Every sequential solution also goes to the solution sink as "seq_part1" / "seq_part2" with its smeared source.  CorrSpace =
 * POSITION_SPACE and HighMomForm are errors; CorrFileFormat = HDF5_FORM warns and writes ASCII.  Off: no file, no extra solve, no
 * extra sink call. */
void qudaAmdSetThreepOutput(int enable);
/* seconds of the last calls on this rank (device events): source construction, ghost exchange, stencil, projection */
void qudaAmdThreepLastTimings(double secs[4]);

/* ILDG gauge configurations in LIME containers (the step in front of loadGaugeQuda in the QKXTM drivers).  qudaAmdReadLimeGauge
 * has the semantics of readLimeGauge / readLimeGaugeSmeared (qkxtm/QKXTM_read_conf.h:107-400, :819-835): every rank reads the
 * sub-block of its grid coordinates from the "ildg-binary-data" record into the even-odd QDP arrays gauge[4] (fp64, allocated
 * by the caller for the LOCAL volume), sets param->X to the local extents from "ildg-format", compares kappa of "xlf-info" with
 * inv_param (may be NULL) and applies no boundary condition.  The container format is restated in csrc/lime_io.cpp (c-lime is
 * not a dependency).  qudaAmdWriteLimeGauge writes such a file from one rank (xlf_info may be NULL). */
void qudaAmdReadLimeGauge(void **gauge, const char *fname, QudaGaugeParam *param, QudaInvertParam *inv_param, const int gridSize[4]);
void qudaAmdWriteLimeGauge(void **gauge, const char *fname, const QudaGaugeParam *param, const char *xlf_info);

/* RCCL bootstrap (the transport that replaces the reference's MPI layer, lib/comm_mpi.cpp:50-155): rank 0 obtains a
 * 128-byte id, the launcher broadcasts it out of band, every rank calls qudaAmdCommInit BEFORE initCommsGridQuda / initQuda. */
void qudaAmdCommGetUniqueId(void *out128);
void qudaAmdCommInit(const void *id128, int rank, int size);
int qudaAmdCommRank(void);
int qudaAmdCommSize(void);
void qudaAmdCommCoords(int coords[4]);
void qudaAmdCommBarrier(void);
void qudaAmdCommAllreduce(double *data, int n);   /* sum over ranks, in place */
void qudaAmdCommAllreduceMax(double *data, int n);

/* single-process emulation of a partitioned dimension (reference tests --partition, commDimPartitionedSet) */
void qudaAmdSetPartitionMask(int mask);

/* Raw device images of the resident fields, for checks of the layout contract (reference lib/color_spinor_field.cpp:129-216:
 * stride = volumeCB + pad, bytes per parity rounded up to 1 KiB, odd half at bytes / 2, fp32 norm array for 16-bit fields):
 * spinor info = {volume, volumeCB, stride, pad, nSpin, nColor, precision, fieldOrder, siteSubset, gammaBasis, bytes, norm_bytes,
 *   device address of v, of norm, byte offset of the odd half, of the odd norms, reals per plane entry (2 fp64 | 4 fp32 | 8 16-bit),
 *   twistFlavor, x[0], location};
 * gauge info (which: 0 precise, 1 sloppy, 2 precondition) = {address, bytes, stride, bytes of one (parity, direction) block,
 *   precision, reconstruct, Vh, boundary sign folded into the links, t_boundary};
 * clover info = {address of A, of the inverse, of the A norms, of the inverse norms, stride, bytes per parity, norm bytes per parity,
 *   precision, bytes, Vh, twisted}.  qudaAmdRawDeviceCopy copies `bytes` from a device address to the host. */
void qudaAmdSpinorRawInfo(const void *field, long long info[20]);
void qudaAmdGaugeRawInfo(int which, long long info[12]);
void qudaAmdCloverRawInfo(int which, long long info[12]);
void qudaAmdRawDeviceCopy(void *h_dst, long long device_address, size_t bytes);

/* stream the kernels are launched on (hipStream_t), for callers that bracket work with their own events */
void *qudaAmdComputeStream(void);
void qudaAmdDeviceSynchronize(void);
/* halo transport in use: -1 not decided yet (no partitioned Dslash so far), 0 staged RCCL send/recv, 1 direct peer stores
 * into IPC-mapped ghost zones (the reference's "p2p" vs staged comms policies, lib/dslash_policy.cuh:838-998) */
int qudaAmdHaloTransport(void);
int qudaAmdHaloWireFormat(void);   /* wire format of the peer-store ghost zones in use: 0 flag-in-data {word, flag} halves, 1 self-validating 16-byte atoms {3 words, flag} (dslash.h haloWireFormat) */
/* launch geometry of the fine-grid stencil kernel, the counterpart of the reference's autotuner entries for the dslash kernels
 * (lib/tune.cpp, TuneParam block / grid): key = "block" (threads per block, 0 automatic), "remap" (XCD-aware block mapping),
 * "order" (legacy slab order), "tiled" / "nxz" / "tz" / "tt" (plane-tiled block order: XCDs along z, tile extents),
 * "store_aux", "link_aux", "lds_pad".  Results never depend on these. */
void qudaAmdSetDslashTune(const char *key, int value);

#ifdef __cplusplus
}
#endif
#endif
