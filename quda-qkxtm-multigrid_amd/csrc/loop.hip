// loop.hip — disconnected quark loops of the QKXTM drivers on the device: the one-end-trick contractions with one covariant
// derivative of a solution vector, momentum projection per time slice, accumulation over the noise vectors in momentum space, the
// sum over ranks and the reference's ASCII writer.
//
// Reference: oneEndTrick_w_One_Der (lib/qudaQKXTM_Loops_Kepler.cpp:300-497), contractGamma5Kernel
// (lib/dslash_core/contract_core.h:65-336), CovD::M (lib/covDev.cu), performFFT / createLoopMomenta
// (lib/qudaQKXTM_Kepler_utils.cpp:255-357), writeLoops_ASCII (lib/qudaQKXTM_Loops_Kepler.cpp:501-575).
//
// With x the solution as the solver leaves it, phi = g5 D_W x (the kappa-normalised Wilson or Wilson-clover operator, mu = 0),
// F_mu v(x) = U_mu(x) v(x + mu), B_mu v(x) = U_mu(x - mu)^+ v(x - mu) and the open-spin, colour-traced building block
//      C[u, v][4a + b] = sum_c conj(u[(a + 2) mod 4, c]) v[b, c]          (UKQCD basis: (u^+ g5)_a v_b)
// every vector adds, per site, 18 blocks of 16 complex numbers:
//      k = 0      Scalar   -= C[x, x]                      k = 1       dOp     += C[x, phi]
//      k = 2 + mu Loops    -= C[x, (F - B) x] - C[(F - B) x, x]
//      k = 6 + mu LoopsCv  -= C[x, (F + B) x] + C[(F + B) x, x]
//      k = 10 + mu LpsDw   += C[x, (F - B) phi] - C[(F - B) x, phi]
//      k = 14 + mu LpsDwCv += C[x, (F + B) phi] + C[(F + B) x, phi]
// (the reference's four terms per block, folded with the linearity of C in each argument).
//
// Fused path (default): ONE stencil kernel forms D x = (F -+ B) x and D phi in registers and writes the blocks of a chunk of time
// slices, cs[k][site][16]; eight threads share a site (direction mu x sign of B), each writes two blocks (and one of the two
// ultra-local ones).  The staged blocks are projected onto the momenta with a fixed number of partial sums in a fixed order and
// added to the accumulator [18][T_local][Nmoms][16], which lives in momentum space: there is no position-space accumulator.
// QUDA_AMD_LOOP_FUSED=0: the reference's chain of single-direction covariant shifts (applyCovariantShift) and pairwise
// contractions in its call order, the in-library cross-check.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "basis.h"
#include "blas.h"
#include "comm_quda.h"
#include "contract_stencil.h"
#include "device_io.h"
#include "interface_internal.h"
#include "p2p.h"
#include "qa_core.h"
#include "qkxtm_internal.h"
#include "quda_amd_ext.h"

namespace quda {

namespace loop {

constexpr int NBLK = 18, NGM = 16;

struct LoopArg : StencilGeom {
  const double *x[2], *phi[2];   // parity blocks of the two fields, device basis: fields 0 and 1 of the ghost zones
};

// o[4a + b] = w1 C[u1, v1] + w2 C[u2, v2], spinors in the UKQCD basis as 24 reals
__device__ __forceinline__ void block2(double2 *o, const double *u1, const double *v1, double w1, const double *u2, const double *v2, double w2) {
#pragma unroll
  for (int a = 0; a < 4; a++)
#pragma unroll
    for (int b = 0; b < 4; b++) {
      double re1 = 0, im1 = 0, re2 = 0, im2 = 0;
#pragma unroll
      for (int c = 0; c < 3; c++) {   // the two sums interleaved: the order the register allocation of the fused kernel was settled with
        colour_mac(re1, im1, u1 + 6 * ((a + 2) & 3), v1 + 6 * b, c);
        colour_mac(re2, im2, u2 + 6 * ((a + 2) & 3), v2 + 6 * b, c);
      }
      o[4 * a + b] = make_double2(w1 * re1 + w2 * re2, w1 * im1 + w2 * im2);
    }
}
__device__ __forceinline__ void block1(double2 *o, const double *u, const double *v, double w) {
#pragma unroll
  for (int a = 0; a < 4; a++)
#pragma unroll
    for (int b = 0; b < 4; b++) {
      double re = 0, im = 0;
      spin_dot(re, im, u + 6 * ((a + 2) & 3), v + 6 * b);
      o[4 * a + b] = make_double2(w * re, w * im);
    }
}

// ---- the fused stencil: 32 sites x 8 (mu, sign) tasks per work-group ----
template <int R> __global__ void __launch_bounds__(256) loop_fused_kernel(const LoopArg a) {
  const int lane = threadIdx.x & 31, j = threadIdx.x >> 5;
  const long s = (long)blockIdx.x * 32 + lane;
  if (s >= a.S) return;
  const int X0 = a.X0, Y = a.Y, Z = a.Z, T = a.T;
  long l = s;
  const int xc = (int)(l % X0); l /= X0;
  const int y = (int)(l % Y); l /= Y;
  const int z = (int)(l % Z);
  const int t = a.t0 + (int)(l / Z);
  const int parity = (xc + y + z + t) & 1;
  const int idx = (((t * Z + z) * Y + y) * X0 + xc) >> 1;
  const int mu = j >> 1;
  const double sg = (j & 1) ? 1.0 : -1.0;   // D = F + sg B

  const HopNeighbours h = hop_neighbours(mu, xc, y, z, t, X0, Y, Z, T, a.tsign_fwd, a.tsign_bwd);
  const int op = 1 - parity;
  const double *gxF = ghost_zone(a, mu, 0, parity, 0), *gxB = ghost_zone(a, mu, 0, parity, 1);
  const double *gpF = ghost_zone(a, mu, 1, parity, 0), *gpB = ghost_zone(a, mu, 1, parity, 1);
  const int fcb = a.faceCB[mu];

  double Dx[24], Dp[24];
  {
    double U[18], psi[24], v[24];
    Link<double, R>::load(U, a.gauge[parity] + (size_t)(2 * mu) * a.link_bytes, a.g_stride, idx, h.signF);
    load_site(psi, a.x[op], a.sp_stride, h.idxF, gxF, fcb, h.face, h.crossF);
#pragma unroll
    for (int sp = 0; sp < 4; sp++) su3_mv(Dx + 6 * sp, U, psi + 6 * sp);
    load_site(psi, a.phi[op], a.sp_stride, h.idxF, gpF, fcb, h.face, h.crossF);
#pragma unroll
    for (int sp = 0; sp < 4; sp++) su3_mv(Dp + 6 * sp, U, psi + 6 * sp);
    Link<double, R>::load(U, a.gauge[parity] + (size_t)(2 * mu + 1) * a.link_bytes, a.g_stride, idx, h.signB);
    load_site(psi, a.x[op], a.sp_stride, h.idxB, gxB, fcb, h.face, h.crossB);
#pragma unroll
    for (int sp = 0; sp < 4; sp++) su3_mv(v + 6 * sp, U, psi + 6 * sp);
#pragma unroll
    for (int k = 0; k < 24; k++) psi[k] = Dx[k] + sg * v[k];
    rotate_basis(Dx, psi, BASIS_DR_TO_UKQCD);
    load_site(psi, a.phi[op], a.sp_stride, h.idxB, gpB, fcb, h.face, h.crossB);
#pragma unroll
    for (int sp = 0; sp < 4; sp++) su3_mv(v + 6 * sp, U, psi + 6 * sp);
#pragma unroll
    for (int k = 0; k < 24; k++) psi[k] = Dp[k] + sg * v[k];
    rotate_basis(Dp, psi, BASIS_DR_TO_UKQCD);
  }
  double x[24], ph[24];
  {
    double r[24];
    Planar<double, 24>::load(r, a.x[parity], a.sp_stride, idx, nullptr, idx);
    rotate_basis(x, r, BASIS_DR_TO_UKQCD);
    Planar<double, 24>::load(r, a.phi[parity], a.sp_stride, idx, nullptr, idx);
    rotate_basis(ph, r, BASIS_DR_TO_UKQCD);
  }
  const int kstd = ((j & 1) ? 6 : 2) + mu;
  block2(a.cs + ((long)kstd * a.S + s) * NGM, x, Dx, -1.0, Dx, x, -sg);
  block2(a.cs + ((long)(kstd + 8) * a.S + s) * NGM, x, Dp, 1.0, Dx, ph, sg);
  if (j == 0) block1(a.cs + s * NGM, x, x, -1.0);
  if (j == 1) block1(a.cs + ((long)a.S + s) * NGM, x, ph, 1.0);
}

// ---- the unfused chain: cs[k][site] (=, +=) w C[u, v] for full device fields u, v ----
__global__ void __launch_bounds__(256) pair_contract_kernel(double2 *cs, long S, int k, const double *u0, const double *u1, const double *v0, const double *v1, int stride,
                                                            int X0, int Y, int Z, int t0, double w, int accumulate) {
  const long s = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= S) return;
  long l = s;
  const int xc = (int)(l % X0); l /= X0;
  const int y = (int)(l % Y); l /= Y;
  const int z = (int)(l % Z);
  const int t = t0 + (int)(l / Z);
  const int parity = (xc + y + z + t) & 1;
  const int idx = (((t * Z + z) * Y + y) * X0 + xc) >> 1;
  double r[24], u[24], v[24];
  Planar<double, 24>::load(r, parity ? u1 : u0, stride, idx, nullptr, idx);
  rotate_basis(u, r, BASIS_DR_TO_UKQCD);
  Planar<double, 24>::load(r, parity ? v1 : v0, stride, idx, nullptr, idx);
  rotate_basis(v, r, BASIS_DR_TO_UKQCD);
  double2 o[NGM];
  block1(o, u, v, w);
  double2 *dst = cs + ((long)k * S + s) * NGM;
#pragma unroll
  for (int i = 0; i < NGM; i++) {
    if (accumulate) { const double2 c = dst[i]; o[i].x += c.x; o[i].y += c.y; }
    dst[i] = o[i];
  }
}

// g5 in the device (DeGrand-Rossi) basis: diag(1, 1, -1, -1)
__global__ void __launch_bounds__(256) gamma5_kernel(double *v, int stride, int Vh) {
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= Vh) return;
  double2 *p = (double2 *)v;
#pragma unroll
  for (int k = 6; k < 12; k++) {
    double2 c = p[(size_t)k * stride + idx];
    p[(size_t)k * stride + idx] = make_double2(-c.x, -c.y);
  }
}

// acc += s * one over n doubles: a weighted vector joins a running sum (the exact part of the loops, weights 1 / lambda)
__global__ void __launch_bounds__(256) accum_scaled_add_kernel(double *acc, const double *one, double s, long n) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) acc[i] += s * one[i];
}

}  // namespace loop

// momenta of the loops (createLoopMomenta): pz outermost, py, px innermost, each component 0 .. L/2-1, -L/2 .. -1 over the GLOBAL extent
std::vector<int> loopMomenta(const int L[3], int Q_sq) {
  std::vector<int> m;
  for (int pz = 0; pz < L[2]; pz++)
    for (int py = 0; py < L[1]; py++)
      for (int px = 0; px < L[0]; px++) {
        const int n0 = px < L[0] / 2 ? px : px - L[0], n1 = py < L[1] / 2 ? py : py - L[1], n2 = pz < L[2] / 2 ? pz : pz - L[2];
        if (n0 * n0 + n1 * n1 + n2 * n2 <= Q_sq) { m.push_back(n0); m.push_back(n1); m.push_back(n2); }
      }
  return m;
}

static void globalL(int L[3]) {
  const LatticeGeom &g = residentGeom();
  for (int d = 0; d < 3; d++) L[d] = g.X[d] * commGrid().dims[d];
}

// cumulative sums of the 18 blocks over the noise vectors, in momentum space, this rank's time slices
LoopAccum *loopAccumCreate(int Q_sq) {
  if (Q_sq < 0) errorQuda("loop contraction: Q_sq = %d", Q_sq);
  int L[3];
  globalL(L);
  return new MomAccum(loop::NBLK, loopMomenta(L, Q_sq));
}

// read at every contraction, so one process can time both paths (tools/loop_timing.py)
static bool fusedEnabled() {
  const char *e = getenv("QUDA_AMD_LOOP_FUSED");
  return e ? atoi(e) != 0 : true;
}

static double g_loopSecs[4] = {0, 0, 0, 0};   // phi, stencil / chain, projection, total of the last contraction

// phi = g5 D_W x with the operator classes: Wilson (twisted mass) or Wilson-clover (twisted clover) at mu = 0, kappa-normalised
static void makePhi(ColorSpinorField &phi, const ColorSpinorField &x, QudaInvertParam *param) {
  DiracParam dp;
  dp.matpcType = QUDA_MATPC_EVEN_EVEN;
  dp.dagger = QUDA_DAG_NO;
  dp.gauge = gaugePrecise;
  dp.kappa = param->kappa;
  dp.mass = 1.0 / (2.0 * param->kappa) - 4.0;
  dp.mu = 0.0;
  if (param->dslash_type == QUDA_TWISTED_CLOVER_DSLASH) {
    if (!cloverPrecise) errorQuda("loop contraction: Clover field not allocated");
    if (cloverPrecise->precision != QUDA_DOUBLE_PRECISION) errorQuda("loop contraction: the resident clover term must be fp64 (clover_cuda_prec)");
    dp.type = QUDA_TWISTED_CLOVER_DIRAC;   // A + i mu g5 - kappa D at mu = 0: the Wilson-clover operator
    dp.clover = cloverPrecise;
  } else if (param->dslash_type == QUDA_TWISTED_MASS_DSLASH) {
    dp.type = QUDA_WILSON_DIRAC;
  } else {
    errorQuda("loop contraction: the one-end trick works only for twisted-mass and twisted-clover fermions (dslash_type %d)", param->dslash_type);
  }
  Dirac *dW = Dirac::create(dp);
  dW->M(phi, x);
  delete dW;
  const int Vh = residentGeom().Vh;
  for (int parity = 0; parity < 2; parity++) {
    ColorSpinorField &h = parity ? phi.Odd() : phi.Even();
    hipLaunchKernelGGL(loop::gamma5_kernel, dim3((Vh + 255) / 256), dim3(256), 0, computeStream(), (double *)h.V(), h.Stride(), Vh);
  }
  HIP_CHECK(hipGetLastError());
}

// the reference's chain for the time slices [t0, t0 + nt): shifted fields are whole-lattice, made once per call (chunk 0) by the caller
struct ChainFields { ColorSpinorField *Fx[4], *Bx[4], *Fp[4], *Bp[4]; };

static void shiftFull(ColorSpinorField &out, const ColorSpinorField &in, int dir) {
  applyCovariantShift(out.Even(), in.Odd(), *gaugePrecise, 0, dir, 1.0, nullptr, 0.0);
  applyCovariantShift(out.Odd(), in.Even(), *gaugePrecise, 1, dir, 1.0, nullptr, 0.0);
}

static void chainChunk(double2 *cs, long S, int t0, const ColorSpinorField &x, const ColorSpinorField &phi, const ChainFields &F, const LatticeGeom &g) {
  const int stride = x.Stride();
  auto contract = [&](int k, const ColorSpinorField &u, const ColorSpinorField &v, double w, bool add) {
    hipLaunchKernelGGL(loop::pair_contract_kernel, dim3((unsigned)((S + 255) / 256)), dim3(256), 0, computeStream(), cs, S, k, (const double *)u.Even().V(),
                       (const double *)u.Odd().V(), (const double *)v.Even().V(), (const double *)v.Odd().V(), stride, g.X[0], g.X[1], g.X[2], t0, w, add ? 1 : 0);
    HIP_CHECK(hipGetLastError());
  };
  const size_t blk = (size_t)S * loop::NGM * sizeof(double2);
  auto copyBlock = [&](int dst, int src) {
    HIP_CHECK(hipMemcpyAsync(cs + (size_t)dst * S * loop::NGM, cs + (size_t)src * S * loop::NGM, blk, hipMemcpyDeviceToDevice, computeStream()));
  };
  // LOCAL (:366-390)
  contract(1, x, phi, 1.0, false);
  contract(0, x, x, -1.0, false);
  // generalised one-end trick (:397-444): S = term0 + term3 - term2 - term1 -> k = 10 + mu, C = the sum of the four -> k = 14 + mu
  for (int mu = 0; mu < 4; mu++) {
    const int kS = 10 + mu, kC = 14 + mu;
    contract(kS, x, *F.Fp[mu], 1.0, false);
    contract(kS, *F.Bx[mu], phi, 1.0, true);
    copyBlock(kC, kS);
    contract(kC, *F.Fx[mu], phi, 1.0, true);
    contract(kS, *F.Fx[mu], phi, -1.0, true);
    contract(kC, x, *F.Bp[mu], 1.0, true);
    contract(kS, x, *F.Bp[mu], -1.0, true);
  }
  // standard one-end trick (:446-490), subtracted from the accumulators: every weight negated
  for (int mu = 0; mu < 4; mu++) {
    const int kS = 2 + mu, kC = 6 + mu;
    contract(kS, x, *F.Fx[mu], -1.0, false);
    contract(kS, *F.Bx[mu], x, -1.0, true);
    copyBlock(kC, kS);
    contract(kC, *F.Fx[mu], x, -1.0, true);
    contract(kS, *F.Fx[mu], x, 1.0, true);
    contract(kC, x, *F.Bx[mu], -1.0, true);
    contract(kS, x, *F.Bx[mu], 1.0, true);
  }
}

// A += scale * the 18 blocks of the vector x (full fp64 device field as the solver leaves it), projected onto A's momenta
void loopContractAdd(LoopAccum &A, ColorSpinorField &x, QudaInvertParam *param, double scale) {
  using namespace loop;
  if (scale != 1.0) {   // the blocks of x alone in a second accumulator of the same shape, then one weighted add: the kernels below stay as they are
    MomAccum one(A.nblk, A.moms);
    loopContractAdd(one, x, param, 1.0);
    const long n = (long)A.nblk * A.Lt * (long)A.per();
    hipLaunchKernelGGL(accum_scaled_add_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, computeStream(), (double *)A.d, (const double *)one.d, scale, n);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipStreamSynchronize(computeStream()));
    return;
  }
  if (!gaugePrecise) errorQuda("loop contraction: Gauge field not allocated");
  if (x.Location() != QUDA_CUDA_FIELD_LOCATION || x.Precision() != QUDA_DOUBLE_PRECISION || x.SiteSubset() != QUDA_FULL_SITE_SUBSET || x.Nspin() != 4 || x.Ncolor() != 3)
    errorQuda("loop contraction: expected a full fp64 device spinor");
  if (gaugePrecise->precision != QUDA_DOUBLE_PRECISION) errorQuda("loop contraction: the resident precise links must be fp64 (cuda_prec of the gauge field)");
  const LatticeGeom &g = residentGeom();
  const CommGrid &cg = commGrid();
  const int Vs = g.X[0] * g.X[1] * g.X[2];
  hipStream_t st = computeStream();
  hipEvent_t ev[3];   // start, phi made, ghost zones / shifted fields made
  for (int i = 0; i < 3; i++) HIP_CHECK(hipEventCreate(&ev[i]));
  HIP_CHECK(hipEventRecord(ev[0], st));

  if (x.TwistFlavor() != QUDA_TWIST_PLUS && x.TwistFlavor() != QUDA_TWIST_MINUS) x.changeTwist(QUDA_TWIST_PLUS);   // mu = 0: the flavour does not enter
  ColorSpinorField phi(x);
  makePhi(phi, x, param);
  HIP_CHECK(hipEventRecord(ev[1], st));

  static const int tchunk = [] { const char *e = getenv("QUDA_AMD_LOOP_TCHUNK"); return e ? atoi(e) : 0; }();   // measurement aid: time slices per chunk
  int gx[3];
  for (int d = 0; d < 3; d++) gx[d] = cg.coords[d] * g.X[d];
  double secs[2];
  const bool fused = fusedEnabled();
  if (fused) {
    LoopArg arg;
    memset(&arg, 0, sizeof(arg));
    arg.x[0] = (const double *)x.Even().V(); arg.x[1] = (const double *)x.Odd().V();
    arg.phi[0] = (const double *)phi.Even().V(); arg.phi[1] = (const double *)phi.Odd().V();
    arg.sp_stride = x.Stride();
    if (phi.Stride() != x.Stride()) errorQuda("loop contraction: stride mismatch");
    fillStencilGeom(arg, *gaugePrecise, g, cg);
    GhostZones ghosts(arg, {&x, &phi}, g, cg);
    HIP_CHECK(hipEventRecord(ev[2], st));
    stageAndProject(A, gx, tchunk, [&](int t0, int nt, double2 *cs) {
      arg.t0 = t0; arg.S = (long)nt * Vs; arg.cs = cs;
      launchByRecon((int)gaugePrecise->reconstruct, loop_fused_kernel<18>, loop_fused_kernel<12>, loop_fused_kernel<8>, dim3((unsigned)((arg.S + 31) / 32)), dim3(256), arg);
    }, secs);
  } else {
    ChainFields F;
    for (int mu = 0; mu < 4; mu++) {
      F.Fx[mu] = new ColorSpinorField(x); F.Bx[mu] = new ColorSpinorField(x); F.Fp[mu] = new ColorSpinorField(x); F.Bp[mu] = new ColorSpinorField(x);
      shiftFull(*F.Fx[mu], x, 2 * mu); shiftFull(*F.Bx[mu], x, 2 * mu + 1);
      shiftFull(*F.Fp[mu], phi, 2 * mu); shiftFull(*F.Bp[mu], phi, 2 * mu + 1);
    }
    HIP_CHECK(hipEventRecord(ev[2], st));
    stageAndProject(A, gx, tchunk, [&](int t0, int nt, double2 *cs) { chainChunk(cs, (long)nt * Vs, t0, x, phi, F, g); }, secs);
    for (int mu = 0; mu < 4; mu++) { delete F.Fx[mu]; delete F.Bx[mu]; delete F.Fp[mu]; delete F.Bp[mu]; }
  }
  p2pCheck("loopContractAdd");
  // total: up to the first chunk, then the chunks; the covariant shifts of the chain run before the first chunk and count as its stencil
  g_loopSecs[0] = elapsedSecs(ev[0], ev[1]); g_loopSecs[2] = secs[1];
  g_loopSecs[3] = elapsedSecs(ev[0], ev[2]) + secs[0] + secs[1];
  g_loopSecs[1] = fused ? secs[0] : g_loopSecs[3] - g_loopSecs[0] - g_loopSecs[2];
  for (int i = 0; i < 3; i++) (void)hipEventDestroy(ev[i]);
}

static const char *const loopTypeName[6] = {"Scalar", "dOp", "Loops", "LoopsCv", "LpsDw", "LpsDwCv"};
static const bool loopTypeOneD[6] = {false, false, true, true, true, true};
static const int loopTypeFirst[6] = {0, 1, 2, 6, 10, 14};

// writeLoops_ASCII: one file per loop type and time rank r, holding that rank's time slices; rank 0 writes them all.
// tsmTag = nullptr: <pref>_<type>.loop.<NNNN>.<nT>_<r>; "NLP" / "NHP": <pref>_<tag><NNNN>_<type>.loop.<nT>_<r>; nnnn < 0 (the exact part): <pref>_<type>.loop.<nT>_<r>
void loopWriteAscii(const LoopAccum &A, const char *pref, const char *tsmTag, int nnnn) {
  const CommGrid &cg = commGrid();
  const int Lt = A.Lt, nT = cg.dims[3], T = Lt * nT, Nm = A.Nm;
  std::vector<double> glob((size_t)loop::NBLK * T * Nm * loop::NGM * 2);
  A.get(glob.data());   // collective: [18][T global][Nmoms][16][re, im], the same numbers on every rank
  if (cg.rank != 0) return;
  for (int type = 0; type < 6; type++)
    for (int r = 0; r < nT; r++) {
      char name[1024];
      if (tsmTag) snprintf(name, sizeof(name), "%s_%s%04d_%s.loop.%d_%d", pref, tsmTag, nnnn, loopTypeName[type], nT, r);
      else if (nnnn < 0) snprintf(name, sizeof(name), "%s_%s.loop.%d_%d", pref, loopTypeName[type], nT, r);
      else snprintf(name, sizeof(name), "%s_%s.loop.%04d.%d_%d", pref, loopTypeName[type], nnnn, nT, r);
      for (int mu = 0; mu < (loopTypeOneD[type] ? 4 : 1); mu++) {
        FILE *f = fopen(name, mu == 0 ? "w" : "a");
        if (!f) errorQuda("Cannot open %s to write the loop", name);
        const int k = loopTypeFirst[type] + mu;
        for (int ip = 0; ip < Nm; ip++)
          for (int lt = 0; lt < Lt; lt++) {
            const int t = lt + r * Lt;
            for (int gm = 0; gm < 16; gm++) {
              const double *v = &glob[((((size_t)k * T + t) * Nm + ip) * loop::NGM + gm) * 2];
              if (loopTypeOneD[type])
                fprintf(f, "%02d %02d %02d %+d %+d %+d %+16.15e %+16.15e\n", t, gm, mu, A.moms[3 * ip], A.moms[3 * ip + 1], A.moms[3 * ip + 2], 0.25 * v[0], 0.25 * v[1]);
              else
                fprintf(f, "%02d %02d %+d %+d %+d %+16.15e %+16.15e\n", t, gm, A.moms[3 * ip], A.moms[3 * ip + 1], A.moms[3 * ip + 2], v[0], v[1]);
            }
          }
        fclose(f);
      }
    }
}

static bool g_loopOutput = false;
bool loopOutputEnabled() { return g_loopOutput; }

}  // namespace quda

using namespace quda;

extern "C" {

int qudaAmdLoopMomenta(const int L[3], int Q_sq, int *moms, int max_moms) {
  if (!L || L[0] < 1 || L[1] < 1 || L[2] < 1 || Q_sq < 0) errorQuda("qudaAmdLoopMomenta: bad extents or Q_sq = %d", Q_sq);
  return copyMomenta(loopMomenta(L, Q_sq), moms, max_moms, "qudaAmdLoopMomenta");
}

void qudaAmdSetLoopOutput(int enable) { g_loopOutput = enable != 0; }

void qudaAmdContractLoop(double *out, const void *h_solution, QudaInvertParam *param, int Q_sq) {
  if (!gaugePrecise) errorQuda("qudaAmdContractLoop: Gauge field not allocated");
  if (!out || !h_solution || !param) errorQuda("qudaAmdContractLoop: NULL argument");
  const LatticeGeom &g = residentGeom();
  const QudaTwistFlavorType fl = (param->twist_flavor == QUDA_TWIST_MINUS) ? QUDA_TWIST_MINUS : QUDA_TWIST_PLUS;
  ColorSpinorParam cp = deviceSpinorParam(QUDA_DOUBLE_PRECISION, QUDA_FULL_SITE_SUBSET, fl);
  cp.create = QUDA_ZERO_FIELD_CREATE;
  ColorSpinorField v(cp);
  lexToDevice(v, (const double *)h_solution, g, true);
  LoopAccum *A = loopAccumCreate(Q_sq);
  loopContractAdd(*A, v, param);
  A->get(out);
  delete A;
}

void qudaAmdLoopLastTimings(double secs[4]) {
  for (int i = 0; i < 4; i++) secs[i] = g_loopSecs[i];
}

}  // extern "C"
