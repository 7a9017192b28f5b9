// clover_force.hip — the clover part of the twisted-clover fermion force and the force of the clover determinant (DESIGN §3
// "Twisted-clover force"): the derivative of the clover term with respect to the links, and the two site-local kernels that feed it.
//
// A tensor field T holds six 3x3 colour matrices per site, one per plane f = mu (mu - 1) / 2 + nu (nu < mu: F10, F20, F21, F30, F31, F32).
//
// Derivative.  L_T(U) = sum_x sum_f Re tr(T_f(x) F_f(x; U)), F = (Q - Q^dag) / 8 the clover-leaf field strength, and G[T] its force:
// sum_links Re tr(Theta G) = d/d eps L_T(exp(eps Theta) U).  With K_mu_nu = (T_f - T_f^dag) / 8 = -K_nu_mu, L_T is the sum over all
// plaquettes and their four corners c of Re tr(K(c) P_c), P_c the plaquette read from c.  The link (x, mu) lies, for each nu != mu, in the
// plaquette above and the one below it; read from the link in the orientation that does not dagger it, each is U_mu(x) a b c with three
// more links, and the derivative puts K at each corner the walk passes:
//   V += K(c0) a b c + a K(c1) b c + a b K(c2) c + a b c K(c3)          G_mu(x) = TA(U_mu(x) V)
//   above: a b c = U_nu(x + mu) U_mu(x + nu)^dag U_nu(x)^dag,            corners x + mu, x + mu + nu, x + nu, x,    K = K_mu_nu
//   below: a b c = U_nu(x + mu - nu)^dag U_mu(x - nu)^dag U_nu(x - nu),  corners x + mu, x + mu - nu, x - nu, x,    K = K_nu_mu
// The four insertions share the running products: S = K0 a + a K1; S = S b + (a b) K2; S = S c + (a b c) K3 is 8 products of 3x3
// matrices per plaquette, 48 per link, and one more in force_epilogue.  A gather without atomics: one thread per (site, parity, direction),
// a wave per direction and the four directions of 64 sites in one block, as ferm_force_kernel.  Every link comes through load_link, so
// the anti-periodic sign (stored in 18-real links, put back through tsign on reconstructed ones) cancels within each plaquette; in a
// direction of extent 2 the sites x + nu and x - nu coincide and both plaquettes are still walked.  Unpartitioned lattices only.
//
// sigma outer product   T_f(x) (+)= sum_i c_i[parity] sum_s phase_f(s) X_i(x)[perm_f(s), b] conj(Y_i(x)[s, a])       (element [b][a])
// sigma trace           T_f(x) (+)= c[parity] sum_s phase_f(s) B(x)[(perm_f(s), b), (s, a)],   B = A (A^2 + mu2)^-1
// sigma_mu_nu = (i / 2) [gamma_mu, gamma_nu] in the chiral (DeGrand-Rossi) basis of the device spinors has one entry per row:
// (sigma_f)[s][perm_f(s)] = i^k_f(s), and it does not mix the chiralities, so B enters through its two 6x6 blocks.  One thread per
// (site, parity, plane): a wave per plane, the six planes of 64 sites in one block.
#include "dispatch.h"
#include "gauge_device.h"

#include <cmath>
#include <cstring>

namespace quda {

// ---- the tensor field ----
static constexpr size_t kPlaneDoubles = 48;   // per site of one parity pair: 2 x 24 (a MatField)
__host__ __device__ inline MatField tensorPlane(double *T, int Vh, int f) { return {T + (size_t)f * kPlaneDoubles * Vh, Vh}; }

// host order [site][f][3][3][re, im] <-> the six planar matrix fields
__global__ void __launch_bounds__(384) tensor_load_kernel(double *T, const double *host, int Vh) {
  const int gid = blockIdx.x * 64 + (threadIdx.x & 63);
  if (gid >= 2 * Vh) return;
  const int f = threadIdx.x >> 6, par = gid >= Vh, idx = gid - par * Vh;
  const double *h = host + ((size_t)gid * 6 + f) * 18;
  M3 m;
#pragma unroll
  for (int k = 0; k < 9; k++) { m.re[k] = h[2 * k]; m.im[k] = h[2 * k + 1]; }
  mf_store(m, tensorPlane(T, Vh, f), par, idx);
}
__global__ void __launch_bounds__(384) tensor_save_kernel(double *host, double *T, int Vh) {
  const int gid = blockIdx.x * 64 + (threadIdx.x & 63);
  if (gid >= 2 * Vh) return;
  const int f = threadIdx.x >> 6, par = gid >= Vh, idx = gid - par * Vh;
  M3 m;
  mf_load(m, tensorPlane(T, Vh, f), par, idx);
  double *h = host + ((size_t)gid * 6 + f) * 18;
#pragma unroll
  for (int k = 0; k < 9; k++) { h[2 * k] = m.re[k]; h[2 * k + 1] = m.im[k]; }
}

TensorField::TensorField(const LatticeGeom &g) : geom(g), bytes((size_t)6 * kPlaneDoubles * g.Vh * sizeof(double)), data(nullptr) {
  HIP_CHECK(qaMalloc((void **)&data, bytes));
  HIP_CHECK(hipMemsetAsync(data, 0, bytes, computeStream()));
}
TensorField::~TensorField() { if (data) (void)hipFree(data); }
void TensorField::load(const double *h_tensor) {
  const size_t n = (size_t)geom.V * 108 * sizeof(double);
  double *stage = (double *)stagingBuffer(n);
  hipStream_t s = computeStream();
  HIP_CHECK(hipMemcpyAsync(stage, h_tensor, n, hipMemcpyHostToDevice, s));
  hipLaunchKernelGGL(tensor_load_kernel, dim3((2 * geom.Vh + 63) / 64), dim3(384), 0, s, data, stage, geom.Vh);
  HIP_CHECK(hipGetLastError());
  HIP_CHECK(hipStreamSynchronize(s));
}
void TensorField::save(double *h_tensor) const {
  const size_t n = (size_t)geom.V * 108 * sizeof(double);
  double *stage = (double *)stagingBuffer(n);
  hipStream_t s = computeStream();
  hipLaunchKernelGGL(tensor_save_kernel, dim3((2 * geom.Vh + 63) / 64), dim3(384), 0, s, stage, data, geom.Vh);
  HIP_CHECK(hipGetLastError());
  HIP_CHECK(hipMemcpyAsync(h_tensor, stage, n, hipMemcpyDeviceToHost, s));
  HIP_CHECK(hipStreamSynchronize(s));
}

// the launch between two device events; its time counts towards fermForceLastKernelSecs
template <typename Launch> static void timedLaunch(Launch &&launch) {
  hipStream_t s = computeStream();
  hipEvent_t ev[2];
  for (int k = 0; k < 2; k++) HIP_CHECK(hipEventCreate(&ev[k]));
  HIP_CHECK(hipEventRecord(ev[0], s));
  launch(s);
  HIP_CHECK(hipGetLastError());
  HIP_CHECK(hipEventRecord(ev[1], s));
  HIP_CHECK(hipStreamSynchronize(s));
  float ms = 0;
  HIP_CHECK(hipEventElapsedTime(&ms, ev[0], ev[1]));
  fermForceAddKernelSecs(1e-3 * ms, false);
  for (int k = 0; k < 2; k++) (void)hipEventDestroy(ev[k]);
}

// ---- sigma in the chiral basis: row s of sigma_f has the single entry i^phase(s) in column perm(s) ----
template <int F> struct Sigma {
  static constexpr bool swap = !(F == 0 || F == 5);   // F10 and F32 are diagonal, the others exchange the spins within a chirality
  __host__ __device__ static constexpr int perm(int s) { return swap ? (s ^ 1) : s; }
  __host__ __device__ static constexpr int phase(int s) {
    return F == 0 ? ((s & 1) ? 0 : 2) : F == 1 ? ((s & 1) ? 3 : 1) : F == 2 ? 2 : F == 3 ? (s < 2 ? 0 : 2) : F == 4 ? ((s == 0 || s == 3) ? 1 : 3) : ((s == 0 || s == 3) ? 0 : 2);
  }
};
// (ar, ai) += i^k (zr, zi); k is a constant once the spin loops are unrolled
__device__ __forceinline__ void acc_phase(int k, double &ar, double &ai, double zr, double zi) {
  if (k == 0) { ar += zr; ai += zi; }
  else if (k == 1) { ar -= zi; ai += zr; }
  else if (k == 2) { ar -= zr; ai -= zi; }
  else { ar += zi; ai -= zr; }
}
// T_f(x) = (accumulate ? T_f(x) : 0) + (cr + i ci) m
__device__ __forceinline__ void tensor_update(double *T, int Vh, int f, int par, int idx, const M3 &m, double cr, double ci, int accumulate) {
  M3 o;
  const MatField P = tensorPlane(T, Vh, f);
  if (accumulate) mf_load(o, P, par, idx);
  else {
#pragma unroll
    for (int k = 0; k < 9; k++) o.re[k] = o.im[k] = 0;
  }
#pragma unroll
  for (int k = 0; k < 9; k++) { o.re[k] += cr * m.re[k] - ci * m.im[k]; o.im[k] += cr * m.im[k] + ci * m.re[k]; }
  mf_store(o, P, par, idx);
}

// ---- sigma outer product ----
struct SigmaOprodArg {
  double *T;
  int Vh, n, sp_stride, accumulate;
  const double *x[kFermForceMaxFields][2], *y[kFermForceMaxFields][2];      // parity blocks (even, odd)
  double cr[kFermForceMaxFields][2], ci[kFermForceMaxFields][2];
};
template <int F> __device__ __forceinline__ void sigma_oprod_plane(M3 &acc, const SigmaOprodArg &a, int par, int idx) {
  for (int i = 0; i < a.n; i++) {
    double X[24], Y[24];
    Planar<double, 24>::load(X, a.x[i][par], a.sp_stride, idx, nullptr, idx);
    Planar<double, 24>::load(Y, a.y[i][par], a.sp_stride, idx, nullptr, idx);
    const double cr = a.cr[i][par], ci = a.ci[i][par];
#pragma unroll
    for (int b = 0; b < 3; b++)
#pragma unroll
      for (int c = 0; c < 3; c++) {
        double re = 0, im = 0;
#pragma unroll
        for (int s = 0; s < 4; s++) {
          const double xr = X[6 * Sigma<F>::perm(s) + 2 * b], xi = X[6 * Sigma<F>::perm(s) + 2 * b + 1], yr = Y[6 * s + 2 * c], yi = Y[6 * s + 2 * c + 1];
          acc_phase(Sigma<F>::phase(s), re, im, xr * yr + xi * yi, xi * yr - xr * yi);
        }
        acc.re[3 * b + c] += cr * re - ci * im; acc.im[3 * b + c] += cr * im + ci * re;
      }
  }
}
__global__ void __launch_bounds__(384) sigma_oprod_kernel(const SigmaOprodArg a) {
  const int gid = blockIdx.x * 64 + (threadIdx.x & 63);
  if (gid >= 2 * a.Vh) return;
  const int f = threadIdx.x >> 6, par = gid >= a.Vh, idx = gid - par * a.Vh;
  M3 acc;
#pragma unroll
  for (int k = 0; k < 9; k++) acc.re[k] = acc.im[k] = 0;
  switch (f) {
    case 0: sigma_oprod_plane<0>(acc, a, par, idx); break;
    case 1: sigma_oprod_plane<1>(acc, a, par, idx); break;
    case 2: sigma_oprod_plane<2>(acc, a, par, idx); break;
    case 3: sigma_oprod_plane<3>(acc, a, par, idx); break;
    case 4: sigma_oprod_plane<4>(acc, a, par, idx); break;
    default: sigma_oprod_plane<5>(acc, a, par, idx); break;
  }
  tensor_update(a.T, a.Vh, f, par, idx, acc, 1.0, 0.0, a.accumulate);
}

static void checkSigmaField(const ColorSpinorField *f, const ColorSpinorField *like, const LatticeGeom &g) {
  if (!f || f->Location() != QUDA_CUDA_FIELD_LOCATION || f->Precision() != QUDA_DOUBLE_PRECISION || f->SiteSubset() != QUDA_PARITY_SITE_SUBSET || f->Nspin() != 4 ||
      f->Ncolor() != 3 || f->Nflavor() != 1)
    errorQuda("clover sigma outer product: expected fp64 one-flavour device parity spinors");
  if (f->Stride() != like->Stride() || f->VolumeCB4() != g.Vh)
    errorQuda("clover sigma outer product: the fields differ in stride or volume (stride %d, %d sites per parity against %d, %d)", f->Stride(), f->VolumeCB4(),
              like->Stride(), g.Vh);
}

void cloverSigmaOprod(TensorField &T, const std::vector<SigmaOprodPair> &pairs, bool accumulate) {
  const size_t n = pairs.size();
  if (!n) errorQuda("clover sigma outer product: no fields");
  const LatticeGeom &geom = T.geom;
  for (const SigmaOprodPair &p : pairs)
    for (int q = 0; q < 2; q++) { checkSigmaField(p.x[q], pairs[0].x[0], geom); checkSigmaField(p.y[q], pairs[0].x[0], geom); }
  for (size_t first = 0; first < n; first += kFermForceMaxFields) {
    const size_t last = first + kFermForceMaxFields < n ? first + kFermForceMaxFields : n;
    SigmaOprodArg arg;
    memset(&arg, 0, sizeof(arg));
    arg.T = T.data;
    arg.Vh = geom.Vh;
    arg.sp_stride = pairs[0].x[0]->Stride();
    arg.accumulate = accumulate || first > 0;
    for (size_t i = first; i < last; i++) {
      const int k = arg.n++;
      for (int q = 0; q < 2; q++) {
        arg.x[k][q] = (const double *)pairs[i].x[q]->V(); arg.y[k][q] = (const double *)pairs[i].y[q]->V();
        arg.cr[k][q] = pairs[i].cr[q]; arg.ci[k][q] = pairs[i].ci[q];
      }
    }
    timedLaunch([&](hipStream_t s) { hipLaunchKernelGGL(sigma_oprod_kernel, dim3((2 * geom.Vh + 63) / 64), dim3(384), 0, s, arg); });
  }
}

// ---- sigma trace of B = A (A^2 + mu2)^-1 ----
// element (i, j) of a Hermitian 6x6 block in packed order (6 diagonal reals, then the 15 strictly-lower entries column by column)
__device__ __forceinline__ void herm_elem(double &re, double &im, const double *C, int i, int j) {
  if (i == j) { re = C[i]; im = 0; }
  else if (i > j) { const int k = 15 - (6 - j) * (5 - j) / 2 + i - j - 1; re = C[6 + 2 * k]; im = C[6 + 2 * k + 1]; }
  else { const int k = 15 - (6 - i) * (5 - i) / 2 + j - i - 1; re = C[6 + 2 * k]; im = -C[6 + 2 * k + 1]; }
}
struct SigmaTraceArg {
  double *T;
  const char *A, *Ainv;       // fp64 clover blocks and their (twisted) inverse
  size_t parity_bytes;
  int Vh, cl_stride, accumulate, product;   // product 0: the stored inverse is A^-1 (an untwisted field), which is B itself
  double cr[2], ci[2];
};
template <int F> __device__ __forceinline__ void sigma_trace_plane(M3 &acc, const SigmaTraceArg &a, int par, int idx) {
  // one chirality at a time (not unrolled: the blocks of both in flight at once are 288 registers); the phase is then a wave-uniform
  // run-time value that only selects the arithmetic, the register indices stay static
#pragma unroll 1
  for (int chi = 0; chi < 2; chi++) {
    double C[36], D[36];
    const size_t off = (size_t)par * a.parity_bytes + (size_t)chi * 36 * sizeof(double) * a.cl_stride;
    Planar<double, 36>::load(D, a.Ainv + off, a.cl_stride, idx, nullptr, idx);
    if (a.product) Planar<double, 36>::load(C, a.A + off, a.cl_stride, idx, nullptr, idx);
#pragma unroll
    for (int sl = 0; sl < 2; sl++) {
      const int s = 2 * chi + sl, pl = Sigma<F>::perm(s) - 2 * chi;   // the row spin within the block
#pragma unroll
      for (int b = 0; b < 3; b++)
#pragma unroll
        for (int c = 0; c < 3; c++) {
          // B[(pl, b), (sl, c)]
          double re = 0, im = 0;
          if (a.product) {
#pragma unroll
            for (int k = 0; k < 6; k++) {
              double ar, ai, dr, di;
              herm_elem(ar, ai, C, 3 * pl + b, k);
              herm_elem(dr, di, D, k, 3 * sl + c);
              re += ar * dr - ai * di; im += ar * di + ai * dr;
            }
          } else {
            herm_elem(re, im, D, 3 * pl + b, 3 * sl + c);
          }
          acc_phase(Sigma<F>::phase(s), acc.re[3 * b + c], acc.im[3 * b + c], re, im);
        }
    }
  }
}
__global__ void __launch_bounds__(384) sigma_trace_kernel(const SigmaTraceArg a) {
  const int gid = blockIdx.x * 64 + (threadIdx.x & 63);
  if (gid >= 2 * a.Vh) return;
  const int f = threadIdx.x >> 6, par = gid >= a.Vh, idx = gid - par * a.Vh;
  M3 acc;
#pragma unroll
  for (int k = 0; k < 9; k++) acc.re[k] = acc.im[k] = 0;
  switch (f) {
    case 0: sigma_trace_plane<0>(acc, a, par, idx); break;
    case 1: sigma_trace_plane<1>(acc, a, par, idx); break;
    case 2: sigma_trace_plane<2>(acc, a, par, idx); break;
    case 3: sigma_trace_plane<3>(acc, a, par, idx); break;
    case 4: sigma_trace_plane<4>(acc, a, par, idx); break;
    default: sigma_trace_plane<5>(acc, a, par, idx); break;
  }
  tensor_update(a.T, a.Vh, f, par, idx, acc, a.cr[par], a.ci[par], a.accumulate);
}

void cloverSigmaTrace(TensorField &T, const CloverField &clover, const double cr[2], const double ci[2], bool accumulate) {
  if (!(clover.geom == T.geom)) errorQuda("clover sigma trace: clover and tensor geometry differ");
  if (clover.precision != QUDA_DOUBLE_PRECISION) errorQuda("clover sigma trace: the clover term is held in precision %d; an fp64 clover field (clover_cuda_prec) is needed", clover.precision);
  SigmaTraceArg arg;
  memset(&arg, 0, sizeof(arg));
  arg.T = T.data;
  arg.A = (const char *)clover.clover; arg.Ainv = (const char *)clover.cloverInv;
  arg.parity_bytes = clover.parity_bytes;
  arg.Vh = T.geom.Vh; arg.cl_stride = clover.stride;
  arg.accumulate = accumulate;
  arg.product = clover.twisted;
  for (int q = 0; q < 2; q++) { arg.cr[q] = cr[q]; arg.ci[q] = ci[q]; }
  timedLaunch([&](hipStream_t s) { hipLaunchKernelGGL(sigma_trace_kernel, dim3((2 * arg.Vh + 63) / 64), dim3(384), 0, s, arg); });
}

// ---- the derivative of the clover term ----
struct CloverDerivArg {
  GaugeView g;
  double *mom, *T;
  int Vh;
  double coeff;
};
// c += a b
__device__ __forceinline__ void m3_mac(M3 &c, const M3 &a, const M3 &b) {
#pragma unroll
  for (int i = 0; i < 3; i++)
#pragma unroll
    for (int j = 0; j < 3; j++) {
      double r = c.re[i * 3 + j], m = c.im[i * 3 + j];
#pragma unroll
      for (int k = 0; k < 3; k++) { r += a.re[i * 3 + k] * b.re[k * 3 + j] - a.im[i * 3 + k] * b.im[k * 3 + j]; m += a.re[i * 3 + k] * b.im[k * 3 + j] + a.im[i * 3 + k] * b.re[k * 3 + j]; }
      c.re[i * 3 + j] = r; c.im[i * 3 + j] = m;
    }
}
// c = x + dm mu^ + dn nu^; mu and nu are wave-uniform and the coordinates stay in registers (static indices)
__device__ __forceinline__ void corner(int *c, const int *x, int mu, int dm, int nu, int dn) {
#pragma unroll
  for (int d = 0; d < 4; d++) c[d] = x[d] + (d == mu ? dm : 0) + (d == nu ? dn : 0);
}
// K = s (T_f - T_f^dag) / 8 at the coordinates xin, one step outside the lattice at most
__device__ __forceinline__ void load_k(M3 &K, const CloverDerivArg &a, int f, double s, const int *xin) {
  int x[4];
#pragma unroll
  for (int d = 0; d < 4; d++) { x[d] = xin[d]; if (x[d] < 0) x[d] += a.g.X[d]; if (x[d] >= a.g.X[d]) x[d] -= a.g.X[d]; }
  const int par = (x[0] + x[1] + x[2] + x[3]) & 1;
  const int idx = (((x[3] * a.g.X[2] + x[2]) * a.g.X[1] + x[1]) * a.g.X[0] + x[0]) >> 1;
  mf_load(K, tensorPlane(a.T, a.Vh, f), par, idx);
  const double h = 0.125 * s;
  // in place, a pair (i, j), (j, i) at a time: K_ij = h (t_ij - conj t_ji), K_ji = -conj K_ij; the diagonal keeps its imaginary part
#pragma unroll
  for (int i = 0; i < 3; i++) {
    K.re[4 * i] = 0; K.im[4 * i] *= 2.0 * h;
#pragma unroll
    for (int j = i + 1; j < 3; j++) {
      const double re = h * (K.re[3 * i + j] - K.re[3 * j + i]), im = h * (K.im[3 * i + j] + K.im[3 * j + i]);
      K.re[3 * i + j] = re; K.im[3 * i + j] = im; K.re[3 * j + i] = -re; K.im[3 * j + i] = im;
    }
  }
}
// P <- P L or P L^dag, S <- S L(^dag) + P K(c): one more link of the walk and the insertion at the corner behind it
template <typename T, int R>
__device__ __forceinline__ void walk_step(M3 &S, M3 &P, const CloverDerivArg &a, int dir, const int *at, bool dag, int f, double s, const int *c) {
  M3 L;
  load_link<T, R>(L, a.g, dir, at);
  if (dag) { m3_mul_right_dag(S, L); m3_mul_right_dag(P, L); }
  else { m3_mul_right(S, L); m3_mul_right(P, L); }
  load_k(L, a, f, s, c);
  m3_mac(S, P, L);
}
// V += K(c0) a b c + a K(c1) b c + a b K(c2) c + a b c K(c3) for the plaquette above (side 0) or below (side 1) the link (x, mu) in nu
template <typename T, int R> __device__ __forceinline__ void add_plaquette(M3 &V, const CloverDerivArg &a, const int *x, int mu, int nu, int side) {
  const int f = mu > nu ? mu * (mu - 1) / 2 + nu : nu * (nu - 1) / 2 + mu;
  const double s = ((mu > nu) != (side != 0)) ? 1.0 : -1.0;   // K_mu_nu above, K_nu_mu = -K_mu_nu below
  const int dn = side ? -1 : 1;
  int c0[4], c1[4], c2[4], at[4];
  corner(c0, x, mu, 1, nu, 0);
  corner(c1, x, mu, 1, nu, dn);
  corner(c2, x, mu, 0, nu, dn);
  M3 S, P;
  // first link: U_nu(x + mu) above, U_nu(x + mu - nu)^dag below
  corner(at, x, mu, 1, nu, side ? -1 : 0);
  load_k(S, a, f, s, c0);
  load_link<T, R>(P, a.g, nu, at);
  if (side) { M3 t; m3_dag(t, P); P = t; }
  m3_mul_right(S, P);
  {
    M3 K;
    load_k(K, a, f, s, c1);
    m3_mac(S, P, K);
  }
  // second link: U_mu(x + nu)^dag above, U_mu(x - nu)^dag below
  walk_step<T, R>(S, P, a, mu, c2, true, f, s, c2);
  // third link: U_nu(x)^dag above, U_nu(x - nu) below
  corner(at, x, mu, 0, nu, side ? -1 : 0);   // (not side ? c2 : x: a run-time choice between two arrays puts both into scratch)
  walk_step<T, R>(S, P, a, nu, at, side == 0, f, s, x);
#pragma unroll
  for (int k = 0; k < 9; k++) { V.re[k] += S.re[k]; V.im[k] += S.im[k]; }
}

template <typename T, int R> __global__ void __launch_bounds__(256) clover_deriv_kernel(const CloverDerivArg a) {
  const int gid = blockIdx.x * 64 + (threadIdx.x & 63);
  if (gid >= 2 * a.Vh) return;
  const int mu = threadIdx.x >> 6;
  const int parity = gid >= a.Vh, idx = gid - parity * a.Vh;
  int x[4];
  {
    const int Xh = a.g.X[0] >> 1;
    int l = idx;
    const int xh = l % Xh; l /= Xh;
    x[1] = l % a.g.X[1]; l /= a.g.X[1];
    x[2] = l % a.g.X[2]; x[3] = l / a.g.X[2];
    x[0] = 2 * xh + ((x[1] + x[2] + x[3] + parity) & 1);
  }
  M3 V;
#pragma unroll
  for (int k = 0; k < 9; k++) V.re[k] = V.im[k] = 0;
  // the six plaquettes one after the other (not unrolled: the loads of several at once do not fit the register file)
#pragma unroll 1
  for (int nu = 0; nu < 4; nu++) {
    if (nu == mu) continue;
#pragma unroll 1
    for (int side = 0; side < 2; side++) add_plaquette<T, R>(V, a, x, mu, nu, side);
  }
  M3 U;
  load_link<T, R>(U, a.g, mu, x);
  force_epilogue(a.mom + ((size_t)gid * 4 + mu) * 10, U, V, -a.coeff);   // mom <- TA(mom + coeff U V)
}

void checkCloverDerivativeUnpartitioned(const char *fn) {
  const CommGrid &cg = commGrid();
  int mask = 0;
  for (int d = 0; d < 4; d++) if (cg.partitioned(d)) mask |= 1 << d;
  if (mask)
    errorQuda("%s: the derivative of the clover term needs links and tensors two hops away and runs on unpartitioned lattices only (partitioned directions%s%s%s%s, mask 0x%x)",
              fn, mask & 1 ? " x" : "", mask & 2 ? " y" : "", mask & 4 ? " z" : "", mask & 8 ? " t" : "", mask);
}

void cloverDerivativeForce(MomField &mom, const GaugeField &U, const TensorField &T, double coeff) {
  checkCloverDerivativeUnpartitioned("cloverDerivativeForce");
  if (!(U.geom == mom.geom) || !(U.geom == T.geom)) errorQuda("clover derivative: gauge, momentum and tensor geometry differ");
  CloverDerivArg arg;
  memset(&arg, 0, sizeof(arg));
  arg.g = viewOf(U);
  arg.mom = mom.data;
  arg.T = T.data;
  arg.Vh = U.geom.Vh;
  arg.coeff = coeff;
  const int nb = (2 * arg.Vh + 63) / 64;
  timedLaunch([&](hipStream_t s) {
    forLinkType(U, [&](auto t, auto r) { hipLaunchKernelGGL((clover_deriv_kernel<decltype(t), decltype(r)::value>), dim3(nb), dim3(256), 0, s, arg); });
  });
}

}  // namespace quda
