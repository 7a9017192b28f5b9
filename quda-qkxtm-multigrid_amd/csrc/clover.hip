// clover.hip — the clover term: storage, upload and download in the packed host order, the (twisted) inverse, and the construction
// from the resident links, by direct gathers or by transport (the leaves: gauge_obs.hip cloverLeaves).  Reference behaviour
// restated: lib/clover_invert.cu:56-85 (twisted inverse), lib/field_strength_tensor.cu, lib/clover_quda.cu (construction).
#include "dispatch.h"
#include "gauge_device.h"

#include <cmath>

namespace quda {

CloverField::CloverField(const LatticeGeom &g, QudaPrecision prec)
    : geom(g), precision(prec), stride(g.Vh + gaugePadSites()), clover(nullptr), cloverInv(nullptr), norm(nullptr), invNorm(nullptr), twisted(false), mu2(0) {
  parity_bytes = alignUp((size_t)stride * 72 * (int)prec, 1024);
  bytes = 2 * parity_bytes;
  HIP_CHECK(qaMalloc(&clover, bytes));
  HIP_CHECK(qaMalloc(&cloverInv, bytes));
  parity_norm_bytes = 0;
  if (prec == QUDA_HALF_PRECISION) {
    parity_norm_bytes = (size_t)2 * stride * sizeof(float);
    HIP_CHECK(qaMalloc((void **)&norm, 2 * parity_norm_bytes));
    HIP_CHECK(qaMalloc((void **)&invNorm, 2 * parity_norm_bytes));
  }
  trlog[0] = trlog[1] = 0;
  coeff = NAN;
}
CloverField::~CloverField() {
  if (clover) (void)hipFree(clover);
  if (cloverInv) (void)hipFree(cloverInv);
  if (norm) (void)hipFree(norm);
  if (invNorm) (void)hipFree(invNorm);
}

template <typename TDev, typename THost>
__global__ void clover_load_kernel(char *dev, float *norm, size_t parity_bytes, int stride, const THost *host, int Vh) {
  using real = typename Store<TDev>::real;
  const int gid = blockIdx.x * blockDim.x + threadIdx.x;
  if (gid >= 2 * Vh) return;
  const int parity = gid >= Vh, idx = gid - parity * Vh;
#pragma unroll
  for (int chi = 0; chi < 2; chi++) {
    real C[36];
    const THost *h = host + (((size_t)parity * Vh + idx) * 2 + chi) * 36;
#pragma unroll
    for (int k = 0; k < 36; k++) C[k] = (real)h[k];
    Planar<TDev, 36>::store(C, dev + (size_t)parity * parity_bytes + (size_t)chi * 36 * sizeof(TDev) * stride, stride, idx,
                            norm ? norm + (size_t)parity * 2 * stride : nullptr, chi * stride + idx);
  }
}

template <typename TDev, typename THost>
__global__ void clover_save_kernel(THost *host, const char *dev, const float *norm, size_t parity_bytes, int stride, int Vh) {
  using real = typename Store<TDev>::real;
  const int gid = blockIdx.x * blockDim.x + threadIdx.x;
  if (gid >= 2 * Vh) return;
  const int parity = gid >= Vh, idx = gid - parity * Vh;
#pragma unroll
  for (int chi = 0; chi < 2; chi++) {
    real C[36];
    Planar<TDev, 36>::load(C, dev + (size_t)parity * parity_bytes + (size_t)chi * 36 * sizeof(TDev) * stride, stride, idx,
                           norm ? norm + (size_t)parity * 2 * stride : nullptr, chi * stride + idx);
    THost *h = host + (((size_t)parity * Vh + idx) * 2 + chi) * 36;
#pragma unroll
    for (int k = 0; k < 36; k++) h[k] = (THost)C[k];
  }
}

// (A^2 + mu2)^-1 (squared == 0: A^-1) per chiral block, computed in fp64 registers by Gauss-Jordan on the
// Hermitian 6x6 (small, setup-time only; reference lib/clover_invert.cu:56-85 uses Cholesky).
template <typename TDev>
__global__ void clover_invert_kernel(char *inv, float *invNorm, const char *A, const float *Anorm, size_t parity_bytes, int stride, int Vh,
                                     double mu2, int squared, double *trlog) {
  using real = typename Store<TDev>::real;
  const int gid = blockIdx.x * blockDim.x + threadIdx.x;
  if (gid >= 2 * Vh) return;
  const int parity = gid >= Vh, idx = gid - parity * Vh;
  double tl = 0.0;
  for (int chi = 0; chi < 2; chi++) {
    real C[36];
    Planar<TDev, 36>::load(C, A + (size_t)parity * parity_bytes + (size_t)chi * 36 * sizeof(TDev) * stride, stride, idx,
                           Anorm ? Anorm + (size_t)parity * 2 * stride : nullptr, chi * stride + idx);
    double M[6][6][2], S[6][12][2];
    for (int r = 0; r < 6; r++)
      for (int c = 0; c < 6; c++) {
        if (r == c) { M[r][c][0] = C[r]; M[r][c][1] = 0; }
        else if (r > c) { const int k = 15 - (6 - c) * (5 - c) / 2 + r - c - 1; M[r][c][0] = C[6 + 2 * k]; M[r][c][1] = C[6 + 2 * k + 1]; }
        else { const int k = 15 - (6 - r) * (5 - r) / 2 + c - r - 1; M[r][c][0] = C[6 + 2 * k]; M[r][c][1] = -C[6 + 2 * k + 1]; }
      }
    for (int r = 0; r < 6; r++)
      for (int c = 0; c < 6; c++) {
        double re, im;
        if (squared) {
          re = 0; im = 0;
          for (int k = 0; k < 6; k++) {
            re += M[r][k][0] * M[k][c][0] - M[r][k][1] * M[k][c][1];
            im += M[r][k][0] * M[k][c][1] + M[r][k][1] * M[k][c][0];
          }
          if (r == c) re += mu2;
        } else { re = M[r][c][0]; im = M[r][c][1]; }
        S[r][c][0] = re; S[r][c][1] = im;
        S[r][c + 6][0] = r == c; S[r][c + 6][1] = 0;
      }
    for (int p = 0; p < 6; p++) {
      int best = p; double bm = 0;
      for (int r = p; r < 6; r++) { const double m = S[r][p][0] * S[r][p][0] + S[r][p][1] * S[r][p][1]; if (m > bm) { bm = m; best = r; } }
      if (best != p)
        for (int c = 0; c < 12; c++)
          for (int zz = 0; zz < 2; zz++) { const double tt = S[p][c][zz]; S[p][c][zz] = S[best][c][zz]; S[best][c][zz] = tt; }
      const double pr = S[p][p][0], pi = S[p][p][1], den = pr * pr + pi * pi;
      tl += 0.5 * log(den);
      const double ir = pr / den, ii = -pi / den;
      for (int c = 0; c < 12; c++) {
        const double re = S[p][c][0] * ir - S[p][c][1] * ii, im = S[p][c][0] * ii + S[p][c][1] * ir;
        S[p][c][0] = re; S[p][c][1] = im;
      }
      for (int r = 0; r < 6; r++) {
        if (r == p) continue;
        const double fr = S[r][p][0], fi = S[r][p][1];
        for (int c = 0; c < 12; c++) {
          S[r][c][0] -= fr * S[p][c][0] - fi * S[p][c][1];
          S[r][c][1] -= fr * S[p][c][1] + fi * S[p][c][0];
        }
      }
    }
    real O[36];
    for (int r = 0; r < 6; r++) O[r] = (real)S[r][r + 6][0];
    for (int c = 0; c < 6; c++)
      for (int r = c + 1; r < 6; r++) {
        const int k = 15 - (6 - c) * (5 - c) / 2 + r - c - 1;
        O[6 + 2 * k] = (real)(0.5 * (S[r][c + 6][0] + S[c][r + 6][0]));
        O[6 + 2 * k + 1] = (real)(0.5 * (S[r][c + 6][1] - S[c][r + 6][1]));
      }
    Planar<TDev, 36>::store(O, inv + (size_t)parity * parity_bytes + (size_t)chi * 36 * sizeof(TDev) * stride, stride, idx,
                            invNorm ? invNorm + (size_t)parity * 2 * stride : nullptr, chi * stride + idx);
  }
  if (trlog) atomicAdd(&trlog[parity], tl);
}

// ---- clover term from the gauge field (reference computeFmunu, lib/field_strength_tensor.cu:30-192, and computeClover,
// lib/clover_quda.cu:41-139): one thread per site builds the six clover-leaf field strengths F_mu_nu = (Q - Q^dag)/8 and folds
// them straight into the four 3x3 colour blocks of the two chiral blocks, B1[ch] = i c (F0 -/+ F5), B2[ch] = c (F1 +/- F4 -
// i (F2 -/+ F3)); each chiral block is [[1 - B1, B2^dag], [B2, 1 + B1]].  Arithmetic in fp64 whatever the link precision;
// output = the TRUE clover matrix in packed order (the reference's native order stores half of it). ----
// leaf = A^(dag) B^(dag) C^(dag) D^(dag) of the links (mu_k at x_k), accumulated into Q
template <typename T, int R>
__device__ __forceinline__ void add_leaf(M3 &Q, const GaugeView &g, int m0, const int *x0, bool d0, int m1, const int *x1, bool d1, int m2, const int *x2, bool d2,
                                         int m3, const int *x3, bool d3) {
  M3 a, b, t;
  load_link<T, R>(a, g, m0, x0); if (d0) { m3_dag(t, a); a = t; }
  load_link<T, R>(b, g, m1, x1); if (d1) { m3_dag(t, b); b = t; }
  m3_mul(t, a, b);
  load_link<T, R>(b, g, m2, x2); if (d2) { m3_dag(a, b); b = a; }
  m3_mul(a, t, b);
  load_link<T, R>(b, g, m3, x3); if (d3) { m3_dag(t, b); b = t; }
  m3_mul(t, a, b);
#pragma unroll
  for (int k = 0; k < 9; k++) { Q.re[k] += t.re[k]; Q.im[k] += t.im[k]; }
}

template <typename T, int R>
__global__ void __launch_bounds__(128) clover_from_gauge_kernel(double *packed, GaugeView g, double coeff, int Vh) {
  const int gid = blockIdx.x * blockDim.x + threadIdx.x;
  if (gid >= 2 * Vh) return;
  const int parity = gid >= Vh, idx = gid - parity * Vh;
  int x[4];
  {
    const int Xh = g.X[0] >> 1;
    int l = idx;
    const int xh = l % Xh; l /= Xh;
    x[1] = l % g.X[1]; l /= g.X[1];
    x[2] = l % g.X[2]; x[3] = l / g.X[2];
    x[0] = 2 * xh + ((x[1] + x[2] + x[3] + parity) & 1);
  }
  M3 b1[2], b2[2];
#pragma unroll
  for (int c = 0; c < 2; c++)
#pragma unroll
    for (int k = 0; k < 9; k++) { b1[c].re[k] = b1[c].im[k] = b2[c].re[k] = b2[c].im[k] = 0; }
  for (int mu = 1; mu < 4; mu++)
    for (int nu = 0; nu < mu; nu++) {
      M3 Q;
#pragma unroll
      for (int k = 0; k < 9; k++) Q.re[k] = Q.im[k] = 0;
      int xpm[4], xpn[4], xmm[4], xmn[4], xpn_mm[4], xpm_mn[4], xmm_mn[4];
#pragma unroll
      for (int d = 0; d < 4; d++) xpm[d] = xpn[d] = xmm[d] = xmn[d] = xpn_mm[d] = xpm_mn[d] = xmm_mn[d] = x[d];
      xpm[mu]++; xpn[nu]++; xmm[mu]--; xmn[nu]--; xpn_mm[nu]++; xpn_mm[mu]--; xpm_mn[mu]++; xpm_mn[nu]--; xmm_mn[mu]--; xmm_mn[nu]--;
      add_leaf<T, R>(Q, g, mu, x, false, nu, xpm, false, mu, xpn, true, nu, x, true);            // U(x,mu) U(x+mu,nu) U^(x+nu,mu) U^(x,nu)
      add_leaf<T, R>(Q, g, nu, x, false, mu, xpn_mm, true, nu, xmm, true, mu, xmm, false);       // U(x,nu) U^(x+nu-mu,mu) U^(x-mu,nu) U(x-mu,mu)
      add_leaf<T, R>(Q, g, nu, xmn, true, mu, xmn, false, nu, xpm_mn, false, mu, x, true);       // U^(x-nu,nu) U(x-nu,mu) U(x+mu-nu,nu) U^(x,mu)
      add_leaf<T, R>(Q, g, mu, xmm, true, nu, xmm_mn, true, mu, xmm_mn, false, nu, xmn, false);  // U^(x-mu,mu) U^(x-mu-nu,nu) U(x-mu-nu,mu) U(x-nu,nu)
      // F = (Q - Q^dag) / 8, scattered into the blocks (F index = mu(mu-1)/2 + nu)
      M3 F;
      m3_fmunu(F, Q);
      clover_add_fmunu(b1, b2, mu * (mu - 1) / 2 + nu, coeff, F);
    }
  for (int ch = 0; ch < 2; ch++) clover_pack_block(packed + (((size_t)parity * Vh + idx) * 2 + ch) * 36, b1[ch], b2[ch]);
}

// ---- the same construction on a grid-decomposed lattice: the four leaves of a plane by transport (gauge_obs.hip cloverLeaves), no
// links from neighbouring ranks but the nearest ----
// F = (Q - Q^dag)/8 with Q = P + A + B + C, scattered into the four colour blocks (same table as clover_from_gauge_kernel)
__global__ void cl_accum_kernel(MatField b1_0, MatField b1_1, MatField b2_0, MatField b2_1, MatField P, MatField A, MatField B, MatField C, int fi, double coeff,
                                int first, int Vh) {
  const int gid = blockIdx.x * blockDim.x + threadIdx.x;
  if (gid >= 2 * Vh) return;
  const int par = gid >= Vh, idx = gid - par * Vh;
  M3 F, b1[2], b2[2];
  leaf_sum_fmunu(F, P, A, B, C, par, idx);
  if (first) {
#pragma unroll
    for (int c = 0; c < 2; c++)
#pragma unroll
      for (int k = 0; k < 9; k++) { b1[c].re[k] = b1[c].im[k] = b2[c].re[k] = b2[c].im[k] = 0; }
  } else {
    mf_load(b1[0], b1_0, par, idx); mf_load(b1[1], b1_1, par, idx); mf_load(b2[0], b2_0, par, idx); mf_load(b2[1], b2_1, par, idx);
  }
  clover_add_fmunu(b1, b2, fi, coeff, F);
  mf_store(b1[0], b1_0, par, idx); mf_store(b1[1], b1_1, par, idx); mf_store(b2[0], b2_0, par, idx); mf_store(b2[1], b2_1, par, idx);
}
__global__ void cl_pack_kernel(double *packed, MatField b1_0, MatField b1_1, MatField b2_0, MatField b2_1, int Vh) {
  const int gid = blockIdx.x * blockDim.x + threadIdx.x;
  if (gid >= 2 * Vh) return;
  const int par = gid >= Vh, idx = gid - par * Vh;
  for (int ch = 0; ch < 2; ch++) {
    M3 b1, b2;
    mf_load(b1, ch ? b1_1 : b1_0, par, idx);
    mf_load(b2, ch ? b2_1 : b2_0, par, idx);
    clover_pack_block(packed + (((size_t)par * Vh + idx) * 2 + ch) * 36, b1, b2);
  }
}

static void cloverFromGaugeDecomposed(double *stage, const GaugeField &U, double coeff) {
  const int Vh = U.geom.Vh;
  MatPool pool(Vh, 9);   // the leaves W[0..4], then b1[0], b1[1], b2[0], b2[1]
  MatField W[5] = {pool[0], pool[1], pool[2], pool[3], pool[4]};
  bool first = true;
  for (int mu = 1; mu < 4; mu++)
    for (int nu = 0; nu < mu; nu++) {
      cloverLeaves(W, U, mu, nu);
      launchSites(cl_accum_kernel, Vh, 128, pool[5], pool[6], pool[7], pool[8], W[4], W[1], W[2], W[3], mu * (mu - 1) / 2 + nu, coeff, first ? 1 : 0, Vh);
      first = false;
    }
  launchSites(cl_pack_kernel, Vh, 128, stage, pool[5], pool[6], pool[7], pool[8], Vh);
  HIP_CHECK(hipStreamSynchronize(computeStream()));
}

void CloverField::computeFromGauge(const GaugeField &U, double coeff) {
  if (!(U.geom == geom)) errorQuda("gauge and clover geometry differ");
  if (U.anisotropy != 1.0) errorQuda("cannot compute anisotropic clover field");
  double *stage = (double *)stagingBuffer((size_t)geom.V * 72 * sizeof(double));
  if (usesTransport("QUDA_AMD_CLOVER_TRANSPORT")) cloverFromGaugeDecomposed(stage, U, coeff);   // the variable: for the tests
  else forLinkType(U, [&](auto t, auto r) { launchSites(clover_from_gauge_kernel<decltype(t), decltype(r)::value>, geom.Vh, 128, stage, viewOf(U), coeff, geom.Vh); });
  forPrecision(precision, [&](auto t) { launchSites(clover_load_kernel<decltype(t), double>, geom.Vh, 256, (char *)clover, norm, parity_bytes, stride, stage, geom.Vh); });
  HIP_CHECK(hipStreamSynchronize(computeStream()));
  this->coeff = coeff;
}

template <typename TDev, typename THost> static void cloverLoad(CloverField &c, void *dev, float *nrm, const void *host) {
  const size_t n = (size_t)c.geom.V * 72 * sizeof(THost);
  void *stage = stagingBuffer(n);
  HIP_CHECK(hipMemcpyAsync(stage, host, n, hipMemcpyHostToDevice, computeStream()));
  launchSites(clover_load_kernel<TDev, THost>, c.geom.Vh, 256, (char *)dev, nrm, c.parity_bytes, c.stride, (const THost *)stage, c.geom.Vh);
  HIP_CHECK(hipStreamSynchronize(computeStream()));
}

void CloverField::loadPacked(const void *h_clover, const void *h_inv, QudaPrecision cpu_prec) {
  const auto load = [&](void *dev, float *nrm, const void *host) {
    forPrecision(precision, [&](auto t) {
      if (cpu_prec == QUDA_DOUBLE_PRECISION) cloverLoad<decltype(t), double>(*this, dev, nrm, host);
      else cloverLoad<decltype(t), float>(*this, dev, nrm, host);
    });
  };
  if (h_clover) { load(clover, norm, h_clover); coeff = NAN; }
  if (h_inv) load(cloverInv, invNorm, h_inv);
}

void CloverField::computeInverse(double mu2_, bool twisted_) {
  mu2 = mu2_;
  twisted = twisted_ || mu2_ != 0.0;
  double *d_trlog = nullptr;
  HIP_CHECK(qaMalloc((void **)&d_trlog, 2 * sizeof(double)));
  HIP_CHECK(hipMemsetAsync(d_trlog, 0, 2 * sizeof(double), computeStream()));
  forPrecision(precision, [&](auto t) {
    launchSites(clover_invert_kernel<decltype(t)>, geom.Vh, 128, (char *)cloverInv, invNorm, (const char *)clover, norm, parity_bytes, stride, geom.Vh, mu2_, twisted ? 1 : 0, d_trlog);
  });
  HIP_CHECK(hipMemcpyAsync(trlog, d_trlog, 2 * sizeof(double), hipMemcpyDeviceToHost, computeStream()));
  HIP_CHECK(hipStreamSynchronize(computeStream()));
  HIP_CHECK(hipFree(d_trlog));
}

// the term or its inverse (dev, with its norms nrm) to the host in packed order
static void cloverSave(const CloverField &c, void *h_out, QudaPrecision cpu_prec, const void *dev, const float *nrm) {
  const size_t n = (size_t)c.geom.V * 72 * (int)cpu_prec;
  void *stage = stagingBuffer(n);
  forPrecision(c.precision, [&](auto t) {
    using TD = decltype(t);
    if (cpu_prec == QUDA_DOUBLE_PRECISION) launchSites(clover_save_kernel<TD, double>, c.geom.Vh, 256, (double *)stage, (const char *)dev, nrm, c.parity_bytes, c.stride, c.geom.Vh);
    else launchSites(clover_save_kernel<TD, float>, c.geom.Vh, 256, (float *)stage, (const char *)dev, nrm, c.parity_bytes, c.stride, c.geom.Vh);
  });
  HIP_CHECK(hipMemcpyAsync(h_out, stage, n, hipMemcpyDeviceToHost, computeStream()));
  HIP_CHECK(hipStreamSynchronize(computeStream()));
}
void CloverField::savePackedInverse(void *h_inv, QudaPrecision cpu_prec) const { cloverSave(*this, h_inv, cpu_prec, cloverInv, invNorm); }
void CloverField::savePacked(void *h_clover, QudaPrecision cpu_prec) const { cloverSave(*this, h_clover, cpu_prec, clover, norm); }

}  // namespace quda
