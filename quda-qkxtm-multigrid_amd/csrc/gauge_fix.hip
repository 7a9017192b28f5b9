// gauge_fix.hip — Landau and Coulomb gauge fixing by overrelaxation (reference lib/gauge_fix_ovr.cu, lib/gauge_fix_ovr_hit_devf.cuh,
// lib/interface_quda.cpp:5716-5826).  DESIGN section 3 "Gauge fixing".
//
// D = 3 (Coulomb, gauge_dir == 3) or 4 (Landau) directions enter F = sum_x sum_{mu<D} Re tr U_mu(x) / (3 D V), which the sweeps
// maximise, and theta = sum_x tr(Delta Delta^dag) / (3 V), Delta = B - B^dag - tr(B - B^dag)/3, B = sum_{mu<D} [U_mu(x - mu) - U_mu(x)].
// One iteration sweeps the even sites, then the odd ones.  At a site the SU(2) subgroups (0,1), (1,2), (0,2) are hit in turn: the
// four reals a of the subgroup's part of sum_mu [U_mu(x - mu) + U_mu(x)^dag] are overrelaxed to g, and g goes onto all eight links of
// the site, U_mu(x) <- g U_mu(x), U_mu(x - mu) <- U_mu(x - mu) g^dag, before the next subgroup is looked at.
//
// The sweep gives one link to one lane: eight lanes own a site, and a wave holds eight sites link-major, lane = 8 link + site (links
// 0..3 forward, 4..7 backward), so the eight lanes of one link read eight consecutive sites: one 128-byte line per 16-byte vector of
// the planar layout.  A lane keeps its link as M = U (forward) or M = U^T (backward), so that both kinds of update are the same row
// operation M <- g' M with g' = g (forward) or conj g (backward), and the code has no branch on the kind of link.  The four sums go
// across the eight lanes of a site by an xor butterfly of wave shuffles (xor 8, 16, 32; no LDS, no barrier); every lane ends up with
// the same bits and computes g itself.  (The site-major map, lane = 8 site + link with xor 1, 2, 4, measured 2.4 % slower per
// iteration at 32^4: DESIGN section 3.)
//
// Two formulations, as for the gauge force:
//   direct     the backward lanes read and write the forward link stored at x - mu in the other parity; unpartitioned lattices only;
//   transport  the backward links come to the site by the ghost-aware shift, the sweep writes the forward links of the active parity
//              and the field g(x) (the product of the three hits there, 1 on the other parity), and the backward links are updated
//              as U_mu <- U_mu shift(g, mu)^dag on the whole lattice; any partition mask or rank grid.
#include "dispatch.h"
#include "gauge_device.h"

#include <chrono>
#include <cmath>

namespace quda {

void comm_allreduce(double *data, int n);   // comm.cpp

struct FixGeom { int X[4]; int Vh; };

// rows P and Q of m <- the SU(2) matrix [[alpha, beta], [-conj beta, conj alpha]] times them
template <int P, int Q> __device__ __forceinline__ void su2_rows(M3 &m, double ar, double ai, double br, double bi) {
#pragma unroll
  for (int j = 0; j < 3; j++) {
    const double pr = m.re[3 * P + j], pi = m.im[3 * P + j], qr = m.re[3 * Q + j], qi = m.im[3 * Q + j];
    m.re[3 * P + j] = (ar * pr - ai * pi) + (br * qr - bi * qi);
    m.im[3 * P + j] = (ar * pi + ai * pr) + (br * qi + bi * qr);
    m.re[3 * Q + j] = (ar * qr + ai * qi) - (br * pr + bi * pi);
    m.im[3 * Q + j] = (ar * qi - ai * qr) - (br * pi - bi * pr);
  }
}

// one overrelaxation hit of subgroup (P, Q) on the lane's link m (and, WITH_G, on the site's matrix gm, which only the lane of link 0
// keeps).  sgn = +1: m is a forward link; -1: the transpose of a backward link.  counts: the link's direction is one of the D fixed
// ones.  Every lane of the wave runs through the shuffles, whether its site exists or not.
template <int P, int Q, bool WITH_G> __device__ __forceinline__ void su2_hit(M3 &m, M3 &gm, double sgn, bool counts, double omega) {
  double a0 = 0, a1 = 0, a2 = 0, a3 = 0;
  if (counts) {
    a0 = m.re[3 * P + P] + m.re[3 * Q + Q];
    a1 = -sgn * (m.im[3 * P + Q] + m.im[3 * Q + P]);
    a2 = m.re[3 * Q + P] - m.re[3 * P + Q];
    a3 = -sgn * (m.im[3 * P + P] - m.im[3 * Q + Q]);
  }
#pragma unroll
  for (int off = 8; off < 64; off <<= 1) {   // the lanes of a site are 8 apart
    a0 += __shfl_xor(a0, off, 64); a1 += __shfl_xor(a1, off, 64);
    a2 += __shfl_xor(a2, off, 64); a3 += __shfl_xor(a3, off, 64);
  }
  const double a0s = a0 * a0, as = a1 * a1 + a2 * a2 + a3 * a3;
  const double xh = (omega * a0s + as) / (a0s + as);
  const double r = 1.0 / sqrt(a0s + xh * xh * as), s = xh * r;
  a0 *= r; a1 *= s; a2 *= s; a3 *= s;
  // g_pp = a0 + i a3, g_pq = a2 + i a1; conj g for the transposed backward link
  su2_rows<P, Q>(m, a0, sgn * a3, a2, sgn * a1);
  if (WITH_G) su2_rows<P, Q>(gm, a0, a3, a2, a1);
}

// the 18 reals of site idx of one parity block (24 Vh doubles, planar 16-byte vectors), transposed on the way if tr
__device__ __forceinline__ void lane_load(M3 &m, const double *block, int Vh, int idx, bool tr) {
  double v[18];
#pragma unroll
  for (int k = 0; k < 9; k++) {
    const double2 t = *reinterpret_cast<const double2 *>(block + ((size_t)k * Vh + idx) * 2);
    v[2 * k] = t.x; v[2 * k + 1] = t.y;
  }
#pragma unroll
  for (int i = 0; i < 3; i++)
#pragma unroll
    for (int j = 0; j < 3; j++) {
      m.re[3 * i + j] = tr ? v[2 * (3 * j + i)] : v[2 * (3 * i + j)];
      m.im[3 * i + j] = tr ? v[2 * (3 * j + i) + 1] : v[2 * (3 * i + j) + 1];
    }
}
__device__ __forceinline__ void lane_store(const M3 &m, double *block, int Vh, int idx, bool tr) {
#pragma unroll
  for (int i = 0; i < 3; i++)
#pragma unroll
    for (int j = 0; j < 3; j++) {
      const int k = 3 * i + j, kt = 3 * j + i;
      *reinterpret_cast<double2 *>(block + ((size_t)k * Vh + idx) * 2) = make_double2(tr ? m.re[kt] : m.re[k], tr ? m.im[kt] : m.im[k]);
    }
}
__device__ __forceinline__ void m3_unit(M3 &m) {
#pragma unroll
  for (int k = 0; k < 9; k++) { m.re[k] = (k % 4 == 0) ? 1.0 : 0.0; m.im[k] = 0; }
}
// coordinates of checkerboard site idx of the given parity
__device__ __forceinline__ void site_coords(int *x, const FixGeom &g, int parity, int idx) {
  const int Xh = g.X[0] >> 1;
  int l = idx;
  const int xh = l % Xh; l /= Xh;
  x[1] = l % g.X[1]; l /= g.X[1];
  x[2] = l % g.X[2]; x[3] = l / g.X[2];
  x[0] = 2 * xh + ((x[1] + x[2] + x[3] + parity) & 1);
}
// checkerboard index of x - mu (in the other parity)
__device__ __forceinline__ int backward_index(const int *x, const FixGeom &g, int mu) {
  int y[4] = {x[0], x[1], x[2], x[3]};
#pragma unroll
  for (int d = 0; d < 4; d++)
    if (d == mu) y[d] = y[d] == 0 ? g.X[d] - 1 : y[d] - 1;
  return (((y[3] * g.X[2] + y[2]) * g.X[1] + y[1]) * g.X[0] + y[0]) >> 1;
}

// MODE 0: direct sweep; 1: direct sweep that also updates the transformation G(x) <- g G(x); 2: the site kernel of the transport
// formulation (backward links from `bwd` at the site itself, not written back; gf <- the product of the hits, 1 on the other parity).
// links (and bwd): the four matrix fields of the directions, one behind the other.  256 threads = 32 sites of the active parity.
enum { FIX_DIRECT = 0, FIX_DIRECT_G = 1, FIX_TRANSPORT = 2 };
template <int MODE>
__global__ void __launch_bounds__(256) gauge_fix_sweep_kernel(double *links, const double *bwd, MatField gf, FixGeom g, int parity, int D, double omega) {
  const int Vh = g.Vh;
  const int tid = blockIdx.x * blockDim.x + threadIdx.x;
  const int site = (tid >> 6) * 8 + (threadIdx.x & 7), link = (threadIdx.x >> 3) & 7;   // wave tid >> 6 holds sites 8 wave .. 8 wave + 7
  const bool valid = site < Vh, back = link >= 4;
  const int mu = link & 3;
  const size_t fieldDoubles = (size_t)2 * 24 * Vh, parDoubles = (size_t)24 * Vh;
  // where this lane's link lives
  double *block = links + mu * fieldDoubles + parity * parDoubles;
  int idx = site;
  if (back) {
    if (MODE == FIX_TRANSPORT) {
      block = const_cast<double *>(bwd) + mu * fieldDoubles + parity * parDoubles;
    } else if (valid) {
      int x[4];
      site_coords(x, g, parity, site);
      idx = backward_index(x, g, mu);
      block = links + mu * fieldDoubles + (1 - parity) * parDoubles;
    }
  }
  M3 m, gm;
#pragma unroll
  for (int k = 0; k < 9; k++) { m.re[k] = m.im[k] = 0; }
  if (valid) lane_load(m, block, Vh, idx, back);
  constexpr bool WITH_G = MODE != FIX_DIRECT;
  if (WITH_G) {
    m3_unit(gm);
    if (MODE == FIX_DIRECT_G && valid && link == 0) mf_load(gm, gf, parity, site);
  }
  const double sgn = back ? -1.0 : 1.0;
  const bool counts = mu < D;
  su2_hit<0, 1, WITH_G>(m, gm, sgn, counts, omega);
  su2_hit<1, 2, WITH_G>(m, gm, sgn, counts, omega);
  su2_hit<0, 2, WITH_G>(m, gm, sgn, counts, omega);
  if (!valid) return;
  if (!(MODE == FIX_TRANSPORT && back)) lane_store(m, block, Vh, idx, back);
  if (WITH_G && link == 0) mf_store(gm, gf, parity, site);
  if (MODE == FIX_TRANSPORT && link == 1) {
    m3_unit(gm);
    mf_store(gm, gf, 1 - parity, site);
  }
}

// per-block partial sums of sum_{mu<D} Re tr U_mu(x) -> partial[block] and tr(Delta Delta^dag) -> partial[nb + block]; one thread per
// site.  DIRECT: U_mu(x - mu) from the other parity by index; else from the shifted fields bwd at the site itself
template <bool DIRECT>
__global__ void __launch_bounds__(256) gauge_fix_quality_kernel(double *partial, const double *links, const double *bwd, FixGeom g, int D) {
  const int Vh = g.Vh;
  const int gid = blockIdx.x * blockDim.x + threadIdx.x;
  double tr = 0, th = 0;
  if (gid < 2 * Vh) {
    const int par = gid >= Vh, idx = gid - par * Vh;
    const size_t fieldDoubles = (size_t)2 * 24 * Vh, parDoubles = (size_t)24 * Vh;
    int x[4];
    if (DIRECT) site_coords(x, g, par, idx);
    M3 B, u;
#pragma unroll
    for (int k = 0; k < 9; k++) B.re[k] = B.im[k] = 0;
    for (int mu = 0; mu < D; mu++) {
      lane_load(u, links + mu * fieldDoubles + par * parDoubles, Vh, idx, false);
      tr += (u.re[0] + u.re[4]) + u.re[8];
#pragma unroll
      for (int k = 0; k < 9; k++) { B.re[k] -= u.re[k]; B.im[k] -= u.im[k]; }
      if (DIRECT) lane_load(u, links + mu * fieldDoubles + (1 - par) * parDoubles, Vh, backward_index(x, g, mu), false);
      else lane_load(u, bwd + mu * fieldDoubles + par * parDoubles, Vh, idx, false);
#pragma unroll
      for (int k = 0; k < 9; k++) { B.re[k] += u.re[k]; B.im[k] += u.im[k]; }
    }
    // Delta = B - B^dag - tr(B - B^dag)/3: anti-Hermitian, the trace of B - B^dag is 2 i Im tr B
    const double t3 = 2.0 * ((B.im[0] + B.im[4]) + B.im[8]) * (1.0 / 3.0);
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
      for (int j = 0; j < 3; j++) {
        const double dr = B.re[3 * i + j] - B.re[3 * j + i];
        const double di = B.im[3 * i + j] + B.im[3 * j + i] - (i == j ? t3 : 0.0);
        th += dr * dr + di * di;
      }
  }
  tr = block_sum_256(tr);
  __syncthreads();   // block_sum_256 reuses its four LDS slots
  th = block_sum_256(th);
  if (threadIdx.x == 0) { partial[blockIdx.x] = tr; partial[gridDim.x + blockIdx.x] = th; }
}

// every link of F onto SU(3) in place (polar_su3, as project_su3_kernel); a link off by more than tol afterwards counts as a failure
__global__ void __launch_bounds__(128) gauge_fix_reunit_kernel(MatField F, int *failures, double tol, int Vh) {
  const int gid = blockIdx.x * blockDim.x + threadIdx.x;
  if (gid >= 2 * Vh) return;
  const int par = gid >= Vh, idx = gid - par * Vh;
  M3 u;
  mf_load(u, F, par, idx);
  polar_su3(u, 1e-15);
  // a singular link comes out of the projection as NaN, which fmax in unitarity_deviation drops: 0 x entry is NaN for NaN and infinity
  double nan = 0;
#pragma unroll
  for (int k = 0; k < 9; k++) nan += 0.0 * u.re[k] + 0.0 * u.im[k];
  if (!(unitarity_deviation(u) <= tol) || nan != 0.0) atomicAdd(failures, 1);
  mf_store(u, F, par, idx);
}

// the time links from checkerboard index first on (the last time slice) change sign, both parities
__global__ void gauge_fix_flip_kernel(MatField F, int first, int Vh) {
  const int gid = blockIdx.x * blockDim.x + threadIdx.x;
  if (gid >= 2 * Vh) return;
  const int par = gid >= Vh, idx = gid - par * Vh;
  if (idx < first) return;
  M3 u;
  mf_load(u, F, par, idx);
#pragma unroll
  for (int k = 0; k < 9; k++) { u.re[k] = -u.re[k]; u.im[k] = -u.im[k]; }
  mf_store(u, F, par, idx);
}

__global__ void gauge_fix_unit_kernel(MatField out, int Vh) {
  const int gid = blockIdx.x * blockDim.x + threadIdx.x;
  if (gid >= 2 * Vh) return;
  const int par = gid >= Vh, idx = gid - par * Vh;
  M3 m;
  m3_unit(m);
  mf_store(m, out, par, idx);
}

namespace {

// the fields of one gauge-fixing run and the steps on them
struct GaugeFixer {
  const LatticeGeom &geom;
  const int Vh, D, nb;
  const bool transport;
  FixGeom fg;
  MatPool pool;
  MatField F[4], Bk[4], gf, T, G;   // forward links; [transport] backward links, hit product, scratch; [transform] G
  double *d_partial;
  int *d_fail;
  bool withG;

  GaugeFixer(const LatticeGeom &geom, int D, bool transport, bool withG)
      : geom(geom), Vh(geom.Vh), D(D), nb((2 * geom.Vh + 255) / 256), transport(transport),
        pool(geom.Vh, 4 + (transport ? 6 : 0) + (withG ? 1 : 0), (size_t)2 * ((2 * geom.Vh + 255) / 256) + 1), withG(withG) {
    for (int d = 0; d < 4; d++) fg.X[d] = geom.X[d];
    fg.Vh = Vh;
    int n = 0;
    for (int mu = 0; mu < 4; mu++) F[mu] = pool[n++];
    if (transport) {
      for (int mu = 0; mu < 4; mu++) Bk[mu] = pool[n++];
      gf = pool[n++]; T = pool[n++];
    } else {
      for (int mu = 0; mu < 4; mu++) Bk[mu] = F[mu];
      gf = T = F[0];
    }
    G = withG ? pool[n++] : F[0];
    d_partial = pool[n].p;
    d_fail = (int *)(d_partial + 2 * nb);
  }

  template <int MODE> void launchSweep(MatField g, int parity, double omega) {
    hipLaunchKernelGGL(gauge_fix_sweep_kernel<MODE>, dim3((Vh + 31) / 32), dim3(256), 0, computeStream(), F[0].p, (const double *)Bk[0].p, g, fg, parity, D, omega);
    HIP_CHECK(hipGetLastError());
  }
  void sweep(int parity, double omega) {
    if (!transport) {
      if (withG) launchSweep<FIX_DIRECT_G>(G, parity, omega); else launchSweep<FIX_DIRECT>(G, parity, omega);
      return;
    }
    for (int mu = 0; mu < 4; mu++) shiftField(Bk[mu], F[mu], geom, 2 * mu + 1);   // U_mu(x - mu)
    launchSweep<FIX_TRANSPORT>(gf, parity, omega);
    if (withG) mfMul(G, gf, G, 0, 0, 0);
    for (int mu = 0; mu < 4; mu++) {
      shiftField(T, gf, geom, 2 * mu);     // g(x + mu): the unit matrix where x is active
      mfMul(F[mu], F[mu], T, 0, 1, 0);
    }
  }
  void quality(double out[2]) {
    hipStream_t s = computeStream();
    if (transport) {
      for (int mu = 0; mu < D; mu++) shiftField(Bk[mu], F[mu], geom, 2 * mu + 1);
      hipLaunchKernelGGL(gauge_fix_quality_kernel<false>, dim3(nb), dim3(256), 0, s, d_partial, (const double *)F[0].p, (const double *)Bk[0].p, fg, D);
    } else {
      hipLaunchKernelGGL(gauge_fix_quality_kernel<true>, dim3(nb), dim3(256), 0, s, d_partial, (const double *)F[0].p, (const double *)F[0].p, fg, D);
    }
    HIP_CHECK(hipGetLastError());
    double v[2] = {sumPartials(d_partial, nb), sumPartials(d_partial + nb, nb)};
    comm_allreduce(v, 2);
    double Vglobal = (double)geom.V;
    for (int d = 0; d < 4; d++) Vglobal *= commGrid().dims[d];
    out[0] = v[0] / (3.0 * D * Vglobal);
    out[1] = v[1] / (3.0 * Vglobal);
  }
  void reunitarize() {
    hipStream_t s = computeStream();
    HIP_CHECK(hipMemsetAsync(d_fail, 0, sizeof(int), s));
    for (int mu = 0; mu < 4; mu++) launchSites(gauge_fix_reunit_kernel, Vh, 128, F[mu], d_fail, 1e-12, Vh);
    int fail = 0;
    HIP_CHECK(hipMemcpyAsync(&fail, d_fail, sizeof(int), hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));
    double f = fail;
    comm_allreduce(&f, 1);
    if (f > 0) errorQuda("Error in the unitarization: %ld links are not unitary to 1e-12 after the projection", (long)f);
  }
  // the anti-periodic sign of the time links on the last time slice of the last rank in t: taken off or put back
  void flipBoundary(const GaugeField &U) {
    if (U.t_boundary != QUDA_ANTI_PERIODIC_T || commGrid().coords[3] != commGrid().dims[3] - 1) return;
    launchSites(gauge_fix_flip_kernel, Vh, 128, F[3], (Vh / geom.X[3]) * (geom.X[3] - 1), Vh);
  }
};

double secondsSince(std::chrono::steady_clock::time_point t0) { return std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count(); }

}  // namespace

bool gaugeFixUsesTransport() { return usesTransport("QUDA_AMD_GAUGE_FIX_TRANSPORT"); }   // the variable: for tests and timing

void gaugeFixQuality(const GaugeField &U, int gauge_dir, double out[2]) {
  GaugeFixer fix(U.geom, gauge_dir == 3 ? 3 : 4, gaugeFixUsesTransport(), false);
  for (int mu = 0; mu < 4; mu++) extractForwardLinks(fix.F[mu], U, mu);
  fix.flipBoundary(U);
  fix.quality(out);
}

GaugeFixResult gaugeFixOVR(void *const h_out[4], double *h_transform, const GaugeField &U, int gauge_dir, int nsteps, int verbose_interval, double omega,
                           double tolerance, int reunit_interval, int stop_theta, double secs[3]) {
  if (reunit_interval <= 0) errorQuda("gauge fixing: reunit_interval = %d: the links are projected when iteration %% reunit_interval == reunit_interval - 1, so it has to be at least 1", reunit_interval);
  if (nsteps < 0) errorQuda("gauge fixing: Nsteps = %d", nsteps);
  auto t0 = std::chrono::steady_clock::now();
  const LatticeGeom &geom = U.geom;
  const int Vh = geom.Vh;
  GaugeFixer fix(geom, gauge_dir == 3 ? 3 : 4, gaugeFixUsesTransport(), h_transform != nullptr);
  hipStream_t s = computeStream();
  for (int mu = 0; mu < 4; mu++) extractForwardLinks(fix.F[mu], U, mu);
  fix.flipBoundary(U);
  if (h_transform) launchSites(gauge_fix_unit_kernel, Vh, 128, fix.G, Vh);
  HIP_CHECK(hipStreamSynchronize(s));
  secs[0] = secondsSince(t0);
  t0 = std::chrono::steady_clock::now();

  GaugeFixResult res = {0, 0, 0, 0};
  double q[2];
  fix.quality(q);
  res.F = q[0]; res.theta = q[1];
  if (verbose_interval > 0) printfQuda("Step: %d\tAction: %.16e\ttheta: %.16e\n", 0, res.F, res.theta);
  int iter = 0;
  while (iter < nsteps) {
    fix.sweep(0, omega);
    fix.sweep(1, omega);
    if (iter % reunit_interval == reunit_interval - 1) fix.reunitarize();
    fix.quality(q);
    res.delta = fabs(q[0] - res.F);
    res.F = q[0]; res.theta = q[1];
    iter++;
    if (verbose_interval > 0 && iter % verbose_interval == 0)
      printfQuda("Step: %d\tAction: %.16e\ttheta: %.16e\tDelta: %.16e\n", iter, res.F, res.theta, res.delta);
    if (stop_theta ? (res.theta < tolerance) : (res.delta < tolerance)) break;
  }
  res.iterations = iter;
  if (iter % reunit_interval != 0) fix.reunitarize();   // unless the last iteration just did
  HIP_CHECK(hipStreamSynchronize(s));
  secs[1] = secondsSince(t0);
  t0 = std::chrono::steady_clock::now();

  fix.flipBoundary(U);
  matFieldsToHost(h_out, geom, [&](int mu) { return fix.F[mu]; }, matFieldToQdp);
  if (h_transform) {
    const size_t bytes = (size_t)geom.V * 18 * sizeof(double);
    double *stage = (double *)stagingBuffer(bytes);
    matFieldToQdp(stage, fix.G, 0);
    HIP_CHECK(hipMemcpyAsync(h_transform, stage, bytes, hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));
  }
  secs[2] = secondsSince(t0);
  return res;
}

}  // namespace quda
