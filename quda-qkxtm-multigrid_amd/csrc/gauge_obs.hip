// gauge_obs.hip — observables and smearing of the gauge field in the transport formulation: matrix fields of forward links and their
// ghost-aware shifts, the clover leaves, staples with APE and stout smearing, the plaquette, the links back in host order, field
// strength and topological charge; and the host helpers that gauge_device.h declares for clover.hip, gauge_md.hip and ferm_force.hip.
#include "dispatch.h"
#include "gauge_device.h"

#include <cmath>
#include <cstdlib>
#include <utility>
#include <vector>

#include "blas.h"
#include "dslash.h"

namespace quda {

// ================================================================================================================
// Matrix fields: the forward links of a resident field, shifts, products
GaugeView viewOf(const GaugeField &U) {
  GaugeView g;
  g.data = (const char *)U.data; g.link_bytes = U.link_bytes; g.stride = U.stride;
  for (int d = 0; d < 4; d++) g.X[d] = U.geom.X[d];
  // anti-periodic sign of the reconstructed third row (recon-12): on the last / first rank in t only
  const bool first_t = commGrid().coords[3] == 0, last_t = commGrid().coords[3] == commGrid().dims[3] - 1;
  g.tsign = (U.t_boundary == QUDA_ANTI_PERIODIC_T && last_t) ? -1 : 1;
  g.tsign_bwd = (U.t_boundary == QUDA_ANTI_PERIODIC_T && first_t) ? -1 : 1;
  return g;
}

bool usesTransport(const char *envName) {
  bool transport = false;
  for (int d = 0; d < 4; d++) transport = transport || commGrid().partitioned(d);
  const char *e = getenv(envName);
  return transport || (e && atoi(e));
}

double sumPartials(const double *d_partial, int nb) {
  std::vector<double> partial(nb);
  HIP_CHECK(hipMemcpyAsync(partial.data(), d_partial, (size_t)nb * sizeof(double), hipMemcpyDeviceToHost, computeStream()));
  HIP_CHECK(hipStreamSynchronize(computeStream()));
  double sum = 0;
  for (int b = 0; b < nb; b++) sum += partial[b];
  return sum;
}

template <typename T, int R> __global__ void cl_extract_kernel(MatField out, GaugeView g, int mu, int Vh) {
  const int gid = blockIdx.x * blockDim.x + threadIdx.x;
  if (gid >= 2 * Vh) return;
  const int par = gid >= Vh, idx = gid - par * Vh;
  M3 u;
  load_w<T, R>(u, g, par, idx, 2 * mu, time_coord(g, idx));
  mf_store(u, out, par, idx);
}
void extractForwardLinks(MatField F, const GaugeField &U, int mu) {
  forLinkType(U, [&](auto t, auto r) { launchSites(cl_extract_kernel<decltype(t), decltype(r)::value>, U.geom.Vh, 128, F, viewOf(U), mu, U.geom.Vh); });
}

// out(x) = in(x + dhat(dir)) of a matrix field, both parities (dir = 2 mu: forward, 2 mu + 1: backward)
void shiftField(MatField out, MatField in, const LatticeGeom &geom, int dir) {
  for (int par = 0; par < 2; par++) applyShift(out.par(par), in.par(1 - par), geom, geom.Vh, par, dir);
}

// out (+)= op(A) op(B), op = identity or Hermitian conjugate
__global__ void mf_mul_kernel(MatField out, MatField A, MatField B, int dagA, int dagB, int accumulate, int Vh) {
  const int gid = blockIdx.x * blockDim.x + threadIdx.x;
  if (gid >= 2 * Vh) return;
  const int par = gid >= Vh, idx = gid - par * Vh;
  M3 a, b, t, c;
  mf_load(a, A, par, idx); if (dagA) { m3_dag(t, a); a = t; }
  mf_load(b, B, par, idx); if (dagB) { m3_dag(t, b); b = t; }
  m3_mul(c, a, b);
  if (accumulate) {
    mf_load(t, out, par, idx);
#pragma unroll
    for (int k = 0; k < 9; k++) { c.re[k] += t.re[k]; c.im[k] += t.im[k]; }
  }
  mf_store(c, out, par, idx);
}
void mfMul(MatField out, MatField A, MatField B, int dagA, int dagB, int accumulate) {
  launchSites(mf_mul_kernel, out.Vh, 128, out, A, B, dagA, dagB, accumulate, out.Vh);
}
__global__ void mf_add_kernel(MatField out, MatField in, int Vh) {
  const int gid = blockIdx.x * blockDim.x + threadIdx.x;
  if (gid >= 2 * Vh) return;
  const int par = gid >= Vh, idx = gid - par * Vh;
  M3 a, b;
  mf_load(a, out, par, idx); mf_load(b, in, par, idx);
#pragma unroll
  for (int k = 0; k < 9; k++) { a.re[k] += b.re[k]; a.im[k] += b.im[k]; }
  mf_store(a, out, par, idx);
}

// ================================================================================================================
// The clover leaves by transport.  A leaf that starts at x - mu, x - nu or x - mu - nu is the plaquette P_mu_nu of that site carried
// to x along the links in between (U^dag P U), so instead of gathering links from up to three neighbouring ranks (corners included)
// the field P is built once from forward-shifted links and then transported with ghost-aware nearest-neighbour shifts (dslash.h
// applyShift): Q = P + T_mu P + T_nu P + T_nu T_mu P, (T_mu F)(x) = U_mu(x - mu)^dag F(x - mu) U_mu(x - mu) — and U_mu(x - mu)^dag
// is stored at x (bidirectional links).  Shared by the decomposed clover construction (clover.hip) and the field strength below.

// P = U_mu(x) Gnu(x) Gmu(x)^dag U_nu(x)^dag with Gnu = U_nu(x + mu), Gmu = U_mu(x + nu)
template <typename T, int R> __global__ void cl_plaq_kernel(MatField P, MatField Gnu, MatField Gmu, GaugeView g, int mu, int nu, int Vh) {
  const int gid = blockIdx.x * blockDim.x + threadIdx.x;
  if (gid >= 2 * Vh) return;
  const int par = gid >= Vh, idx = gid - par * Vh, t = time_coord(g, idx);
  M3 a, b, c, d;
  load_w<T, R>(a, g, par, idx, 2 * mu, t);
  mf_load(b, Gnu, par, idx);
  m3_mul(c, a, b);
  mf_load(b, Gmu, par, idx); m3_dag(a, b);
  m3_mul(d, c, a);
  load_w<T, R>(b, g, par, idx, 2 * nu, t); m3_dag(a, b);
  m3_mul(c, d, a);
  mf_store(c, P, par, idx);
}
// out = W S W^dag with W = U_mu(x - mu)^dag (slot 2 mu + 1) and S = F(x - mu) already shifted to x
template <typename T, int R> __global__ void cl_transport_kernel(MatField out, MatField S, GaugeView g, int mu, int Vh) {
  const int gid = blockIdx.x * blockDim.x + threadIdx.x;
  if (gid >= 2 * Vh) return;
  const int par = gid >= Vh, idx = gid - par * Vh;
  M3 w, s, a, b;
  load_w<T, R>(w, g, par, idx, 2 * mu + 1, time_coord(g, idx));
  mf_load(s, S, par, idx);
  m3_mul(a, w, s);
  m3_dag(b, w);
  m3_mul(s, a, b);
  mf_store(s, out, par, idx);
}

void cloverLeaves(MatField W[5], const GaugeField &U, int mu, int nu) {
  const LatticeGeom &geom = U.geom;
  const GaugeView g = viewOf(U);
  forLinkType(U, [&](auto t, auto r) {
    using T = decltype(t);
    constexpr int R = decltype(r)::value;
    const int Vh = geom.Vh;
    launchSites(cl_extract_kernel<T, R>, Vh, 128, W[0], g, nu, Vh);
    launchSites(cl_extract_kernel<T, R>, Vh, 128, W[1], g, mu, Vh);
    shiftField(W[2], W[0], geom, 2 * mu);   // U_nu(x + mu)
    shiftField(W[3], W[1], geom, 2 * nu);   // U_mu(x + nu)
    launchSites(cl_plaq_kernel<T, R>, Vh, 128, W[4], W[2], W[3], g, mu, nu, Vh);   // P
    shiftField(W[0], W[4], geom, 2 * mu + 1);
    launchSites(cl_transport_kernel<T, R>, Vh, 128, W[1], W[0], g, mu, Vh);        // A = T_mu P
    shiftField(W[0], W[4], geom, 2 * nu + 1);
    launchSites(cl_transport_kernel<T, R>, Vh, 128, W[2], W[0], g, nu, Vh);        // B = T_nu P
    shiftField(W[0], W[1], geom, 2 * nu + 1);
    launchSites(cl_transport_kernel<T, R>, Vh, 128, W[3], W[0], g, nu, Vh);        // C = T_nu T_mu P
  });
}

// ================================================================================================================
// APE smearing of the spatial links and the plaquette (reference lib/gauge_ape.cu:44-156,
// include/su3_project.cuh:23-124, lib/interface_quda.cpp:5565-5640, lib/gauge_plaq.cu:38-152).  Same transport formulation as
// the clover leaves above: forward links as 3x3 matrix fields, neighbours through the ghost-aware
// nearest-neighbour shift (applyShift), so a grid-decomposed lattice needs no extended gauge halo and no corner exchange
// (the reference: copyExtendedGauge + exchangeExtendedGhost every step).  fp64 throughout.
//   upper staple of (x, nu) in the mu-nu plane:  U_mu(x) U_nu(x+mu) U_mu(x+nu)^dag
//   lower staple:                                [U_mu^dag U_nu T_nu(U_mu)](x - mu)      (built at x - mu, then shifted to x)

// computeAPEStep: TestU = (1 - alpha) + alpha/4 S U^dag, projected; U' = TestU U
__global__ void ape_project_kernel(MatField Unew, MatField S, MatField U, double alpha, double tol, int Vh) {
  const int gid = blockIdx.x * blockDim.x + threadIdx.x;
  if (gid >= 2 * Vh) return;
  const int par = gid >= Vh, idx = gid - par * Vh;
  M3 s, u, ud, t;
  mf_load(s, S, par, idx); mf_load(u, U, par, idx);
  const double f = alpha / 4.0;
#pragma unroll
  for (int k = 0; k < 9; k++) { s.re[k] *= f; s.im[k] *= f; }
  m3_dag(ud, u);
  m3_mul(t, s, ud);
  t.re[0] += 1.0 - alpha; t.re[4] += 1.0 - alpha; t.re[8] += 1.0 - alpha;
  polar_su3(t, tol);
  m3_mul(s, t, u);
  mf_store(s, Unew, par, idx);
}
// sum over sites of Re tr [A B C^dag D^dag] into acc[slot] (block tree + one atomic per block)
__global__ void __launch_bounds__(256) plaq_trace_kernel(double *acc, int slot, MatField A, MatField B, MatField Cm, MatField D, int Vh) {
  const int gid = blockIdx.x * blockDim.x + threadIdx.x;
  double tr = 0;
  if (gid < 2 * Vh) {
    const int par = gid >= Vh, idx = gid - par * Vh;
    M3 a, b, t, t2, d;
    mf_load(a, A, par, idx); mf_load(b, B, par, idx);
    m3_mul(t, a, b);
    mf_load(a, Cm, par, idx); m3_dag(d, a); m3_mul(t2, t, d);
    mf_load(a, D, par, idx); m3_dag(d, a); m3_mul(t, t2, d);
    tr = t.re[0] + t.re[4] + t.re[8];
  }
  tr = block_sum_256(tr);
  if (threadIdx.x == 0) atomicAdd(acc + slot, tr);
}
// forward links of one direction -> host QDP order (even sites then odd, 18 reals per site)
__global__ void mf_to_qdp_kernel(double *qdp, MatField F, int Vh) {
  const int gid = blockIdx.x * blockDim.x + threadIdx.x;
  if (gid >= 2 * Vh) return;
  const int par = gid >= Vh, idx = gid - par * Vh;
  M3 u;
  mf_load(u, F, par, idx);
  double *o = qdp + (size_t)gid * 18;
#pragma unroll
  for (int k = 0; k < 9; k++) { o[2 * k] = u.re[k]; o[2 * k + 1] = u.im[k]; }
}
void matFieldToQdp(double *stage, MatField F, int) { launchSites(mf_to_qdp_kernel, F.Vh, 128, stage, F, F.Vh); }

// S = sum over the smeared directions mu != nu (mu < ndir) of the upper and the lower staple of (x, nu); F: the forward links of
// the previous step, W1, W2, T1, T2: scratch.  Shared by the APE and the stout step.
static void stapleSum(MatField S, const MatField *F, int nu, int ndir, MatField W1, MatField W2, MatField T1, MatField T2, const LatticeGeom &geom) {
  HIP_CHECK(hipMemsetAsync(S.p, 0, (size_t)2 * 24 * geom.Vh * sizeof(double), computeStream()));
  for (int mu = 0; mu < ndir; mu++) {
    if (mu == nu) continue;
    shiftField(W1, F[nu], geom, 2 * mu);   // U_nu(x + mu)
    shiftField(W2, F[mu], geom, 2 * nu);   // U_mu(x + nu)
    mfMul(T1, F[mu], W1, 0, 0, 0);         // U_mu(x) U_nu(x+mu)
    mfMul(S, T1, W2, 0, 1, 1);             // S += ... U_mu(x+nu)^dag
    mfMul(T1, F[mu], F[nu], 1, 0, 0);      // U_mu(x)^dag U_nu(x)
    mfMul(T2, T1, W2, 0, 0, 0);            // ... U_mu(x+nu)
    shiftField(T1, T2, geom, 2 * mu + 1);  // carried from x - mu to x
    launchSites(mf_add_kernel, geom.Vh, 128, S, T1, geom.Vh);
  }
}

// nSteps smearing steps of the directions 0 .. ndir-1 on a copy of U; update(Unew, S, Uold) launches the link update of one
// direction from its staple sum.  The result is a new fp64 field without reconstruction.
template <typename Update> static GaugeField *smearLinks(const GaugeField &U, unsigned nSteps, int ndir, Update update) {
  const LatticeGeom &geom = U.geom;
  HostLinks host(geom.V);
  {
    MatPool pool(geom.Vh, 13);
    MatField F[4] = {pool[0], pool[1], pool[2], pool[3]}, G[4] = {pool[4], pool[5], pool[6], pool[7]};
    const MatField S = pool[8], W1 = pool[9], W2 = pool[10], T1 = pool[11], T2 = pool[12];
    for (int mu = 0; mu < 4; mu++) extractForwardLinks(F[mu], U, mu);
    for (unsigned step = 0; step < nSteps; step++) {
      for (int nu = 0; nu < ndir; nu++) {
        stapleSum(S, F, nu, ndir, W1, W2, T1, T2, geom);
        update(G[nu], S, F[nu]);
      }
      // every direction of a step is smeared from the links of the previous step (the reference reads a copy, :5621-5627)
      for (int nu = 0; nu < ndir; nu++) std::swap(F[nu], G[nu]);
    }
    matFieldsToHost(host.ptr, geom, [&](int mu) { return F[mu]; }, matFieldToQdp);
  }
  // back through the loader: it builds the bidirectional layout and fetches the backward links that live on the neighbour ranks
  GaugeField *out = new GaugeField(geom, QUDA_DOUBLE_PRECISION, QUDA_RECONSTRUCT_NO, U.t_boundary, U.anisotropy);
  out->loadQDP(host.ptr, QUDA_DOUBLE_PRECISION);
  return out;
}

GaugeField *apeSmear(const GaugeField &U, unsigned nSteps, double alpha) {
  const double tol = 1e-15;   // DOUBLE_TOL, lib/gauge_ape.cu:9
  return smearLinks(U, nSteps, 3, [&](MatField Unew, MatField S, MatField Uold) { launchSites(ape_project_kernel, U.geom.Vh, 128, Unew, S, Uold, alpha, tol, U.geom.Vh); });
}

// ================================================================================================================
// Stout smearing (Morningstar and Peardon, hep-lat/0311018; reference lib/gauge_stout.cu, include/quda_matrix.h exponentiate_iQ,
// lib/interface_quda.cpp:5640-5713).  Staples as for APE; per link
//   Omega = rho S U^dag,   Q = (i/2) [(Omega^dag - Omega) - tr(Omega^dag - Omega)/3],   U' = exp(iQ) U.
// U^dag stands where the reference inverts U: the same matrix for unitary links, without the division.
// exp(iQ): su3_exp_iq, gauge_device.h.

// one thread per site and parity: Unew = exp(iQ) U with Q from the staple sum S
__global__ void __launch_bounds__(128) stout_update_kernel(MatField Unew, MatField S, MatField U, double rho, int Vh) {
  const int gid = blockIdx.x * blockDim.x + threadIdx.x;
  if (gid >= 2 * Vh) return;
  const int par = gid >= Vh, idx = gid - par * Vh;
  M3 s, u, t, om, q;
  mf_load(s, S, par, idx); mf_load(u, U, par, idx);
  m3_dag(t, u);
  m3_mul(om, s, t);   // Omega / rho
  // Q_ij = (i/2) (conj(Om_ji) - Om_ij) - delta_ij (i/6) tr(Om^dag - Om);  tr(Om^dag - Om) = -2i sum_k Im Om_kk.  rho multiplies the
  // differences, not Omega: rho a - rho b contracts to fma(rho, a, -(rho b)), which is not 0 for a = b and would leave Q
  // Hermitian only to rounding (and the unit gauge not a fixed point)
  const double h = 0.5 * rho, tr3 = rho * ((om.im[0] + om.im[4] + om.im[8]) * (1.0 / 3.0));
#pragma unroll
  for (int i = 0; i < 3; i++)
#pragma unroll
    for (int j = 0; j < 3; j++) {
      q.re[3 * i + j] = h * (om.im[3 * j + i] + om.im[3 * i + j]);
      q.im[3 * i + j] = h * (om.re[3 * j + i] - om.re[3 * i + j]);
    }
  q.re[0] -= tr3; q.re[4] -= tr3; q.re[8] -= tr3;
  su3_exp_iq(t, q);
  m3_mul(s, t, u);
  mf_store(s, Unew, par, idx);
}

// test hook (qudaAmdSu3ExpIQ): out[n] = exp(i q[n]) through the function the stout kernel calls; 18 reals per matrix, row-major re/im
__global__ void __launch_bounds__(128) su3_exp_iq_kernel(double *out, const double *in, int n) {
  const int gid = blockIdx.x * blockDim.x + threadIdx.x;
  if (gid >= n) return;
  M3 q, e;
#pragma unroll
  for (int k = 0; k < 9; k++) { q.re[k] = in[(size_t)gid * 18 + 2 * k]; q.im[k] = in[(size_t)gid * 18 + 2 * k + 1]; }
  su3_exp_iq(e, q);
#pragma unroll
  for (int k = 0; k < 9; k++) { out[(size_t)gid * 18 + 2 * k] = e.re[k]; out[(size_t)gid * 18 + 2 * k + 1] = e.im[k]; }
}

void su3ExpIQ(int n, const double *h_q, double *h_out) {
  if (n <= 0) return;
  const size_t bytes = (size_t)n * 18 * sizeof(double);
  double *d = nullptr;
  HIP_CHECK(qaMalloc((void **)&d, 2 * bytes));
  hipStream_t s = computeStream();
  HIP_CHECK(hipMemcpyAsync(d, h_q, bytes, hipMemcpyHostToDevice, s));
  hipLaunchKernelGGL(su3_exp_iq_kernel, dim3((n + 127) / 128), dim3(128), 0, s, d + (size_t)n * 18, d, n);
  HIP_CHECK(hipGetLastError());
  HIP_CHECK(hipMemcpyAsync(h_out, d + (size_t)n * 18, bytes, hipMemcpyDeviceToHost, s));
  HIP_CHECK(hipStreamSynchronize(s));
  HIP_CHECK(hipFree(d));
}

// ndir = 3: the spatial links from spatial staples (performSTOUTnStep); ndir = 4: all links from the staples of all six planes
GaugeField *stoutSmear(const GaugeField &U, unsigned nSteps, double rho, int ndir) {
  if (ndir != 3 && ndir != 4) errorQuda("stoutSmear: %d smeared directions (3 or 4)", ndir);
  return smearLinks(U, nSteps, ndir, [&](MatField Unew, MatField S, MatField Uold) { launchSites(stout_update_kernel, U.geom.Vh, 128, Unew, S, Uold, rho, U.geom.Vh); });
}
void saveGaugeQDP(const GaugeField &U, void *const h_gauge[4], QudaPrecision cpu_prec) {
  if (cpu_prec != QUDA_DOUBLE_PRECISION) errorQuda("saving links: fp64 host fields only");
  linksToHost(h_gauge, U, matFieldToQdp);
}

// plq[0] = mean of the spatial and temporal averages, plq[1] = spatial, plq[2] = temporal (lib/gauge_plaq.cu:129-153)
void plaquette(const GaugeField &U, double plq[3]) {
  const LatticeGeom &geom = U.geom;
  MatPool pool(geom.Vh, 6, 2);   // the forward links, two shifted fields, the two sums
  const MatField F[4] = {pool[0], pool[1], pool[2], pool[3]}, W1 = pool[4], W2 = pool[5];
  double *d_acc = pool[6].p;
  HIP_CHECK(hipMemsetAsync(d_acc, 0, 2 * sizeof(double), computeStream()));
  for (int mu = 0; mu < 4; mu++) extractForwardLinks(F[mu], U, mu);
  for (int mu = 0; mu < 3; mu++)
    for (int nu = mu + 1; nu < 4; nu++) {
      shiftField(W1, F[nu], geom, 2 * mu);
      shiftField(W2, F[mu], geom, 2 * nu);
      launchSites(plaq_trace_kernel, geom.Vh, 256, d_acc, nu < 3 ? 0 : 1, F[mu], W1, W2, F[nu], geom.Vh);
    }
  double h[2];
  HIP_CHECK(hipMemcpyAsync(h, d_acc, 2 * sizeof(double), hipMemcpyDeviceToHost, computeStream()));
  HIP_CHECK(hipStreamSynchronize(computeStream()));
  comm_allreduce(h, 2);
  const double norm = 9.0 * (double)geom.V * commGrid().size;
  plq[1] = h[0] / norm; plq[2] = h[1] / norm; plq[0] = 0.5 * (plq[1] + plq[2]);
}

// ================================================================================================================
// Topological charge from the clover-leaf field strength (reference lib/field_strength_tensor.cu, lib/qcharge_quda.cu,
// lib/interface_quda.cpp:5940-5991): F_mu_nu = (Q_mu_nu - Q_mu_nu^dag)/8, no trace removed, the leaves by the transport above;
//   q(x) = [Re tr(F10 F32) + Re tr(F30 F21) - Re tr(F20 F31)] / (4 pi^2),   Q = sum_x q(x).
__global__ void fmunu_kernel(MatField F, MatField P, MatField A, MatField B, MatField C, int Vh) {
  const int gid = blockIdx.x * blockDim.x + threadIdx.x;
  if (gid >= 2 * Vh) return;
  const int par = gid >= Vh, idx = gid - par * Vh;
  M3 m;
  leaf_sum_fmunu(m, P, A, B, C, par, idx);
  mf_store(m, F, par, idx);
}
__device__ __forceinline__ double re_tr_mul(const M3 &a, const M3 &b) {
  double r = 0;
#pragma unroll
  for (int i = 0; i < 3; i++)
#pragma unroll
    for (int j = 0; j < 3; j++) r += a.re[3 * i + j] * b.re[3 * j + i] - a.im[3 * i + j] * b.im[3 * j + i];
  return r;
}
struct FmunuFields { MatField f[6]; };
// q(x) for every site (even sites then odd) and one partial sum per block, in a fixed order (block_sum_256).  No atomics: the
// partials are added in block order by the host, so the same field gives the same bits.
__global__ void __launch_bounds__(256) qcharge_density_kernel(double *q, double *partial, FmunuFields F, int Vh) {
  const int gid = blockIdx.x * blockDim.x + threadIdx.x;
  double v = 0;
  if (gid < 2 * Vh) {
    const int par = gid >= Vh, idx = gid - par * Vh;
    M3 a, b;
    mf_load(a, F.f[0], par, idx); mf_load(b, F.f[5], par, idx);
    v = re_tr_mul(a, b);
    mf_load(a, F.f[3], par, idx); mf_load(b, F.f[2], par, idx);
    v += re_tr_mul(a, b);
    mf_load(a, F.f[1], par, idx); mf_load(b, F.f[4], par, idx);
    v -= re_tr_mul(a, b);
    v *= 1.0 / (4.0 * M_PI * M_PI);
    q[gid] = v;
  }
  v = block_sum_256(v);
  if (threadIdx.x == 0) partial[blockIdx.x] = v;
}

// the global charge; h_density (may be NULL) receives this rank's q(x), even sites then odd
double topologicalCharge(const GaugeField &U, double *h_density) {
  const int Vh = U.geom.Vh, nb = (2 * Vh + 255) / 256;   // the grid depends on the volume only
  MatPool pool(Vh, 11, (size_t)2 * Vh + nb);             // five leaves, six field strengths; q(x), the partial sums
  MatField W[5] = {pool[0], pool[1], pool[2], pool[3], pool[4]};
  FmunuFields F;
  for (int i = 0; i < 6; i++) F.f[i] = pool[5 + i];
  double *d_q = pool[11].p, *d_partial = d_q + (size_t)2 * Vh;
  for (int mu = 1; mu < 4; mu++)
    for (int nu = 0; nu < mu; nu++) {
      cloverLeaves(W, U, mu, nu);
      launchSites(fmunu_kernel, Vh, 128, F.f[mu * (mu - 1) / 2 + nu], W[4], W[1], W[2], W[3], Vh);
    }
  launchSites(qcharge_density_kernel, Vh, 256, d_q, d_partial, F, Vh);
  if (h_density) HIP_CHECK(hipMemcpyAsync(h_density, d_q, (size_t)2 * Vh * sizeof(double), hipMemcpyDeviceToHost, computeStream()));
  double Q = sumPartials(d_partial, nb);
  comm_allreduce(&Q, 1);
  return Q;
}

}  // namespace quda
