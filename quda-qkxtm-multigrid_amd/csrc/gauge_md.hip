// gauge_md.hip — the gauge sector of molecular dynamics: the path-product force, the link update, the momentum action and the
// SU(3) projection (reference lib/gauge_force.cu, lib/gauge_update_quda.cu, lib/momentum.cu, lib/interface_quda.cpp:5187-5247).
//
// Momentum: one traceless anti-Hermitian 3x3 matrix A per link, ten reals in host and device memory alike,
//   [site (even sites, then odd)][mu][Re A01, Im A01, Re A02, Im A02, Re A12, Im A12, Im A00, Im A11, Im A22, 0]
// (the reference's MILC order of a reconstruct-10 field, include/gauge_field_order.h:424-456); A10 = -conj A01 and so on, and the
// diagonal has no real part.  The device field keeps the host order, so upload and download are plain copies.
//
// Paths (lib/gauge_force.cu:51-52): directions 0..3 step forwards in x, y, z, t, 7 - d steps backwards in d.  For every site x and
// direction mu the walk starts at x + mu and multiplies the links it meets from left to right, a forward step d from y with U_d(y)
// and on to y + d, a backward step on to y - d with U_d(y - d)^dag (:86-129).  V_mu(x) = sum_i coeff_i product_i skips the paths of
// coefficient 0, and A_mu(x) <- TA(A_mu(x) - eb3 U_mu(x) V_mu(x)) with TA(M) = (M - M^dag)/2 - tr(M - M^dag)/6 (:131-140).
//
// Two formulations of V, as for the clover term (clover_from_gauge_kernel / cloverFromGaugeDecomposed):
//   direct     one thread per (site, parity, direction) gathers the links of every path itself; unpartitioned lattices only;
//   transport  the partial products R_k(y) = L_k(y) R_{k+1}(y') are matrix fields carried one hop at a time by the ghost-aware
//              shift, so no rank ever needs more than its nearest neighbours' links; any partition mask or rank grid.
// Both end in force_epilogue, which multiplies with U_mu(x), takes TA, accumulates into the momentum and packs it.
#include "dispatch.h"
#include "gauge_device.h"

#include <cstring>

namespace quda {

void comm_allreduce(double *data, int n);   // comm.cpp

// the path table of one force call.  Every index into it is the same in all lanes of a wave (direction from blockIdx.y, the loop
// counters), and it lives in constant memory, so the steps, lengths and coefficients arrive through scalar loads
struct ForceTable {
  int num_paths;
  int length[kGaugeForceMaxPaths];
  double coeff[kGaugeForceMaxPaths];
  signed char step[4][kGaugeForceMaxPaths][kGaugeForceMaxLength];
};
__constant__ ForceTable c_force;

MomField::MomField(const LatticeGeom &g) : geom(g), bytes((size_t)g.V * 40 * sizeof(double)), data(nullptr) {
  HIP_CHECK(qaMalloc((void **)&data, bytes));
  zero();
}
MomField::~MomField() { if (data) (void)hipFree(data); }
void MomField::zero() { HIP_CHECK(hipMemsetAsync(data, 0, bytes, computeStream())); }
void MomField::load(const void *h_mom) {
  HIP_CHECK(hipMemcpyAsync(data, h_mom, bytes, hipMemcpyHostToDevice, computeStream()));
  HIP_CHECK(hipStreamSynchronize(computeStream()));
}
void MomField::save(void *h_mom) const {
  HIP_CHECK(hipMemcpyAsync(h_mom, data, bytes, hipMemcpyDeviceToHost, computeStream()));
  HIP_CHECK(hipStreamSynchronize(computeStream()));
}

// y[dir] += s (s = +1 or -1), wrapped into the lattice after every single step: a path may cross the same boundary more than once
// (extent 2), which one wrap of the summed displacement would miss.  dir is wave-uniform; y stays in registers (static indices)
__device__ __forceinline__ void hop(int *y, int dir, int s, const GaugeView &g) {
#pragma unroll
  for (int k = 0; k < 4; k++)
    if (k == dir) {
      const int v = y[k] + s;
      y[k] = v < 0 ? v + g.X[k] : (v >= g.X[k] ? v - g.X[k] : v);
    }
}
// ---- direct gather: one thread per (site, parity), the direction in blockIdx.y.  Running product, loaded link and accumulator are
// the three live matrices (54 fp64 = 108 VGPRs); arithmetic in fp64 whatever the link precision ----
template <typename T, int R>
__global__ void __launch_bounds__(128) gauge_force_kernel(double *mom, GaugeView g, double eb3, int Vh) {
  const int gid = blockIdx.x * blockDim.x + threadIdx.x;
  if (gid >= 2 * Vh) return;
  const int mu = blockIdx.y;
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
  M3 V;
#pragma unroll
  for (int k = 0; k < 9; k++) V.re[k] = V.im[k] = 0;
  const int n = c_force.num_paths;
  for (int i = 0; i < n; i++) {
    const double c = c_force.coeff[i];
    if (c == 0) continue;
    int y[4] = {x[0], x[1], x[2], x[3]};
    hop(y, mu, +1, g);
    M3 A, B;
    const int len = c_force.length[i];
    for (int j = 0; j < len; j++) {
      const int d = c_force.step[mu][i][j];
      const bool fwd = d < 4;
      const int dir = fwd ? d : 7 - d;
      if (!fwd) hop(y, dir, -1, g);
      load_link<T, R>(B, g, dir, y);
      if (j == 0) {
        if (fwd) A = B; else m3_dag(A, B);
      } else {
        if (fwd) m3_mul_right(A, B); else m3_mul_right_dag(A, B);
      }
      if (fwd) hop(y, dir, +1, g);
    }
    if (len > 0) {
#pragma unroll
      for (int k = 0; k < 9; k++) { V.re[k] += c * A.re[k]; V.im[k] += c * A.im[k]; }
    }
  }
  M3 U;
  load_link<T, R>(U, g, mu, x);
  force_epilogue(mom + ((size_t)gid * 4 + mu) * 10, U, V, eb3);
}

// ---- transport ----
__global__ void mf_identity_kernel(MatField out, int Vh) {
  const int gid = blockIdx.x * blockDim.x + threadIdx.x;
  if (gid >= 2 * Vh) return;
  const int par = gid >= Vh, idx = gid - par * Vh;
  M3 m;
#pragma unroll
  for (int k = 0; k < 9; k++) { m.re[k] = (k % 4 == 0) ? 1.0 : 0.0; m.im[k] = 0; }
  mf_store(m, out, par, idx);
}
// acc += c in
__global__ void mf_axpy_kernel(MatField acc, double c, MatField in, int Vh) {
  const int gid = blockIdx.x * blockDim.x + threadIdx.x;
  if (gid >= 2 * Vh) return;
  const int par = gid >= Vh, idx = gid - par * Vh;
  M3 a, b;
  mf_load(a, acc, par, idx); mf_load(b, in, par, idx);
#pragma unroll
  for (int k = 0; k < 9; k++) { a.re[k] += c * b.re[k]; a.im[k] += c * b.im[k]; }
  mf_store(a, acc, par, idx);
}
__global__ void __launch_bounds__(128) force_epilogue_kernel(double *mom, MatField U, MatField V, int mu, double eb3, int Vh) {
  const int gid = blockIdx.x * blockDim.x + threadIdx.x;
  if (gid >= 2 * Vh) return;
  const int par = gid >= Vh, idx = gid - par * Vh;
  M3 u, v;
  mf_load(u, U, par, idx); mf_load(v, V, par, idx);
  force_epilogue(mom + ((size_t)gid * 4 + mu) * 10, u, v, eb3);
}

// R_{n+1} = 1; a forward step d gives R_k(y) = U_d(y) R_{k+1}(y + d), a backward step R_k(y) = [U_d^dag R_{k+1}](y - d); the path's
// product seen from x is R_1(x + mu).  One shift and one product per link, every shift a single hop.
static void gaugeForceTransport(MomField &mom, const GaugeField &U, double eb3, int ***path, const int *length, const double *coeff, int num_paths) {
  const LatticeGeom &geom = U.geom;
  const int Vh = geom.Vh;
  MatPool pool(Vh, 8);
  const MatField F[4] = {pool[0], pool[1], pool[2], pool[3]}, Rf = pool[4], T = pool[5], acc = pool[6], Vf = pool[7];
  for (int mu = 0; mu < 4; mu++) extractForwardLinks(F[mu], U, mu);
  for (int mu = 0; mu < 4; mu++) {
    HIP_CHECK(hipMemsetAsync(acc.p, 0, pool.fieldDoubles() * sizeof(double), computeStream()));
    for (int i = 0; i < num_paths; i++) {
      if (coeff[i] == 0 || length[i] <= 0) continue;
      launchSites(mf_identity_kernel, Vh, 128, Rf, Vh);
      for (int j = length[i] - 1; j >= 0; j--) {
        const int d = path[mu][i][j];
        if (d < 4) {
          shiftField(T, Rf, geom, 2 * d);         // R(y + d)
          mfMul(Rf, F[d], T, 0, 0, 0);
        } else {
          mfMul(T, F[7 - d], Rf, 1, 0, 0);        // U_d(y)^dag R(y), wanted at y + d
          shiftField(Rf, T, geom, 2 * (7 - d) + 1);
        }
      }
      launchSites(mf_axpy_kernel, Vh, 128, acc, coeff[i], Rf, Vh);
    }
    shiftField(Vf, acc, geom, 2 * mu);
    launchSites(force_epilogue_kernel, Vh, 128, mom.data, F[mu], Vf, mu, eb3, Vh);
  }
  HIP_CHECK(hipStreamSynchronize(computeStream()));
}

bool gaugeForceUsesTransport() { return usesTransport("QUDA_AMD_GAUGE_FORCE_TRANSPORT"); }   // the variable: for tests and timing

void gaugeForce(MomField &mom, const GaugeField &U, double eb3, int ***path, const int *length, const double *coeff, int num_paths, int max_length) {
  if (!(U.geom == mom.geom)) errorQuda("gauge and momentum geometry differ");
  if (max_length > kGaugeForceMaxLength) errorQuda("gauge force: max_length = %d exceeds the cap of %d links per path", max_length, kGaugeForceMaxLength);
  if (num_paths < 0 || num_paths > kGaugeForceMaxPaths) errorQuda("gauge force: num_paths = %d outside 0..%d", num_paths, kGaugeForceMaxPaths);
  for (int i = 0; i < num_paths; i++) {
    if (length[i] < 0 || length[i] > max_length) errorQuda("gauge force: path %d has length %d, max_length = %d", i, length[i], max_length);
    for (int mu = 0; mu < 4; mu++)
      for (int j = 0; j < length[i]; j++)
        if (path[mu][i][j] < 0 || path[mu][i][j] > 7) errorQuda("gauge force: path %d of direction %d, step %d = %d outside 0..7", i, mu, j, path[mu][i][j]);
  }
  if (gaugeForceUsesTransport()) { gaugeForceTransport(mom, U, eb3, path, length, coeff, num_paths); return; }
  ForceTable tab;
  memset(&tab, 0, sizeof(tab));
  tab.num_paths = num_paths;
  for (int i = 0; i < num_paths; i++) {
    tab.length[i] = length[i]; tab.coeff[i] = coeff[i];
    for (int mu = 0; mu < 4; mu++)
      for (int j = 0; j < length[i]; j++) tab.step[mu][i][j] = (signed char)path[mu][i][j];
  }
  hipStream_t s = computeStream();
  HIP_CHECK(hipMemcpyToSymbolAsync(HIP_SYMBOL(c_force), &tab, sizeof(tab), 0, hipMemcpyHostToDevice, s));
  HIP_CHECK(hipStreamSynchronize(s));   // tab is a stack object
  const GaugeView g = viewOf(U);
  const int Vh = U.geom.Vh, bs = 128, nb = (2 * Vh + bs - 1) / bs;
  forLinkType(U, [&](auto t, auto r) {
    hipLaunchKernelGGL((gauge_force_kernel<decltype(t), decltype(r)::value>), dim3(nb, 4), dim3(bs), 0, s, mom.data, g, eb3, Vh);
  });
  HIP_CHECK(hipGetLastError());
  HIP_CHECK(hipStreamSynchronize(s));
}

// ---- link update (lib/gauge_update_quda.cu:109-152): the trace of A removed; exact: U <- exp(dt A) U through su3_exp_iq with
// Q = -i dt A; else the eighth-order Horner form R = (dt/r) A R + U, r = 8..1, from R = U.  conj_mom: the complex conjugate of A,
// entry by entry (not A^dag).  One thread per (site, parity) of direction mu; the new links leave in host QDP order ----
__global__ void __launch_bounds__(128) gauge_update_kernel(double *qdp, MatField F, const double *mom, int mu, double dt, int conj_mom, int exact, int Vh) {
  const int gid = blockIdx.x * blockDim.x + threadIdx.x;
  if (gid >= 2 * Vh) return;
  const int par = gid >= Vh, idx = gid - par * Vh;
  M3 u, a, r;
  mf_load(u, F, par, idx);
  const double *m = mom + ((size_t)gid * 4 + mu) * 10;
  const double cs = conj_mom ? -1.0 : 1.0;   // conj A: the imaginary parts change sign
  const double tr = (m[6] + m[7] + m[8]) * (1.0 / 3.0);
  a.re[0] = a.re[4] = a.re[8] = 0;
  a.im[0] = cs * (m[6] - tr); a.im[4] = cs * (m[7] - tr); a.im[8] = cs * (m[8] - tr);
  a.re[1] = m[0]; a.im[1] = cs * m[1]; a.re[3] = -m[0]; a.im[3] = cs * m[1];
  a.re[2] = m[2]; a.im[2] = cs * m[3]; a.re[6] = -m[2]; a.im[6] = cs * m[3];
  a.re[5] = m[4]; a.im[5] = cs * m[5]; a.re[7] = -m[4]; a.im[7] = cs * m[5];
  if (exact) {
    M3 q, e;
#pragma unroll
    for (int k = 0; k < 9; k++) { q.re[k] = dt * a.im[k]; q.im[k] = -(dt * a.re[k]); }
    su3_exp_iq(e, q);
    m3_mul(r, e, u);
  } else {
    r = u;
    for (int o = 8; o >= 1; o--) {
      M3 t;
      m3_mul(t, a, r);
      const double f = dt / o;
#pragma unroll
      for (int k = 0; k < 9; k++) { r.re[k] = f * t.re[k] + u.re[k]; r.im[k] = f * t.im[k] + u.im[k]; }
    }
  }
  double *o = qdp + (size_t)gid * 18;
#pragma unroll
  for (int k = 0; k < 9; k++) { o[2 * k] = r.re[k]; o[2 * k + 1] = r.im[k]; }
}

// ---- SU(3) projection (lib/interface_quda.cpp:5187-5247): the polar projection and determinant phase of the APE step (polar_su3)
// on every link; a link whose max |U^dag U - 1| still exceeds tol afterwards counts as a failure.  The anti-periodic sign of the
// time links on the last time slice (det -1) is taken off before the projection and put back after it ----
__global__ void __launch_bounds__(128) project_su3_kernel(double *qdp, int *failures, MatField F, int sign_t, double tol, int Vh) {
  const int gid = blockIdx.x * blockDim.x + threadIdx.x;
  if (gid >= 2 * Vh) return;
  const int par = gid >= Vh, idx = gid - par * Vh;
  M3 u;
  mf_load(u, F, par, idx);
  const double sg = (sign_t >= 0 && idx >= sign_t) ? -1.0 : 1.0;   // sign_t: first checkerboard index of the last time slice (t runs slowest), or -1
#pragma unroll
  for (int k = 0; k < 9; k++) { u.re[k] *= sg; u.im[k] *= sg; }
  polar_su3(u, 1e-15);
  if (!(unitarity_deviation(u) <= tol)) atomicAdd(failures, 1);
  double *o = qdp + (size_t)gid * 18;
#pragma unroll
  for (int k = 0; k < 9; k++) { o[2 * k] = sg * u.re[k]; o[2 * k + 1] = sg * u.im[k]; }
}

void updateGaugeLinks(void *const h_out[4], const GaugeField &U, const MomField &mom, double dt, bool conj_mom, bool exact) {
  if (!(U.geom == mom.geom)) errorQuda("gauge and momentum geometry differ");
  const int Vh = U.geom.Vh;
  linksToHost(h_out, U, [&](double *stage, MatField F, int mu) { launchSites(gauge_update_kernel, Vh, 128, stage, F, mom.data, mu, dt, conj_mom ? 1 : 0, exact ? 1 : 0, Vh); });
}

long projectSU3Links(void *const h_out[4], const GaugeField &U, double tol) {
  const int Vh = U.geom.Vh;
  int *d_fail = nullptr;
  HIP_CHECK(qaMalloc((void **)&d_fail, sizeof(int)));
  HIP_CHECK(hipMemsetAsync(d_fail, 0, sizeof(int), computeStream()));
  const bool last_t = commGrid().coords[3] == commGrid().dims[3] - 1;
  const int sliceCB = Vh / U.geom.X[3];
  linksToHost(h_out, U, [&](double *stage, MatField F, int mu) {
    const int sign_t = (mu == 3 && U.t_boundary == QUDA_ANTI_PERIODIC_T && last_t) ? sliceCB * (U.geom.X[3] - 1) : -1;
    launchSites(project_su3_kernel, Vh, 128, stage, d_fail, F, sign_t, tol, Vh);
  });
  int fail = 0;
  HIP_CHECK(hipMemcpy(&fail, d_fail, sizeof(int), hipMemcpyDeviceToHost));
  HIP_CHECK(hipFree(d_fail));
  double f = fail;
  comm_allreduce(&f, 1);
  return (long)f;
}

// ---- momentum action (lib/momentum.cu:31-48): sum over links of sum_{j<6} v_j^2 + (1/2) sum_{j=6..8} v_j^2 - 4 = tr(A^dag A)/2 - 4.
// One thread per link, one partial per block in a fixed order (block_sum_256), the partials added in block order by the host as in
// topologicalCharge: the same field gives the same bits ----
__global__ void __launch_bounds__(256) mom_action_kernel(double *partial, const double *mom, long nLinks) {
  const long gid = (long)blockIdx.x * blockDim.x + threadIdx.x;
  double v = 0;
  if (gid < nLinks) {
    const double *m = mom + gid * 10;
    double off = 0, dia = 0;
#pragma unroll
    for (int j = 0; j < 6; j++) off += m[j] * m[j];
#pragma unroll
    for (int j = 6; j < 9; j++) dia += m[j] * m[j];
    v = (off + 0.5 * dia) - 4.0;
  }
  v = block_sum_256(v);
  if (threadIdx.x == 0) partial[blockIdx.x] = v;
}

double momAction(const MomField &mom) {
  const long nLinks = (long)mom.geom.V * 4;
  const int bs = 256, nb = (int)((nLinks + bs - 1) / bs);
  double *d_partial = nullptr;
  HIP_CHECK(qaMalloc((void **)&d_partial, (size_t)nb * sizeof(double)));
  hipLaunchKernelGGL(mom_action_kernel, dim3(nb), dim3(bs), 0, computeStream(), d_partial, mom.data, nLinks);
  HIP_CHECK(hipGetLastError());
  double S = sumPartials(d_partial, nb);
  HIP_CHECK(hipFree(d_partial));
  comm_allreduce(&S, 1);
  return S;
}

}  // namespace quda
