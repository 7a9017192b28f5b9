// momproj.hip — the tail that the two-point (contract.hip), loop (loop.hip) and three-point (threep.hip) contractions share: the
// momentum-space accumulator, the chunked stage-and-project driver, momentum projection of staged per-site blocks of 16 complex
// numbers with a fixed summation order, and the sum over ranks.  The contract is stated at the declarations in qkxtm_internal.h.
//
// Reference: performFFT (lib/qudaQKXTM_Kepler_utils.cpp:300-357), the Fourier transform of the two-point functions
// (lib/qudaQKXTM_Contraction_Kepler.cpp), both followed by an MPI reduction over the spatial ranks.
#include <algorithm>
#include <cmath>
#include <cstring>

#include "comm_quda.h"
#include "p2p.h"
#include "qkxtm_internal.h"

namespace quda {

namespace momproj {

constexpr int NGM = 16;
constexpr int NPART = 64;   // partial sums per (block, time slice, momentum): fixed, whatever the lattice or the launch
constexpr int NLANE = 16;   // site lanes of a partial sum, reduced in order
constexpr int MB_SMALL = 8, MB_LARGE = 36;   // momenta per projection block: 36 holds Q_sq <= 4 (33 momenta) in one pass over the staged blocks

// part[(((k * nt + tl) * NPART + p) * Nm + m) * 16 + gm] = sum over the p-th fixed share of the slice's sites of e^{-2 pi i n.x / L} cs[k][tl, site][gm],
// x the GLOBAL coordinate.  One phase per (site, momentum) serves the 16 entries of a block; it is the product of three factors from
// per-direction tables in LDS.  A share is summed by NLANE site lanes (sites s0 + lane, s0 + lane + NLANE, ...), then the lanes in order.
template <int MB> __global__ void __launch_bounds__(256) project_kernel(double2 *part, const double2 *cs, long S, int Vs, int nt, const int *moms, int Nm, int nmb, int X0, int Y, int Z,
                                                           int gx0, int gx1, int gx2, int L0, int L1, int L2) {
  extern __shared__ double2 lds[];
  double2 *ex = lds, *ey = ex + MB * X0, *ez = ey + MB * Y, *red = ez + MB * Z;
  // the momentum chunks of one share are neighbours in the launch order: they read the same staged data at the same time
  const int p = blockIdx.x / nmb, tl = blockIdx.y, k = blockIdx.z, m0 = (blockIdx.x % nmb) * MB;
  const int nm = min(MB, Nm - m0);
  for (int i = threadIdx.x; i < MB * (X0 + Y + Z); i += blockDim.x) {
    int m, c, L, n, gc;
    if (i < MB * X0) { m = i / X0; c = i % X0; L = L0; gc = c + gx0; n = m < nm ? moms[3 * (m0 + m)] : 0; }
    else if (i < MB * (X0 + Y)) { const int q = i - MB * X0; m = q / Y; c = q % Y; L = L1; gc = c + gx1; n = m < nm ? moms[3 * (m0 + m) + 1] : 0; }
    else { const int q = i - MB * (X0 + Y); m = q / Z; c = q % Z; L = L2; gc = c + gx2; n = m < nm ? moms[3 * (m0 + m) + 2] : 0; }
    const long kk = (((long)n * gc) % L + L) % L;   // reduced mod L so the phase argument stays small
    double sn, cn;
    sincos(2.0 * M_PI * (double)kk / L, &sn, &cn);
    lds[i] = make_double2(cn, -sn);
  }
  __syncthreads();
  const int gm = threadIdx.x & 15, sl = threadIdx.x >> 4;
  const long s0 = (long)Vs * p / NPART, s1 = (long)Vs * (p + 1) / NPART;
  double2 acc[MB];
#pragma unroll
  for (int m = 0; m < MB; m++) acc[m] = make_double2(0, 0);
  const double2 *src = cs + ((long)k * S + (long)tl * Vs) * NGM + gm;
  for (long s = s0 + sl; s < s1; s += NLANE) {
    const int x = (int)(s % X0), y = (int)((s / X0) % Y), z = (int)(s / ((long)X0 * Y));
    const double2 c = src[s * NGM];
#pragma unroll
    for (int m = 0; m < MB; m++) {
      const double2 a = ex[m * X0 + x], b = ey[m * Y + y], d = ez[m * Z + z];
      const double2 ab = make_double2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x);
      const double2 ph = make_double2(ab.x * d.x - ab.y * d.y, ab.x * d.y + ab.y * d.x);
      acc[m].x += c.x * ph.x - c.y * ph.y;
      acc[m].y += c.x * ph.y + c.y * ph.x;
    }
  }
#pragma unroll
  for (int m = 0; m < MB; m++) {
    red[threadIdx.x] = acc[m];
    __syncthreads();
    if (sl == 0 && m < nm) {
      double2 r = red[gm];
      for (int q = 1; q < NLANE; q++) { r.x += red[q * 16 + gm].x; r.y += red[q * 16 + gm].y; }
      part[((((long)k * nt + tl) * NPART + p) * Nm + m0 + m) * NGM + gm] = r;
    }
    __syncthreads();
  }
}

// acc[((k * Lt + t0 + tl) * Nm + m) * 16 + gm] += sum_p part[...], p = 0 .. NPART-1 in order
__global__ void __launch_bounds__(256) reduce_kernel(double2 *acc, const double2 *part, int nblk, int nt, int Lt, int t0, int Nm) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const long per = (long)Nm * NGM;
  if (i >= (long)nblk * nt * per) return;
  const int k = (int)(i / (nt * per)), tl = (int)((i / per) % nt);
  const long r = i % per;
  double2 sum = make_double2(0, 0);
  for (int p = 0; p < NPART; p++) {
    const double2 c = part[(((long)k * nt + tl) * NPART + p) * per + r];
    sum.x += c.x; sum.y += c.y;
  }
  double2 *dst = acc + ((long)k * Lt + t0 + tl) * per + r;
  const double2 old = *dst;
  *dst = make_double2(old.x + sum.x, old.y + sum.y);
}

}  // namespace momproj

void momentumProject(double2 *acc, const double2 *cs, int nblk, int t0, int nt, int Lt, const int *d_moms, int Nm, const int X[3], const int gx[3], const int L[3]) {
  using namespace momproj;
  if (nblk < 1 || nblk > 65535 || nt < 1 || nt > 65535 || t0 < 0 || t0 + nt > Lt || Nm < 1) errorQuda("momentum projection: nblk = %d, slices [%d, %d) of %d, %d momenta", nblk, t0, t0 + nt, Lt, Nm);
  // all momenta in one pass where the phase tables of MB_LARGE momenta fit into 64 KiB of LDS, else chunks of MB_SMALL
  auto ldsOf = [&](int mb) { return ((size_t)mb * (X[0] + X[1] + X[2]) + 256) * sizeof(double2); };
  const bool large = Nm > MB_SMALL && Nm <= MB_LARGE && ldsOf(MB_LARGE) <= 64 * 1024;
  const int mbs = large ? MB_LARGE : MB_SMALL;
  const int nmb = (Nm + mbs - 1) / mbs;
  const size_t ldsBytes = ldsOf(mbs);
  if (ldsBytes > 64 * 1024) errorQuda("momentum projection: spatial extents %d %d %d exceed the phase tables", X[0], X[1], X[2]);
  const int Vs = X[0] * X[1] * X[2];
  const long S = (long)nt * Vs;
  double2 *part = (double2 *)stagingBuffer((size_t)nblk * nt * NPART * Nm * NGM * sizeof(double2));
  hipStream_t st = computeStream();
  hipLaunchKernelGGL(large ? project_kernel<MB_LARGE> : project_kernel<MB_SMALL>, dim3(NPART * nmb, nt, nblk), dim3(256), ldsBytes, st, part, cs, S, Vs, nt, d_moms, Nm, nmb, X[0],
                     X[1], X[2], gx[0], gx[1], gx[2], L[0], L[1], L[2]);
  const long nred = (long)nblk * nt * Nm * NGM;
  hipLaunchKernelGGL(reduce_kernel, dim3((unsigned)((nred + 255) / 256)), dim3(256), 0, st, acc, part, nblk, nt, Lt, t0, Nm);
  HIP_CHECK(hipGetLastError());
}

void gatherTimeBlocks(double *out, const double *d_loc, int nblk, int Lt, size_t per) {
  const CommGrid &cg = commGrid();
  const int T = Lt * cg.dims[3];
  const size_t total = (size_t)nblk * T * per;
  std::vector<double> loc((size_t)nblk * Lt * per);
  HIP_CHECK(hipMemcpyAsync(loc.data(), d_loc, loc.size() * sizeof(double), hipMemcpyDeviceToHost, computeStream()));
  HIP_CHECK(hipStreamSynchronize(computeStream()));
  memset(out, 0, total * sizeof(double));
  for (int k = 0; k < nblk; k++) memcpy(out + ((size_t)k * T + (size_t)cg.coords[3] * Lt) * per, &loc[(size_t)k * Lt * per], (size_t)Lt * per * sizeof(double));
  if (cg.size == 1) return;
  std::vector<double> all(total * cg.size);
  commAllgatherBytes(out, all.data(), total * sizeof(double));
  for (size_t i = 0; i < total; i++) {
    double v = 0;
    for (int r = 0; r < cg.size; r++) v += all[(size_t)r * total + i];
    out[i] = v;
  }
}

MomAccum::MomAccum(int nblk_, std::vector<int> moms_) : nblk(nblk_), Lt(residentGeom().X[3]), Nm((int)moms_.size() / 3), moms(std::move(moms_)) {
  HIP_CHECK(hipMalloc(&d, (size_t)nblk * Lt * per() * sizeof(double)));
  HIP_CHECK(hipMalloc(&d_moms, moms.size() * sizeof(int)));
  HIP_CHECK(hipMemcpyAsync(d_moms, moms.data(), moms.size() * sizeof(int), hipMemcpyHostToDevice, computeStream()));
  zero();
}
MomAccum::~MomAccum() { (void)hipFree(d); (void)hipFree(d_moms); }
void MomAccum::zero() { HIP_CHECK(hipMemsetAsync(d, 0, (size_t)nblk * Lt * per() * sizeof(double), computeStream())); }
void MomAccum::get(double *out) const { gatherTimeBlocks(out, (const double *)d, nblk, Lt, per()); }

double elapsedSecs(hipEvent_t a, hipEvent_t b) {
  float ms = 0;
  HIP_CHECK(hipEventElapsedTime(&ms, a, b));
  return ms * 1e-3;
}

void stageAndProject(MomAccum &A, const int gx[3], int maxSlicesPerChunk, const std::function<void(int t0, int nt, double2 *cs)> &stage, double secs[2]) {
  const LatticeGeom &g = residentGeom();
  const CommGrid &cg = commGrid();
  if (A.Lt != g.X[3]) errorQuda("contraction: the accumulator belongs to another lattice");
  hipStream_t st = computeStream();
  const int Vs = g.X[0] * g.X[1] * g.X[2], Lt = A.Lt;
  const int L[3] = {g.X[0] * cg.dims[0], g.X[1] * cg.dims[1], g.X[2] * cg.dims[2]};
  // time slices per chunk: the staged blocks stay below 2 GiB
  const size_t perSlice = (size_t)Vs * A.nblk * momproj::NGM * sizeof(double2);
  int tc = (int)std::max<size_t>(1, std::min<size_t>((size_t)Lt, ((size_t)2 << 30) / perSlice));
  if (maxSlicesPerChunk > 0) tc = std::min(tc, maxSlicesPerChunk);
  double2 *cs = nullptr;
  HIP_CHECK(hipMalloc(&cs, perSlice * tc));
  std::vector<hipEvent_t> marks;   // per chunk: before the staging kernels, after them, after the projection
  auto mark = [&]() { if (!secs) return; hipEvent_t e; HIP_CHECK(hipEventCreate(&e)); HIP_CHECK(hipEventRecord(e, st)); marks.push_back(e); };
  for (int t0 = 0; t0 < Lt; t0 += tc) {
    const int nt = std::min(tc, Lt - t0);
    mark();
    stage(t0, nt, cs);
    mark();
    momentumProject(A.d, cs, A.nblk, t0, nt, Lt, A.d_moms, A.Nm, g.X, gx, L);
    mark();
  }
  HIP_CHECK(hipStreamSynchronize(st));
  if (secs) secs[0] = secs[1] = 0;
  for (size_t i = 0; i < marks.size(); i += 3) {
    secs[0] += elapsedSecs(marks[i], marks[i + 1]);
    secs[1] += elapsedSecs(marks[i + 1], marks[i + 2]);
  }
  for (hipEvent_t e : marks) (void)hipEventDestroy(e);
  (void)hipFree(cs);
}

int copyMomenta(const std::vector<int> &m, int *moms, int max_moms, const char *fname) {
  const int n = (int)m.size() / 3;
  if (moms) {
    if (max_moms < n) errorQuda("%s: %d momenta do not fit into max_moms = %d", fname, n, max_moms);
    memcpy(moms, m.data(), m.size() * sizeof(int));
  }
  return n;
}

}  // namespace quda

using namespace quda;

extern "C" {

void qudaAmdMomentumProject(double *h_acc, const double *h_cs, int nblk, int t0, int nt, int Lt, const int *moms, int Nm, const int X[3], const int gx[3], const int L[3]) {
  if (!h_acc || !h_cs || !moms || !X || !gx || !L) errorQuda("qudaAmdMomentumProject: NULL argument");
  if (nblk < 1 || nt < 1 || Lt < 1 || Nm < 1 || X[0] < 1 || X[1] < 1 || X[2] < 1 || L[0] < 1 || L[1] < 1 || L[2] < 1) errorQuda("qudaAmdMomentumProject: bad extents");
  const size_t accBytes = (size_t)nblk * Lt * Nm * momproj::NGM * sizeof(double2);
  const size_t csBytes = (size_t)nblk * nt * X[0] * X[1] * X[2] * momproj::NGM * sizeof(double2);
  hipStream_t st = computeStream();
  double2 *acc = nullptr, *cs = nullptr;
  int *d_moms = nullptr;
  HIP_CHECK(hipMalloc(&acc, accBytes));
  HIP_CHECK(hipMalloc(&cs, csBytes));
  HIP_CHECK(hipMalloc(&d_moms, (size_t)Nm * 3 * sizeof(int)));
  HIP_CHECK(hipMemcpyAsync(acc, h_acc, accBytes, hipMemcpyHostToDevice, st));
  HIP_CHECK(hipMemcpyAsync(cs, h_cs, csBytes, hipMemcpyHostToDevice, st));
  HIP_CHECK(hipMemcpyAsync(d_moms, moms, (size_t)Nm * 3 * sizeof(int), hipMemcpyHostToDevice, st));
  momentumProject(acc, cs, nblk, t0, nt, Lt, d_moms, Nm, X, gx, L);
  HIP_CHECK(hipMemcpyAsync(h_acc, acc, accBytes, hipMemcpyDeviceToHost, st));
  HIP_CHECK(hipStreamSynchronize(st));
  (void)hipFree(acc); (void)hipFree(cs); (void)hipFree(d_moms);
}

}  // extern "C"
