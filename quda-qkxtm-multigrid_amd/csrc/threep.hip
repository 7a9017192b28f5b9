// threep.hip — nucleon three-point functions by the fixed-sink sequential method on the device: the sequential source on the sink
// time slice, and the contraction of the twelve sequential solutions with a forward propagator into the ultra-local operators, the
// one-derivative operators and the conserved current.
//
// Reference: calcMG_threepTwop_EvenOdd (lib/interface_quda.cpp:6560-6950), seqSourceFixSinkPart{1,2}_core_Kepler.h,
// fixSinkContractions_{local,noether,oneD}_core_Kepler.h (lib/code_pieces_Kepler), writeThrp_ASCII
// (lib/qudaQKXTM_Contraction_Kepler.cpp:2842-3003).
//
// All spin matrices are in the UKQCD basis of gamma_host.h and are built on the host from explicit gamma products.
//
// Sequential source.  P[x; mu, nu; a, b] a propagator (sink spin / colour mu, a; source column nu, b), U3 / D3 the sink-smeared,
// unrotated up / down propagators.  With A = C g5, Q = (U3, D3, U3) for the proton and (D3, U3, D3) for the neutron,
//      N[x; k, n] = sum eps_abc eps_def A_ij A_lm ( Q0[i,l;a,d] Q1[j,m;b,e] Q2[k,n;c,f] - Q0[i,n;a,f] Q1[j,m;b,e] Q2[k,l;c,d] ),
//      f(x) = sum_kn G_tm[n][k] N[x; k, n],    G_tm = R_p G R_p,  R_p = (1 + p i g5) / sqrt2,  p = +1 proton, -1 neutron,
// part 1 is df / dQ0 + df / dQ2 (the flavour that occurs twice), part 2 df / dQ1.  f is linear in every slot, so the derivative is
// f with that slot left open: sigma_(nu', c')[x; nu, c] = df / dP[x; nu, nu'; c, c'].  The solver gets g5 conj(sigma), smeared.
//
// Contraction.  y_(pi, b) the twelve sequential solutions, q[x; kappa, pi; a, b] = conj((g5 y_(pi, b))[x; kappa, a]), F the forward
// propagator.  With the building block of the loops, C[u, v][4 kappa + lambda] = sum_a conj(u[(kappa + 2) mod 4, a]) v[lambda, a]
// (g5 exchanges spin kappa and kappa + 2), and the covariant shifts (Fw v)(x) = U_mu(x) v(x + mu), (Bw v)(x) = U_mu(x - mu)^+ v(x - mu),
// the nine 4 x 4 matrices per site are sums over the twelve columns of
//      S0 = C[y, F],    A_mu + D_mu = C[y, Fw F] + C[Bw y, F],    B_mu + C_mu = C[y, Bw F] + C[Fw y, F].
// One stencil kernel writes them for a chunk of time slices into cs[9][site][16]; nine threads share a site (S0, and direction x
// {A + D, B + C}), in nine neighbouring work-groups.  A thread streams the twelve columns and holds the 4 x 4 accumulator, one link
// and two spinors (two passes over the columns, one per link).  The shared momentum projection (momproj.hip) takes the staged blocks;
// the operator tables, the factor 1/4 and the wrap sign act on its result.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "basis.h"
#include "blas.h"
#include "comm_quda.h"
#include "contract_stencil.h"
#include "device_io.h"
#include "gamma_host.h"
#include "interface_internal.h"
#include "p2p.h"
#include "qa_core.h"
#include "qkxtm_internal.h"
#include "quda_amd_ext.h"
#include "qudaQKXTM_Kepler_utils.h"

namespace quda {

namespace threep {

using namespace gammah;

constexpr int NBLK = 9, NGM = 16, NCOL = 12;

// ================================ the sequential source ================================
struct SeqArg {
  int acol[4];        // A = C g5 is a signed permutation: A[i][acol[i]] = aval[i]
  double2 aval[4];
  double2 G[4][4];    // G_tm[n][k]
  int part;           // 1: both slots of the doubly present flavour open, 2: the slot of the other flavour
};

// out[column nu' c'][site][nu, c] = (g5 conj(sigma))[nu, c] on the sites of the local time slice tl; P2 the flavour that occurs twice
// (slots 0 and 2), P1 the other (slot 1).  One thread per (site of the slice, column).
__global__ void __launch_bounds__(64) seq_source_kernel(double *out, const double2 *P2, const double2 *P1, long V, int Vs, int tl, const SeqArg a) {
  const int s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= Vs) return;
  const int col = blockIdx.y, nup = col / 3, cp = col % 3;
  const long site = (long)tl * Vs + s;
  int ainv[4];
  for (int i = 0; i < 4; i++) ainv[a.acol[i]] = i;
  double2 *o = (double2 *)(out + ((size_t)col * V + site) * 24);
  for (int nu = 0; nu < 4; nu++)
    for (int c = 0; c < 3; c++) {
      double2 res = make_double2(0, 0);
      for (int term = 0; term < 2; term++) {
        // sink slot sl -> source slot pi[sl]: direct (0, 1, 2), exchange (2, 1, 0) with weight -1
        int pi[3];
        pi[0] = term ? 2 : 0; pi[1] = 1; pi[2] = term ? 0 : 2;
        for (int r = 0; r < 3; r++) {
          if ((a.part == 1) == (r == 1)) continue;
          const int q = pi[r];   // the source slot of the open propagator
          // sink spins (i, j = acol[i], k), source spins (l, m = acol[l], n): the open slot fixes one of (i, k) and one of (l, n)
          const int ilo = r == 0 ? nu : (r == 1 ? ainv[nu] : 0), ihi = r == 2 ? 3 : ilo;
          const int klo = r == 2 ? nu : 0, khi = r == 2 ? nu : 3;
          const int llo = q == 0 ? nup : (q == 1 ? ainv[nup] : 0), lhi = q == 2 ? 3 : llo;
          const int nlo = q == 2 ? nup : 0, nhi = q == 2 ? nup : 3;
          for (int e1 = 0; e1 < 6; e1++) {
            if (c_eps[e1][r] != c) continue;
            for (int e2 = 0; e2 < 6; e2++) {
              if (c_eps[e2][q] != cp) continue;
              const double w = (term ? -1.0 : 1.0) * c_eps_sign[e1] * c_eps_sign[e2];
              for (int i = ilo; i <= ihi; i++)
                for (int k = klo; k <= khi; k++)
                  for (int l = llo; l <= lhi; l++)
                    for (int n = nlo; n <= nhi; n++) {
                      int ss[3], ts[3];
                      ss[0] = i; ss[1] = a.acol[i]; ss[2] = k;
                      ts[0] = l; ts[1] = a.acol[l]; ts[2] = n;
                      double2 v = cmul(cmul(a.aval[i], a.aval[l]), a.G[n][k]);
                      for (int sl = 0; sl < 3; sl++) {
                        if (sl == r) continue;
                        const double2 *P = sl == 1 ? P1 : P2;
                        v = cmul(v, P[prop_index(ss[sl], ts[pi[sl]], c_eps[e1][sl], c_eps[e2][pi[sl]], V, site)]);
                      }
                      res.x += w * v.x; res.y += w * v.y;
                    }
            }
          }
        }
      }
      o[(nu ^ 2) * 3 + c] = make_double2(res.x, -res.y);   // g5 conj: spin nu of sigma goes to spin nu ^ 2
    }
}

// ================================ the contraction stencil ================================
struct ThreepArg : StencilGeom {
  const double *y[NCOL][2], *F[NCOL][2];   // parity blocks of the twelve columns, UKQCD basis: fields col and 12 + col of the ghost zones
};

// acc[4 kappa + lambda] += sum_c conj(u[(kappa + 2) mod 4, c]) v[lambda, c]
__device__ __forceinline__ void accumulate(double *acc, const double *u, const double *v) {
#pragma unroll
  for (int k = 0; k < 4; k++)
#pragma unroll
    for (int l = 0; l < 4; l++) spin_dot(acc[2 * (4 * k + l)], acc[2 * (4 * k + l) + 1], u + 6 * ((k + 2) & 3), v + 6 * l);
}

// A work-group holds 128 sites of one parity and ONE task, so the field pointers, the links' block and the direction are uniform: task 8
// is S0, task j < 8 direction mu = j / 2, j even A + D, j odd B + C.  The nine tasks of a group of sites are neighbours in the launch
// order and read the same columns.
template <int R> __global__ void __launch_bounds__(128) threep_stencil_kernel(const ThreepArg a) {
  const int j = blockIdx.x % 9, parity = blockIdx.y, op = 1 - parity;
  const long ih = (long)(blockIdx.x / 9) * 128 + threadIdx.x;   // checkerboard site of the chunk
  if (2 * ih >= a.S) return;
  const int X0 = a.X0, Y = a.Y, Z = a.Z, T = a.T, Xh = X0 >> 1;
  const int idx = (int)((long)a.t0 * (Xh * Y * Z) + ih);
  int l = idx / Xh;
  const int y = l % Y; l /= Y;
  const int z = l % Z, t = l / Z;
  const int xc = 2 * (idx % Xh) + ((y + z + t + parity) & 1);
  const long s = 2 * ih + (xc & 1);                             // lexicographic site of the chunk
  double acc[2 * NGM];
#pragma unroll
  for (int k = 0; k < 2 * NGM; k++) acc[k] = 0;
  double psi[24], v[24];

  if (j == 8) {
#pragma unroll 1
    for (int col = 0; col < NCOL; col++) {
      Planar<double, 24>::load(psi, a.y[col][parity], a.sp_stride, idx, nullptr, idx);
      Planar<double, 24>::load(v, a.F[col][parity], a.sp_stride, idx, nullptr, idx);
      accumulate(acc, psi, v);
    }
  } else {
    const int mu = j >> 1, bc = j & 1;
    const HopNeighbours h = hop_neighbours(mu, xc, y, z, t, X0, Y, Z, T, a.tsign_fwd, a.tsign_bwd);
    // the neighbour that F comes from (forward for A, backward for B) and the one that y comes from (the opposite)
    const int dF = bc, dQ = 1 - bc;
    const int idxFn = bc ? h.idxB : h.idxF, idxQn = bc ? h.idxF : h.idxB, face = h.face;
    const bool crossFn = bc ? h.crossB : h.crossF, crossQn = bc ? h.crossF : h.crossB;
    const int fcb = a.faceCB[mu];
    double U[18];
    // first pass over the columns: C[y, U F(x +- mu)]
    Link<double, R>::load(U, a.gauge[parity] + (size_t)(2 * mu + dF) * a.link_bytes, a.g_stride, idx, bc ? h.signB : h.signF);
#pragma unroll 1
    for (int col = 0; col < NCOL; col++) {
      const double *gF = ghost_zone(a, mu, NCOL + col, parity, dF);
      load_site(psi, a.F[col][op], a.sp_stride, idxFn, gF, fcb, face, crossFn);
#pragma unroll
      for (int sp = 0; sp < 4; sp++) su3_mv(v + 6 * sp, U, psi + 6 * sp);
      Planar<double, 24>::load(psi, a.y[col][parity], a.sp_stride, idx, nullptr, idx);
      accumulate(acc, psi, v);
    }
    // second pass: C[U y(x -+ mu), F]
    Link<double, R>::load(U, a.gauge[parity] + (size_t)(2 * mu + dQ) * a.link_bytes, a.g_stride, idx, bc ? h.signF : h.signB);
#pragma unroll 1
    for (int col = 0; col < NCOL; col++) {
      const double *gQ = ghost_zone(a, mu, col, parity, dQ);
      load_site(psi, a.y[col][op], a.sp_stride, idxQn, gQ, fcb, face, crossQn);
#pragma unroll
      for (int sp = 0; sp < 4; sp++) su3_mv(v + 6 * sp, U, psi + 6 * sp);
      Planar<double, 24>::load(psi, a.F[col][parity], a.sp_stride, idx, nullptr, idx);
      accumulate(acc, v, psi);
    }
  }
  const int blk = j == 8 ? 0 : 1 + 4 * (j & 1) + (j >> 1);
  double2 *o = a.cs + ((long)blk * a.S + s) * NGM;
#pragma unroll
  for (int k = 0; k < NGM; k++) o[k] = make_double2(acc[2 * k], acc[2 * k + 1]);
}

// ================================ host: spin tables ================================
static M4 operatorMatrix(int i, int s) {
  const cd I(0, 1), sg((double)s, 0);
  const M4 g5 = gammaU(5);
  if (i == 0) return (sg * I) * g5;
  if (i <= 4) return gammaU(i);
  if (i == 5) return (sg * I) * mid4();
  if (i <= 9) return g5 * gammaU(i - 5);
  const int pair[6][2] = {{1, 2}, {1, 3}, {2, 3}, {4, 1}, {4, 2}, {4, 3}};
  return sg * (g5 * gammaU(pair[i - 10][0]) * gammaU(pair[i - 10][1]));
}

// G_tm = R_p G R_p for the projector pid (enum WHICHPROJECTOR) and the particle (enum WHICHPARTICLE)
static M4 projectorMatrix(int pid, int particle) {
  const cd I(0, 1);
  const M4 one = mid4(), g5 = gammaU(5), P4 = cd(0.25, 0) * (one + gammaU(4));
  auto G5Gk = [&](int k) { return P4 * (I * (g5 * gammaU(k))); };
  M4 G;
  if (pid == G4) G = P4;
  else if (pid == G5G123) G = G5Gk(1) + G5Gk(2) + G5Gk(3);
  else G = G5Gk(pid - G5G1 + 1);
  const double p = particle == PROTON ? 1.0 : -1.0;
  const M4 R = cd(1.0 / sqrt(2.0), 0) * (one + (cd(0, p)) * g5);
  return R * G * R;
}

static void checkParam(const QudaAmdThreepParam *p, const char *fname) {
  const LatticeGeom &g = residentGeom();
  const CommGrid &cg = commGrid();
  for (int d = 0; d < 4; d++)
    if (p->sourcePosition[d] < 0 || p->sourcePosition[d] >= g.X[d] * cg.dims[d]) errorQuda("%s: source position %d out of range in dimension %d", fname, p->sourcePosition[d], d);
  if (p->tsinkSource < 0 || p->tsinkSource >= g.X[3] * cg.dims[3]) errorQuda("%s: tsinkSource = %d", fname, p->tsinkSource);
  if (p->projector < G4 || p->projector > G5G3) errorQuda("%s: projector = %d", fname, p->projector);
  if (p->particle != PROTON && p->particle != NEUTRON) errorQuda("%s: particle = %d (proton and neutron only)", fname, p->particle);
  if (p->part != 1 && p->part != 2) errorQuda("%s: part = %d", fname, p->part);
  if (p->Q_sq < 0 || p->nsmearGauss < 0) errorQuda("%s: Q_sq = %d, nsmearGauss = %d", fname, p->Q_sq, p->nsmearGauss);
}

static double g_threepSecs[4] = {0, 0, 0, 0};   // source construction, ghost exchange, stencil, projection

}  // namespace threep

// +1 where the operator is inserted on the up quark, -1 on the down quark
int threepInsertedFlavor(int particle, int part) { return (particle == PROTON) == (part == 1) ? +1 : -1; }

// out = scale x in with the spin basis changed (BASIS_* of basis.h), full fp64 device fields
__global__ void __launch_bounds__(256) basis_copy_kernel(double *out, const double *in, int stride, size_t parityDoubles, int Vh, int change, double scale) {
  const int idx = blockIdx.x * blockDim.x + threadIdx.x, parity = blockIdx.y;
  if (idx >= Vh) return;
  double r[24], q[24];
  Planar<double, 24>::load(r, in + parity * parityDoubles, stride, idx, nullptr, idx);
  rotate_basis(q, r, change);
#pragma unroll
  for (int k = 0; k < 24; k++) q[k] *= scale;
  Planar<double, 24>::store(q, out + parity * parityDoubles, stride, idx, nullptr, idx);
}

// ukqcd = scale x (the device-basis field dev) in the UKQCD basis, as the contraction reads its columns
void threepToUkqcd(ColorSpinorField &ukqcd, const ColorSpinorField &dev, double scale) {
  const LatticeGeom &g = residentGeom();
  if (ukqcd.Stride() != dev.Stride() || parityDoubles(ukqcd) != parityDoubles(dev)) errorQuda("threep: field layouts differ");
  hipLaunchKernelGGL(basis_copy_kernel, dim3((g.Vh + 255) / 256, 2), dim3(256), 0, computeStream(), (double *)ukqcd.V(), (const double *)dev.V(), dev.Stride(), parityDoubles(dev), g.Vh,
                     BASIS_DR_TO_UKQCD, scale);
  HIP_CHECK(hipGetLastError());
}

// The twelve sequential sources as they go to the solver, src[12] full fp64 device fields in the device basis, from the sink-smeared,
// unrotated propagators in props (flavour 0 up, 1 down).  A rank that does not own the sink slice contributes zeros.
void threepSeqSourceDevice(ColorSpinorField *const src[12], TwopProps &props, const GaugeField *Uape, const QudaAmdThreepParam *p) {
  using namespace threep;
  const LatticeGeom &g = residentGeom();
  const CommGrid &cg = commGrid();
  hipStream_t st = computeStream();
  const size_t vec = (size_t)g.V * 24;
  const int Lt = g.X[3], T = Lt * cg.dims[3], Vs = g.X[0] * g.X[1] * g.X[2];
  const int tg = (p->tsinkSource + p->sourcePosition[3]) % T;
  // the smearing below is collective over the spatial ranks, so every rank goes on; one that does not own the sink slice starts from zero
  double *d_seq = nullptr;
  if (tg / Lt == cg.coords[3]) {
    HIP_CHECK(hipMalloc(&d_seq, NCOL * vec * sizeof(double)));
    HIP_CHECK(hipMemsetAsync(d_seq, 0, NCOL * vec * sizeof(double), st));
    SeqArg a;
    const M4 Cg5 = gammaU(4) * gammaU(2) * gammaU(5), G = projectorMatrix(p->projector, p->particle);
    toSPerm(Cg5, a.acol, a.aval);
    for (int i = 0; i < 4; i++)
      for (int c = 0; c < 4; c++) a.G[i][c] = make_double2(G.a[i][c].real(), G.a[i][c].imag());
    a.part = p->part;
    const int twice = p->particle == PROTON ? 0 : 1;   // the flavour in slots 0 and 2
    hipLaunchKernelGGL(seq_source_kernel, dim3((Vs + 63) / 64, NCOL), dim3(64), 0, st, d_seq, twopPropsData(props, twice), twopPropsData(props, 1 - twice), (long)g.V, Vs, tg % Lt, a);
    HIP_CHECK(hipGetLastError());
  }
  for (int col = 0; col < NCOL; col++) {
    if (d_seq) deviceLexToField(*src[col], d_seq + col * vec, g, true);   // synchronises
    else blas::zero(*src[col]);
    if (Uape && p->nsmearGauss > 0) gaussianSmear(*src[col], *Uape, p->alphaGauss, p->nsmearGauss);
  }
  HIP_CHECK(hipStreamSynchronize(st));
  if (d_seq) (void)hipFree(d_seq);
}

// h_out[12][V * 24] from the unsmeared host propagators h_up / h_dn [12][V * 24] (lexicographic UKQCD)
void threepSeqSource(double *h_out, const double *h_up, const double *h_dn, const GaugeField *Uape, const QudaAmdThreepParam *p) {
  using namespace threep;
  const LatticeGeom &g = residentGeom();
  hipStream_t st = computeStream();
  hipEvent_t ev[2];
  for (int i = 0; i < 2; i++) HIP_CHECK(hipEventCreate(&ev[i]));
  HIP_CHECK(hipEventRecord(ev[0], st));
  const size_t vec = (size_t)g.V * 24;
  ColorSpinorParam cp = deviceSpinorParam(QUDA_DOUBLE_PRECISION, QUDA_FULL_SITE_SUBSET, QUDA_TWIST_NO);
  cp.create = QUDA_ZERO_FIELD_CREATE;
  ColorSpinorField *src[NCOL];
  for (int c = 0; c < NCOL; c++) src[c] = new ColorSpinorField(cp);
  TwopProps *props = twopPropsCreate(g);
  for (int fl = 0; fl < 2; fl++)
    for (int isc = 0; isc < NCOL; isc++) {
      lexToDevice(*src[0], (fl ? h_dn : h_up) + isc * vec, g, false);   // smearing acts on colour: the basis stays UKQCD
      twopAbsorbColumn(*props, fl, isc, *src[0], g, Uape, p->nsmearGauss, p->alphaGauss, false, 1.0);
    }
  threepSeqSourceDevice(src, *props, Uape, p);
  twopPropsDestroy(props);
  for (int c = 0; c < NCOL; c++) { deviceToLex(h_out + c * vec, *src[c], g, true, 1.0); delete src[c]; }
  HIP_CHECK(hipEventRecord(ev[1], st));
  HIP_CHECK(hipStreamSynchronize(st));
  g_threepSecs[0] = elapsedSecs(ev[0], ev[1]);
  for (int i = 0; i < 2; i++) (void)hipEventDestroy(ev[i]);
}

// y[12], F[12]: full fp64 device fields holding the columns in the UKQCD basis.  Outputs (host, any may be NULL): local [T][Nm][16],
// noether [T][Nm][4], oneD [T][Nm][4][16] complex, source-relative time.  Collective.
void threepContract(double *h_local, double *h_noether, double *h_oneD, ColorSpinorField *const y[12], ColorSpinorField *const F[12], const GaugeField &U,
                    const QudaAmdThreepParam *p) {
  using namespace threep;
  if (U.precision != QUDA_DOUBLE_PRECISION) errorQuda("threep contraction: the links must be fp64 (cuda_prec of the gauge field)");
  const LatticeGeom &g = residentGeom();
  const CommGrid &cg = commGrid();
  hipStream_t st = computeStream();
  hipEvent_t ev[2];
  for (int i = 0; i < 2; i++) HIP_CHECK(hipEventCreate(&ev[i]));

  ThreepArg arg;
  memset(&arg, 0, sizeof(arg));
  arg.sp_stride = y[0]->Stride();
  std::vector<const ColorSpinorField *> fields(2 * NCOL);
  for (int c = 0; c < NCOL; c++) {
    if (y[c]->Stride() != arg.sp_stride || F[c]->Stride() != arg.sp_stride) errorQuda("threep contraction: stride mismatch");
    arg.y[c][0] = (const double *)y[c]->Even().V(); arg.y[c][1] = (const double *)y[c]->Odd().V();
    arg.F[c][0] = (const double *)F[c]->Even().V(); arg.F[c][1] = (const double *)F[c]->Odd().V();
    fields[c] = y[c]; fields[NCOL + c] = F[c];
  }
  fillStencilGeom(arg, U, g, cg);
  HIP_CHECK(hipEventRecord(ev[0], st));
  GhostZones ghosts(arg, fields, g, cg);   // column by column
  HIP_CHECK(hipEventRecord(ev[1], st));

  // the '+' phase of the three-point functions: the shared projection with the negated momenta
  std::vector<int> moms = twopMomenta(p->Q_sq);
  for (int &n : moms) n = -n;
  MomAccum A(NBLK, std::move(moms));
  const int Nm = A.Nm, Vs = g.X[0] * g.X[1] * g.X[2], T = g.X[3] * cg.dims[3];
  const size_t per = A.per();
  int gx[3];
  for (int d = 0; d < 3; d++) gx[d] = cg.coords[d] * g.X[d] - p->sourcePosition[d];
  stageAndProject(A, gx, 0, [&](int t0, int nt, double2 *cs) {
    arg.t0 = t0; arg.S = (long)nt * Vs; arg.cs = cs;
    launchByRecon((int)U.reconstruct, threep_stencil_kernel<18>, threep_stencil_kernel<12>, threep_stencil_kernel<8>, dim3((unsigned)((arg.S / 2 + 127) / 128) * 9, 2), dim3(128), arg);
  }, g_threepSecs + 2);
  std::vector<double> glob((size_t)NBLK * T * per);
  A.get(glob.data());
  p2pCheck("threepContract");
  g_threepSecs[1] = elapsedSecs(ev[0], ev[1]);
  for (int i = 0; i < 2; i++) (void)hipEventDestroy(ev[i]);

  // operators, currents, the factor 1/4, source-relative time and the wrap sign on the projected matrices
  const int s = threepInsertedFlavor(p->particle, p->part);
  M4 O[16], Pp[4], Pm[4];
  for (int i = 0; i < 16; i++) O[i] = operatorMatrix(i, s);
  for (int mu = 0; mu < 4; mu++) { Pp[mu] = mid4() + gammaU(mu + 1); Pm[mu] = mid4() + cd(-1, 0) * gammaU(mu + 1); }
  const int t0s = p->sourcePosition[3];
  const double wrap = p->tsinkSource + t0s >= T ? -1.0 : 1.0;
  auto blk = [&](int k, int ts, int m) { return (const cd *)&glob[((size_t)k * T + ts) * per + (size_t)m * 32]; };
  auto trace = [](const M4 &o, const cd *a, const cd *b, double wb) {   // sum o[k][l] (a + wb b)[k][l]
    cd r = 0;
    for (int k = 0; k < 4; k++)
      for (int l = 0; l < 4; l++) r += o.a[k][l] * (b ? a[4 * k + l] + wb * b[4 * k + l] : a[4 * k + l]);
    return r;
  };
  for (int it = 0; it < T; it++) {
    const int ts = (it + t0s) % T;
    for (int m = 0; m < Nm; m++) {
      const size_t tm = (size_t)it * Nm + m;
      if (h_local)
        for (int i = 0; i < 16; i++) {
          const cd r = wrap * trace(O[i], blk(0, ts, m), nullptr, 0);
          h_local[(tm * 16 + i) * 2] = r.real(); h_local[(tm * 16 + i) * 2 + 1] = r.imag();
        }
      for (int mu = 0; mu < 4; mu++) {
        const cd *AD = blk(1 + mu, ts, m), *BC = blk(5 + mu, ts, m);
        if (h_noether) {
          const cd r = 0.25 * wrap * (trace(Pp[mu], BC, nullptr, 0) - trace(Pm[mu], AD, nullptr, 0));
          h_noether[(tm * 4 + mu) * 2] = r.real(); h_noether[(tm * 4 + mu) * 2 + 1] = r.imag();
        }
        if (h_oneD)
          for (int i = 0; i < 16; i++) {
            const cd r = 0.25 * wrap * trace(O[i], AD, BC, -1.0);
            h_oneD[((tm * 4 + mu) * 16 + i) * 2] = r.real(); h_oneD[((tm * 4 + mu) * 16 + i) * 2 + 1] = r.imag();
          }
      }
    }
  }
}

// writeThrp_ASCII: the three files of one (sink separation, projector, part); rank 0 writes.  The arrays are already in source-relative
// time and carry the wrap sign.
void threepWriteAscii(const char *filename_out, const QudaAmdThreepParam *p, int T, const double *h_local, const double *h_noether, const double *h_oneD) {
  if (commGrid().rank != 0) return;
  const std::vector<int> moms = twopMomenta(p->Q_sq);
  const int Nm = (int)moms.size() / 3;
  const char *particle = p->particle == PROTON ? "proton" : "neutron", *flavor = threepInsertedFlavor(p->particle, p->part) > 0 ? "up" : "down";
  const char *type[3] = {"ultra_local", "noether", "oneD"};
  FILE *f[3];
  for (int k = 0; k < 3; k++) {
    char name[4096];
    snprintf(name, sizeof(name), "%s.%s.%s.%s.SS.%02d.%02d.%02d.%02d.dat", filename_out, particle, flavor, type[k], p->sourcePosition[0], p->sourcePosition[1],
             p->sourcePosition[2], p->sourcePosition[3]);
    f[k] = fopen(name, "w");
    if (!f[k]) errorQuda("threep: cannot open %s for writing", name);
  }
  for (int iop = 0; iop < 16; iop++)
    for (int it = 0; it < T; it++)
      for (int m = 0; m < Nm; m++) {
        const double *v = h_local + (((size_t)it * Nm + m) * 16 + iop) * 2;
        fprintf(f[0], "%d \t %d \t %+d %+d %+d \t %+e %+e\n", iop, it, moms[3 * m], moms[3 * m + 1], moms[3 * m + 2], v[0], v[1]);
      }
  for (int dir = 0; dir < 4; dir++)
    for (int it = 0; it < T; it++)
      for (int m = 0; m < Nm; m++) {
        const double *v = h_noether + (((size_t)it * Nm + m) * 4 + dir) * 2;
        fprintf(f[1], "%d \t %d \t %+d %+d %+d \t %+e %+e\n", dir, it, moms[3 * m], moms[3 * m + 1], moms[3 * m + 2], v[0], v[1]);
      }
  for (int iop = 0; iop < 16; iop++)
    for (int dir = 0; dir < 4; dir++)
      for (int it = 0; it < T; it++)
        for (int m = 0; m < Nm; m++) {
          const double *v = h_oneD + ((((size_t)it * Nm + m) * 4 + dir) * 16 + iop) * 2;
          fprintf(f[2], "%d \t %d \t %d \t %+d %+d %+d \t %+e %+e\n", iop, dir, it, moms[3 * m], moms[3 * m + 1], moms[3 * m + 2], v[0], v[1]);
        }
  for (int k = 0; k < 3; k++) fclose(f[k]);
}

static bool g_threepOutput = false;
bool threepOutputEnabled() { return g_threepOutput; }

}  // namespace quda

using namespace quda;

extern "C" {

static void storeMatrix(const gammah::M4 &m, double out[32]) {
  for (int r = 0; r < 4; r++)
    for (int c = 0; c < 4; c++) { out[2 * (4 * r + c)] = m.a[r][c].real(); out[2 * (4 * r + c) + 1] = m.a[r][c].imag(); }
}

void qudaAmdThreepOperator(int i, int s, double out[32]) {
  if (i < 0 || i > 15 || (s != 1 && s != -1) || !out) errorQuda("qudaAmdThreepOperator: i = %d, s = %d", i, s);
  storeMatrix(threep::operatorMatrix(i, s), out);
}

void qudaAmdThreepProjector(int pid, int particle, double out[32]) {
  if (pid < G4 || pid > G5G3 || (particle != PROTON && particle != NEUTRON) || !out) errorQuda("qudaAmdThreepProjector: projector = %d, particle = %d", pid, particle);
  storeMatrix(threep::projectorMatrix(pid, particle), out);
}

void qudaAmdSetThreepOutput(int enable) { g_threepOutput = enable != 0; }

void qudaAmdThreepLastTimings(double secs[4]) {
  for (int i = 0; i < 4; i++) secs[i] = threep::g_threepSecs[i];
}

void qudaAmdThreepSeqSource(void *h_out, const void *h_prop_up, const void *h_prop_dn, void **gauge_APE, const QudaAmdThreepParam *p) {
  if (!gaugePrecise) errorQuda("qudaAmdThreepSeqSource: Gauge field not allocated");
  if (!p || !h_out || !h_prop_up || !h_prop_dn) errorQuda("qudaAmdThreepSeqSource: NULL argument");
  threep::checkParam(p, "qudaAmdThreepSeqSource");
  const LatticeGeom &g = residentGeom();
  if (p->nsmearGauss > 0 && !gauge_APE && !gaugeSmeared) errorQuda("qudaAmdThreepSeqSource: gauge_APE is NULL and no smeared field is resident (performAPEnStep)");
  GaugeField *U = p->nsmearGauss > 0 ? (gauge_APE ? loadLexGauge(gauge_APE, g) : gaugeSmeared) : nullptr;
  threepSeqSource((double *)h_out, (const double *)h_prop_up, (const double *)h_prop_dn, U, p);
  if (U && gauge_APE) delete U;
}

void qudaAmdContractThreep(double *h_local, double *h_noether, double *h_oneD, const void *h_seq, const void *h_fwd, void **gauge, const QudaAmdThreepParam *p) {
  if (!gaugePrecise) errorQuda("qudaAmdContractThreep: Gauge field not allocated");
  if (!p || !h_seq || !h_fwd) errorQuda("qudaAmdContractThreep: NULL argument");
  threep::checkParam(p, "qudaAmdContractThreep");
  const LatticeGeom &g = residentGeom();
  GaugeField *U = gauge ? loadLexGauge(gauge, g) : gaugePrecise;
  {
    ColorSpinorParam cp = deviceSpinorParam(QUDA_DOUBLE_PRECISION, QUDA_FULL_SITE_SUBSET, QUDA_TWIST_NO);
    cp.create = QUDA_ZERO_FIELD_CREATE;
    ColorSpinorField *y[12], *F[12];
    const size_t vec = (size_t)g.V * 24;
    for (int c = 0; c < 12; c++) {
      y[c] = new ColorSpinorField(cp); F[c] = new ColorSpinorField(cp);
      lexToDevice(*y[c], (const double *)h_seq + c * vec, g, false);   // the links act on colour: the basis stays UKQCD
      lexToDevice(*F[c], (const double *)h_fwd + c * vec, g, false);
    }
    threepContract(h_local, h_noether, h_oneD, y, F, *U, p);
    for (int c = 0; c < 12; c++) { delete y[c]; delete F[c]; }
  }
  if (gauge) delete U;
}

}  // extern "C"
