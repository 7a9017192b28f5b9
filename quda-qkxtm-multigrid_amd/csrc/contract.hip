// contract.hip — two-point correlators of the QKXTM drivers on the device: rotation of the propagators to the physical (twisted)
// basis, meson and baryon contractions site by site into the staged blocks that the shared momentum projection reads (momproj.hip,
// which also sums over the ranks) and the reference's ASCII writers.
//
// Reference: calcMG_threepTwop_EvenOdd (lib/interface_quda.cpp:6960-7030), rotateToPhysicalBase_core_Kepler.h,
// contractMesons_core_Kepler.h, contractBaryons_core_Kepler.h, writeTwop{Mesons,Baryons}_ASCII
// (lib/qudaQKXTM_Contraction_Kepler.cpp:849-905, :1563-1590), the momentum list createMomenta (lib/qudaQKXTM_Kepler_kernels.cu:96-114).
//
// Propagator layout on the device: P[flavour][(mu*4 + nu)*9 + a*3 + b][site] complex, mu / a the sink spin / colour, nu / b those
// of the source, site lexicographic in the LOCAL lattice; UKQCD spin basis, as the reference contracts them.
//
// The spin tensors are built here from explicit gamma matrices of the UKQCD basis (g4 = diag(1, 1, -1, -1), g5 = [[0, 1], [1, 0]]
// in 2x2 blocks, gk = [[0, i sk], [-i sk, 0]] so that g1 g2 g3 g4 = g5; C = g4 g2).  Every matrix that occurs is a signed
// permutation with entries in {+-1, +-i}, which is what the kernels use:
//  * meson channel G = g5 Gamma for Gamma = g5, 1, g5g1 .. g5g4, g1 .. g4:   c = Tr[P G P^+ G] = sum P_ab G_bc conj(P_dc) G_da;
//  * baryon channels: sum over eps_abc eps_a'b'c' and the spins of the two diquark quarks,
//      sum A_{alpha beta} B_{beta' alpha'} x (the Wick contractions of the three quarks, open spins gamma / gamma'),
//    B = M^T for the source diquark matrix M_{alpha' beta'}: nucleon (A, M) = (Cg5, Cg5), nucleon-Roper (Cg5, C) then x g5 on the
//    right, Roper-nucleon (C, Cg5) g5 on the left, Roper-Roper (C, C) g5 on both sides; Delta (A, M) = (Cgk, g4 (Cgk)^+ g4), all
//    six contractions of three equal quarks
//    (deltapp_deltamm_kk) or the eight of the (1/3)-weighted uud combination (deltap_deltaz_kk).
//  * Each Wick contraction is either a TRACE term (the open spins on one propagator: s = sum D_xy Q_xy, times P_gamma gamma') or a
//    CHAIN term (Y D^T Z)_gamma gamma' with the colour-contracted diquark D_xy = A~_xu P_uv B~_vy built first (host: termFor).
#include <cmath>
#include <complex>
#include <cstdio>
#include <cstring>
#include <vector>

#include "basis.h"
#include "contract_stencil.h"
#include "device_io.h"
#include "gamma_host.h"
#include "interface_internal.h"
#include "lex_index.h"
#include "qa_core.h"
#include "qkxtm_internal.h"
#include "quda_amd_ext.h"
#include "comm_quda.h"

namespace quda {

namespace twop {

constexpr int NMES = 10, NBAR = 10;
// staged blocks of 16 complex values per site: block fl holds the 10 meson channels of flavour fl (entries 10..15 zero), block
// 2 + fl * 10 + ch the open spins [4][4] of baryon channel ch
constexpr int NBLK = 2 + 2 * NBAR;
constexpr int MAX_TERMS = 64;

struct SPerm { int col[4]; double2 val[4]; };    // row r holds val[r] in column col[r]
struct Term {
  double w;
  int chain;          // 0: trace term, 1: chain term
  int pi[3];          // sink slot (alpha, beta, gamma) -> source slot (alpha', beta', gamma')
  int f[3];           // 0: first quark of the flavour assignment (u for the proton), 1: second (d)
  int sm, sp;         // sink slot of the diquark propagator, of the partner (trace) / right (chain) propagator
  int acol[4];        // A~_{x u}: u = acol[x]
  double2 aval[4];
  int brow[4];        // B~_{v y}: v = brow[y]
  double2 bval[4];
};
struct Channel { int first, n, g5L, g5R; };

__constant__ SPerm c_mes[NMES];
__constant__ Term c_terms[MAX_TERMS];
__constant__ Channel c_chan[NBAR];

__device__ __forceinline__ double2 cmulc(double2 a, double2 b) { return make_double2(a.x * b.x + a.y * b.y, a.y * b.x - a.x * b.y); }   // a conj(b)
__device__ __forceinline__ double2 cadd(double2 a, double2 b) { return make_double2(a.x + b.x, a.y + b.y); }
__device__ __forceinline__ double2 cscale(double s, double2 a) { return make_double2(s * a.x, s * a.y); }

// ---- (1 + s i g5) / sqrt2 on both spin indices, in place: P' = R P R, g5 couples spin mu with mu ^ 2 ----
__global__ void __launch_bounds__(256) rotate_kernel(double2 *P, long V, double sign) {
  const long site = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (site >= V) return;
  for (int ab = 0; ab < 9; ab++) {
    double2 p[4][4], q[4][4];
#pragma unroll
    for (int m = 0; m < 4; m++)
#pragma unroll
      for (int n = 0; n < 4; n++) p[m][n] = P[((m * 4 + n) * 9 + ab) * V + site];
#pragma unroll
    for (int m = 0; m < 4; m++)
#pragma unroll
      for (int n = 0; n < 4; n++) {
        const double2 x = cadd(p[m ^ 2][n], p[m][n ^ 2]);   // times s i
        const double2 y = p[m ^ 2][n ^ 2];                    // times (s i)^2 = -1
        q[m][n] = make_double2(0.5 * (p[m][n].x - sign * x.y - y.x), 0.5 * (p[m][n].y + sign * x.x - y.y));
      }
#pragma unroll
    for (int m = 0; m < 4; m++)
#pragma unroll
      for (int n = 0; n < 4; n++) P[((m * 4 + n) * 9 + ab) * V + site] = q[m][n];
  }
}

// ---- one column (source spin nu, colour b) from a full fp64 device spinor (even-odd, planar) ----

__global__ void __launch_bounds__(256) field_to_prop_kernel(double2 *P, long V, const double *dev, int stride, size_t parityDoubles, int Vh, int Xh, int Y, int Z,
                                                            int change, double scale, int nu, int b) {
  const int idx = blockIdx.x * blockDim.x + threadIdx.x, parity = blockIdx.y;
  if (idx >= Vh) return;
  double r[24], q[24];
  Planar<double, 24>::load(r, dev + parity * parityDoubles, stride, idx, nullptr, idx);
  if (change) rotate_basis(q, r, change);
  const double *s = change ? q : r;
  const long site = lex_of(idx, parity, Xh, Y, Z);
#pragma unroll
  for (int mu = 0; mu < 4; mu++)
#pragma unroll
    for (int a = 0; a < 3; a++) P[((mu * 4 + nu) * 9 + a * 3 + b) * V + site] = make_double2(scale * s[(mu * 3 + a) * 2], scale * s[(mu * 3 + a) * 2 + 1]);
}

// ---- mesons: out[flavour][s][channel], sites of one time slice ----
__global__ void __launch_bounds__(128) meson_kernel(double2 *out, const double2 *P0, const double2 *P1, long V, int Vs, int t) {
  const int s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= Vs) return;
  const long site = (long)t * Vs + s;
  for (int fl = 0; fl < 2; fl++) {
    const double2 *P = fl ? P1 : P0;
    for (int ch = 0; ch < NMES; ch++) {
      const SPerm &G = c_mes[ch];
      double2 acc = make_double2(0, 0);
      for (int be = 0; be < 4; be++)
        for (int de = 0; de < 4; de++) {
          const double2 gg = cmul(G.val[be], G.val[de]);
          double2 sum = make_double2(0, 0);
#pragma unroll
          for (int ab = 0; ab < 9; ab++) sum = cadd(sum, cmulc(P[((G.col[de] * 4 + be) * 9 + ab) * V + site], P[((de * 4 + G.col[be]) * 9 + ab) * V + site]));
          acc = cadd(acc, cmul(gg, sum));
        }
      out[((long)fl * Vs + s) * 16 + ch] = acc;
    }
    for (int ch = NMES; ch < 16; ch++) out[((long)fl * Vs + s) * 16 + ch] = make_double2(0, 0);   // nothing uninitialised is projected
  }
}

// ---- baryons: out[2 + flavour * 10 + channel][s][gamma * 4 + gamma'] ----
__global__ void __launch_bounds__(64) baryon_kernel(double2 *out, const double2 *P0, const double2 *P1, long V, int Vs, int t) {
  const int s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= Vs) return;
  const int ch = blockIdx.y, fl = blockIdx.z;
  const long site = (long)t * Vs + s;
  double2 acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; i++)
#pragma unroll
    for (int j = 0; j < 4; j++) acc[i][j] = make_double2(0, 0);
  const Channel C = c_chan[ch];
  for (int it = C.first; it < C.first + C.n; it++) {
    const Term &T = c_terms[it];
    const double2 *Pm = (T.f[T.sm] ^ fl) ? P1 : P0;
    const double2 *Pp = (T.f[T.sp] ^ fl) ? P1 : P0;
    const double2 *Po = (T.f[2] ^ fl) ? P1 : P0;
    for (int e1 = 0; e1 < 6; e1++)
      for (int e2 = 0; e2 < 6; e2++) {
        const double w = T.w * c_eps_sign[e1] * c_eps_sign[e2];
        int csrc[3];
        csrc[0] = c_eps[e2][0]; csrc[1] = c_eps[e2][1]; csrc[2] = c_eps[e2][2];
        const int cm = c_eps[e1][T.sm], cmp = csrc[T.pi[T.sm]];
        const int cp = c_eps[e1][T.sp], cpp = csrc[T.pi[T.sp]];
        const int co = c_eps[e1][2], cop = csrc[T.pi[2]];
        double2 D[4][4];   // colour-fixed diquark D_xy = A~_{x u} P_{u v} B~_{v y}
#pragma unroll
        for (int x = 0; x < 4; x++)
#pragma unroll
          for (int y = 0; y < 4; y++) D[x][y] = cmul(cmul(T.aval[x], T.bval[y]), Pm[prop_index(T.acol[x], T.brow[y], cm, cmp, V, site)]);
        if (!T.chain) {
          // the open spins on one propagator: sum_xy D_xy Q_xy times P_{gamma gamma'}
          double2 sc = make_double2(0, 0);
#pragma unroll
          for (int x = 0; x < 4; x++)
#pragma unroll
            for (int y = 0; y < 4; y++) sc = cadd(sc, cmul(D[x][y], Pp[prop_index(x, y, cp, cpp, V, site)]));
          sc = cscale(w, sc);
#pragma unroll
          for (int g = 0; g < 4; g++)
#pragma unroll
            for (int gp = 0; gp < 4; gp++) acc[g][gp] = cadd(acc[g][gp], cmul(sc, Po[prop_index(g, gp, co, cop, V, site)]));
        } else {
          // (Y D^T Z)_{gamma gamma'}: Y = P_{gamma y} of the sink gamma quark, Z = P_{x gamma'} of the quark that reaches gamma'
          double2 E[4][4];   // E_{y gp} = sum_x D_xy Z_{x gp}
#pragma unroll
          for (int y = 0; y < 4; y++)
#pragma unroll
            for (int gp = 0; gp < 4; gp++) {
              double2 e = make_double2(0, 0);
#pragma unroll
              for (int x = 0; x < 4; x++) e = cadd(e, cmul(D[x][y], Pp[prop_index(x, gp, cp, cpp, V, site)]));
              E[y][gp] = e;
            }
#pragma unroll
          for (int g = 0; g < 4; g++) {
            double2 Yg[4];
#pragma unroll
            for (int y = 0; y < 4; y++) Yg[y] = cscale(w, Po[prop_index(g, y, co, cop, V, site)]);
#pragma unroll
            for (int gp = 0; gp < 4; gp++) {
              double2 e = acc[g][gp];
#pragma unroll
              for (int y = 0; y < 4; y++) e = cadd(e, cmul(Yg[y], E[y][gp]));
              acc[g][gp] = e;
            }
          }
        }
      }
  }
  // g5 (UKQCD: spin mu <-> mu ^ 2) on the sink and / or source side of the Roper channels
  double2 *o = out + ((long)(2 + fl * NBAR + ch) * Vs + s) * 16;
#pragma unroll
  for (int g = 0; g < 4; g++)
#pragma unroll
    for (int gp = 0; gp < 4; gp++) {
      const int gg = C.g5L ? (g ^ 2) : g, ggp = C.g5R ? (gp ^ 2) : gp;
      double2 v = acc[0][0];
#pragma unroll
      for (int i = 0; i < 4; i++)
#pragma unroll
        for (int j = 0; j < 4; j++)
          if (i == gg && j == ggp) v = acc[i][j];
      o[g * 4 + gp] = v;
    }
}

// ================================ host: gamma algebra, term lists ================================
using namespace gammah;   // M4, gammaU and the matrix helpers (gamma_host.h)

// one Wick contraction: sink slot s goes to source slot pi[s]; flavours f[s]; A_{alpha beta}, B_{beta' alpha'}
static Term termFor(double w, const int pi[3], const int f[3], const M4 &A, const M4 &B) {
  Term t;
  t.w = w;
  for (int k = 0; k < 3; k++) { t.pi[k] = pi[k]; t.f[k] = f[k]; }
  t.chain = pi[2] != 2;
  // the partner (trace) / right (chain) propagator: the sink slot whose source end is open (chain) or, for a trace, slot 0;
  // the diquark propagator is the other of the two sink slots alpha, beta
  int sp;
  if (t.chain) sp = pi[0] == 2 ? 0 : 1;
  else sp = 0;
  const int sm = 1 - sp;
  t.sm = sm; t.sp = sp;
  // D_xy = A~_{x u} P_{u v} B~_{v y}: x runs over the sink index of slot sp, u over that of slot sm (A or A^T); v over the source index of
  // pi[sm], y over the other source slot of the two diquark slots alpha', beta' (B or B^T)
  const M4 At = sp == 0 ? A : transpose(A);
  const int ysrc = t.chain ? pi[2] : pi[sp];   // source slot on the y side
  const M4 Bt = ysrc == 0 ? B : transpose(B);  // B~_{v y} = B_{beta' alpha'} with y = alpha' (ysrc 0) or y = beta'
  toSPerm(At, t.acol, t.aval);
  int bcol[4]; double2 bv[4];
  toSPerm(transpose(Bt), bcol, bv);           // column y of B~ holds its entry in row brow[y]
  for (int y = 0; y < 4; y++) { t.brow[y] = bcol[y]; t.bval[y] = bv[y]; }
  return t;
}

struct Tables {
  SPerm mes[NMES];
  Term terms[MAX_TERMS];
  Channel chan[NBAR];
  int nterms = 0;
};

static Tables buildTables() {
  Tables T;
  const M4 one = mid4(), g5 = gammaU(5), C = gammaU(4) * gammaU(2);
  // mesons: G = g5 Gamma, Gamma = g5, 1, g5g1, g5g2, g5g3, g5g4, g1, g2, g3, g4
  const M4 Gam[NMES] = {g5, one, g5 * gammaU(1), g5 * gammaU(2), g5 * gammaU(3), g5 * gammaU(4), gammaU(1), gammaU(2), gammaU(3), gammaU(4)};
  for (int ch = 0; ch < NMES; ch++) toSPerm(g5 * Gam[ch], T.mes[ch].col, T.mes[ch].val);

  auto add = [&](double w, std::initializer_list<int> pi, std::initializer_list<int> f, const M4 &A, const M4 &B) {
    int p[3], q[3], k = 0;
    for (int v : pi) p[k++] = v;
    k = 0;
    for (int v : f) q[k++] = v;
    if (T.nterms >= MAX_TERMS) errorQuda("twop: too many terms");
    T.terms[T.nterms++] = termFor(w, p, q, A, B);
  };
  auto nucleon = [&](int ch, const M4 &A, const M4 &B, int g5L, int g5R) {
    T.chan[ch] = {T.nterms, 2, g5L, g5R};
    add(+1, {0, 1, 2}, {0, 1, 0}, A, B);   // u(alpha, alpha') d(beta, beta') u(gamma, gamma')
    add(-1, {2, 1, 0}, {0, 1, 0}, A, B);   // u(alpha, gamma') d(beta, beta') u(gamma, alpha')
  };
  // sink diquark matrix A_{alpha beta}, source diquark matrix M_{alpha' beta'}: B_{beta' alpha'} = M^T
  const M4 Cg5 = C * g5;
  nucleon(0, Cg5, transpose(Cg5), 0, 0);
  nucleon(1, Cg5, transpose(C), 0, 1);
  nucleon(2, C, transpose(Cg5), 1, 0);
  nucleon(3, C, transpose(C), 1, 1);
  const int perms[6][3] = {{0, 1, 2}, {1, 2, 0}, {2, 0, 1}, {0, 2, 1}, {2, 1, 0}, {1, 0, 2}};
  const double psign[6] = {1, 1, 1, -1, -1, -1};
  for (int k = 1; k <= 3; k++) {
    const M4 A = C * gammaU(k), B = transpose(gammaU(4) * dagger(A) * gammaU(4));
    // deltapp / deltamm: three equal quarks, all six contractions with the sign of the permutation
    T.chan[3 + k] = {T.nterms, 6, 0, 0};
    for (int p = 0; p < 6; p++) add(psign[p], {perms[p][0], perms[p][1], perms[p][2]}, {0, 0, 0}, A, B);
    // deltap / deltaz: (1/3) [ 2 (uud + udu) contractions ... ] as the isospin-3/2 projection of the uud interpolator
    T.chan[6 + k] = {T.nterms, 8, 0, 0};
    const double t3 = 1.0 / 3.0;
    add(-4 * t3, {2, 1, 0}, {0, 1, 0}, A, B);
    add(+2 * t3, {1, 2, 0}, {0, 1, 0}, A, B);
    add(+2 * t3, {2, 0, 1}, {0, 0, 1}, A, B);
    add(-2 * t3, {0, 2, 1}, {0, 0, 1}, A, B);
    add(-2 * t3, {0, 2, 1}, {0, 1, 0}, A, B);
    add(-1 * t3, {1, 0, 2}, {0, 0, 1}, A, B);
    add(+1 * t3, {0, 1, 2}, {0, 0, 1}, A, B);
    add(+4 * t3, {0, 1, 2}, {0, 1, 0}, A, B);
  }
  return T;
}

// __constant__ memory is per device: the tables go to every device the process computes on
static void uploadTables() {
  static bool done[64] = {};
  int dev = 0;
  HIP_CHECK(hipGetDevice(&dev));
  if (dev < 0 || dev >= 64) errorQuda("twop: device ordinal %d", dev);
  if (done[dev]) return;
  const Tables T = buildTables();
  HIP_CHECK(hipMemcpyToSymbol(HIP_SYMBOL(c_mes), T.mes, sizeof(T.mes)));
  HIP_CHECK(hipMemcpyToSymbol(HIP_SYMBOL(c_terms), T.terms, sizeof(Term) * T.nterms));
  HIP_CHECK(hipMemcpyToSymbol(HIP_SYMBOL(c_chan), T.chan, sizeof(T.chan)));
  done[dev] = true;
}

}  // namespace twop

// momenta with |n|^2 <= Q_sq: shells iQ = 0 .. Q_sq, inside a shell nx, ny, nz each from +iQ down to -iQ
std::vector<int> twopMomenta(int Q_sq) {
  std::vector<int> m;
  for (int iQ = 0; iQ <= Q_sq; iQ++)
    for (int nx = iQ; nx >= -iQ; nx--)
      for (int ny = iQ; ny >= -iQ; ny--)
        for (int nz = iQ; nz >= -iQ; nz--)
          if (nx * nx + ny * ny + nz * nz == iQ) { m.push_back(nx); m.push_back(ny); m.push_back(nz); }
  return m;
}

// The two propagators of one source on the device, filled column by column
struct TwopProps {
  double2 *P[2] = {nullptr, nullptr};
  long V = 0;
  explicit TwopProps(const LatticeGeom &g) : V(g.V) {
    for (int f = 0; f < 2; f++) {
      HIP_CHECK(hipMalloc(&P[f], (size_t)144 * V * sizeof(double2)));
      HIP_CHECK(hipMemsetAsync(P[f], 0, (size_t)144 * V * sizeof(double2), computeStream()));
    }
  }
  ~TwopProps() { for (int f = 0; f < 2; f++) if (P[f]) (void)hipFree(P[f]); }
  TwopProps(const TwopProps &) = delete;
  TwopProps &operator=(const TwopProps &) = delete;
};

TwopProps *twopPropsCreate(const LatticeGeom &g) { return new TwopProps(g); }
void twopPropsDestroy(TwopProps *p) { delete p; }
double2 *twopPropsData(TwopProps &p, int fl) { return p.P[fl]; }

// column isc = nu * 3 + b of flavour fl from a full fp64 device spinor: sink smearing (colour only, any spin basis), basis change to
// UKQCD if the field is in the device basis, scale
void twopAbsorbColumn(TwopProps &props, int fl, int isc, ColorSpinorField &v, const LatticeGeom &g, const GaugeField *U, int nsmear, double alpha, bool deviceBasis,
                      double scale) {
  if (U && nsmear > 0) gaussianSmear(v, *U, alpha, nsmear);
  hipLaunchKernelGGL(twop::field_to_prop_kernel, dim3((g.Vh + 255) / 256, 2), dim3(256), 0, computeStream(), props.P[fl], props.V, (const double *)v.V(), v.Stride(),
                     parityDoubles(v), g.Vh, g.Xh, g.X[1], g.X[2], deviceBasis ? BASIS_DR_TO_UKQCD : BASIS_NONE, scale, isc / 3, isc % 3);
  HIP_CHECK(hipGetLastError());
}

// rotate, contract, project, sum over ranks, reorder to source-relative time (baryons: sign -1 where t + t0 wraps)
void twopContract(TwopProps &props, const LatticeGeom &g, const int src[4], int Q_sq, double *h_mes, double *h_bar) {
  using namespace twop;
  uploadTables();
  const CommGrid &cg = commGrid();
  const int Vs = g.X[0] * g.X[1] * g.X[2], T = g.X[3] * cg.dims[3];
  const long V = props.V;
  hipStream_t st = computeStream();
  hipLaunchKernelGGL(rotate_kernel, dim3((unsigned)((V + 255) / 256)), dim3(256), 0, st, props.P[0], V, +1.0);
  hipLaunchKernelGGL(rotate_kernel, dim3((unsigned)((V + 255) / 256)), dim3(256), 0, st, props.P[1], V, -1.0);
  HIP_CHECK(hipGetLastError());
  MomAccum A(NBLK, twopMomenta(Q_sq));
  const int Nm = A.Nm;
  const size_t per = A.per();
  // phases relative to the source: the origin of the local lattice minus the source position
  int gx[3];
  for (int d = 0; d < 3; d++) gx[d] = cg.coords[d] * g.X[d] - src[d];
  stageAndProject(A, gx, 1, [&](int t, int, double2 *cs) {   // the kernels take one time slice
    hipLaunchKernelGGL(meson_kernel, dim3((Vs + 127) / 128), dim3(128), 0, st, cs, props.P[0], props.P[1], V, Vs, t);
    hipLaunchKernelGGL(baryon_kernel, dim3((Vs + 63) / 64, NBAR, 2), dim3(64), 0, st, cs, props.P[0], props.P[1], V, Vs, t);
    HIP_CHECK(hipGetLastError());
  }, nullptr);
  std::vector<double> glob((size_t)NBLK * T * per);
  A.get(glob.data());
  for (int it = 0; it < T; it++) {
    const int ts = (it + src[3]) % T;
    const double sign = it + src[3] >= T ? -1.0 : 1.0;
    for (int m = 0; m < Nm; m++)
      for (int fl = 0; fl < 2; fl++) {
        if (h_mes) memcpy(h_mes + (((size_t)it * Nm + m) * 2 + fl) * NMES * 2, &glob[((size_t)fl * T + ts) * per + (size_t)m * 32], NMES * 2 * sizeof(double));
        for (int ch = 0; ch < NBAR && h_bar; ch++) {
          const double *G = &glob[((size_t)(2 + fl * NBAR + ch) * T + ts) * per + (size_t)m * 32];
          double *o = h_bar + ((((size_t)it * Nm + m) * 2 + fl) * NBAR + ch) * 32;
          for (int k = 0; k < 32; k++) o[k] = sign * G[k];
        }
      }
  }
}

// the reference's ASCII files; rank 0 writes.  Channel order: mesons pseudoscalar, scalar, g5g1, g5g2, g5g3, g5g4, g1, g2, g3, g4;
// baryons nucl_nucl, nucl_roper, roper_nucl, roper_roper, deltapp_deltamm_11/22/33, deltap_deltaz_11/22/33
void twopWriteAscii(const char *fname_twop, const int src[4], int Q_sq, int T, const double *h_mes, const double *h_bar) {
  if (commGrid().rank != 0) return;
  const std::vector<int> moms = twopMomenta(Q_sq);
  const int Nm = (int)moms.size() / 3;
  char name[4096];
  snprintf(name, sizeof(name), "%s.mesons.SS.%02d.%02d.%02d.%02d.dat", fname_twop, src[0], src[1], src[2], src[3]);
  FILE *f = fopen(name, "w");
  if (!f) errorQuda("twop: cannot open %s for writing", name);
  for (int ip = 0; ip < twop::NMES; ip++)
    for (int it = 0; it < T; it++)
      for (int m = 0; m < Nm; m++) {
        const double *v = h_mes + ((size_t)it * Nm + m) * 2 * twop::NMES * 2;
        fprintf(f, "%d \t %d \t %+d %+d %+d \t %+e %+e \t %+e %+e\n", ip, it, moms[3 * m], moms[3 * m + 1], moms[3 * m + 2], v[2 * ip], v[2 * ip + 1],
                v[2 * (twop::NMES + ip)], v[2 * (twop::NMES + ip) + 1]);
      }
  fclose(f);
  snprintf(name, sizeof(name), "%s.baryons.SS.%02d.%02d.%02d.%02d.dat", fname_twop, src[0], src[1], src[2], src[3]);
  f = fopen(name, "w");
  if (!f) errorQuda("twop: cannot open %s for writing", name);
  for (int ip = 0; ip < twop::NBAR; ip++)
    for (int it = 0; it < T; it++)
      for (int m = 0; m < Nm; m++)
        for (int g = 0; g < 4; g++)
          for (int gp = 0; gp < 4; gp++) {
            const double *v = h_bar + ((size_t)it * Nm + m) * 2 * twop::NBAR * 16 * 2;
            const size_t k0 = ((size_t)(0 * twop::NBAR + ip) * 16 + g * 4 + gp) * 2, k1 = ((size_t)(1 * twop::NBAR + ip) * 16 + g * 4 + gp) * 2;
            fprintf(f, "%d \t %d \t %+d %+d %+d \t %d %d \t %+e %+e \t %+e %+e\n", ip, it, moms[3 * m], moms[3 * m + 1], moms[3 * m + 2], g, gp, v[k0], v[k0 + 1], v[k1],
                    v[k1 + 1]);
          }
  fclose(f);
}

static bool g_twopOutput = false;
bool twopOutputEnabled() { return g_twopOutput; }

}  // namespace quda

using namespace quda;

extern "C" {

int qudaAmdTwopMomenta(int Q_sq, int *moms, int max_moms) {
  if (Q_sq < 0) errorQuda("qudaAmdTwopMomenta: Q_sq = %d", Q_sq);
  return copyMomenta(twopMomenta(Q_sq), moms, max_moms, "qudaAmdTwopMomenta");
}

int qudaAmdTwopTimeExtent(void) {
  if (!gaugePrecise) errorQuda("qudaAmdTwopTimeExtent: Gauge field not allocated");
  return residentGeom().X[3] * commGrid().dims[3];
}

void qudaAmdSetTwopOutput(int enable) { g_twopOutput = enable != 0; }

void qudaAmdContractTwop(double *h_mesons, double *h_baryons, const void *h_prop_up, const void *h_prop_dn, void **gauge_APE, const QudaAmdTwopParam *p) {
  if (!gaugePrecise) errorQuda("qudaAmdContractTwop: Gauge field not allocated");
  if (!p || !h_prop_up || !h_prop_dn) errorQuda("qudaAmdContractTwop: NULL argument");
  if (p->Q_sq < 0 || p->nsmearGauss < 0) errorQuda("qudaAmdContractTwop: Q_sq = %d, nsmearGauss = %d", p->Q_sq, p->nsmearGauss);
  const LatticeGeom &g = residentGeom();
  const CommGrid &cg = commGrid();
  for (int d = 0; d < 4; d++)
    if (p->sourcePosition[d] < 0 || p->sourcePosition[d] >= g.X[d] * cg.dims[d]) errorQuda("qudaAmdContractTwop: source position %d out of range in dimension %d", p->sourcePosition[d], d);
  if (p->nsmearGauss > 0 && !gauge_APE && !gaugeSmeared) errorQuda("qudaAmdContractTwop: gauge_APE is NULL and no smeared field is resident (performAPEnStep)");
  GaugeField *U = p->nsmearGauss > 0 ? (gauge_APE ? loadLexGauge(gauge_APE, g) : gaugeSmeared) : nullptr;
  {
    TwopProps props(g);
    ColorSpinorParam cp = deviceSpinorParam(QUDA_DOUBLE_PRECISION, QUDA_FULL_SITE_SUBSET, QUDA_TWIST_NO);
    cp.create = QUDA_ZERO_FIELD_CREATE;
    ColorSpinorField v(cp);
    const size_t vec = (size_t)g.V * 24;
    for (int fl = 0; fl < 2; fl++)
      for (int isc = 0; isc < 12; isc++) {
        lexToDevice(v, (const double *)(fl ? h_prop_dn : h_prop_up) + isc * vec, g, false);   // smearing acts on colour: the basis stays UKQCD
        twopAbsorbColumn(props, fl, isc, v, g, U, p->nsmearGauss, p->alphaGauss, false, 1.0);
      }
    twopContract(props, g, p->sourcePosition, p->Q_sq, h_mesons, h_baryons);
  }
  if (U && gauge_APE) delete U;
}

}  // extern "C"
