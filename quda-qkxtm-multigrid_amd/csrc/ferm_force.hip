// ferm_force.hip — the fermion force of molecular dynamics for Wilson, degenerate twisted-mass, doublet and twisted-clover pseudofermions: the outer
// product kernel and the driver that builds its fields from the solutions of an even-odd solve (DESIGN §3 "Fermion force").
//
// Outer product of two full spinor fields, forward neighbours only, projectors placed as in the stencil (forward hop (1 - g_mu) U psi(x+mu)):
//   O_mu[X, Y](x) = tr_spin[(1 - g_mu) X(x + mu) Y^dag(x) + (1 + g_mu) Y(x + mu) X^dag(x)]      a 3x3 colour matrix
//   A_mu(x) <- TA(A_mu(x) - sum_i c_i U_mu(x) O_mu[X_i, Y_i](x))                                 force_epilogue with V = sum_i c_i O_mu
// 1 -+ g_mu = T^dag T with T the two rows spin_project keeps, so each term is the sum over the two half-spinor components h of
// (T X(x + mu))_h (T Y(x))_h^dag: 2 x 9 complex multiply-adds instead of 4 x 9, and no reconstruction.
//
// One thread per (site, parity, direction), a wave per direction and the four directions of 64 sites in one block; all pairs (X_i, Y_i) in
// one launch, so the link and the momentum are read and written once.  A doublet enters as two pairs (its two flavours) with the same coefficient.
// Neighbours of a partitioned direction come from the ghost zones of the contractions (GhostZones / load_site).
#include "contract_stencil.h"
#include "dispatch.h"
#include "dslash_arg.h"
#include "gauge_device.h"

#include "blas.h"
#include "dirac.h"
#include "interface_internal.h"

#include <cstring>

namespace quda {

struct FermForceArg : StencilGeom {
  GaugeView g;
  double *mom;
  int Vh, n;                                                                // n pairs; X_i is field 2 i of the ghost zones, Y_i field 2 i + 1
  const double *x[kFermForceMaxFields][2], *y[kFermForceMaxFields][2];      // parity blocks (even, odd)
  double c[kFermForceMaxFields];
};

// V_ab += c sum_h n[h, a] conj(o[h, b]) for the half spinors n (neighbour) and o (own site), 12 reals each: [h][colour][re, im]
__device__ __forceinline__ void outer_acc(M3 &V, const double *n, const double *o, double c) {
#pragma unroll
  for (int a = 0; a < 3; a++)
#pragma unroll
    for (int b = 0; b < 3; b++) {
      double re = 0, im = 0;
#pragma unroll
      for (int h = 0; h < 2; h++) {
        const double nr = n[6 * h + 2 * a], ni = n[6 * h + 2 * a + 1], orr = o[6 * h + 2 * b], oi = o[6 * h + 2 * b + 1];
        re += nr * orr + ni * oi;
        im += ni * orr - nr * oi;
      }
      V.re[3 * a + b] += c * re; V.im[3 * a + b] += c * im;
    }
}

// V += sum_i c_i O_MU[X_i, Y_i](x).  The pair index is the same in all lanes: pointers and coefficients come through scalar loads
template <int MU> __device__ __forceinline__ void oprod_dir(M3 &V, const FermForceArg &a, int parity, int idx, int xc, int y, int z, int t) {
  const HopNeighbours h = hop_neighbours(MU, xc, y, z, t, a.X0, a.Y, a.Z, a.T, 1.0, 1.0);
  const int op = 1 - parity, fcb = a.faceCB[MU];
  for (int i = 0; i < a.n; i++) {
    const double c = a.c[i];
    double psi[24], hn[12], ho[12];
    // (1 - g_mu) X(x + mu) Y^dag(x)
    Planar<double, 24>::load(psi, a.y[i][parity], a.sp_stride, idx, nullptr, idx);
    spin_project<MU>(ho, psi, 1.0);
    load_site(psi, a.x[i][op], a.sp_stride, h.idxF, ghost_zone(a, MU, 2 * i, parity, 0), fcb, h.face, h.crossF);
    spin_project<MU>(hn, psi, 1.0);
    outer_acc(V, hn, ho, c);
    // (1 + g_mu) Y(x + mu) X^dag(x)
    Planar<double, 24>::load(psi, a.x[i][parity], a.sp_stride, idx, nullptr, idx);
    spin_project<MU>(ho, psi, -1.0);
    load_site(psi, a.y[i][op], a.sp_stride, h.idxF, ghost_zone(a, MU, 2 * i + 1, parity, 0), fcb, h.face, h.crossF);
    spin_project<MU>(hn, psi, -1.0);
    outer_acc(V, hn, ho, c);
  }
}

// a block is 64 sites x 4 directions, one wave per direction: mu is wave-uniform, and the four waves that read X(x), Y(x) of the same 64
// sites and write the four momenta of those sites run on one CU
template <typename T, int R> __global__ void __launch_bounds__(256) ferm_force_kernel(const FermForceArg a) {
  const int gid = blockIdx.x * 64 + (threadIdx.x & 63);
  if (gid >= 2 * a.Vh) return;
  const int mu = threadIdx.x >> 6;
  const int parity = gid >= a.Vh, idx = gid - parity * a.Vh;
  int x[4];
  {
    const int Xh = a.X0 >> 1;
    int l = idx;
    const int xh = l % Xh; l /= Xh;
    x[1] = l % a.Y; l /= a.Y;
    x[2] = l % a.Z; x[3] = l / a.Z;
    x[0] = 2 * xh + ((x[1] + x[2] + x[3] + parity) & 1);
  }
  M3 V;
#pragma unroll
  for (int k = 0; k < 9; k++) V.re[k] = V.im[k] = 0;
  switch (mu) {
    case 0: oprod_dir<0>(V, a, parity, idx, x[0], x[1], x[2], x[3]); break;
    case 1: oprod_dir<1>(V, a, parity, idx, x[0], x[1], x[2], x[3]); break;
    case 2: oprod_dir<2>(V, a, parity, idx, x[0], x[1], x[2], x[3]); break;
    default: oprod_dir<3>(V, a, parity, idx, x[0], x[1], x[2], x[3]); break;
  }
  M3 U;
  load_link<T, R>(U, a.g, mu, x);   // the link as the stencil sees it: the anti-periodic sign stored (18 reals) or through tsign
  force_epilogue(a.mom + ((size_t)gid * 4 + mu) * 10, U, V, 1.0);
}

static double g_kernelSecs = 0;
double fermForceLastKernelSecs() { return g_kernelSecs; }
void fermForceAddKernelSecs(double secs, bool reset) { g_kernelSecs = (reset ? 0 : g_kernelSecs) + secs; }

static void checkForceField(const ColorSpinorField &f, const ColorSpinorField &like, const LatticeGeom &g) {
  if (f.Location() != QUDA_CUDA_FIELD_LOCATION || f.Precision() != QUDA_DOUBLE_PRECISION || f.SiteSubset() != QUDA_FULL_SITE_SUBSET || f.Nspin() != 4 || f.Ncolor() != 3)
    errorQuda("fermion force: expected full fp64 device spinors");
  if (f.Nflavor() != like.Nflavor() || f.Even().Stride() != like.Even().Stride() || f.Even().VolumeCB4() != g.Vh)
    errorQuda("fermion force: the fields differ in flavours, stride or volume (%d flavours, stride %d, %d sites per parity against %d, %d, %d)",
              f.Nflavor(), f.Even().Stride(), f.Even().VolumeCB4(), like.Nflavor(), like.Even().Stride(), g.Vh);
}

void fermionOprodForce(MomField &mom, const GaugeField &U, const std::vector<ColorSpinorField *> &X, const std::vector<ColorSpinorField *> &Y,
                       const std::vector<double> &coeff) {
  if (!(U.geom == mom.geom)) errorQuda("gauge and momentum geometry differ");
  const size_t n = X.size();
  if (Y.size() != n || coeff.size() != n) errorQuda("fermion force: %zu X fields, %zu Y fields, %zu coefficients", n, Y.size(), coeff.size());
  g_kernelSecs = 0;
  if (!n) return;
  const LatticeGeom &geom = U.geom;
  const CommGrid &cg = commGrid();
  for (size_t i = 0; i < n; i++) { checkForceField(*X[i], *X[0], geom); checkForceField(*Y[i], *X[0], geom); }
  const int nf = X[0]->Nflavor(), Vh = geom.Vh, bs = 256, nb = (2 * Vh + 63) / 64;
  const size_t perLaunch = kFermForceMaxFields / nf;
  hipStream_t s = computeStream();
  hipEvent_t ev[2];
  for (int k = 0; k < 2; k++) HIP_CHECK(hipEventCreate(&ev[k]));
  for (size_t first = 0; first < n; first += perLaunch) {
    const size_t last = first + perLaunch < n ? first + perLaunch : n;
    FermForceArg arg;
    memset(&arg, 0, sizeof(arg));
    fillStencilGeom(arg, U, geom, cg);
    arg.g = viewOf(U);
    arg.mom = mom.data;
    arg.Vh = Vh;
    arg.sp_stride = X[0]->Even().Stride();
    std::vector<FullFieldView> views;
    for (size_t i = first; i < last; i++)
      for (int f = 0; f < nf; f++) {   // flavour f of a parity doublet begins f Vh plane entries (double2) into every plane
        const size_t off = (size_t)f * Vh * 2;
        const int k = arg.n++;
        arg.x[k][0] = (const double *)X[i]->Even().V() + off; arg.x[k][1] = (const double *)X[i]->Odd().V() + off;
        arg.y[k][0] = (const double *)Y[i]->Even().V() + off; arg.y[k][1] = (const double *)Y[i]->Odd().V() + off;
        arg.c[k] = coeff[i];
        views.push_back({{arg.x[k][0], arg.x[k][1]}, arg.sp_stride});
        views.push_back({{arg.y[k][0], arg.y[k][1]}, arg.sp_stride});
      }
    GhostZones ghosts(arg, views.data(), views.size(), geom, cg);
    HIP_CHECK(hipEventRecord(ev[0], s));
    forLinkType(U, [&](auto t, auto r) { hipLaunchKernelGGL((ferm_force_kernel<decltype(t), decltype(r)::value>), dim3(nb), dim3(bs), 0, s, arg); });
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipEventRecord(ev[1], s));
    HIP_CHECK(hipStreamSynchronize(s));   // the ghost zones go out of scope
    float ms = 0;
    HIP_CHECK(hipEventElapsedTime(&ms, ev[0], ev[1]));
    g_kernelSecs += 1e-3 * ms;
  }
  for (int k = 0; k < 2; k++) (void)hipEventDestroy(ev[k]);
}

// The fields of the force of phi^dag (Mh^dag Mh)^-1 phi at x = (Mh^dag Mh)^-1 phi on parity p0 (p1 the other), R the site term of the
// operator (1, 1 + i a g5, the flavour twist, or A + i a g5 of twisted clover) and every operator in the kappa normalisation of the Dirac classes:
//   asymmetric  Mh = R - k^2 D R^-1 D       X = (x, R^-1 D x),  y = Mh x,         Y = (y, R^-dag D^dag y)
//   symmetric   Mh = 1 - k^2 R^-1 D R^-1 D   X = (x, R^-1 D x),  y = R^-dag Mh x,  Y = (y, R^-dag D^dag y)
// dS = -d|Mh x|^2 = 2 k^2 sum Re tr(T U O[X, Y]), so F = 2 k^2 TA(U O[X, Y]) and the kernel's coefficient is -dt coeff 2 k^2 s^2 with
// s the factor the mass normalisations put on Mh: 1 / (4 k^2) (mass) or 1 / (2 k) (asymmetric mass), as massRescale does for the solve.
// Twisted clover moves R = A(U) + i a g5 with the links as well: with w = Mh x
//   asymmetric  w^dag d_A Mh x = Y0^dag dA X0 + k^2 Y1^dag dA X1
//   symmetric   w^dag d_A Mh x = Y0^dag dA (X0 - w) + k^2 Y1^dag dA X1            (R0^-1 D R1^-1 D x = (x - w) / k^2)
// and Y^dag dA X = i c sum_f tr(dF_f S_f[X, Y]), so the clover part is the derivative G[T] (clover_force.hip) of the tensor field
// T_f = -2 s^2 i c w_p sum_i dt coeff_i S_f[X'_i, Y_i], w_p = 1 on p0 and k^2 on p1, X' = X with x - w on p0 in the symmetric case:
// one sigma outer product launch (per kFermForceMaxFields solutions) and one derivative launch after the hop kernel.
void tmForce(MomField &mom, const GaugeField &U, double dt, const std::vector<ColorSpinorField *> &x, const std::vector<double> &coeff, QudaInvertParam *inv) {
  const size_t n = x.size();
  if (coeff.size() != n) errorQuda("fermion force: %zu solutions, %zu coefficients", n, coeff.size());
  const bool clover = inv->dslash_type == QUDA_TWISTED_CLOVER_DSLASH;
  const bool twisted = inv->dslash_type == QUDA_TWISTED_MASS_DSLASH;
  const QudaMatPCType mpc = inv->matpc_type;
  const bool asym = mpc == QUDA_MATPC_EVEN_EVEN_ASYMMETRIC || mpc == QUDA_MATPC_ODD_ODD_ASYMMETRIC;
  const bool even = mpc == QUDA_MATPC_EVEN_EVEN || mpc == QUDA_MATPC_EVEN_EVEN_ASYMMETRIC;
  if (!even && mpc != QUDA_MATPC_ODD_ODD && mpc != QUDA_MATPC_ODD_ODD_ASYMMETRIC) errorQuda("fermion force: matpc_type %d undefined", mpc);
  if (!twisted && !clover && asym) errorQuda("fermion force: the Wilson operator has the symmetric matpc types only (matpc_type %d)", mpc);
  DiracParam dp;
  setDiracParam(dp, inv, true);
  dp.dagger = QUDA_DAG_NO;
  Dirac *d = Dirac::create(dp);
  DiracWilson *hop = static_cast<DiracWilson *>(d);                                       // the plain hop D, D^dag
  DiracTwistedMassPC *tm = twisted ? static_cast<DiracTwistedMassPC *>(d) : nullptr;      // R^-1, R^-dag
  DiracTwistedCloverPC *tc = clover ? static_cast<DiracTwistedCloverPC *>(d) : nullptr;
  const QudaParity p0 = even ? QUDA_EVEN_PARITY : QUDA_ODD_PARITY, p1 = even ? QUDA_ODD_PARITY : QUDA_EVEN_PARITY;
  // out = R^-1 in (R^-dag under Dagger(QUDA_DAG_YES)) on parity p
  const auto rinv = [&](ColorSpinorField &out, const ColorSpinorField &in, QudaParity p) {
    if (tm) tm->TwistInv(out, in);
    else if (tc) tc->TwistCloverInv(out, in, p);
    else blas::copy(out, in);
  };

  ColorSpinorParam fp = deviceSpinorParam(QUDA_DOUBLE_PRECISION, QUDA_FULL_SITE_SUBSET, fieldTwistFlavor(*inv));
  fp.create = QUDA_ZERO_FIELD_CREATE;
  std::vector<ColorSpinorField *> X(n), Y(n), XW(n, nullptr);
  std::vector<double> c(n);
  double s = 1.0;
  if (inv->mass_normalization == QUDA_MASS_NORMALIZATION) s = 0.25 / (inv->kappa * inv->kappa);
  else if (inv->mass_normalization == QUDA_ASYMMETRIC_MASS_NORMALIZATION) s = 0.5 / inv->kappa;
  ColorSpinorParam pp = deviceSpinorParam(QUDA_DOUBLE_PRECISION, QUDA_PARITY_SITE_SUBSET, fieldTwistFlavor(*inv));
  ColorSpinorField *t = new ColorSpinorField(pp);
  for (size_t i = 0; i < n; i++) {
    if (x[i]->SiteSubset() != QUDA_PARITY_SITE_SUBSET || x[i]->Precision() != QUDA_DOUBLE_PRECISION) errorQuda("fermion force: the solutions are fp64 parity fields");
    X[i] = new ColorSpinorField(fp); Y[i] = new ColorSpinorField(fp);
    ColorSpinorField &x0 = even ? X[i]->Even() : X[i]->Odd(), &x1 = even ? X[i]->Odd() : X[i]->Even();
    ColorSpinorField &y0 = even ? Y[i]->Even() : Y[i]->Odd(), &y1 = even ? Y[i]->Odd() : Y[i]->Even();
    blas::copy(x0, *x[i]);
    d->Dagger(QUDA_DAG_NO);
    d->Dslash(x1, x0, p1);                      // R^-1 D x (Wilson: D x)
    if ((tm || tc) && !asym) {                  // y = R^-dag Mh x
      d->M(*t, x0);
      if (tc) { XW[i] = new ColorSpinorField(pp); blas::xmyz(x0, *t, *XW[i]); }   // x - w
      d->Dagger(QUDA_DAG_YES);
      rinv(y0, *t, p0);
    } else { d->M(y0, x0); d->Dagger(QUDA_DAG_YES); }                              // y = Mh x
    hop->DiracWilson::Dslash(*t, y0, p1);       // D^dag y
    rinv(y1, *t, p1);
    d->Dagger(QUDA_DAG_NO);
    c[i] = -dt * coeff[i] * 2.0 * inv->kappa * inv->kappa * s * s;
  }
  fermionOprodForce(mom, U, X, Y, c);
  if (tc) {
    const int q0 = even ? 0 : 1, q1 = 1 - q0;
    std::vector<SigmaOprodPair> pairs(n);
    for (size_t i = 0; i < n; i++) {
      SigmaOprodPair &p = pairs[i];
      p.x[0] = &X[i]->Even(); p.x[1] = &X[i]->Odd(); p.y[0] = &Y[i]->Even(); p.y[1] = &Y[i]->Odd();
      if (XW[i]) p.x[q0] = XW[i];
      p.cr[0] = p.cr[1] = 0;
      p.ci[q0] = -2.0 * s * s * inv->clover_coeff * dt * coeff[i];
      p.ci[q1] = p.ci[q0] * inv->kappa * inv->kappa;
    }
    TensorField T(U.geom);
    cloverSigmaOprod(T, pairs, false);
    cloverDerivativeForce(mom, U, T, 1.0);
  }
  for (size_t i = 0; i < n; i++) { delete X[i]; delete Y[i]; delete XW[i]; }
  delete t;
  delete d;
}

}  // namespace quda
