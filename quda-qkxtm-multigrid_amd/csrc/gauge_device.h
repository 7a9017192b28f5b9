// gauge_device.h — the 3x3 colour-matrix device code that clover.hip (clover construction), gauge_obs.hip (smearing, plaquette,
// topological charge), gauge_md.hip (gauge force, link update, SU(3) projection) and gauge_fix.hip (gauge fixing) share, and ferm_force.hip with them: the matrix
// type and its products, the resident-link loader, the epilogue of both force kernels, matrix fields with their load/store, the
// polar SU(3) projection, exp(iQ), the clover-leaf sum with its scatter into the clover blocks and the block sum of the reductions;
// and the host helpers of the transport formulation: pools of matrix fields, links to the host, ordered sums.
#pragma once

#include "fields.h"
#include "device_io.h"

namespace quda {

// ---- 3x3 complex matrices in fp64 and the gather of a resident link ----
struct M3 { double re[9], im[9]; };
__device__ __forceinline__ void m3_mul(M3 &c, const M3 &a, const M3 &b) {
#pragma unroll
  for (int i = 0; i < 3; i++)
#pragma unroll
    for (int j = 0; j < 3; j++) {
      double r = 0, m = 0;
#pragma unroll
      for (int k = 0; k < 3; k++) { r += a.re[i * 3 + k] * b.re[k * 3 + j] - a.im[i * 3 + k] * b.im[k * 3 + j]; m += a.re[i * 3 + k] * b.im[k * 3 + j] + a.im[i * 3 + k] * b.re[k * 3 + j]; }
      c.re[i * 3 + j] = r; c.im[i * 3 + j] = m;
    }
}
__device__ __forceinline__ void m3_dag(M3 &c, const M3 &a) {
#pragma unroll
  for (int i = 0; i < 3; i++)
#pragma unroll
    for (int j = 0; j < 3; j++) { c.re[i * 3 + j] = a.re[j * 3 + i]; c.im[i * 3 + j] = -a.im[j * 3 + i]; }
}
// A <- A B in place, row by row: a row of the product needs that row of A only, so six reals of scratch registers are enough
__device__ __forceinline__ void m3_mul_right(M3 &a, const M3 &b) {
#pragma unroll
  for (int i = 0; i < 3; i++) {
    double r[3], m[3];
#pragma unroll
    for (int j = 0; j < 3; j++) {
      r[j] = 0; m[j] = 0;
#pragma unroll
      for (int k = 0; k < 3; k++) { r[j] += a.re[i * 3 + k] * b.re[k * 3 + j] - a.im[i * 3 + k] * b.im[k * 3 + j]; m[j] += a.re[i * 3 + k] * b.im[k * 3 + j] + a.im[i * 3 + k] * b.re[k * 3 + j]; }
    }
#pragma unroll
    for (int j = 0; j < 3; j++) { a.re[i * 3 + j] = r[j]; a.im[i * 3 + j] = m[j]; }
  }
}
// A <- A B^dag in place
__device__ __forceinline__ void m3_mul_right_dag(M3 &a, const M3 &b) {
#pragma unroll
  for (int i = 0; i < 3; i++) {
    double r[3], m[3];
#pragma unroll
    for (int j = 0; j < 3; j++) {
      r[j] = 0; m[j] = 0;
#pragma unroll
      for (int k = 0; k < 3; k++) { r[j] += a.re[i * 3 + k] * b.re[j * 3 + k] + a.im[i * 3 + k] * b.im[j * 3 + k]; m[j] += a.im[i * 3 + k] * b.re[j * 3 + k] - a.re[i * 3 + k] * b.im[j * 3 + k]; }
    }
#pragma unroll
    for (int j = 0; j < 3; j++) { a.re[i * 3 + j] = r[j]; a.im[i * 3 + j] = m[j]; }
  }
}

// m (the ten reals of A_mu(x)) <- TA(A - eb3 U V), lib/gauge_force.cu:131-140.  The stored A is anti-Hermitian already, so only its
// trace and the product W = U V go through the projection:
//   off-diagonal  A_ij - eb3 (W_ij - conj W_ji)/2,   diagonal  d_i - (d_0 + d_1 + d_2)/3 with d_i = Im A_ii - eb3 Im W_ii
__device__ __forceinline__ void force_epilogue(double *m, const M3 &U, const M3 &V, double eb3) {
  M3 W;
  m3_mul(W, U, V);
  double a[10];
#pragma unroll
  for (int k = 0; k < 10; k++) a[k] = m[k];
  const double h = 0.5 * eb3;
  a[0] -= h * (W.re[1] - W.re[3]); a[1] -= h * (W.im[1] + W.im[3]);
  a[2] -= h * (W.re[2] - W.re[6]); a[3] -= h * (W.im[2] + W.im[6]);
  a[4] -= h * (W.re[5] - W.re[7]); a[5] -= h * (W.im[5] + W.im[7]);
  const double d0 = a[6] - eb3 * W.im[0], d1 = a[7] - eb3 * W.im[4], d2 = a[8] - eb3 * W.im[8];
  const double tr = (d0 + d1 + d2) * (1.0 / 3.0);
  a[6] = d0 - tr; a[7] = d1 - tr; a[8] = d2 - tr; a[9] = 0;
#pragma unroll
  for (int k = 0; k < 10; k++) m[k] = a[k];
}
struct GaugeView { const char *data; size_t link_bytes; int stride; int X[4]; int tsign, tsign_bwd; };
// U_mu at the (possibly out-of-range, wrapped) coordinates x: the forward link stored at its own site
template <typename T, int R> __device__ __forceinline__ void load_link(M3 &U, const GaugeView &g, int mu, const int *xin) {
  using real = typename Store<T>::real;
  int x[4];
#pragma unroll
  for (int d = 0; d < 4; d++) { x[d] = xin[d]; if (x[d] < 0) x[d] += g.X[d]; if (x[d] >= g.X[d]) x[d] -= g.X[d]; }
  const int par = (x[0] + x[1] + x[2] + x[3]) & 1;
  const int idx = (((x[3] * g.X[2] + x[2]) * g.X[1] + x[1]) * g.X[0] + x[0]) >> 1;
  real u[18];
  // the host links carry the anti-periodic sign on the last time slice; recon-12 stores rows 0,1 as given and has to put the
  // sign back on the reconstructed third row (in the plaquette the two boundary links of a leaf then cancel their signs)
  const real sign = (R != 18 && mu == 3 && x[3] == g.X[3] - 1) ? (real)g.tsign : (real)1;   // (recon-8: u0 of the reconstruction)
  Link<T, R>::load(u, g.data + ((size_t)par * 8 + 2 * mu) * g.link_bytes, g.stride, idx, sign);
#pragma unroll
  for (int k = 0; k < 9; k++) { U.re[k] = u[2 * k]; U.im[k] = u[2 * k + 1]; }
}

// ---- a 3x3 matrix per site: planar fp64, 24 reals per site (18 used), both parities ----
struct MatField { double *p; int Vh; __host__ __device__ double *par(int q) const { return p + (size_t)q * 24 * Vh; } };
__device__ __forceinline__ void mf_load(M3 &m, const MatField &f, int par, int idx) {
  double v[24];
  Planar<double, 24>::load(v, f.par(par), f.Vh, idx, nullptr, idx);
#pragma unroll
  for (int k = 0; k < 9; k++) { m.re[k] = v[2 * k]; m.im[k] = v[2 * k + 1]; }
}
__device__ __forceinline__ void mf_store(const M3 &m, const MatField &f, int par, int idx) {
  double v[24];
#pragma unroll
  for (int k = 0; k < 9; k++) { v[2 * k] = m.re[k]; v[2 * k + 1] = m.im[k]; }
#pragma unroll
  for (int k = 18; k < 24; k++) v[k] = 0;
  Planar<double, 24>::store(v, f.par(par), f.Vh, idx, nullptr, idx);
}
// stored matrix `slot` (2 mu: U_mu(x); 2 mu + 1: U_mu(x - mu)^dag) of site (par, idx) at time coordinate t
template <typename T, int R> __device__ __forceinline__ void load_w(M3 &U, const GaugeView &g, int par, int idx, int slot, int t) {
  using real = typename Store<T>::real;
  real sign = 1;
  if (R != 18 && (slot >> 1) == 3) sign = (slot & 1) ? (t == 0 ? (real)g.tsign_bwd : (real)1) : (t == g.X[3] - 1 ? (real)g.tsign : (real)1);
  real u[18];
  Link<T, R>::load(u, g.data + ((size_t)par * 8 + slot) * g.link_bytes, g.stride, idx, sign);
#pragma unroll
  for (int k = 0; k < 9; k++) { U.re[k] = u[2 * k]; U.im[k] = u[2 * k + 1]; }
}
__device__ __forceinline__ int time_coord(const GaugeView &g, int idx) { return idx / ((g.X[0] >> 1) * g.X[1] * g.X[2]); }

// ---- determinant, inverse, polar projection onto SU(3) ----
__device__ __forceinline__ void m3_det(double &dr, double &di, const M3 &a) {
  dr = 0; di = 0;
#pragma unroll
  for (int c = 0; c < 3; c++) {
    const int c1 = (c + 1) % 3, c2 = (c + 2) % 3;
    const double mr = (a.re[3 + c1] * a.re[6 + c2] - a.im[3 + c1] * a.im[6 + c2]) - (a.re[3 + c2] * a.re[6 + c1] - a.im[3 + c2] * a.im[6 + c1]);
    const double mi = (a.re[3 + c1] * a.im[6 + c2] + a.im[3 + c1] * a.re[6 + c2]) - (a.re[3 + c2] * a.im[6 + c1] + a.im[3 + c2] * a.re[6 + c1]);
    dr += a.re[c] * mr - a.im[c] * mi;
    di += a.re[c] * mi + a.im[c] * mr;
  }
}
__device__ __forceinline__ void m3_inverse(M3 &o, const M3 &a) {   // adjugate / determinant
  double dr, di;
  m3_det(dr, di, a);
  const double n = dr * dr + di * di, ir = dr / n, ii = -di / n;
#pragma unroll
  for (int i = 0; i < 3; i++)
#pragma unroll
    for (int j = 0; j < 3; j++) {
      const int r1 = (j + 1) % 3, r2 = (j + 2) % 3, c1 = (i + 1) % 3, c2 = (i + 2) % 3;
      const double cr = (a.re[3 * r1 + c1] * a.re[3 * r2 + c2] - a.im[3 * r1 + c1] * a.im[3 * r2 + c2]) - (a.re[3 * r1 + c2] * a.re[3 * r2 + c1] - a.im[3 * r1 + c2] * a.im[3 * r2 + c1]);
      const double ci = (a.re[3 * r1 + c1] * a.im[3 * r2 + c2] + a.im[3 * r1 + c1] * a.re[3 * r2 + c2]) - (a.re[3 * r1 + c2] * a.im[3 * r2 + c1] + a.im[3 * r1 + c2] * a.re[3 * r2 + c1]);
      o.re[3 * i + j] = cr * ir - ci * ii;
      o.im[3 * i + j] = cr * ii + ci * ir;
    }
}
// su3_project.cuh polarSu3: Newton iteration X <- (X + X^-dag)/2 until X is unitary to tol (elementwise, X vs (X^-1)^dag),
// then the phase of the determinant is divided out.  Capped at 100 sweeps (the reference loops until the test passes).
__device__ __forceinline__ void polar_su3(M3 &m, double tol) {
  M3 out = m, inv;
  m3_inverse(inv, out);
  for (int sweep = 0; sweep < 100; sweep++) {
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
      for (int j = 0; j < 3; j++) {
        out.re[3 * i + j] = 0.5 * (out.re[3 * i + j] + inv.re[3 * j + i]);
        out.im[3 * i + j] = 0.5 * (out.im[3 * i + j] - inv.im[3 * j + i]);
      }
    m3_inverse(inv, out);
    bool bad = false;
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
      for (int j = 0; j < 3; j++) bad = bad || fabs(out.re[3 * i + j] - inv.re[3 * j + i]) > tol || fabs(out.im[3 * i + j] + inv.im[3 * j + i]) > tol;
    if (!bad) break;
  }
  double dr, di;
  m3_det(dr, di, out);
  const double mod = pow(dr * dr + di * di, 1.0 / 6.0), angle = atan2(di, dr) / -3.0;
  const double cr = cos(angle) / mod, ci = sin(angle) / mod;
#pragma unroll
  for (int k = 0; k < 9; k++) { m.re[k] = out.re[k] * cr - out.im[k] * ci; m.im[k] = out.re[k] * ci + out.im[k] * cr; }
}

// max |U^dag U - 1| over the entries: how far a projected link still is from unitary
__device__ __forceinline__ double unitarity_deviation(const M3 &u) {
  M3 d, p;
  m3_dag(d, u);
  m3_mul(p, d, u);
  p.re[0] -= 1.0; p.re[4] -= 1.0; p.re[8] -= 1.0;
  double dev = 0;
#pragma unroll
  for (int k = 0; k < 9; k++) dev = fmax(dev, fmax(fabs(p.re[k]), fabs(p.im[k])));
  return dev;
}

// ---- exp(iQ) of a traceless Hermitian Q ----
// exp(iQ) = f0 + f1 Q + f2 Q^2 of a traceless Hermitian Q by the Cayley-Hamilton form (eqs. 14-34 of the paper):
//   c0 = tr Q^3 / 3 = det Q,  c1 = tr Q^2 / 2,  c0max = 2 (c1/3)^(3/2),  theta = acos(c0 / c0max),
//   u = sqrt(c1/3) cos(theta/3),  w = sqrt(c1) sin(theta/3),  f_j = h_j / (9 u^2 - w^2).
// c0 < 0 goes through f_j(-c0) = (-1)^j conj f_j(c0), so theta/3 <= pi/6 and 9 u^2 - w^2 = c1 (3 cos^2 - sin^2) >= 2 c1 > 0.
// The only other divisions are by c0max and by w in xi0 = sin(w)/w: xi0 takes its even Taylor polynomial for |w| <= 0.05, and
// below c1 = 1e-60 (c0max would underflow towards 0; c1 = 0 means Q = 0) the result is 1 + iQ, exact to c1/2: the unit matrix
// for Q = 0.  Rounding can push c0 / c0max past 1 at the degenerate point; it is clamped.
__device__ __forceinline__ void su3_exp_iq(M3 &E, const M3 &Q) {
  double c1 = 0;
#pragma unroll
  for (int k = 0; k < 9; k++) c1 += Q.re[k] * Q.re[k] + Q.im[k] * Q.im[k];   // tr Q^2 = sum |Q_ij|^2 for Hermitian Q
  c1 *= 0.5;
  if (c1 < 1e-60) {
#pragma unroll
    for (int k = 0; k < 9; k++) { E.re[k] = -Q.im[k]; E.im[k] = Q.re[k]; }
    E.re[0] += 1.0; E.re[4] += 1.0; E.re[8] += 1.0;
    return;
  }
  M3 Q2;
  m3_mul(Q2, Q, Q);
  double c0 = 0;   // tr(Q Q^2) = sum_ij Q_ij (Q^2)_ji, real
#pragma unroll
  for (int i = 0; i < 3; i++)
#pragma unroll
    for (int j = 0; j < 3; j++) c0 += Q.re[3 * i + j] * Q2.re[3 * j + i] - Q.im[3 * i + j] * Q2.im[3 * j + i];
  c0 *= 1.0 / 3.0;
  const bool neg = c0 < 0;
  c0 = fabs(c0);
  const double c13 = c1 * (1.0 / 3.0), c0max = 2.0 * c13 * sqrt(c13);   // > 0: c1 >= 1e-60
  const double theta3 = acos(fmin(c0 / c0max, 1.0)) * (1.0 / 3.0);
  const double u = sqrt(c13) * cos(theta3), w = sqrt(c1) * sin(theta3);
  const double u2 = u * u, w2 = w * w, cw = cos(w);
  const double xi0 = fabs(w) <= 0.05 ? 1.0 - w2 * (1.0 / 6.0) * (1.0 - w2 * (1.0 / 20.0) * (1.0 - w2 * (1.0 / 42.0))) : sin(w) / w;
  double s2u, c2u, su, cu;
  sincos(2.0 * u, &s2u, &c2u);
  sincos(u, &su, &cu);
  // h_j = a_j e^{2iu} + e^{-iu} (b_j + i d_j)
  const double b0 = 8.0 * u2 * cw, d0 = 2.0 * u * (3.0 * u2 + w2) * xi0;
  const double b1 = -2.0 * u * cw, d1 = (3.0 * u2 - w2) * xi0;
  const double b2 = -cw, d2 = -3.0 * u * xi0;
  const double a0 = u2 - w2, a1 = 2.0 * u, inv = 1.0 / (9.0 * u2 - w2);
  double fr[3], fi[3];
  fr[0] = (a0 * c2u + cu * b0 + su * d0) * inv; fi[0] = (a0 * s2u + cu * d0 - su * b0) * inv;
  fr[1] = (a1 * c2u + cu * b1 + su * d1) * inv; fi[1] = (a1 * s2u + cu * d1 - su * b1) * inv;
  fr[2] = (c2u + cu * b2 + su * d2) * inv;      fi[2] = (s2u + cu * d2 - su * b2) * inv;
  if (neg) { fi[0] = -fi[0]; fr[1] = -fr[1]; fi[2] = -fi[2]; }
#pragma unroll
  for (int k = 0; k < 9; k++) {
    E.re[k] = fr[1] * Q.re[k] - fi[1] * Q.im[k] + fr[2] * Q2.re[k] - fi[2] * Q2.im[k];
    E.im[k] = fr[1] * Q.im[k] + fi[1] * Q.re[k] + fr[2] * Q2.im[k] + fi[2] * Q2.re[k];
  }
  E.re[0] += fr[0]; E.re[4] += fr[0]; E.re[8] += fr[0];
  E.im[0] += fi[0]; E.im[4] += fi[0]; E.im[8] += fi[0];
}

// ---- the clover leaves: field strength, its scatter into the colour blocks of the clover term, the packed chiral block ----
// F = (Q - Q^dag) / 8
__device__ __forceinline__ void m3_fmunu(M3 &F, const M3 &Q) {
#pragma unroll
  for (int i = 0; i < 3; i++)
#pragma unroll
    for (int j = 0; j < 3; j++) {
      F.re[i * 3 + j] = 0.125 * (Q.re[i * 3 + j] - Q.re[j * 3 + i]);
      F.im[i * 3 + j] = 0.125 * (Q.im[i * 3 + j] + Q.im[j * 3 + i]);
    }
}
// F = (Q - Q^dag) / 8 of the leaf sum Q = P + A + B + C at site (par, idx)
__device__ __forceinline__ void leaf_sum_fmunu(M3 &F, const MatField &P, const MatField &A, const MatField &B, const MatField &C, int par, int idx) {
  M3 Q, m;
  mf_load(Q, P, par, idx);
  mf_load(m, A, par, idx);
#pragma unroll
  for (int k = 0; k < 9; k++) { Q.re[k] += m.re[k]; Q.im[k] += m.im[k]; }
  mf_load(m, B, par, idx);
#pragma unroll
  for (int k = 0; k < 9; k++) { Q.re[k] += m.re[k]; Q.im[k] += m.im[k]; }
  mf_load(m, C, par, idx);
#pragma unroll
  for (int k = 0; k < 9; k++) { Q.re[k] += m.re[k]; Q.im[k] += m.im[k]; }
  m3_fmunu(F, Q);
}
// F_mu_nu (index fi = mu (mu - 1) / 2 + nu) folded into the colour blocks of the two chiral blocks ch: B1[ch] = i c (F0 -/+ F5),
// B2[ch] = c (F1 +/- F4 - i (F2 -/+ F3)).   i c F = c (-fm + i fr);   c F = c (fr + i fm);   -i c F = c (fm - i fr)
__device__ __forceinline__ void clover_add_fmunu(M3 *b1, M3 *b2, int fi, double coeff, const M3 &F) {
#pragma unroll
  for (int k = 0; k < 9; k++) {
    const double fr = F.re[k], fm = F.im[k];
    switch (fi) {
      case 0: b1[0].re[k] += -coeff * fm; b1[0].im[k] += coeff * fr; b1[1].re[k] += -coeff * fm; b1[1].im[k] += coeff * fr; break;
      case 5: b1[0].re[k] -= -coeff * fm; b1[0].im[k] -= coeff * fr; b1[1].re[k] += -coeff * fm; b1[1].im[k] += coeff * fr; break;
      case 1: b2[0].re[k] += coeff * fr; b2[0].im[k] += coeff * fm; b2[1].re[k] += coeff * fr; b2[1].im[k] += coeff * fm; break;
      case 4: b2[0].re[k] += coeff * fr; b2[0].im[k] += coeff * fm; b2[1].re[k] -= coeff * fr; b2[1].im[k] -= coeff * fm; break;
      case 2: b2[0].re[k] += coeff * fm; b2[0].im[k] -= coeff * fr; b2[1].re[k] += coeff * fm; b2[1].im[k] -= coeff * fr; break;
      default: b2[0].re[k] -= coeff * fm; b2[0].im[k] += coeff * fr; b2[1].re[k] += coeff * fm; b2[1].im[k] -= coeff * fr; break;  // fi == 3
    }
  }
}
// one chiral block [[1 - B1, B2^dag], [B2, 1 + B1]] in packed order: 6 diagonal reals, then the 15 strictly-lower entries column by
// column (tests/clover_reference.cpp:45-53)
__device__ __forceinline__ void clover_pack_block(double *A, const M3 &b1, const M3 &b2) {
  for (int i = 0; i < 3; i++) { A[i] = 1.0 - b1.re[i * 3 + i]; A[i + 3] = 1.0 + b1.re[i * 3 + i]; }
  int k = 0;
  for (int col = 0; col < 6; col++)
    for (int row = col + 1; row < 6; row++, k++) {
      double re, im;
      const int rs = row / 3, rc = row % 3, cs = col / 3, cc = col % 3;
      if (rs == 0) { re = -b1.re[rc * 3 + cc]; im = -b1.im[rc * 3 + cc]; }          // spin 0 x spin 0: -B1
      else if (cs == 1) { re = b1.re[rc * 3 + cc]; im = b1.im[rc * 3 + cc]; }       // spin 1 x spin 1: +B1
      else { re = b2.re[rc * 3 + cc]; im = b2.im[rc * 3 + cc]; }                    // spin 1 x spin 0: B2
      A[6 + 2 * k] = re; A[6 + 2 * k + 1] = im;
    }
}

// the sum of v over the 256 threads of a block, in thread 0: the lanes of a wave by shuffle, the four wave sums through LDS and
// added left to right, so the same values give the same bits
__device__ __forceinline__ double block_sum_256(double v) {
  __shared__ double lds[4];
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = v;
  __syncthreads();
  return ((lds[0] + lds[1]) + lds[2]) + lds[3];
}

// ---- host side (gauge_obs.hip) ----
// the view of a resident field, its forward links of one direction as a matrix field, out(x) = in(x + dhat(dir)) (dir = 2 mu: forward,
// 2 mu + 1: backward; ghost-aware), and out (+)= op(A) op(B) site by site
GaugeView viewOf(const GaugeField &U);
void extractForwardLinks(MatField F, const GaugeField &U, int mu);
void shiftField(MatField out, MatField in, const LatticeGeom &geom, int dir);
void mfMul(MatField out, MatField A, MatField B, int dagA, int dagB, int accumulate);
// F in host QDP order (even sites then odd, 18 reals per site) at stage, a device pointer: the launch of matFieldsToHost
void matFieldToQdp(double *stage, MatField F, int mu);
// the four clover leaves of the mu-nu plane by transport: on return W[4] = P, W[1] = T_mu P, W[2] = T_nu P, W[3] = T_nu T_mu P
// (W[0] is scratch)
void cloverLeaves(MatField W[5], const GaugeField &U, int mu, int nu);
// any direction partitioned, or the environment variable envName set and not 0: the transport formulation instead of direct gathers
bool usesTransport(const char *envName);
// the nb per-block partial sums of a reduction kernel, added in block order by the host (this rank's part); synchronises the stream
double sumPartials(const double *d_partial, int nb);

int gaugePadSites();                  // fields.hip: plane padding (sites) of the link and clover fields
void *stagingBuffer(size_t bytes);    // fields.hip: the library's one grow-only device buffer; valid until the next call
inline size_t alignUp(size_t n, size_t a) { return (n + a - 1) / a * a; }

// n matrix fields, and `extra` doubles behind them, in one device allocation that lives as long as the pool
struct MatPool {
  double *pool = nullptr;
  const int Vh;
  MatPool(int Vh, int n, size_t extra = 0) : Vh(Vh) { HIP_CHECK(qaMalloc((void **)&pool, (n * fieldDoubles() + extra) * sizeof(double))); }
  ~MatPool() { (void)hipFree(pool); }
  MatPool(const MatPool &) = delete;
  MatPool &operator=(const MatPool &) = delete;
  size_t fieldDoubles() const { return (size_t)2 * 24 * Vh; }
  MatField operator[](int i) const { return {pool + i * fieldDoubles(), Vh}; }   // i = n: the extra doubles begin at its p
};

// One direction at a time: the matrix field links(mu) -> launch(stage, F, mu), which writes host QDP order (even sites then odd, 18
// reals per site) into the staging buffer -> host array h_out[mu]
template <typename Links, typename Launch> void matFieldsToHost(void *const h_out[4], const LatticeGeom &geom, Links links, Launch launch) {
  const size_t bytes = (size_t)geom.V * 18 * sizeof(double);
  double *stage = (double *)stagingBuffer(bytes);
  hipStream_t s = computeStream();
  for (int mu = 0; mu < 4; mu++) {
    launch(stage, links(mu), mu);
    HIP_CHECK(hipMemcpyAsync(h_out[mu], stage, bytes, hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));
  }
}
// the same from the forward links of a resident field
template <typename Launch> void linksToHost(void *const h_out[4], const GaugeField &U, Launch launch) {
  MatPool pool(U.geom.Vh, 1);
  matFieldsToHost(h_out, U.geom, [&](int mu) { extractForwardLinks(pool[0], U, mu); return pool[0]; }, launch);
}

}  // namespace quda
