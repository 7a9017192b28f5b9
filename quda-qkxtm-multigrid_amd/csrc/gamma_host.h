// gamma_host.h — host-side 4x4 complex matrices and the gamma matrices of the UKQCD basis, from which the contraction files
// (contract.hip, threep.hip) build their spin tables by explicit products.
#pragma once

#include <complex>

#include "qa_core.h"

namespace quda {
namespace gammah {

typedef std::complex<double> cd;
struct M4 { cd a[4][4]; };
inline M4 mzero() { M4 m; for (int i = 0; i < 4; i++) for (int j = 0; j < 4; j++) m.a[i][j] = 0; return m; }
inline M4 mid4() { M4 m = mzero(); for (int i = 0; i < 4; i++) m.a[i][i] = 1; return m; }
inline M4 operator*(const M4 &x, const M4 &y) {
  M4 r = mzero();
  for (int i = 0; i < 4; i++) for (int j = 0; j < 4; j++) for (int k = 0; k < 4; k++) r.a[i][j] += x.a[i][k] * y.a[k][j];
  return r;
}
inline M4 operator+(const M4 &x, const M4 &y) { M4 r; for (int i = 0; i < 4; i++) for (int j = 0; j < 4; j++) r.a[i][j] = x.a[i][j] + y.a[i][j]; return r; }
inline M4 operator*(cd s, const M4 &x) { M4 r; for (int i = 0; i < 4; i++) for (int j = 0; j < 4; j++) r.a[i][j] = s * x.a[i][j]; return r; }
inline M4 transpose(const M4 &x) { M4 r; for (int i = 0; i < 4; i++) for (int j = 0; j < 4; j++) r.a[i][j] = x.a[j][i]; return r; }
inline M4 dagger(const M4 &x) { M4 r; for (int i = 0; i < 4; i++) for (int j = 0; j < 4; j++) r.a[i][j] = std::conj(x.a[j][i]); return r; }

// UKQCD basis: g_k = [[0, i s_k], [-i s_k, 0]], g4 = diag(1, 1, -1, -1), g5 = g1 g2 g3 g4 = [[0, 1], [1, 0]]
inline M4 gammaU(int mu) {
  const cd I(0, 1);
  const cd s[3][2][2] = {{{0, 1}, {1, 0}}, {{0, -I}, {I, 0}}, {{1, 0}, {0, -1}}};
  M4 g = mzero();
  if (mu == 4) { g.a[0][0] = g.a[1][1] = 1; g.a[2][2] = g.a[3][3] = -1; return g; }
  if (mu == 5) return gammaU(1) * gammaU(2) * gammaU(3) * gammaU(4);
  for (int i = 0; i < 2; i++) for (int j = 0; j < 2; j++) { g.a[i][2 + j] = I * s[mu - 1][i][j]; g.a[2 + i][j] = -I * s[mu - 1][i][j]; }
  return g;
}

// m as a signed permutation: row r holds val[r] in column col[r]
inline void toSPerm(const M4 &m, int col[4], double2 val[4]) {
  for (int r = 0; r < 4; r++) {
    int n = 0;
    for (int c = 0; c < 4; c++)
      if (std::abs(m.a[r][c]) > 1e-12) { col[r] = c; val[r] = make_double2(m.a[r][c].real(), m.a[r][c].imag()); n++; }
    if (n != 1) errorQuda("spin matrix is not a signed permutation");
  }
}

}  // namespace gammah
}  // namespace quda
