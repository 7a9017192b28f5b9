// gcr_core.h — the coefficients of one Krylov cycle of restarted GCR for ONE right-hand side, and the back substitution that turns them into
// the solution update (reference lib/inv_gcr_quda.cpp:125-157).  Host arithmetic on std::complex<double> only: GCR (solver.cpp) holds one,
// the lockstep multi-source GCR (block_solver.cpp) one per source, the GCR of the block coarse cycle (block_coarse_cycle.cpp) one per column.
#pragma once

#include <complex>
#include <vector>

namespace quda {

struct GcrCoeffs {
  int nK = 0;
  std::vector<std::complex<double>> alpha;   // alpha[k] = (Ap_k, r)
  std::vector<double> gamma;                 // gamma[k] = |Ap_k| before its normalisation
  std::vector<std::complex<double>> beta;    // beta(i, k) = (Ap_i, Ap_k) for i < k, row-major with leading dimension nK
  explicit GcrCoeffs(int nK_ = 0) : nK(nK_), alpha(nK_), gamma(nK_), beta((size_t)nK_ * nK_) {}
  std::complex<double> &b(int i, int k) { return beta[(size_t)i * nK + k]; }
  // delta_a = (alpha_a - sum_{j > a} beta_aj delta_j) / gamma_a for the first k directions, a descending and j ascending; a direction with
  // gamma_a == 0 (an all-zero padding column of a block field: the other GCRs stop with "GCR breakdown" before they get here) gets delta_a = 0
  void backSubstitute(int k, std::complex<double> *delta) const {
    for (int a = k - 1; a >= 0; a--) {
      std::complex<double> d = alpha[a];
      for (int j = a + 1; j < k; j++) d -= beta[(size_t)a * nK + j] * delta[j];
      delta[a] = gamma[a] == 0.0 ? std::complex<double>(0.0) : d / gamma[a];
    }
  }
};

}  // namespace quda
