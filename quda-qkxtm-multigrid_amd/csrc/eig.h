// eig.h — what eigensolver.cpp calls in eig.hip: the panel kernels of the Lanczos eigensolver and the deflation projector.
//
// A PanelView describes m fp64 device vectors of the same shape as 2n real "rows": vector j starts at v[j] (a device table of base
// pointers) and consists of nseg segments of segLen doubles that start segStride doubles apart (a full ColorSpinorField: the even
// half and the odd half; the flat BLAS kernels of blas.hip walk the fields the same way, plane padding included).
#pragma once

#include <hip/hip_runtime.h>

namespace quda {

constexpr int kEigMaxVectors = 256;

struct PanelView {
  double *const *v;   // device table of m base pointers
  int m;
  long segLen, segStride;
  int nseg;
  long rows() const { return segLen * nseg; }
};

// c[j] = (v_j, w) = sum conj(v_j) w for j < m, rank-local, on the host as c[m][re, im].  One launch, one read of w from memory; the
// number of blocks depends on the length only, every block adds its tiles in order, the last block adds the blocks in order.
void eigBlockDot(double *h_c, const PanelView &V, const double *w);
// w -= sum_{j<m} c[j] v_j, c[m][re, im] on the host
void eigBlockAxpy(double *w, const double *h_c, const PanelView &V);
// V[:, 0..k) <- V[:, 0..m) Q in place, Q real m x k row-major on the host (fp64 matrix cores)
void eigRotate(const PanelView &V, int k, const double *h_Q);
// out = d3 tm1 + d2 tm2 + d1 atm2 over n doubles per segment (out may alias tm1)
void eigChebyUpdate(double *out, const double *tm1, const double *tm2, const double *atm2, double d3, double d2, double d1, long segLen, long segStride, int nseg);
void eigKernelsEnd();   // frees the scratch buffers

}  // namespace quda
