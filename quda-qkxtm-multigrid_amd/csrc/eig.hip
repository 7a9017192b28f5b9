// eig.hip — the panel kernels of the thick-restart Lanczos eigensolver and of the deflation projector (eigensolver.cpp), fp64, gfx950.
//
// The basis of the Lanczos process is up to 256 full device fields.  Every step orthogonalises the new vector against all of them
// (two passes of classical Gram-Schmidt) and every restart compresses the basis with the matrix of Ritz coefficients; blas::multiDot /
// multiCaxpy stop at 20 fields and return their sums through the host per call.  Here:
//   eig_block_dot_kernel   c[j] = (v_j, w), j < m: a block stages a tile of w in LDS (the one read of w), wave q takes the vectors
//                          j = q, q + 4, ... and streams the tile of v_j past it; shuffle sum over the lanes, the tiles of a block in
//                          order, the blocks in order by the last block (completion counter: lastBlockFinishes of reduce.h, as finish_reduction of blas.hip);
//   eig_block_axpy_kernel  w -= sum_j c[j] v_j: the coefficients in LDS, two complex numbers of w per thread;
//   eig_rotate_kernel      V[:, 0..k) <- V[:, 0..m) Q in place on the fp64 matrix cores (v_mfma_f64_16x16x4_f64): a block owns 32
//                          real rows of ALL m vectors, stages them in LDS (m x 32 x 8 B <= 64 KiB), synchronises and only then writes
//                          the k output columns, which is what makes the in-place update safe;
//   eig_cheby_kernel       out = d3 tm1 + d2 tm2 + d1 (A tm2), one step of the Chebyshev recurrence of the filter.
// A vector is walked as segments (eig.h PanelView).
#include <vector>

#include "eig.h"
#include "qa_core.h"
#include "reduce.h"

namespace quda {

namespace eig {

constexpr int DOT_TILE = 2048;     // complex numbers of w per tile: 32 KiB of LDS
constexpr int DOT_MAX_BLOCKS = 1024;
constexpr int ROT_ROWS = 32;

// ---- c[j] = (v_j, w) ----
__global__ void __launch_bounds__(256) eig_block_dot_kernel(double *const *V, int m, const double *w, long segC, long segStrideC, long tilesPerSeg, long ntiles, double *part,
                                                            unsigned *count, double *out) {
  __shared__ double2 sw[DOT_TILE];
  __shared__ double2 sacc[kEigMaxVectors];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int j = threadIdx.x; j < m; j += 256) sacc[j] = make_double2(0.0, 0.0);
  for (long t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const long seg = t / tilesPerSeg, e0 = (t % tilesPerSeg) * DOT_TILE;
    const long base = seg * segStrideC + e0;
    const int n = (int)(segC - e0 < DOT_TILE ? segC - e0 : DOT_TILE);
    __syncthreads();   // the previous tile is consumed (and sacc is zero)
    const double2 *wc = (const double2 *)w + base;
    for (int i = threadIdx.x; i < DOT_TILE; i += 256) sw[i] = i < n ? wc[i] : make_double2(0.0, 0.0);
    __syncthreads();
    for (int j = wave; j < m; j += 4) {
      const double2 *vj = (const double2 *)V[j] + base;
      double re = 0, im = 0;
#pragma unroll 8
      for (int q = 0; q < DOT_TILE / 64; q++) {
        const int i = lane + 64 * q;
        if (i < n) {
          const double2 v = vj[i], x = sw[i];
          re += v.x * x.x + v.y * x.y;
          im += v.x * x.y - v.y * x.x;
        }
      }
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) { re += __shfl_xor(re, off, 64); im += __shfl_xor(im, off, 64); }
      if (lane == 0) { sacc[j].x += re; sacc[j].y += im; }   // vector j belongs to this wave alone
    }
  }
  __syncthreads();
  for (int j = threadIdx.x; j < m; j += 256) {
    __hip_atomic_store(&part[((size_t)blockIdx.x * m + j) * 2], sacc[j].x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(&part[((size_t)blockIdx.x * m + j) * 2 + 1], sacc[j].y, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  lastBlockFinishes(count, [&] {
    for (int j = threadIdx.x; j < 2 * m; j += 256) {
      double v = 0;
      for (int b = 0; b < (int)gridDim.x; b++) v += __hip_atomic_load(&part[(size_t)b * 2 * m + j], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      out[j] = v;
    }
  });
}

// ---- w -= sum_j c[j] v_j ----
__global__ void __launch_bounds__(256) eig_block_axpy_kernel(double *w, double *const *V, int m, const double *c, long segC, long segStrideC, long blocksPerSeg) {
  __shared__ double2 sc[kEigMaxVectors];
  for (int j = threadIdx.x; j < m; j += 256) sc[j] = make_double2(c[2 * j], c[2 * j + 1]);
  __syncthreads();
  const long seg = blockIdx.x / blocksPerSeg, e0 = (blockIdx.x % blocksPerSeg) * 512 + threadIdx.x;
  const long base = seg * segStrideC;
  const bool ok0 = e0 < segC, ok1 = e0 + 256 < segC;
  if (!ok0) return;
  double2 *wc = (double2 *)w + base;
  double2 a0 = wc[e0], a1 = ok1 ? wc[e0 + 256] : make_double2(0.0, 0.0);
#pragma unroll 4
  for (int j = 0; j < m; j++) {
    const double2 *vj = (const double2 *)V[j] + base;
    const double2 cj = sc[j];
    const double2 v0 = vj[e0];
    a0.x -= cj.x * v0.x - cj.y * v0.y;
    a0.y -= cj.x * v0.y + cj.y * v0.x;
    if (ok1) {
      const double2 v1 = vj[e0 + 256];
      a1.x -= cj.x * v1.x - cj.y * v1.y;
      a1.y -= cj.x * v1.y + cj.y * v1.x;
    }
  }
  wc[e0] = a0;
  if (ok1) wc[e0 + 256] = a1;
}

// ---- V[:, 0..k) <- V[:, 0..m) Q ----
// v_mfma_f64_16x16x4_f64 computes D[16][16] += A[16][4] B[4][16]; lane l holds A[l & 15][l >> 4], B[l >> 4][l & 15] and the four
// results D[(l >> 4) + 4 i][l & 15], i < 4.  Here A = Q^T (16 output columns x 4 basis vectors) and B = the panel transposed (4 basis
// vectors x 16 rows), so a lane holds the SAME row of four output columns and 16 lanes store 16 consecutive rows of one column.
// LDS image: panel[half][j][16 rows], half = rows 0..15 / 16..31 of the panel, so the 64 lanes of a B operand read 64 consecutive doubles.
typedef double double4_t __attribute__((ext_vector_type(4)));

__global__ void __launch_bounds__(256) eig_rotate_kernel(double *const *V, int m, int k, const double *Q, long segLen, long segStride, long rows) {
  extern __shared__ double panel[];
  const int m4 = (m + 3) & ~3;
  const long r0 = (long)blockIdx.x * ROT_ROWS;
  {
    const int row = threadIdx.x & 31;
    const long r = r0 + row;
    const bool ok = r < rows;
    const long off = ok ? (r / segLen) * segStride + r % segLen : 0;
    for (int j = threadIdx.x >> 5; j < m4; j += 8) panel[((row >> 4) * m4 + j) * 16 + (row & 15)] = (ok && j < m) ? V[j][off] : 0.0;
  }
  __syncthreads();   // every read of the panel's rows is done: from here on the block may overwrite columns 0 .. k-1
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int l15 = lane & 15, l4 = lane >> 4;
  const double *p0 = panel + l4 * 16 + l15, *p1 = p0 + m4 * 16;
  for (int ct = wave; ct * 16 < k; ct += 4) {
    const int c = ct * 16 + l15;   // the output column of this lane's A operand
    const bool cok = c < k;
    double4_t acc0 = {0.0, 0.0, 0.0, 0.0}, acc1 = {0.0, 0.0, 0.0, 0.0};
    for (int kk = 0; kk < m4; kk += 4) {
      const int j = kk + l4;
      const double q = (cok && j < m) ? Q[(size_t)j * k + c] : 0.0;
      acc0 = __builtin_amdgcn_mfma_f64_16x16x4f64(q, p0[kk * 16], acc0, 0, 0, 0);
      acc1 = __builtin_amdgcn_mfma_f64_16x16x4f64(q, p1[kk * 16], acc1, 0, 0, 0);
    }
#pragma unroll
    for (int half = 0; half < 2; half++) {
      const long r = r0 + half * 16 + l15;
      if (r >= rows) continue;
      const long off = (r / segLen) * segStride + r % segLen;
#pragma unroll
      for (int i = 0; i < 4; i++) {
        const int oc = ct * 16 + l4 + 4 * i;
        if (oc < k) V[oc][off] = half ? acc1[i] : acc0[i];
      }
    }
  }
}

// ---- out = d3 tm1 + d2 tm2 + d1 atm2 ----
__global__ void __launch_bounds__(256) eig_cheby_kernel(double *out, const double *tm1, const double *tm2, const double *atm2, double d3, double d2, double d1, long segC,
                                                        long segStrideC, long blocksPerSeg) {
  const long seg = blockIdx.x / blocksPerSeg, e = (blockIdx.x % blocksPerSeg) * 256 + threadIdx.x;
  if (e >= segC) return;
  const long i = seg * segStrideC + e;
  const double2 a = ((const double2 *)tm1)[i], b = ((const double2 *)tm2)[i], c = ((const double2 *)atm2)[i];
  ((double2 *)out)[i] = make_double2(d3 * a.x + d2 * b.x + d1 * c.x, d3 * a.y + d2 * b.y + d1 * c.y);
}

// scratch of the launchers: partial sums, coefficients, the counter; Q
static double *d_part = nullptr, *d_coef = nullptr, *d_Q = nullptr;
static unsigned *d_count = nullptr;
static size_t partDoubles = 0;

static void ensureScratch(size_t part) {
  if (!d_coef) {
    HIP_CHECK(qaMalloc(&d_coef, 2 * kEigMaxVectors * sizeof(double)));
    HIP_CHECK(qaMalloc(&d_Q, (size_t)kEigMaxVectors * kEigMaxVectors * sizeof(double)));
    HIP_CHECK(qaMalloc(&d_count, sizeof(unsigned)));
    HIP_CHECK(hipMemset(d_count, 0, sizeof(unsigned)));
  }
  if (part > partDoubles) {
    if (d_part) (void)hipFree(d_part);
    HIP_CHECK(qaMalloc(&d_part, part * sizeof(double)));
    partDoubles = part;
  }
}

static void checkView(const PanelView &V, const char *what) {
  if (V.m < 1 || V.m > kEigMaxVectors) errorQuda("%s: %d vectors (1 .. %d)", what, V.m, kEigMaxVectors);
  if (V.nseg < 1 || V.segLen < 2 || (V.segLen & 1) || (V.segStride & 1) || (V.nseg > 1 && V.segStride < V.segLen))
    errorQuda("%s: segments of %ld doubles, %ld apart (even lengths, no overlap)", what, V.segLen, V.segStride);
}

}  // namespace eig

void eigBlockDot(double *h_c, const PanelView &V, const double *w) {
  using namespace eig;
  checkView(V, "eigBlockDot");
  const long segC = V.segLen / 2, tilesPerSeg = (segC + DOT_TILE - 1) / DOT_TILE, ntiles = tilesPerSeg * V.nseg;
  const int nblocks = (int)(ntiles < DOT_MAX_BLOCKS ? ntiles : DOT_MAX_BLOCKS);   // a function of the length alone: the order of the sums is fixed
  ensureScratch((size_t)nblocks * V.m * 2);
  hipStream_t s = computeStream();
  hipLaunchKernelGGL(eig_block_dot_kernel, dim3(nblocks), dim3(256), 0, s, V.v, V.m, w, segC, V.segStride / 2, tilesPerSeg, ntiles, d_part, d_count, d_coef);
  HIP_CHECK(hipGetLastError());
  HIP_CHECK(hipMemcpyAsync(h_c, d_coef, (size_t)2 * V.m * sizeof(double), hipMemcpyDeviceToHost, s));
  HIP_CHECK(hipStreamSynchronize(s));
}

void eigBlockAxpy(double *w, const double *h_c, const PanelView &V) {
  using namespace eig;
  checkView(V, "eigBlockAxpy");
  ensureScratch(0);
  const long segC = V.segLen / 2, blocksPerSeg = (segC + 511) / 512;
  hipStream_t s = computeStream();
  HIP_CHECK(hipMemcpyAsync(d_coef, h_c, (size_t)2 * V.m * sizeof(double), hipMemcpyHostToDevice, s));
  hipLaunchKernelGGL(eig_block_axpy_kernel, dim3((unsigned)(blocksPerSeg * V.nseg)), dim3(256), 0, s, w, V.v, V.m, d_coef, segC, V.segStride / 2, blocksPerSeg);
  HIP_CHECK(hipGetLastError());
  HIP_CHECK(hipStreamSynchronize(s));   // h_c is pageable: the copy above must have left it before the caller reuses it
}

void eigRotate(const PanelView &V, int k, const double *h_Q) {
  using namespace eig;
  checkView(V, "eigRotate");
  if (k < 1 || k > V.m) errorQuda("eigRotate: k = %d of m = %d", k, V.m);
  ensureScratch(0);
  hipStream_t s = computeStream();
  HIP_CHECK(hipMemcpyAsync(d_Q, h_Q, (size_t)V.m * k * sizeof(double), hipMemcpyHostToDevice, s));
  const long rows = V.rows();
  const int m4 = (V.m + 3) & ~3;
  const size_t lds = (size_t)2 * m4 * 16 * sizeof(double);   // 64 KiB at m = 256
  hipLaunchKernelGGL(eig_rotate_kernel, dim3((unsigned)((rows + ROT_ROWS - 1) / ROT_ROWS)), dim3(256), lds, s, V.v, V.m, k, d_Q, V.segLen, V.segStride, rows);
  HIP_CHECK(hipGetLastError());
  HIP_CHECK(hipStreamSynchronize(s));
}

void eigChebyUpdate(double *out, const double *tm1, const double *tm2, const double *atm2, double d3, double d2, double d1, long segLen, long segStride, int nseg) {
  using namespace eig;
  const long segC = segLen / 2, blocksPerSeg = (segC + 255) / 256;
  hipLaunchKernelGGL(eig_cheby_kernel, dim3((unsigned)(blocksPerSeg * nseg)), dim3(256), 0, computeStream(), out, tm1, tm2, atm2, d3, d2, d1, segC, segStride / 2, blocksPerSeg);
  HIP_CHECK(hipGetLastError());
}

void eigKernelsEnd() {
  using namespace eig;
  if (d_part) (void)hipFree(d_part);
  if (d_coef) { (void)hipFree(d_coef); (void)hipFree(d_Q); (void)hipFree(d_count); }
  d_part = d_coef = d_Q = nullptr; d_count = nullptr; partDoubles = 0;
}

}  // namespace quda
