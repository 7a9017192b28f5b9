// transfer_setup.hip — building and inspecting V (see transfer.h; R and P of the solve phase: transfer.hip): the fill from the null vectors, block orthonormalisation
// (CholeskyQR2, Gram-Schmidt), the site map of the aggregates, the fp16 mirror, single columns of V and the direct Galerkin product on the matrix cores.
#include "transfer_device.h"
#include "device_io.h"   // pk:: packed fp32 complex arithmetic

#include <cstring>

namespace quda {

// ---- V fill + block Gram-Schmidt ----
struct VecList { const float *ev[kMaxVec]; const float *od[kMaxVec]; };

template <int NV> __global__ void fillv_kernel(float *V, VecList B, int stride, int Vh, const int *block_to_fine, int blockVol, int K, int nvec, long total) {
  const long t = blockIdx.x * (long)blockDim.x + threadIdx.x;  // over (A, b)
  if (t >= total) return;
  const long A = t / blockVol;
  const int b = (int)(t - A * blockVol);
  const int f = block_to_fine[t];
  const int parity = f >= Vh, x = f - parity * Vh;
  if (NV == 4 && K % 2 == 0) {
    // 16-byte reads (two components of one vector share a plane entry) and 16-byte writes (the two vectors of a pair share a V entry)
    float4 *V4 = reinterpret_cast<float4 *>(V);
    for (int vp = 0; vp < nvec / 2; vp++) {
      const float4 *b0 = reinterpret_cast<const float4 *>(parity ? B.od[2 * vp] : B.ev[2 * vp]);
      const float4 *b1 = reinterpret_cast<const float4 *>(parity ? B.od[2 * vp + 1] : B.ev[2 * vp + 1]);
      for (int m = 0; m < K / 2; m++) {
        const float4 u = b0[(size_t)m * stride + x], w = b1[(size_t)m * stride + x];
        V4[(((size_t)A * K + 2 * m) * (nvec / 2) + vp) * blockVol + b] = make_float4(u.x, u.y, w.x, w.y);
        V4[(((size_t)A * K + 2 * m + 1) * (nvec / 2) + vp) * blockVol + b] = make_float4(u.z, u.w, w.z, w.w);
      }
    }
    return;
  }
  for (int v = 0; v < nvec; v++) {
    const float *base = parity ? B.od[v] : B.ev[v];
    for (int k = 0; k < K; k++) {
      const size_t i = fidx<NV>(stride, x, k);
      const size_t o = ((((size_t)A * K + k) * (nvec / 2) + v / 2) * blockVol + b) * 4 + (v & 1) * 2;
      V[o] = base[i]; V[o + 1] = base[i + 1];
    }
  }
}

__device__ __forceinline__ double2 block_sum2d(double2 v, double2 *lds) {
  for (int off = 32; off > 0; off >>= 1) { v.x += __shfl_down(v.x, off, 64); v.y += __shfl_down(v.y, off, 64); }
  const int wave = threadIdx.x >> 6, nw = (blockDim.x + 63) >> 6;
  __syncthreads();
  if ((threadIdx.x & 63) == 0) lds[wave] = v;
  __syncthreads();
  double2 r = lds[0];
  for (int w = 1; w < nw; w++) { r.x += lds[w].x; r.y += lds[w].y; }
  return r;
}

// modified Gram-Schmidt over the nvec vectors of one (aggregate, chirality) block, sums in fp64
// (reference blockGramSchmidt, lib/transfer_util.cu:328-363)
__global__ void block_gs_kernel(float *V, int blockVol, int K, int ncf, int spin_bs, int nvec, const int *only) {
  if (only && !only[blockIdx.x]) return;   // fall-back of the CholeskyQR kernel: just the blocks it flagged
  __shared__ double2 lds[16];
  const int A = blockIdx.x >> 1, chi = blockIdx.x & 1;
  const int Kc = K / 2, n = Kc * blockVol;
  // element e of this block -> (k, b)
  auto addr = [&](int e, int v) -> size_t {
    const int kk = e / blockVol, b = e - kk * blockVol;
    // the kk-th fine spin-colour index whose chirality is chi
    const int nsc = spin_bs * ncf;             // spin-colour values per chirality are contiguous in k = s*ncf + c
    const int k = chi * nsc + kk;
    return ((((size_t)A * K + k) * (nvec / 2) + v / 2) * blockVol + b) * 4 + (v & 1) * 2;
  };
  for (int jc = 0; jc < nvec; jc++) {
    for (int ic = 0; ic < jc; ic++) {
      double2 dot = make_double2(0.0, 0.0);
      for (int e = threadIdx.x; e < n; e += blockDim.x) {
        const size_t ai = addr(e, ic), aj = addr(e, jc);
        const double ar = V[ai], aim = V[ai + 1], br = V[aj], bim = V[aj + 1];
        dot.x += ar * br + aim * bim; dot.y += ar * bim - aim * br;
      }
      dot = block_sum2d(dot, lds);
      for (int e = threadIdx.x; e < n; e += blockDim.x) {
        const size_t ai = addr(e, ic), aj = addr(e, jc);
        const double ar = V[ai], aim = V[ai + 1];
        V[aj] = (float)(V[aj] - (dot.x * ar - dot.y * aim));
        V[aj + 1] = (float)(V[aj + 1] - (dot.x * aim + dot.y * ar));
      }
      __syncthreads();
    }
    double2 nrm = make_double2(0.0, 0.0);
    for (int e = threadIdx.x; e < n; e += blockDim.x) { const size_t aj = addr(e, jc); nrm.x += (double)V[aj] * V[aj] + (double)V[aj + 1] * V[aj + 1]; }
    nrm = block_sum2d(nrm, lds);
    const float scale = nrm.x > 0.0 ? (float)(1.0 / sqrt(nrm.x)) : 0.f;
    for (int e = threadIdx.x; e < n; e += blockDim.x) { const size_t aj = addr(e, jc); V[aj] *= scale; V[aj + 1] *= scale; }
    __syncthreads();
  }
}

// ---- CholeskyQR: the same block orthonormalisation in two passes over the block instead of nvec (nvec - 1) / 2 -----------------
// Q R = V with R upper triangular and a positive diagonal is unique, so Q = V R^-1 with R from the Cholesky factorisation of the
// Gram matrix G = V^dagger V (= R^dagger R) IS the Gram-Schmidt result — but G needs one sweep over the block (all 300 inner
// products of 24 vectors at once, fp64 sums, the block staged through LDS in chunks of 256 elements) and V R^-1 a second one,
// where modified Gram-Schmidt makes 276 dependent sweeps with two block reductions each (0.44 - 0.6 s at 48^3 x 96).  Run twice
// (CholeskyQR2): the second round removes the orthogonality the first one loses to the conditioning of the block — as long as
// eps cond(V)^2 < 1 with the eps of the Gram matrix, which is fp32 here (V is fp32 and a chunk's 256-term sum is fp32: ~1e-6
// relative).  Two guards, both matched to that precision: a Cholesky pivot below kQrPivot x G_jj is round-off, not data, and a
// first-round result whose Gram matrix is further than kQrRound2 from the identity is beyond what the second round repairs.  A block
// that trips either one is flagged and goes to the Gram-Schmidt kernel — that block only; what the first round may already have
// written is V T with T upper triangular with a positive diagonal, which has the same Q.
// Reference semantics: blockGramSchmidt, lib/transfer_util.cu:328-363.
constexpr int kQrChunk = 256;
constexpr double kQrPivot = 1e-5, kQrRound2 = 5e-2;
template <int NVEC> __global__ void __launch_bounds__(256) block_cholqr_kernel(float *V, int blockVol, int K, int ncf, int spin_bs, int *failed, int *failedBlock) {
  constexpr int nvec = NVEC;
  extern __shared__ double smem[];
  // layout: tile [kQrChunk][nvec + 1] float2 | G / L [nvec][nvec] double2 | Rinv [nvec][nvec] float2 | flag
  float2 *tile = reinterpret_cast<float2 *>(smem);
  constexpr int tstride = nvec + 1;
  double2 *G = reinterpret_cast<double2 *>(tile + (size_t)kQrChunk * tstride + (kQrChunk * tstride & 1));
  float2 *Rinv = reinterpret_cast<float2 *>(G + nvec * nvec);
  int *bad = reinterpret_cast<int *>(Rinv + nvec * nvec);
  const int A = blockIdx.x >> 1, chi = blockIdx.x & 1;
  const int Kc = K / 2, n = Kc * blockVol, nsc = spin_bs * ncf;
  constexpr int nvp = nvec / 2, npairs = nvec * (nvec + 1) / 2;
  auto addr4 = [&](int e, int vp) -> size_t {   // float4 index of (element e, vector pair vp)
    const int kk = e / blockVol, b = e - kk * blockVol;
    return (((size_t)A * K + chi * nsc + kk) * nvp + vp) * blockVol + b;
  };
  float4 *V4 = reinterpret_cast<float4 *>(V);
  if (threadIdx.x == 0) *bad = 0;
  for (int round = 0; round < 2; round++) {
    // ---- Gram matrix: pair p = (i <= j) per thread (up to 3 pairs for nvec = 32) ----
    int pi[3], pj[3];
    double2 acc[3];
#pragma unroll
    for (int q = 0; q < 3; q++) {
      const int p = threadIdx.x + 256 * q;
      acc[q] = make_double2(0.0, 0.0);
      pi[q] = pj[q] = -1;
      if (p < npairs) {   // row-major enumeration of the upper triangle
        int i = 0, rem = p;
        while (rem >= nvec - i) { rem -= nvec - i; i++; }
        pi[q] = i; pj[q] = i + rem;
      }
    }
    for (int c0 = 0; c0 < n; c0 += kQrChunk) {
      __syncthreads();
      const int e = c0 + threadIdx.x;
#pragma unroll
      for (int vp = 0; vp < nvp; vp++) {
        const float4 w = e < n ? V4[addr4(e, vp)] : make_float4(0.f, 0.f, 0.f, 0.f);
        tile[threadIdx.x * tstride + 2 * vp] = make_float2(w.x, w.y);
        tile[threadIdx.x * tstride + 2 * vp + 1] = make_float2(w.z, w.w);
      }
      __syncthreads();
#pragma unroll
      for (int q = 0; q < 3; q++) {
        if (pi[q] < 0) continue;
        // fp32 inside a chunk (packed: conj(a) b = two v_pk_fma_f32), fp64 across the chunks: the per-term conversions and fp64
        // multiply-adds made this loop the most expensive part of the kernel (59.5 ms per pass at 48^3 x 96); a chunk's 256-term
        // sum is good to ~1e-6 relative, the second CholeskyQR round and the fp64 chunk sums keep the result at fp32 round-off
        pkf2 part = {0.f, 0.f};
        for (int t = 0; t < kQrChunk; t++) {
          const float2 a = tile[t * tstride + pi[q]], b = tile[t * tstride + pj[q]];
          part = pk::cmac_conj(part, (pkf2){a.x, a.y}, (pkf2){b.x, b.y});
        }
        acc[q].x += (double)part.x; acc[q].y += (double)part.y;
      }
    }
#pragma unroll
    for (int q = 0; q < 3; q++)
      if (pi[q] >= 0) {
        G[pi[q] * nvec + pj[q]] = acc[q]; G[pj[q] * nvec + pi[q]] = make_double2(acc[q].x, -acc[q].y);
        // second round: the first one must have left something close to orthonormal
        if (round == 1 && (fabs(acc[q].x - (pi[q] == pj[q] ? 1.0 : 0.0)) > kQrRound2 || fabs(acc[q].y) > kQrRound2)) *bad = 1;
      }
    __syncthreads();
    if (*bad) break;
    // ---- Cholesky G = L L^dagger in place (lower triangle), column by column; thread i owns row i ----
    for (int j = 0; j < nvec; j++) {
      if ((int)threadIdx.x == j) {
        double d = G[j * nvec + j].x;
        for (int k = 0; k < j; k++) { const double2 l = G[j * nvec + k]; d -= l.x * l.x + l.y * l.y; }
        if (!(d > kQrPivot * G[j * nvec + j].x) || !(d > 0.0)) { *bad = 1; d = 1.0; }
        G[j * nvec + j] = make_double2(sqrt(d), 0.0);
      }
      __syncthreads();
      const int i = threadIdx.x;
      if (i > j && i < nvec) {
        double2 v = G[i * nvec + j];
        for (int k = 0; k < j; k++) {   // -= L[i][k] conj(L[j][k])
          const double2 a = G[i * nvec + k], b = G[j * nvec + k];
          v.x -= a.x * b.x + a.y * b.y; v.y -= a.y * b.x - a.x * b.y;
        }
        const double inv = 1.0 / G[j * nvec + j].x;
        G[i * nvec + j] = make_double2(v.x * inv, v.y * inv);
      }
      __syncthreads();
    }
    if (*bad) break;
    // ---- R = L^dagger (upper); column j of R^-1 by back substitution, thread j ----
    if ((int)threadIdx.x < nvec) {
      const int j = threadIdx.x;
      double2 x[NVEC];
#pragma unroll
      for (int i = nvec - 1; i >= 0; i--) {
        double2 v = make_double2(i == j ? 1.0 : 0.0, 0.0);
#pragma unroll
        for (int k = i + 1; k < nvec; k++) {   // R[i][k] = conj(L[k][i])
          if (k > j) continue;
          const double2 r = G[k * nvec + i];
          v.x -= r.x * x[k].x + r.y * x[k].y; v.y -= r.x * x[k].y - r.y * x[k].x;
        }
        const double inv = 1.0 / G[i * nvec + i].x;
        x[i] = i <= j ? make_double2(v.x * inv, v.y * inv) : make_double2(0.0, 0.0);
      }
#pragma unroll
      for (int i = 0; i < nvec; i++) Rinv[i * nvec + j] = make_float2((float)x[i].x, (float)x[i].y);
    }
    __syncthreads();
    // ---- V <- V R^-1: thread per element ----
    for (int c0 = 0; c0 < n; c0 += 256) {
      const int e = c0 + threadIdx.x;
      if (e >= n) continue;
      float2 v[NVEC];
#pragma unroll
      for (int vp = 0; vp < nvp; vp++) { const float4 w = V4[addr4(e, vp)]; v[2 * vp] = make_float2(w.x, w.y); v[2 * vp + 1] = make_float2(w.z, w.w); }
#pragma unroll
      for (int vp = nvp - 1; vp >= 0; vp--) {   // columns from the right: column j only needs v[0..j], so v can be overwritten in place
        float2 o[2];
#pragma unroll
        for (int h = 1; h >= 0; h--) {
          const int j = 2 * vp + h;
          pkf2 a = {0.f, 0.f};
#pragma unroll
          for (int i = 0; i <= j; i++) { const float2 r = Rinv[i * nvec + j]; a = pk::cmac(a, (pkf2){v[i].x, v[i].y}, (pkf2){r.x, r.y}); }
          o[h] = make_float2(a.x, a.y);
        }
        v[2 * vp] = o[0]; v[2 * vp + 1] = o[1];
        V4[addr4(e, vp)] = make_float4(o[0].x, o[0].y, o[1].x, o[1].y);
      }
    }
    __syncthreads();
  }
  if (threadIdx.x == 0 && *bad) { atomicAdd(failed, 1); failedBlock[blockIdx.x] = 1; }
}

// ================================================================================================
// Direct Galerkin construction, step 2 ("VUV", reference ComputeVUV lib/coarse_op.cuh:487-600) on the matrix cores: for one forward
// direction mu and every aggregate A
//     Y[(chi, v)][(chi', v')] = sum_{x in A} sum_{s in chi, c} conj(V(x)[s, c; v]) [ (1 - gamma_mu) UV(x) ]^{chi'}[s, c; v']      (UV from galerkin_uv_kernel)
// — the sites whose mu-neighbour lies in the next aggregate give the coarse link Y_{2 mu}(A), all others the part S(A) of the local
// matrix (hermitian completion by the caller, coarse.hip).  The probing path gets the same numbers from 2 Nvec passes over V with a
// block reduction per coefficient; here the sum over the 256 sites of the aggregate IS the K dimension of a GEMM:
// per row block chi a real GEMM  M = Nvec rows (v; padded to 16 / 32), N = 4 Nvec real columns ((chi', v') x re / im), K = 256 x 6 x 2
// on v_mfma_f32_16x16x4_f32 (exact fp32).  The projector is applied on the fly: a column of chirality chi' = chi sees UV[s, c] itself, one of the
// other chirality phi(mu, s) UV[partner(mu, s), c] with phi in {+-1, +-i} (table below, read off spin_project / spin_reconstruct of dslash.hip).
// One work-group per aggregate, 8 waves: wave = 4 chi + w takes row block chi of the 64 sites with block coordinate y_mu = w, so the
// class-3 waves hold the link and classes 0..2 the local part without any masking.  A k-step is 4 sites of one (spin-colour, re/im):
//     A operand  lane (row v, kq): Re or Im of V(x_kq)[s, c; v]                      one 8-byte load serves the re and the im step
//     B operand  lane (col (j, o), kq): from w = phi UV(x_kq)[s', c; v'(j)] = (wr, wi):   re step: o ? wi : wr     im step: o ? -wr : wi
// so that column (j, re) collects Vr Wr + Vi Wi and (j, im) Vr Wi - Vi Wr, i.e. conj(V) W.  Operands come straight from global memory
// (every 16-byte word of the aggregate's V / UV rows is used by lanes of the work-group within microseconds: L1 / L2 absorb the pieces);
// partial tiles are summed through LDS and written in the link layout [site][matrix][column pair][row] float4.
// local = 1: UV is a chirality-diagonal site term (twisted clover, galerkin_local_uv_kernel): no cross columns, every class is local.
// Fine level only: 4 x 3 spin-colour, 4^4 aggregates, Nvec 8, 24 or 32, unpartitioned.
// ================================================================================================
typedef float gf32x4 __attribute__((ext_vector_type(4)));
// forward hop (1 - gamma_mu) in the chiral basis of dslash.hip: row s of the OTHER chirality's contribution is i^k UV[partner]
__device__ __constant__ int kGalPartner[4][4] = {{3, 2, 1, 0}, {3, 2, 1, 0}, {2, 3, 0, 1}, {2, 3, 0, 1}};
__device__ __constant__ int kGalPhase[4][4] = {{3, 3, 1, 1}, {0, 2, 2, 0}, {3, 1, 1, 3}, {2, 2, 2, 2}};
// the K loop of one wave (row block CHI, its class of 64 sites).  Branch-free on purpose: the first version selected same / cross rows, the
// phase and the padding rows with conditionals, which the compiler turned into ~300 branches with an s_waitcnt vmcnt(0) behind every load —
// 37 ms per direction at 48^3 x 96, no faster with two work-groups per CU.  Here every lane multiplies what it loads by a complex
// constant fixed before the loop: i^(3 o) for a column of the wave's own chirality (o: the lane's real / imaginary column), i^(phase + 3 o)
// for the other chirality (0 in local mode), 0 for a padding row of A — so that (bre, bim) = c w and the two MFMA steps follow.
template <int NVEC, int CHI, typename SiteB>
__device__ __forceinline__ void galerkin_vuv_accumulate(gf32x4 (&acc)[(NVEC + 15) / 16][NVEC / 4], const float2 *V, const float2 *UV, int A, int Aloc, int mu, int local, int row16, int kq, SiteB site_b, int cmBase) {
  constexpr int NVP = NVEC / 2, MT = (NVEC + 15) / 16, NT = NVEC / 4, BV = 256;
#pragma unroll
  for (int mt = 0; mt < MT; mt++)
#pragma unroll
    for (int nt = 0; nt < NT; nt++) acc[mt][nt] = (gf32x4){0.f, 0.f, 0.f, 0.f};
  const int o = row16 & 1;
  // i^k as (re, im)
  auto ipow = [](int k) -> float2 { k &= 3; return make_float2(k == 0 ? 1.f : (k == 2 ? -1.f : 0.f), k == 1 ? 1.f : (k == 3 ? -1.f : 0.f)); };
  const float2 cSame = ipow(3 * o);
  float2 cCross[2];
#pragma unroll
  for (int h = 0; h < 2; h++) {
    cCross[h] = ipow(kGalPhase[mu][2 * CHI + h] + 3 * o);
    if (local) cCross[h] = make_float2(0.f, 0.f);
  }
  // per-lane element offsets (float2 units) inside a (spin-colour) row of the aggregate: A rows v = 16 mt + row16 (padding rows: clamped, scaled by 0)
  int aOff[MT]; float aScale[MT];
#pragma unroll
  for (int mt = 0; mt < MT; mt++) {
    const int v = 16 * mt + row16, vv = v < NVEC ? v : NVEC - 1;
    aOff[mt] = (vv >> 1) * BV * 2 + (vv & 1);
    aScale[mt] = v < NVEC ? 1.f : 0.f;
  }
  int bOff[NT];
#pragma unroll
  for (int nt = 0; nt < NT; nt++) {
    const int j = 8 * nt + (row16 >> 1), vc = j - (nt >= NT / 2 ? NVEC : 0);
    bOff[nt] = (vc >> 1) * BV * 2 + (vc & 1);
  }
  const float2 *Va = V + (size_t)A * 12 * NVP * BV * 2, *Ua = UV + (size_t)Aloc * 12 * NVP * BV * 2;
  constexpr int ROW = NVP * BV * 2;   // float2 elements per (spin-colour) row
  // spin-colour row outermost, the wave's 64 sites (16 k-steps of 4) inside: with UV in class-major order (cmBase >= 0: the wave's sites are entries
  // cmBase .. cmBase + 63 of every UV row) consecutive k-steps read consecutive 64-byte pieces — every 128-byte line of UV is fetched once
#pragma unroll
  for (int s6 = 0; s6 < 6; s6++) {
    for (int g = 0; g < 16; g++) {
      const int b2 = 2 * site_b(4 * g + kq), u2 = cmBase >= 0 ? 2 * (cmBase + 4 * g + kq) : b2;
      {
      const int spin = 2 * CHI + s6 / 3, col = s6 % 3;
      const int rowSame = (3 * spin + col) * ROW, rowCross = (3 * kGalPartner[mu][spin] + col) * ROW;
      float are[MT], aim[MT], bre[NT], bim[NT];
#pragma unroll
      for (int mt = 0; mt < MT; mt++) {
        const float2 a = Va[rowSame + aOff[mt] + b2];
        are[mt] = aScale[mt] * a.x; aim[mt] = aScale[mt] * a.y;
      }
#pragma unroll
      for (int nt = 0; nt < NT; nt++) {
        constexpr int dummy = 0; (void)dummy;
        const bool same = (nt >= NT / 2) == (CHI == 1);
        const float2 w = Ua[(same ? rowSame : rowCross) + bOff[nt] + u2];
        const float2 c = same ? cSame : cCross[s6 / 3];
        bre[nt] = c.x * w.x - c.y * w.y;
        bim[nt] = c.x * w.y + c.y * w.x;
      }
      // all re steps, then all im steps: consecutive matrix instructions on different accumulators
#pragma unroll
      for (int mt = 0; mt < MT; mt++)
#pragma unroll
        for (int nt = 0; nt < NT; nt++) acc[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(are[mt], bre[nt], acc[mt][nt], 0, 0, 0);
#pragma unroll
      for (int mt = 0; mt < MT; mt++)
#pragma unroll
        for (int nt = 0; nt < NT; nt++) acc[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(aim[mt], bim[nt], acc[mt][nt], 0, 0, 0);
      }
    }
  }
}
template <int NVEC> __global__ void __launch_bounds__(512) galerkin_vuv_kernel(float *G, const float2 *V, const float2 *UV, int mu, int accumulateLocal, int pm, int local, int aggOffset, int classMajor) {
  constexpr int NVP = NVEC / 2, MT = (NVEC + 15) / 16, NT = NVEC / 4, n = 2 * NVEC, BV = 256;
  extern __shared__ float glds[];   // [class][mt][nt][reg][lane], one row block at a time
  const int A = blockIdx.x + aggOffset, lane = threadIdx.x & 63;   // UV holds the aggregates [aggOffset, aggOffset + gridDim) only
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int cls = wave & 3, chiR = wave >> 2;
  const int row16 = lane & 15, kq = lane >> 4;
  // site list of this wave: y_mu = cls, the other three coordinates from pos = 0 .. 63; b = place of the site inside the aggregate
  auto site_b = [&](int pos) -> int {
    int y[4], q = pos;
    for (int d = 0; d < 4; d++) if (d != mu) { y[d] = q & 3; q >>= 2; }
    y[mu] = cls;
    const int lex = ((y[3] * 4 + y[2]) * 4 + y[1]) * 4 + y[0];
    return pm ? ((y[0] + y[1] + y[2] + y[3]) & 1) * (BV / 2) + (lex >> 1) : lex;
  };
  gf32x4 acc[MT][NT];
  const int cmBase = classMajor ? cls * 64 : -1;
  if (chiR == 0) galerkin_vuv_accumulate<NVEC, 0>(acc, V, UV, A, (int)blockIdx.x, mu, local, row16, kq, site_b, cmBase);
  else galerkin_vuv_accumulate<NVEC, 1>(acc, V, UV, A, (int)blockIdx.x, mu, local, row16, kq, site_b, cmBase);
  // ---- partial tiles -> LDS, one row block (chi) at a time so that the buffer is 4 waves x 12 KB and two work-groups share a CU;
  // classes 0..2 summed = local part, class 3 = link ----
  constexpr int TILE = MT * NT * 4 * 64;   // floats per wave
  float4 *G4 = reinterpret_cast<float4 *>(G);
  for (int chi = 0; chi < 2; chi++) {
    if (chi) __syncthreads();
    if (chiR == chi) {
#pragma unroll
      for (int mt = 0; mt < MT; mt++)
#pragma unroll
        for (int nt = 0; nt < NT; nt++)
#pragma unroll
          for (int r = 0; r < 4; r++) glds[cls * TILE + ((mt * NT + nt) * 4 + r) * 64 + lane] = acc[mt][nt][r];
    }
    __syncthreads();
    // output element (row i = (chi, v), complex column j): tile (v / 16, j / 8); D layout: row = 4 (lane / 16) + reg, col = lane & 15
    // local (site-diagonal term of the fine operator): every class belongs to the local matrix, no link is written
    constexpr int HALF = NVEC * (n / 2);   // (row v, column pair) elements of one row block
    for (int e = threadIdx.x + (local ? HALF : 0); e < 2 * HALF; e += blockDim.x) {
      const int which = e / HALF, r2 = e - which * HALF;   // 0: link (class 3), 1: local (classes 0..2)
      const int jp = r2 / NVEC, v = r2 - jp * NVEC, i = chi * NVEC + v, mt = v >> 4, rr = v & 15;
      float val[4];
#pragma unroll
      for (int h = 0; h < 2; h++) {
        const int j = 2 * jp + h, nt = j >> 3;
#pragma unroll
        for (int oo = 0; oo < 2; oo++) {
          const int col = 2 * (j & 7) + oo;
          const int off = ((mt * NT + nt) * 4 + (rr & 3)) * 64 + (rr >> 2) * 16 + col;
          val[2 * h + oo] = which ? glds[off] + glds[TILE + off] + glds[2 * TILE + off] + (local ? glds[3 * TILE + off] : 0.f) : glds[3 * TILE + off];
        }
      }
      const size_t dst = (((size_t)A * 9 + (which ? 8 : 2 * mu)) * (n / 2) + jp) * n + i;
      if (which && accumulateLocal) { const float4 old = G4[dst]; val[0] += old.x; val[1] += old.y; val[2] += old.z; val[3] += old.w; }
      G4[dst] = make_float4(val[0], val[1], val[2], val[3]);
    }
  }
}

bool Transfer::canDirectGalerkin() const {
  static int off = -1;
  if (off < 0) { const char *e = getenv("QUDA_AMD_GALERKIN_DIRECT"); off = (e && !atoi(e)) ? 1 : 0; }
  if (off || fineSpin != 4 || fineColor != 3 || spin_bs != 2 || (Nvec != 8 && Nvec != 24 && Nvec != 32)) return false;
  for (int d = 0; d < 4; d++) if (geo_bs[d] != 4 || Xc[d] == 1 || commGrid().partitioned(d)) return false;
  return true;
}
// forward link Y_{2 mu} and the in-aggregate part S of all coarse sites from UV = galerkinUV(V): slots 2 mu and 8 of the coarse links
void Transfer::directGalerkinVUV(float *links, const float *UV, int mu, bool accumulateLocal, bool local, int aggOffset, int nAggChunk, bool classMajor) const {
  if (!canDirectGalerkin()) errorQuda("direct Galerkin construction not available for this transfer operator");
  const size_t lds = (size_t)4 * ((Nvec + 15) / 16) * (Nvec / 4) * 4 * 64 * sizeof(float);
#define QA_VUV(NV) { static bool attr = false; \
    if (!attr) { HIP_CHECK(hipFuncSetAttribute((const void *)galerkin_vuv_kernel<NV>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds)); attr = true; } \
    hipLaunchKernelGGL((galerkin_vuv_kernel<NV>), dim3(nAggChunk > 0 ? nAggChunk : (int)nAgg), dim3(512), lds, computeStream(), links, (const float2 *)V, (const float2 *)UV, mu, accumulateLocal ? 1 : 0, parityMajor ? 1 : 0, local ? 1 : 0, aggOffset, classMajor ? 1 : 0); }
  if (Nvec == 24) QA_VUV(24) else if (Nvec == 32) QA_VUV(32) else QA_VUV(8)
#undef QA_VUV
  HIP_CHECK(hipGetLastError());
}

// ================================================================================================
Transfer::Transfer(const std::vector<ColorSpinorField *> &B, int Nvec_, int *gbs, int spin_bs_)
    : Nvec(Nvec_), spin_bs(spin_bs_), V(nullptr), V_h(nullptr), block_to_fine(nullptr), fine_to_block(nullptr), flops_(0),
      site_subset(QUDA_FULL_SITE_SUBSET), subset_parity(QUDA_INVALID_PARITY) {
  if ((int)B.size() < Nvec) errorQuda("need %d null vectors, got %zu", Nvec, B.size());
  if (Nvec % 2 || Nvec > kMaxVec) errorQuda("Nvec = %d must be even and <= %d", Nvec, kMaxVec);
  const ColorSpinorField &b0 = *B[0];
  if (b0.SiteSubset() != QUDA_FULL_SITE_SUBSET) errorQuda("null vectors must be full fields");
  fineSpin = b0.Nspin(); fineColor = b0.Ncolor();
  if (fineSpin % spin_bs || fineSpin / spin_bs != 2) errorQuda("spin block %d does not leave two chiralities from %d spins", spin_bs, fineSpin);
  for (int d = 0; d < 4; d++) Xf[d] = b0.X(d);
  // block-size fallback, reference lib/transfer.cpp:31-44
  for (int d = 0; d < 4; d++) {
    while (gbs[d] > 0) {
      if (d == 0 && Xf[0] == gbs[0]) warningQuda("X-dimension length %d cannot block length %d", Xf[0], gbs[0]);
      else if ((Xf[d] / gbs[d] + 1) % 2 == 0) warningQuda("Indexing does not (yet) support odd coarse dimensions: X(%d) = %d", d, Xf[d] / gbs[d]);
      else if ((Xf[d] / gbs[d]) * gbs[d] != Xf[d]) warningQuda("cannot block dim[%d]=%d with block size = %d", d, Xf[d], gbs[d]);
      else break;
      gbs[d] /= 2;
    }
    if (gbs[d] == 0) errorQuda("Unable to block dimension %d", d);
  }
  blockVol = 1; nAgg = 1; fineVol = 1;
  for (int d = 0; d < 4; d++) { geo_bs[d] = gbs[d]; Xc[d] = Xf[d] / gbs[d]; blockVol *= gbs[d]; nAgg *= Xc[d]; fineVol *= Xf[d]; }
  if (blockVol == 1) errorQuda("Total geometric block size is 1");
  if (blockVol > 1024) errorQuda("aggregate of %d sites exceeds one work-group", blockVol);
  if (getVerbosity() >= QUDA_VERBOSE) printfQuda("Transfer: using block size %d x %d x %d x %d\n", geo_bs[0], geo_bs[1], geo_bs[2], geo_bs[3]);
  // order of the sites inside an aggregate: parity-major on the finest level when every block extent is even (transfer_device.h block_coords)
  {
    static int pmEnv = -1;
    if (pmEnv < 0) { const char *e = getenv("QUDA_AMD_V_PARITY_MAJOR"); pmEnv = e ? atoi(e) : 1; }
    parityMajor = pmEnv && fineSpin == 4 && geo_bs[0] % 2 == 0 && geo_bs[1] % 2 == 0 && geo_bs[2] % 2 == 0 && geo_bs[3] % 2 == 0;
  }
  createGeoMap();
  // through the device pool: the next hierarchy (the other twist flavour, a refinement pass) takes the same 24.5 GB at 48^3 x 96 instead of
  // a fresh hipMalloc + hipFree pair (~0.1 s, and the first touch of fresh pages slows every kernel that meets them)
  V = (float *)poolDeviceMalloc(vBytes());
  fillAndOrthonormalise(B);
}

__global__ void v_to_half_kernel(vhalf4_t *out, const float4 *in, size_t n) {
  const size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float4 v = in[i];
  vhalf4_t h;
  h.x = (_Float16)v.x; h.y = (_Float16)v.y; h.z = (_Float16)v.z; h.w = (_Float16)v.w;
  out[i] = h;
}
void Transfer::makeHalf() const {
  if (V_h) return;
  const size_t n4 = vBytes() / sizeof(float4);
  V_h = poolDeviceMalloc(n4 * sizeof(vhalf4_t));
  hipLaunchKernelGGL(v_to_half_kernel, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, computeStream(), (vhalf4_t *)V_h, (const float4 *)V, n4);
  HIP_CHECK(hipGetLastError());
}

Transfer::~Transfer() {
  if (V_h) poolDeviceFree(V_h, 0);
  if (V) poolDeviceFree(V, 0);
  if (block_to_fine) poolDeviceFree(block_to_fine, 0);
  if (fine_to_block) poolDeviceFree(fine_to_block, 0);
}

// reference createGeoMap lib/transfer.cpp:220-258 (fine site -> coarse site), plus the position inside the aggregate
struct GeoMapArg { int Xf[4], Xc[4], bs[4], blockVol, pm; long Vh, Vhc; };
__global__ void geo_map_kernel(int *b2f, int *f2b, GeoMapArg a) {
  const long f = blockIdx.x * (long)blockDim.x + threadIdx.x;
  if (f >= 2 * a.Vh) return;
  const int parity = f >= a.Vh;
  const long i = f - parity * a.Vh;
  const long za = i / (a.Xf[0] / 2); const int xh = (int)(i - za * (a.Xf[0] / 2));
  const long zb = za / a.Xf[1]; const int y = (int)(za - zb * a.Xf[1]);
  const int t = (int)(zb / a.Xf[2]), z = (int)(zb - (long)t * a.Xf[2]);
  const int x[4] = {2 * xh + ((y + z + t + parity) & 1), y, z, t};
  int xc[4], yb[4];
  for (int d = 0; d < 4; d++) { xc[d] = x[d] / a.bs[d]; yb[d] = x[d] % a.bs[d]; }
  const int cpar = (xc[0] + xc[1] + xc[2] + xc[3]) & 1;
  const long clex = ((long)(xc[3] * a.Xc[2] + xc[2]) * a.Xc[1] + xc[1]) * a.Xc[0] + xc[0];
  const long A = cpar * a.Vhc + clex / 2;
  int b = ((yb[3] * a.bs[2] + yb[2]) * a.bs[1] + yb[1]) * a.bs[0] + yb[0];
  if (a.pm) b = ((yb[0] + yb[1] + yb[2] + yb[3]) & 1) * (a.blockVol / 2) + b / 2;   // block extents even: site parity = block-local parity
  b2f[A * a.blockVol + b] = (int)f;
  f2b[f] = (int)(A * a.blockVol + b);
}
void Transfer::createGeoMap() {
  // on the device (round 3): the host loop over 10.6 M sites and its two 42 MB copies cost ~0.1 s of every build at 48^3 x 96
  GeoMapArg a;
  for (int d = 0; d < 4; d++) { a.Xf[d] = Xf[d]; a.Xc[d] = Xc[d]; a.bs[d] = geo_bs[d]; }
  a.blockVol = blockVol; a.pm = parityMajor ? 1 : 0; a.Vh = fineVol / 2; a.Vhc = nAgg / 2;
  block_to_fine = (int *)poolDeviceMalloc(fineVol * sizeof(int));
  fine_to_block = (int *)poolDeviceMalloc(fineVol * sizeof(int));
  hipLaunchKernelGGL(geo_map_kernel, dim3((unsigned)((fineVol + 255) / 256)), dim3(256), 0, computeStream(), block_to_fine, fine_to_block, a);
  HIP_CHECK(hipGetLastError());
}

void Transfer::fillAndOrthonormalise(const std::vector<ColorSpinorField *> &B) {
  VecList vl;
  memset(&vl, 0, sizeof(vl));
  for (int v = 0; v < Nvec; v++) { const FineVec f = fineVec(*B[v]); vl.ev[v] = f.v[0]; vl.od[v] = f.v[1]; }
  const FineVec f0 = fineVec(*B[0]);
  const long total = fineVol;
  const int K = fineSpin * fineColor;
  if (fineSpin == 4) hipLaunchKernelGGL((fillv_kernel<4>), dim3((total + 255) / 256), dim3(256), 0, computeStream(), V, vl, f0.stride, f0.Vh, block_to_fine, blockVol, K, Nvec, total);
  else hipLaunchKernelGGL((fillv_kernel<2>), dim3((total + 255) / 256), dim3(256), 0, computeStream(), V, vl, f0.stride, f0.Vh, block_to_fine, blockVol, K, Nvec, total);
  HIP_CHECK(hipGetLastError());
  static int useQr = -1;
  if (useQr < 0) { const char *e = getenv("QUDA_AMD_BLOCK_ORTHO"); useQr = (e && !strcmp(e, "gs")) ? 0 : 1; }
  int nfail = useQr ? 0 : 1;
  lastGsFallbackBlocks = 0;
  if (useQr) {
    int *d_fail = nullptr;   // [0] number of flagged blocks, [1 + b] flag of (aggregate, chirality) block b
    const size_t failBytes = (1 + 2 * (size_t)nAgg) * sizeof(int);
    d_fail = (int *)poolDeviceMalloc(failBytes);
    HIP_CHECK(hipMemsetAsync(d_fail, 0, failBytes, computeStream()));
    const size_t tileFloats2 = (size_t)kQrChunk * (Nvec + 1) + 1;
    const size_t lds = tileFloats2 * sizeof(float2) + (size_t)Nvec * Nvec * (sizeof(double2) + sizeof(float2)) + 64;
#define QA_QR(NV)                                                                                                                  \
  {                                                                                                                                \
    HIP_CHECK(hipFuncSetAttribute((const void *)block_cholqr_kernel<NV>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));   \
    hipLaunchKernelGGL((block_cholqr_kernel<NV>), dim3(2 * nAgg), dim3(256), lds, computeStream(), V, blockVol, K, fineColor, spin_bs, d_fail, d_fail + 1); \
  }
    switch (Nvec) {
      case 4: QA_QR(4) break;
      case 8: QA_QR(8) break;
      case 24: QA_QR(24) break;
      case 32: QA_QR(32) break;
      default: nfail = 1;   // not instantiated: Gram-Schmidt
    }
#undef QA_QR
    HIP_CHECK(hipGetLastError());
    if (!nfail) HIP_CHECK(hipMemcpyAsync(&nfail, d_fail, sizeof(int), hipMemcpyDeviceToHost, computeStream()));
    HIP_CHECK(hipStreamSynchronize(computeStream()));
    if (nfail && (Nvec == 4 || Nvec == 8 || Nvec == 24 || Nvec == 32)) {
      // flagged blocks hold their original vectors or those times an upper-triangular matrix with a positive diagonal (first round done,
      // second refused): the same Q either way, so the sequential kernel runs on exactly those blocks, in place
      if (getVerbosity() >= QUDA_SUMMARIZE) printfQuda("block orthonormalisation: %d of %ld blocks too ill-conditioned for CholeskyQR2 in fp32, Gram-Schmidt on those\n", nfail, 2 * (long)nAgg);
      hipLaunchKernelGGL(block_gs_kernel, dim3(2 * nAgg), dim3(256), 0, computeStream(), V, blockVol, K, fineColor, spin_bs, Nvec, (const int *)(d_fail + 1));
      HIP_CHECK(hipGetLastError());
      HIP_CHECK(hipStreamSynchronize(computeStream()));
      lastGsFallbackBlocks = nfail;
      nfail = 0;
    }
    poolDeviceFree(d_fail, failBytes);
  }
  if (nfail) hipLaunchKernelGGL(block_gs_kernel, dim3(2 * nAgg), dim3(256), 0, computeStream(), V, blockVol, K, fineColor, spin_bs, Nvec, (const int *)nullptr);
  HIP_CHECK(hipGetLastError());
  HIP_CHECK(hipStreamSynchronize(computeStream()));
}

static ColorSpinorField *zeroField(int nSpin, int nColor, const int *x) {
  ColorSpinorParam p;
  p.location = QUDA_CUDA_FIELD_LOCATION;
  p.nSpin = nSpin; p.nColor = nColor;
  for (int d = 0; d < 4; d++) p.x[d] = x[d];
  p.siteSubset = QUDA_FULL_SITE_SUBSET;
  p.precision = QUDA_SINGLE_PRECISION;
  p.create = QUDA_ZERO_FIELD_CREATE;
  return new ColorSpinorField(p);
}
ColorSpinorField *Transfer::createCoarseField() const { return zeroField(2, Nvec, Xc); }
ColorSpinorField *Transfer::createFineField() const { return zeroField(fineSpin, fineColor, Xf); }

// phi = P e_j for the coarse unit vector j = (chirality, vector) at every coarse site: column j of V, copied out of the
// aggregate-major layout (1/12 of V is touched instead of the whole of it by a prolongation)
template <int NSF, int NCF, int NV>
__global__ void column_kernel(FineVec out, const float4 *V, const int *block_to_fine, int blockVol, int spin_bs, int NVEC, int j, long total) {
  constexpr int K = NSF * NCF;
  const long t = blockIdx.x * (long)blockDim.x + threadIdx.x;
  if (t >= total) return;
  const long A = t / blockVol;
  const int b = (int)(t - A * blockVol);
  const int f = block_to_fine[t];
  const int parity = f >= out.Vh, x = f - parity * out.Vh;
  float *base = out.v[parity];
  const int chi = j / NVEC, v = j - chi * NVEC;
  float2 c[K];
#pragma unroll
  for (int k = 0; k < K; k++) {
    c[k] = make_float2(0.f, 0.f);
    if ((k / NCF) / spin_bs == chi) {
      const float4 w = V[(((size_t)A * K + k) * (NVEC / 2) + (v >> 1)) * blockVol + b];
      c[k] = (v & 1) ? make_float2(w.z, w.w) : make_float2(w.x, w.y);
    }
  }
  if (NV == 4 && K % 2 == 0) {   // two components per plane entry: one 16-byte store instead of four 4-byte ones
#pragma unroll
    for (int m = 0; m < K / 2; m++) reinterpret_cast<float4 *>(base)[(size_t)m * out.stride + x] = make_float4(c[2 * m].x, c[2 * m].y, c[2 * m + 1].x, c[2 * m + 1].y);
  } else {
#pragma unroll
    for (int k = 0; k < K; k++) { const size_t i = fidx<NV>(out.stride, x, k); base[i] = c[k].x; base[i + 1] = c[k].y; }
  }
}

void Transfer::column(ColorSpinorField &fine, int j) const {
  if (fine.SiteSubset() != QUDA_FULL_SITE_SUBSET || fine.Nspin() != fineSpin || fine.Ncolor() != fineColor || fine.Volume() != fineVol) errorQuda("fine field does not match the transfer operator");
  if (j < 0 || j >= 2 * Nvec) errorQuda("coarse component %d of %d", j, 2 * Nvec);
  const FineVec out = fineVec(fine);
  const int bs = 256;
  const long total = fineVol;
  if (fineSpin == 4) hipLaunchKernelGGL((column_kernel<4, 3, 4>), dim3((unsigned)((total + bs - 1) / bs)), dim3(bs), 0, computeStream(), out, (const float4 *)V, block_to_fine, blockVol, spin_bs, Nvec, j, total);
  else {
    switch (fineColor) {
      case 4: hipLaunchKernelGGL((column_kernel<2, 4, 2>), dim3((unsigned)((total + bs - 1) / bs)), dim3(bs), 0, computeStream(), out, (const float4 *)V, block_to_fine, blockVol, spin_bs, Nvec, j, total); break;
      case 8: hipLaunchKernelGGL((column_kernel<2, 8, 2>), dim3((unsigned)((total + bs - 1) / bs)), dim3(bs), 0, computeStream(), out, (const float4 *)V, block_to_fine, blockVol, spin_bs, Nvec, j, total); break;
      case 24: hipLaunchKernelGGL((column_kernel<2, 24, 2>), dim3((unsigned)((total + bs - 1) / bs)), dim3(bs), 0, computeStream(), out, (const float4 *)V, block_to_fine, blockVol, spin_bs, Nvec, j, total); break;
      case 32: hipLaunchKernelGGL((column_kernel<2, 32, 2>), dim3((unsigned)((total + bs - 1) / bs)), dim3(bs), 0, computeStream(), out, (const float4 *)V, block_to_fine, blockVol, spin_bs, Nvec, j, total); break;
      default: errorQuda("column extraction for %d fine colours not instantiated", fineColor);
    }
  }
  HIP_CHECK(hipGetLastError());
}

}  // namespace quda
