// transfer.hip — the transfer operators of the solve phase: restrictor / prolongator kernels and the Transfer methods that launch them (see transfer.h; V: transfer_setup.hip)
#include "transfer_device.h"
#include "device_io.h"   // pk:: packed fp32 complex arithmetic

#include <cstring>
#include <type_traits>

namespace quda {

// ---- restrictor: one work-group per aggregate, one thread per fine site of it.  DUAL (Galerkin construction): the sites whose
// mask.dir neighbour leaves the aggregate go into `out`, the others into `out2`, in ONE pass over V (V is the whole cost) ----
template <int NSF, int NCF, int NVEC, int NV, bool DUAL, bool HALF = false>
__global__ void restrict_kernel(CoarseVec out, CoarseVec out2, FineVec in, const void *V, const int *block_to_fine, int blockVol, int spin_bs, MaskArg mask, AggMap amap) {
  constexpr int K = NSF * NCF;
  __shared__ float4 lds[16];
  const int A = aggregate_of_block(amap), b = threadIdx.x;
  const bool active = b < blockVol && (DUAL || mask_keep(mask, b));
  const bool outside = DUAL && b < blockVol && mask_outside(mask, b);
  float2 r[K];
  bool have = false;
  if (active) {
    const int f = block_to_fine[(size_t)A * blockVol + b];
    const int parity = f >= in.Vh, x = f - parity * in.Vh;
    const float *base = in.v[parity];
    if (base) {   // nullptr: this parity is absent from a single-parity field
      have = true;
load_fine_site<NV, K>(r, base, in.stride, x);
    }
  }
  const int cpar = A >= out.Vh, xc = A - cpar * out.Vh;
  float *ob = out.v[cpar], *ob2 = DUAL ? out2.v[cpar] : nullptr;
  for (int chi = 0; chi < 2; chi++) {
    for (int vp = 0; vp < NVEC / 2; vp++) {
      float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
      if (have) {
#pragma unroll
        for (int k = 0; k < K; k++) {
          if ((k / NCF) / spin_bs != chi) continue;
          const float4 w = load_v<HALF>(V, (((size_t)A * K + k) * (NVEC / 2) + vp) * blockVol + b);
          // conj(V) * r
          acc.x += w.x * r[k].x + w.y * r[k].y; acc.y += w.x * r[k].y - w.y * r[k].x;
          acc.z += w.z * r[k].x + w.w * r[k].y; acc.w += w.z * r[k].y - w.w * r[k].x;
        }
      }
      const int c0 = chi * NVEC + 2 * vp;
      if (DUAL) {
        const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);
        const float4 so = block_sum4(outside ? acc : zero4, lds);
        const float4 si = block_sum4(outside ? zero4 : acc, lds);
        if (threadIdx.x == 0) {
          ob[((size_t)c0 * out.stride + xc) * 2] = so.x; ob[((size_t)c0 * out.stride + xc) * 2 + 1] = so.y;
          ob[((size_t)(c0 + 1) * out.stride + xc) * 2] = so.z; ob[((size_t)(c0 + 1) * out.stride + xc) * 2 + 1] = so.w;
          ob2[((size_t)c0 * out2.stride + xc) * 2] = si.x; ob2[((size_t)c0 * out2.stride + xc) * 2 + 1] = si.y;
          ob2[((size_t)(c0 + 1) * out2.stride + xc) * 2] = si.z; ob2[((size_t)(c0 + 1) * out2.stride + xc) * 2 + 1] = si.w;
        }
      } else {
        const float4 s = block_sum4(acc, lds);
        if (threadIdx.x == 0) {
          ob[((size_t)c0 * out.stride + xc) * 2] = s.x; ob[((size_t)c0 * out.stride + xc) * 2 + 1] = s.y;
          ob[((size_t)(c0 + 1) * out.stride + xc) * 2] = s.z; ob[((size_t)(c0 + 1) * out.stride + xc) * 2 + 1] = s.w;
        }
      }
    }
  }
}

// ---- the restrictor of the solve phase (fine level, no split): the V stream without a barrier per step.  restrict_kernel above sums
// every (chirality, vector pair) step over the work-group behind two barriers with only that step's six V entries in flight: bound
// by latency, and with a single-parity source (even-odd cycle, half of the waves idle) it moved the half V in the time the full one
// takes (0.48 of the HBM roofline at 48^3 x 96 against 0.78 for full fields; fp16 V 0.30).  Here a wave keeps three steps of requests
// in flight (raw register images, converted at their use), sums four steps at a time with a reduce-scatter butterfly (17 cross-lane
// moves per four steps instead of 96) into its own LDS row, and the work-group meets at ONE barrier.  A wave without a site of the
// present parity (parity-major V) issues nothing.
template <int NSF, int NCF, int NVEC, int NV, bool HALF>
__global__ void __launch_bounds__(256) restrict_stream_kernel(CoarseVec out, FineVec in, const void *V, const int *block_to_fine, int blockVol, MaskArg mask, AggMap amap) {
  constexpr int K = NSF * NCF, KH = K / 2, NVP = NVEC / 2, NST = 2 * NVP;
  static_assert(NVP % 4 == 0 && NST <= 64, "steps are summed four at a time");
  typedef typename VRaw<HALF>::type raw_t;
  __shared__ float4 part[4][NST];   // [wave][chirality * NVP + vector pair]
  const int A = aggregate_of_block(amap), b = threadIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = (blockDim.x + 63) >> 6;
  float2 r[K];
#pragma unroll
  for (int k = 0; k < K; k++) r[k] = make_float2(0.f, 0.f);
  bool have = false;
  if (b < blockVol && mask_keep(mask, b)) {
    const int f = block_to_fine[(size_t)A * blockVol + b];
    const int parity = f >= in.Vh, x = f - parity * in.Vh;
    const float *base = in.v[parity];
    if (base) { have = true; load_fine_site<NV, K>(r, base, in.stride, x); }   // nullptr: this parity is absent from a single-parity field
  }
  if (__builtin_amdgcn_ballot_w64(have) == 0) {   // wave-uniform
    if (lane < NST) part[wave][lane] = make_float4(0.f, 0.f, 0.f, 0.f);
  } else {
    // unconditional loads (a lane without a site reads entry 0 against r = 0): a load under a per-lane condition is its own basic
    // block and the wait counts fall back to vmcnt(0)
    const int bl = b < blockVol ? b : 0;
#pragma unroll
    for (int chi = 0; chi < 2; chi++) {
      raw_t w0[KH], w1[KH], w2[KH];
      auto vload = [&](raw_t *dst, int vpl) {
        if (vpl >= NVP) return;
#pragma unroll
        for (int kk = 0; kk < KH; kk++) dst[kk] = load_v_raw<HALF>(V, (((size_t)A * K + chi * KH + kk) * NVP + vpl) * blockVol + bl);
      };
      vload(w0, 0); vload(w1, 1); vload(w2, 2);
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int g = 0; g < NVP / 4; g++) {
        float w[16];
#pragma unroll
        for (int s4 = 0; s4 < 4; s4++) {
          const int vp = 4 * g + s4, ph = vp % 3;
          float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
          for (int kk = 0; kk < KH; kk++) {
            const float4 v = v_unpack(ph == 0 ? w0[kk] : (ph == 1 ? w1[kk] : w2[kk]));
            const float2 rr = r[chi * KH + kk];
            acc.x += v.x * rr.x + v.y * rr.y; acc.y += v.x * rr.y - v.y * rr.x;   // conj(V) r
            acc.z += v.z * rr.x + v.w * rr.y; acc.w += v.z * rr.y - v.w * rr.x;
          }
          w[4 * s4] = acc.x; w[4 * s4 + 1] = acc.y; w[4 * s4 + 2] = acc.z; w[4 * s4 + 3] = acc.w;
          __builtin_amdgcn_sched_barrier(0);
          if (ph == 0) vload(w0, vp + 3); else if (ph == 1) vload(w1, vp + 3); else vload(w2, vp + 3);   // the buffer just used: three steps ahead
          __builtin_amdgcn_sched_barrier(0);
        }
#define QA_BFLY(HALFN, M)                                                                  \
        {                                                                                  \
          const bool up = (lane & M) != 0;                                                 \
          _Pragma("unroll") for (int j = 0; j < HALFN; j++) {                              \
            const float keep = up ? w[HALFN + j] : w[j], give = up ? w[j] : w[HALFN + j]; \
            w[j] = keep + __shfl_xor(give, M, 64);                                         \
          }                                                                                \
        }
        QA_BFLY(8, 1) QA_BFLY(4, 2) QA_BFLY(2, 4) QA_BFLY(1, 8)
#undef QA_BFLY
        w[0] += __shfl_xor(w[0], 16, 64);
        w[0] += __shfl_xor(w[0], 32, 64);
        if (lane < 16) {   // lane l holds the total of value index (bit-reversed l): 4 * step + component
          const int vi = ((lane & 1) << 3) | ((lane & 2) << 1) | ((lane & 4) >> 1) | ((lane & 8) >> 3);
          reinterpret_cast<float *>(&part[wave][chi * NVP + 4 * g])[vi] = w[0];
        }
      }
    }
  }
  __syncthreads();
  if ((int)threadIdx.x < NST) {
    const int it = threadIdx.x;
    float4 s = part[0][it];
    for (int w2 = 1; w2 < nw; w2++) { const float4 t = part[w2][it]; s.x += t.x; s.y += t.y; s.z += t.z; s.w += t.w; }
    const int cpar = A >= out.Vh, xc = A - cpar * out.Vh, c0 = 2 * it;   // = chi * NVEC + 2 * vp
    float *ob = out.v[cpar];
    ob[((size_t)c0 * out.stride + xc) * 2] = s.x; ob[((size_t)c0 * out.stride + xc) * 2 + 1] = s.y;
    ob[((size_t)(c0 + 1) * out.stride + xc) * 2] = s.z; ob[((size_t)(c0 + 1) * out.stride + xc) * 2 + 1] = s.w;
  }
}

// ---- FOUR SOURCES per pass over V (invertMultiSrcQuda, block_mg_cycle.cpp): the restrictor / prolongator of the fine level are pure streams of V
// (2304 B per fine site against 96 B of vector), so a lockstep multi-source cycle that restricts its sources one after the other reads V once per
// source.  Same structure as restrict_stream_kernel / prolong_kernel — three steps of V requests in flight per thread, fenced — with the V entries
// of a step meeting the site's components of four sources; the reduce-scatter butterfly that summed four STEPS of one source there sums one step
// of four SOURCES here (16 values -> lanes 0..15). ----
struct Src4 { FineVec f[4]; CoarseVec c[4]; };
// BLK: the four fine vectors are columns col0 .. col0 + 3 of a pair-major block field of ONE parity (block.h; the multi-source smoother keeps its
// residuals and solutions there): word (x 6 + k) nrhs + column holds components 2k, 2k + 1 — no unpacking into fields in front of the restrictor, no
// packing behind the prolongator
struct Blk4 { float4 *panel; int nrhs, col0, parity, Vh, accumulate; };
template <int NCF, int NVEC, int NV, bool BLK = false>
__global__ void __launch_bounds__(256) restrict_stream4_kernel(Src4 a, const void *V, const int *block_to_fine, int blockVol, MaskArg mask, AggMap amap, Blk4 blk) {
  constexpr int K = 4 * NCF, KH = K / 2, NVP = NVEC / 2, NST = 2 * NVP;
  typedef typename VRaw<false>::type raw_t;
  __shared__ float4 part[4][NST][4];   // [wave][chirality * NVP + vector pair][source]
  const int A = aggregate_of_block(amap), b = threadIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = (blockDim.x + 63) >> 6;
  float2 r[4][K];
#pragma unroll
  for (int s = 0; s < 4; s++)
#pragma unroll
    for (int k = 0; k < K; k++) r[s][k] = make_float2(0.f, 0.f);
  bool have = false;
  if (b < blockVol && mask_keep(mask, b)) {
    const int f = block_to_fine[(size_t)A * blockVol + b];
    if constexpr (BLK) {
      const int parity = f >= blk.Vh, x = f - parity * blk.Vh;
      if (parity == blk.parity) {
        have = true;
        const float4 *p = blk.panel + (size_t)x * 6 * blk.nrhs + blk.col0;
#pragma unroll
        for (int kk = 0; kk < K / 2; kk++)
#pragma unroll
          for (int s = 0; s < 4; s++) {
            const float4 w = p[kk * blk.nrhs + s];
            r[s][2 * kk] = make_float2(w.x, w.y); r[s][2 * kk + 1] = make_float2(w.z, w.w);
          }
      }
    } else {
      const int parity = f >= a.f[0].Vh, x = f - parity * a.f[0].Vh;
      if (a.f[0].v[parity]) {
        have = true;
#pragma unroll
        for (int s = 0; s < 4; s++) load_fine_site<NV, K>(r[s], a.f[s].v[parity], a.f[s].stride, x);
      }
    }
  }
  if (__builtin_amdgcn_ballot_w64(have) == 0) {   // wave-uniform
    for (int e = lane; e < NST * 4; e += 64) part[wave][e >> 2][e & 3] = make_float4(0.f, 0.f, 0.f, 0.f);
  } else {
    const int bl = b < blockVol ? b : 0;
#pragma unroll
    for (int chi = 0; chi < 2; chi++) {
      raw_t w0[KH], w1[KH], w2[KH];
      auto vload = [&](raw_t *dst, int vpl) {
        if (vpl >= NVP) return;
#pragma unroll
        for (int kk = 0; kk < KH; kk++) dst[kk] = load_v_raw<false>(V, (((size_t)A * K + chi * KH + kk) * NVP + vpl) * blockVol + bl);
      };
      vload(w0, 0); vload(w1, 1); vload(w2, 2);
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int vp = 0; vp < NVP; vp++) {
        const int ph = vp % 3;
        float w[16];
#pragma unroll
        for (int s = 0; s < 4; s++) {
          pkf2 accA = {0.f, 0.f}, accB = {0.f, 0.f};   // conj(V) r for the two vectors of the pair: two packed multiply-adds each (the 4 x 6 x 8 scalar ones per step held the kernel at 0.53-0.59)
#pragma unroll
          for (int kk = 0; kk < KH; kk++) {
            const float4 v = v_unpack(ph == 0 ? w0[kk] : (ph == 1 ? w1[kk] : w2[kk]));
            const pkf2 rr = {r[s][chi * KH + kk].x, r[s][chi * KH + kk].y};
            accA = pk::cmacc(accA, (pkf2){v.x, v.y}, rr);
            accB = pk::cmacc(accB, (pkf2){v.z, v.w}, rr);
          }
          w[4 * s] = accA.x; w[4 * s + 1] = accA.y; w[4 * s + 2] = accB.x; w[4 * s + 3] = accB.y;
        }
        __builtin_amdgcn_sched_barrier(0);
        if (ph == 0) vload(w0, vp + 3); else if (ph == 1) vload(w1, vp + 3); else vload(w2, vp + 3);   // the buffer just used: three steps ahead
        __builtin_amdgcn_sched_barrier(0);
#define QA_BFLY(HALFN, M)                                                                  \
        {                                                                                  \
          const bool up = (lane & M) != 0;                                                 \
          _Pragma("unroll") for (int j = 0; j < HALFN; j++) {                              \
            const float keep = up ? w[HALFN + j] : w[j], give = up ? w[j] : w[HALFN + j]; \
            w[j] = keep + __shfl_xor(give, M, 64);                                         \
          }                                                                                \
        }
        QA_BFLY(8, 1) QA_BFLY(4, 2) QA_BFLY(2, 4) QA_BFLY(1, 8)
#undef QA_BFLY
        w[0] += __shfl_xor(w[0], 16, 64);
        w[0] += __shfl_xor(w[0], 32, 64);
        if (lane < 16) {   // lane l holds the total of value index (bit-reversed l) = 4 * source + component
          const int vi = ((lane & 1) << 3) | ((lane & 2) << 1) | ((lane & 4) >> 1) | ((lane & 8) >> 3);
          reinterpret_cast<float *>(&part[wave][chi * NVP + vp][0])[vi] = w[0];
        }
      }
    }
  }
  __syncthreads();
  for (int e = threadIdx.x; e < NST * 4; e += blockDim.x) {
    const int it = e >> 2, s = e & 3;
    float4 t = part[0][it][s];
    for (int w2 = 1; w2 < nw; w2++) { const float4 u = part[w2][it][s]; t.x += u.x; t.y += u.y; t.z += u.z; t.w += u.w; }
    const CoarseVec &o = a.c[s];
    const int cpar = A >= o.Vh, xc = A - cpar * o.Vh, c0 = 2 * it;   // = chi * NVEC + 2 * vp
    float *ob = o.v[cpar];
    ob[((size_t)c0 * o.stride + xc) * 2] = t.x; ob[((size_t)c0 * o.stride + xc) * 2 + 1] = t.y;
    ob[((size_t)(c0 + 1) * o.stride + xc) * 2] = t.z; ob[((size_t)(c0 + 1) * o.stride + xc) * 2 + 1] = t.w;
  }
}
template <int NCF, int NVEC, int NV, bool BLK = false>
__global__ void __launch_bounds__(256) prolong4_kernel(Src4 a, const void *V, const int *block_to_fine, int blockVol, AggMap amap, Blk4 blk) {
  constexpr int K = 4 * NCF, KH = K / 2, NVP = NVEC / 2;
  typedef typename VRaw<false>::type raw_t;
  __shared__ float2 xc_s[4][2 * NVEC];
  const int A = aggregate_of_block(amap), b = threadIdx.x;
  for (int e = threadIdx.x; e < 4 * 2 * NVEC; e += blockDim.x) {
    const int s = e / (2 * NVEC), j = e - s * 2 * NVEC;
    const CoarseVec &in = a.c[s];
    const int cpar = A >= in.Vh, xc = A - cpar * in.Vh;
    const float *p = in.v[cpar] + ((size_t)j * in.stride + xc) * 2;
    xc_s[s][j] = make_float2(p[0], p[1]);
  }
  __syncthreads();
  if (b >= blockVol) return;
  const int f = block_to_fine[(size_t)A * blockVol + b];
  const int fVh = BLK ? blk.Vh : a.f[0].Vh;
  const int parity = f >= fVh, x = f - parity * fVh;
  if (BLK ? parity != blk.parity : !a.f[0].v[parity]) return;   // this parity is absent from single-parity output fields
  pkf2 acc[4][K];
#pragma unroll
  for (int s = 0; s < 4; s++)
#pragma unroll
    for (int k = 0; k < K; k++) acc[s][k] = (pkf2){0.f, 0.f};
#pragma unroll
  for (int chi = 0; chi < 2; chi++) {
    raw_t w0[KH], w1[KH], w2[KH];
    auto vload = [&](raw_t *dst, int vpl) {
      if (vpl >= NVP) return;
#pragma unroll
      for (int kk = 0; kk < KH; kk++) dst[kk] = load_v_raw<false>(V, (((size_t)A * K + chi * KH + kk) * NVP + vpl) * blockVol + b);
    };
    vload(w0, 0); vload(w1, 1); vload(w2, 2);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int vp = 0; vp < NVP; vp++) {
      const int ph = vp % 3;
#pragma unroll
      for (int s = 0; s < 4; s++) {
        const float2 d0 = xc_s[s][chi * NVEC + 2 * vp], d1 = xc_s[s][chi * NVEC + 2 * vp + 1];
        const pkf2 c0 = {d0.x, d0.y}, c1 = {d1.x, d1.y};
#pragma unroll
        for (int kk = 0; kk < KH; kk++) {
          const float4 w = v_unpack(ph == 0 ? w0[kk] : (ph == 1 ? w1[kk] : w2[kk]));
          acc[s][chi * KH + kk] = pk::cmac(pk::cmac(acc[s][chi * KH + kk], (pkf2){w.x, w.y}, c0), (pkf2){w.z, w.w}, c1);   // V c: four packed multiply-adds
        }
      }
      // pin the sums here (as prolong_kernel): without it the multiply-adds sink below the last fence and every load stays live
#pragma unroll
      for (int s = 0; s < 4; s++)
#pragma unroll
        for (int kk = 0; kk < KH; kk++) asm volatile("" : "+v"(acc[s][chi * KH + kk]));
      __builtin_amdgcn_sched_barrier(0);
      if (ph == 0) vload(w0, vp + 3); else if (ph == 1) vload(w1, vp + 3); else vload(w2, vp + 3);
      __builtin_amdgcn_sched_barrier(0);
    }
  }
  if constexpr (BLK) {
    float4 *p = blk.panel + (size_t)x * 6 * blk.nrhs + blk.col0;
#pragma unroll
    for (int kk = 0; kk < K / 2; kk++)
#pragma unroll
      for (int s = 0; s < 4; s++) {
        float4 o = make_float4(acc[s][2 * kk].x, acc[s][2 * kk].y, acc[s][2 * kk + 1].x, acc[s][2 * kk + 1].y);
        if (blk.accumulate) { const float4 w = p[kk * blk.nrhs + s]; o.x += w.x; o.y += w.y; o.z += w.z; o.w += w.w; }
        p[kk * blk.nrhs + s] = o;
      }
    return;
  }
#pragma unroll
  for (int s = 0; s < 4; s++) {
    float *base = a.f[s].v[parity];
    if (NV == 4) {
#pragma unroll
      for (int k = 0; k < K; k += 2) *reinterpret_cast<float4 *>(base + fidx<NV>(a.f[s].stride, x, k)) = make_float4(acc[s][k].x, acc[s][k].y, acc[s][k + 1].x, acc[s][k + 1].y);
    } else {
#pragma unroll
      for (int k = 0; k < K; k++) *reinterpret_cast<float2 *>(base + fidx<NV>(a.f[s].stride, x, k)) = make_float2(acc[s][k].x, acc[s][k].y);
    }
  }
}

// ---- four right-hand sides per pass over V (Galerkin construction of the first coarse level: the 8 single-direction hops of
// one probe are restricted in two launches instead of eight; V is the whole cost of a restriction) ----
struct Multi4 {
  CoarseVec out[4], out2[4];
  FineVec in[4];
  int dir[4];
};
__device__ __forceinline__ bool mask_outside_dir(const MaskArg &m, int dir, int b) {
  const int mu = dir >> 1, fwd = !(dir & 1);
  int y[4];
  block_coords(y, m, b);
  return !m.single[mu] && (fwd ? y[mu] == m.bs[mu] - 1 : y[mu] == 0);
}
// every wave keeps its partial sums of ALL (chirality, vector pair) steps in its own LDS rows, so the steps run back to back
// without a barrier (24 steps x 2 barriers made this kernel 2.5x slower than the V stream); one barrier, then the block sum
template <int NSF, int NCF, int NVEC, int NV>
__global__ void __launch_bounds__(256) restrict4_kernel(Multi4 a, const float4 *V, const int *block_to_fine, int blockVol, int spin_bs, MaskArg mask, AggMap amap) {
  constexpr int K = NSF * NCF, NIT = NVEC;   // steps = 2 chiralities x NVEC / 2 vector pairs
  __shared__ float4 part[4][NIT][8];          // [wave][step][rhs*2 + (0 leaving, 1 staying)]
  const int A = aggregate_of_block(amap), b = threadIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = (blockDim.x + 63) >> 6;
  const bool site = b < blockVol;
  float2 r[4][K];
  bool outside[4];
  if (site) {
    const int f = block_to_fine[(size_t)A * blockVol + b];
    const int parity = f >= a.in[0].Vh, x = f - parity * a.in[0].Vh;
#pragma unroll
    for (int q = 0; q < 4; q++) {
      const float *base = a.in[q].v[parity];
      outside[q] = mask_outside_dir(mask, a.dir[q], b);
load_fine_site<NV, K>(r[q], base, a.in[q].stride, x);
    }
  }
  // The two chiralities are separate (unrolled) loops so that the K / 2 rows of a step are compile-time register indices, and the
  // V entries of step vp + 1 are requested before the cross-lane reduction of step vp: one step's loads -> wait -> sums -> shuffles
  // in series left the kernel latency-bound at two waves per SIMD (10 ms per pass over V against 4.4 ms for the plain restrictor).
  constexpr int KH = K / 2;
#pragma unroll
  for (int chi = 0; chi < 2; chi++) {
  // Three buffers of V entries, statically named and refilled in place right after their use, fenced against the scheduler (which
  // would sink every request down to its use): three steps of requests in flight per thread
  float4 w0[KH], w1[KH], w2[KH];
  // unconditional loads (a thread beyond the aggregate reads entry 0 and its sums are masked out below): a load under a per-lane
  // condition becomes its own basic block, and across blocks the wait-count bookkeeping falls back to vmcnt(0) again
  const int bl = site ? b : 0;
  auto vload = [&](float4 *dst, int vpl) {
    if (vpl >= NVEC / 2) return;
#pragma unroll
    for (int kk = 0; kk < KH; kk++) dst[kk] = load_v<false>(V, (((size_t)A * K + chi * KH + kk) * (NVEC / 2) + vpl) * blockVol + bl);
  };
  vload(w0, 0); vload(w1, 1); vload(w2, 2);
  __builtin_amdgcn_sched_barrier(0);
  // fully unrolled: with a loop the wait-count bookkeeping of the compiler merges to s_waitcnt vmcnt(0) at the loop header and at
  // every use — the three buffers were drained at each step, which is why neither they nor anything else moved this kernel
#pragma unroll
  for (int vp3 = 0; vp3 < NVEC / 2; vp3 += 3) {
#pragma unroll
  for (int ph = 0; ph < 3; ph++) {
    const int vp = vp3 + ph;
    if (vp >= NVEC / 2) break;
    const int it = chi * (NVEC / 2) + vp;
    float4 wc[KH];
#pragma unroll
    for (int kk = 0; kk < KH; kk++) wc[kk] = ph == 0 ? w0[kk] : (ph == 1 ? w1[kk] : w2[kk]);
    float4 acc[4];
#pragma unroll
    for (int q = 0; q < 4; q++) acc[q] = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
    for (int kk = 0; kk < KH; kk++) {
      const float4 w = wc[kk];
      const int k = chi * KH + kk;
#pragma unroll
      for (int q = 0; q < 4; q++) {
        acc[q].x += w.x * r[q][k].x + w.y * r[q][k].y; acc[q].y += w.x * r[q][k].y - w.y * r[q][k].x;
        acc[q].z += w.z * r[q][k].x + w.w * r[q][k].y; acc[q].w += w.z * r[q][k].y - w.w * r[q][k].x;
      }
    }
    // the buffer just used takes the entries of three steps ahead
    __builtin_amdgcn_sched_barrier(0);
    if (ph == 0) vload(w0, vp + 3); else if (ph == 1) vload(w1, vp + 3); else vload(w2, vp + 3);
    __builtin_amdgcn_sched_barrier(0);
    // wave sum of the 32 partial reals (4 right-hand sides x {leaving, staying} x float4) by a reduce-scatter butterfly: at every
    // stage a lane keeps one half of its values and adds the partner's copy of that half, so the five xor stages move
    // 16 + 8 + 4 + 2 + 1 values instead of 32 each, one more adds the two half-waves: 32 cross-lane moves instead of 192
    // (the shuffle chains, not the V stream, held this kernel at 2.3 TB/s)
    float w[32];
#pragma unroll
    for (int q = 0; q < 4; q++) {
      const bool so = site && outside[q], si = site && !outside[q];
      w[8 * q + 0] = so ? acc[q].x : 0.f; w[8 * q + 1] = so ? acc[q].y : 0.f; w[8 * q + 2] = so ? acc[q].z : 0.f; w[8 * q + 3] = so ? acc[q].w : 0.f;
      w[8 * q + 4] = si ? acc[q].x : 0.f; w[8 * q + 5] = si ? acc[q].y : 0.f; w[8 * q + 6] = si ? acc[q].z : 0.f; w[8 * q + 7] = si ? acc[q].w : 0.f;
    }
    // (written out stage by stage: with the stage as a loop variable the register array was indexed dynamically, 1900 selects per step)
#define QA_BFLY(HALF, M)                                                                 \
    {                                                                                    \
      const bool up = (lane & M) != 0;                                                   \
      _Pragma("unroll") for (int j = 0; j < HALF; j++) {                                 \
        const float keep = up ? w[HALF + j] : w[j], give = up ? w[j] : w[HALF + j];     \
        w[j] = keep + __shfl_xor(give, M, 64);                                           \
      }                                                                                  \
    }
    QA_BFLY(16, 1) QA_BFLY(8, 2) QA_BFLY(4, 4) QA_BFLY(2, 8) QA_BFLY(1, 16)
#undef QA_BFLY
    w[0] += __shfl_xor(w[0], 32, 64);
    // lane l < 32 now holds the total of value index sum_s bit_s(l) * (16 >> s)
    if (lane < 32) {
      const int vi = ((lane & 1) << 4) | ((lane & 2) << 2) | (lane & 4) | ((lane & 8) >> 2) | ((lane & 16) >> 4);
      reinterpret_cast<float *>(&part[wave][it][0])[vi] = w[0];
    }
    __builtin_amdgcn_sched_barrier(0);
  }
  }
  }
  __syncthreads();
  const int cpar = A >= a.out[0].Vh, xc = A - cpar * a.out[0].Vh;
  for (int e = threadIdx.x; e < NIT * 8; e += blockDim.x) {
    const int it = e >> 3, o8 = e & 7;
    float4 s = part[0][it][o8];
    for (int w2 = 1; w2 < nw; w2++) { const float4 t = part[w2][it][o8]; s.x += t.x; s.y += t.y; s.z += t.z; s.w += t.w; }
    const int q = o8 >> 1;
    const CoarseVec &o = (o8 & 1) ? a.out2[q] : a.out[q];
    float *ob = o.v[cpar];
    const int chi = it / (NVEC / 2), vp = it - chi * (NVEC / 2), c0 = chi * NVEC + 2 * vp;
    ob[((size_t)c0 * o.stride + xc) * 2] = s.x; ob[((size_t)c0 * o.stride + xc) * 2 + 1] = s.y;
    ob[((size_t)(c0 + 1) * o.stride + xc) * 2] = s.z; ob[((size_t)(c0 + 1) * o.stride + xc) * 2 + 1] = s.w;
  }
}

// ---- small aggregates (blockVol <= 32, the coarse levels: 2^4 = 16 sites).  One thread per site leaves most of a wave idle and
// runs the (chirality, vector pair) iterations one after the other behind block-wide reductions — 0.28 ms for a 37 MB
// transfer.  Here a wave holds 64 / GS groups of GS lanes (GS = blockVol rounded up to a power of two), every group takes its
// own (chi, vp) iteration for the whole aggregate and reduces with GS-wide shuffles: no LDS, no barriers, all iterations
// of an aggregate in flight at once across the 8 waves of its work-group. ----
template <int NSF, int NCF, int NVEC, int NV, bool DUAL, bool HALF>
__global__ void __launch_bounds__(512) restrict_small_kernel(CoarseVec out, CoarseVec out2, FineVec in, const void *V, const int *block_to_fine, int blockVol, int GS,
                                                             int spin_bs, MaskArg mask) {
  constexpr int K = NSF * NCF, NIT = NVEC;   // iterations = 2 chiralities x NVEC/2 vector pairs
  const int A = blockIdx.x;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int groupsPerWave = 64 / GS, b = lane % GS, grp = lane / GS;
  const int slot = wave * groupsPerWave + grp, nslots = (blockDim.x >> 6) * groupsPerWave;
  const bool site = b < blockVol;
  const bool active = site && (DUAL || mask_keep(mask, b));
  const bool outside = DUAL && site && mask_outside(mask, b);
  float2 r[K];
  bool have = false;
  if (active) {
    const int f = block_to_fine[(size_t)A * blockVol + b];
    const int parity = f >= in.Vh, x = f - parity * in.Vh;
    const float *base = in.v[parity];
    if (base) {
      have = true;
load_fine_site<NV, K>(r, base, in.stride, x);
    }
  }
  const int cpar = A >= out.Vh, xc = A - cpar * out.Vh;
  float *ob = out.v[cpar], *ob2 = DUAL ? out2.v[cpar] : nullptr;
  for (int it = slot; it < NIT; it += nslots) {
    const int chi = it / (NVEC / 2), vp = it - chi * (NVEC / 2);
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    if (have) {
#pragma unroll
      for (int k = 0; k < K; k++) {
        if ((k / NCF) / spin_bs != chi) continue;
        const float4 w = load_v<HALF>(V, (((size_t)A * K + k) * (NVEC / 2) + vp) * blockVol + b);
        acc.x += w.x * r[k].x + w.y * r[k].y; acc.y += w.x * r[k].y - w.y * r[k].x;
        acc.z += w.z * r[k].x + w.w * r[k].y; acc.w += w.z * r[k].y - w.w * r[k].x;
      }
    }
    float4 so = acc, si = make_float4(0.f, 0.f, 0.f, 0.f);
    if (DUAL) { if (!outside) { si = acc; so = make_float4(0.f, 0.f, 0.f, 0.f); } }
    for (int off = GS >> 1; off > 0; off >>= 1) {
      so.x += __shfl_down(so.x, off, GS); so.y += __shfl_down(so.y, off, GS); so.z += __shfl_down(so.z, off, GS); so.w += __shfl_down(so.w, off, GS);
      if (DUAL) { si.x += __shfl_down(si.x, off, GS); si.y += __shfl_down(si.y, off, GS); si.z += __shfl_down(si.z, off, GS); si.w += __shfl_down(si.w, off, GS); }
    }
    if (b == 0) {
      const int c0 = chi * NVEC + 2 * vp;
      ob[((size_t)c0 * out.stride + xc) * 2] = so.x; ob[((size_t)c0 * out.stride + xc) * 2 + 1] = so.y;
      ob[((size_t)(c0 + 1) * out.stride + xc) * 2] = so.z; ob[((size_t)(c0 + 1) * out.stride + xc) * 2 + 1] = so.w;
      if (DUAL) {
        ob2[((size_t)c0 * out2.stride + xc) * 2] = si.x; ob2[((size_t)c0 * out2.stride + xc) * 2 + 1] = si.y;
        ob2[((size_t)(c0 + 1) * out2.stride + xc) * 2] = si.z; ob2[((size_t)(c0 + 1) * out2.stride + xc) * 2 + 1] = si.w;
      }
    }
  }
}

// prolongator for small aggregates: the K fine components of a site are spread over the groups / waves the same way
template <int NSF, int NCF, int NVEC, int NV, bool HALF>
__global__ void __launch_bounds__(512) prolong_small_kernel(FineVec out, CoarseVec in, const void *V, const int *block_to_fine, int blockVol, int GS, int spin_bs) {
  constexpr int K = NSF * NCF;
  __shared__ float2 xc_s[2 * NVEC];
  const int A = blockIdx.x;
  const int cpar = A >= in.Vh, xc = A - cpar * in.Vh;
  for (int j = threadIdx.x; j < 2 * NVEC; j += blockDim.x) {
    const float *p = in.v[cpar] + ((size_t)j * in.stride + xc) * 2;
    xc_s[j] = make_float2(p[0], p[1]);
  }
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int groupsPerWave = 64 / GS, b = lane % GS, grp = lane / GS;
  const int slot = wave * groupsPerWave + grp, nslots = (blockDim.x >> 6) * groupsPerWave;
  if (b >= blockVol) return;
  const int f = block_to_fine[(size_t)A * blockVol + b];
  const int parity = f >= out.Vh, x = f - parity * out.Vh;
  float *base = out.v[parity];
  if (!base) return;
  for (int k = slot; k < K; k += nslots) {
    const int chi = (k / NCF) / spin_bs;
    float re = 0.f, im = 0.f;
#pragma unroll 4
    for (int vp = 0; vp < NVEC / 2; vp++) {
      const float4 w = load_v<HALF>(V, (((size_t)A * K + k) * (NVEC / 2) + vp) * blockVol + b);
      const float2 c0 = xc_s[chi * NVEC + 2 * vp], c1 = xc_s[chi * NVEC + 2 * vp + 1];
      re += w.x * c0.x - w.y * c0.y + w.z * c1.x - w.w * c1.y;
      im += w.x * c0.y + w.y * c0.x + w.z * c1.y + w.w * c1.x;
    }
    const size_t i = fidx<NV>(out.stride, x, k);
    base[i] = re; base[i + 1] = im;
  }
}

// ---- prolongator ----
template <int NSF, int NCF, int NVEC, int NV, bool HALF = false>
__global__ void __launch_bounds__(512) prolong_kernel(FineVec out, CoarseVec in, const void *V, const int *block_to_fine, int blockVol, int spin_bs, AggMap amap) {
  constexpr int K = NSF * NCF;
  __shared__ float2 xc_s[2 * NVEC];
  const int A = aggregate_of_block(amap), b = threadIdx.x;
  const int cpar = A >= in.Vh, xc = A - cpar * in.Vh;
  for (int j = threadIdx.x; j < 2 * NVEC; j += blockDim.x) {
    const float *p = in.v[cpar] + ((size_t)j * in.stride + xc) * 2;
    xc_s[j] = make_float2(p[0], p[1]);
  }
  __syncthreads();
  if (b >= blockVol) return;
  const int f = block_to_fine[(size_t)A * blockVol + b];
  const int parity = f >= out.Vh, x = f - parity * out.Vh;
  float *base = out.v[parity];
  if (!base) return;   // this parity is absent from a single-parity output field
  // vector pair outermost: its two coarse coefficients are read from LDS once and meet the K / 2 spin-colour rows of their
  // chirality (k-outer re-read them for every row: 288 LDS reads per thread next to 144 V loads); 16-byte stores where the
  // field order pairs two components (FLOAT4: spin-colour 2 m, 2 m + 1 share a plane entry)
  float2 acc[K];
#pragma unroll
  for (int k = 0; k < K; k++) acc[k] = make_float2(0.f, 0.f);
  if constexpr (NSF == 4) {
    // fine level: three steps of V requests in flight per thread (raw register images, converted at their use), every step fully
    // unrolled and fenced — as a rolled loop the 6 x unroll loads of an iteration were drained before the next ones were issued
    constexpr int KH = K / 2, NVP = NVEC / 2;
    typedef typename VRaw<HALF>::type raw_t;
#pragma unroll
    for (int chi = 0; chi < 2; chi++) {
      raw_t w0[KH], w1[KH], w2[KH];
      auto vload = [&](raw_t *dst, int vpl) {
        if (vpl >= NVP) return;
#pragma unroll
        for (int kk = 0; kk < KH; kk++) dst[kk] = load_v_raw<HALF>(V, (((size_t)A * K + chi * KH + kk) * NVP + vpl) * blockVol + b);
      };
      vload(w0, 0); vload(w1, 1); vload(w2, 2);
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int vp = 0; vp < NVP; vp++) {
        const int ph = vp % 3;
        const float2 c0 = xc_s[chi * NVEC + 2 * vp], c1 = xc_s[chi * NVEC + 2 * vp + 1];
#pragma unroll
        for (int kk = 0; kk < KH; kk++) {
          const float4 w = v_unpack(ph == 0 ? w0[kk] : (ph == 1 ? w1[kk] : w2[kk]));
          acc[chi * KH + kk].x += w.x * c0.x - w.y * c0.y + w.z * c1.x - w.w * c1.y;
          acc[chi * KH + kk].y += w.x * c0.y + w.y * c0.x + w.z * c1.y + w.w * c1.x;
        }
        // pin the sums here: without it the multiply-adds sink below the last fence and every load stays live (256 registers + scratch)
#pragma unroll
        for (int kk = 0; kk < KH; kk++) asm volatile("" : "+v"(acc[chi * KH + kk].x), "+v"(acc[chi * KH + kk].y));
        __builtin_amdgcn_sched_barrier(0);
        if (ph == 0) vload(w0, vp + 3); else if (ph == 1) vload(w1, vp + 3); else vload(w2, vp + 3);
        __builtin_amdgcn_sched_barrier(0);
      }
    }
  } else {
#pragma unroll
  for (int chi = 0; chi < 2; chi++) {
#pragma unroll 2
    for (int vp = 0; vp < NVEC / 2; vp++) {
      const float2 c0 = xc_s[chi * NVEC + 2 * vp], c1 = xc_s[chi * NVEC + 2 * vp + 1];
#pragma unroll
      for (int k = 0; k < K; k++) {
        if (k / (K / 2) != chi) continue;   // two chiralities whatever the spin blocking: rows [0, K/2) and [K/2, K) (= (k / NCF) / spin_bs)
        const float4 w = load_v<HALF>(V, (((size_t)A * K + k) * (NVEC / 2) + vp) * blockVol + b);
        acc[k].x += w.x * c0.x - w.y * c0.y + w.z * c1.x - w.w * c1.y;
        acc[k].y += w.x * c0.y + w.y * c0.x + w.z * c1.y + w.w * c1.x;
      }
    }
  }
  }
  if (NV == 4) {
#pragma unroll
    for (int k = 0; k < K; k += 2) *reinterpret_cast<float4 *>(base + fidx<NV>(out.stride, x, k)) = make_float4(acc[k].x, acc[k].y, acc[k + 1].x, acc[k + 1].y);
  } else {
#pragma unroll
    for (int k = 0; k < K; k++) *reinterpret_cast<float2 *>(base + fidx<NV>(out.stride, x, k)) = acc[k];
  }
}

// ---- host side: every method assembles its arguments from the helpers below and launches through forShape / withV ----
void Transfer::setSiteSubset(QudaSiteSubset subset, QudaParity parity) {
  if (subset == QUDA_PARITY_SITE_SUBSET && parity != QUDA_EVEN_PARITY && parity != QUDA_ODD_PARITY) errorQuda("Undefined parity %d", parity);
  site_subset = subset;
  subset_parity = parity;
}

// the instantiated (fine spin, fine colour, Nvec) shapes as compile-time constants: f(Shape<...>{}).  A kernel that exists for some of the
// shapes only is launched under an `if constexpr` on them, so that no other instantiation appears.
template <int NSF_, int NCF_, int NVEC_> struct Shape {
  static constexpr int NSF = NSF_, NCF = NCF_, NVEC = NVEC_, NV = NSF_ == 4 ? 4 : 2;   // NV: reals per vector of the fine field order
  // the barrier-free stream kernels (restrict_stream_kernel and the four-source pair): fine level, steps summed four at a time
  static constexpr bool stream = NSF_ == 4 && NVEC_ % 8 == 0;
};
template <typename F> static void forShape(const Transfer &T, F &&f) {
  const int fineSpin = T.fineSpin, fineColor = T.fineColor, Nvec = T.Nvec;
  if (fineSpin == 4 && fineColor == 3) {
    switch (Nvec) {
      case 4: f(Shape<4, 3, 4>{}); break;
      case 8: f(Shape<4, 3, 8>{}); break;
      case 24: f(Shape<4, 3, 24>{}); break;
      case 32: f(Shape<4, 3, 32>{}); break;
      default: errorQuda("Nvec = %d not instantiated for the fine level (4, 8, 24, 32)", Nvec);
    }
  } else if (fineSpin == 2 && fineColor == 4 && Nvec == 4) f(Shape<2, 4, 4>{});
  else if (fineSpin == 2 && fineColor == 8 && Nvec == 8) f(Shape<2, 8, 8>{});
  else if (fineSpin == 2 && fineColor == 8 && Nvec == 4) f(Shape<2, 8, 4>{});
  else if (fineSpin == 2 && fineColor == 24 && Nvec == 24) f(Shape<2, 24, 24>{});
  else if (fineSpin == 2 && fineColor == 24 && Nvec == 32) f(Shape<2, 24, 32>{});
  else if (fineSpin == 2 && fineColor == 32 && Nvec == 32) f(Shape<2, 32, 32>{});
  else errorQuda("transfer %d x %d -> Nvec %d not instantiated", fineSpin, fineColor, Nvec);
}

// V as the kernels stream it: f(HALF as std::bool_constant, pointer) with the fp16 mirror or the fp32 master
template <typename F> static void withV(const Transfer &T, bool half, F &&f) {
  if (half) f(std::true_type{}, (const void *)T.V_h);
  else f(std::false_type{}, (const void *)T.V);
}

template <typename... P, typename... A> static void launch(void (*kernel)(P...), int grid, int block, A... args) {
  hipLaunchKernelGGL(kernel, dim3(grid), dim3(block), 0, computeStream(), args...);
  HIP_CHECK(hipGetLastError());
}

// the x-neighbour aggregate order (aggregate_of_block) where the blocking allows it; QUDA_AMD_PROLONG_XGROUP=0 switches it off
static AggMap aggMapOf(const Transfer &T) {
  AggMap amap = {0, T.Xc[0], T.Xc[1], T.Xc[2], T.nAgg / 2};
  static int off = -1;
  if (off < 0) { const char *e = getenv("QUDA_AMD_PROLONG_XGROUP"); off = (e && !atoi(e)) ? 1 : 0; }
  if (!off && T.geo_bs[0] == 4 && T.Xc[0] % 4 == 0 && T.nAgg % 32 == 0) amap.xgroup = T.Xc[0] / 4;
  return amap;
}

static MaskArg maskArg(const Transfer &T, int dir, int boundary) {
  MaskArg m;
  m.dir = dir; m.boundary = boundary; m.pm = T.parityMajor ? 1 : 0;
  for (int d = 0; d < 4; d++) { m.bs[d] = T.geo_bs[d]; m.single[d] = T.Xc[d] == 1; }
  return m;
}

// one work-group per aggregate: whole waves that cover its sites, or — small aggregates (the *_small kernels) — 512 threads in groups of gs lanes
struct WorkGroup { int threads, gs; bool small; };
static WorkGroup workGroup(const Transfer &T) {
  WorkGroup w = {(T.blockVol + 63) / 64 * 64, 1, T.blockVol <= 32};
  while (w.gs < T.blockVol) w.gs <<= 1;
  return w;
}

// the shape of a fine operand; a single-parity one needs setSiteSubset (or is refused: fullOnly).  Returns the parity fineVec takes (-1: a full field)
static int checkFine(const Transfer &T, const ColorSpinorField &fine, bool fullOnly = false) {
  const bool sub = fine.SiteSubset() == QUDA_PARITY_SITE_SUBSET;
  if (sub && !fullOnly && T.site_subset != QUDA_PARITY_SITE_SUBSET) errorQuda("single-parity fine field but the transfer is set to full fields");
  if ((sub && fullOnly) || fine.Nspin() != T.fineSpin || fine.Ncolor() != T.fineColor || (long)fine.VolumeCB() * 2 != T.fineVol) errorQuda("fine field does not match the transfer operator");
  return sub ? (int)T.subset_parity : -1;
}
static CoarseVec checkCoarse(const Transfer &T, const ColorSpinorField &coarse) {
  if (coarse.Nspin() != 2 || coarse.Ncolor() != T.Nvec || coarse.Volume() != T.nAgg) errorQuda("coarse field does not match the transfer operator");
  return coarseVec(coarse);
}

// algorithmic bytes of one pass over V for `sources` vectors: the fraction of V and of the fine vectors that the call touches (vFraction) at
// vBytes per complex entry of V (fp32 or the fp16 mirror), the fine vectors (+ extraFine further passes over one) and the coarse vectors
static double transferBytes(const Transfer &T, double frac, int sources, int vBytes, int extraFine = 0) {
  const double K = (double)T.fineSpin * T.fineColor;
  return frac * T.fineVol * (K * T.Nvec * vBytes + (sources + extraFine) * K * 8.0) + (double)sources * T.nAgg * 2 * T.Nvec * 8;
}
static double vFraction(const ColorSpinorField &fine) { return fine.SiteSubset() == QUDA_PARITY_SITE_SUBSET ? 0.5 : 1.0; }

void Transfer::R(ColorSpinorField &coarse, const ColorSpinorField &fine, int dir, int boundary) const {
  const FineVec in = fineVec(fine, checkFine(*this, fine));
  const CoarseVec out = checkCoarse(*this, coarse);
  const MaskArg m = maskArg(*this, dir, boundary);
  const WorkGroup w = workGroup(*this);
  const AggMap amap = aggMapOf(*this);
  const bool half = coarseHalfStorage() && V_h != nullptr && dir < 0;   // the Galerkin-split variants always use the fp32 master
  // the barrier-free restrictor (restrict_stream_kernel): fine level with two chiralities of K / 2 rows, at most four waves per aggregate
  static int streamOff = -1;
  if (streamOff < 0) { const char *e = getenv("QUDA_AMD_RESTRICT_STREAM"); streamOff = (e && !atoi(e)) ? 1 : 0; }
  const bool stream = !streamOff && !w.small && w.threads <= 256 && spin_bs == 2 && fineSpin == 4 && Nvec % 8 == 0;   // the last two: Shape::stream
  forShape(*this, [&](auto shape) {
    using S = decltype(shape);
    withV(*this, half, [&](auto h, const void *v) {
      constexpr bool HALF = decltype(h)::value;
      if (w.small) launch(restrict_small_kernel<S::NSF, S::NCF, S::NVEC, S::NV, false, HALF>, nAgg, 512, out, out, in, v, block_to_fine, blockVol, w.gs, spin_bs, m);
      else if (!stream) launch(restrict_kernel<S::NSF, S::NCF, S::NVEC, S::NV, false, HALF>, nAgg, w.threads, out, out, in, v, block_to_fine, blockVol, spin_bs, m, amap);
      else if constexpr (S::stream) launch(restrict_stream_kernel<S::NSF, S::NCF, S::NVEC, S::NV, HALF>, nAgg, w.threads, out, in, v, block_to_fine, blockVol, m, amap);
    });
  });
  if (g_acctOn) {   // V once (fp32 or its fp16 mirror; a single-parity source touches half of it) + fine vector + coarse vector
    char tag[48]; snprintf(tag, sizeof(tag), "level %s -> coarse%s", fineSpin == 4 ? "0" : "c", half ? " fp16 V" : "");
    acct(w.small ? "restrict_small_kernel" : (stream ? "restrict_stream_kernel" : "restrict_kernel"), transferBytes(*this, vFraction(fine), 1, half ? 4 : 8), tag);
  }
  flops_ += 8ull * fineSpin * fineColor * Nvec * fineVol;  // reference lib/restrictor.cu:405
}

void Transfer::RSplit(ColorSpinorField &leaving, ColorSpinorField &staying, const ColorSpinorField &fine, int dir) const {
  if (fine.SiteSubset() != QUDA_FULL_SITE_SUBSET) errorQuda("the split restriction works on full fields");
  if (dir < 0 || dir > 7) errorQuda("direction %d", dir);
  const FineVec in = fineVec(fine, checkFine(*this, fine, true));
  const CoarseVec out = checkCoarse(*this, leaving), out2 = checkCoarse(*this, staying);
  const MaskArg m = maskArg(*this, dir, 1);
  const WorkGroup w = workGroup(*this);
  const AggMap amap = aggMapOf(*this);
  forShape(*this, [&](auto shape) {
    using S = decltype(shape);
    if (w.small) launch(restrict_small_kernel<S::NSF, S::NCF, S::NVEC, S::NV, true, false>, nAgg, 512, out, out2, in, (const void *)V, block_to_fine, blockVol, w.gs, spin_bs, m);
    else launch(restrict_kernel<S::NSF, S::NCF, S::NVEC, S::NV, true, false>, nAgg, w.threads, out, out2, in, (const void *)V, block_to_fine, blockVol, spin_bs, m, amap);
  });
  flops_ += 8ull * fineSpin * fineColor * Nvec * fineVol;
}

void Transfer::P(ColorSpinorField &fine, const ColorSpinorField &coarse) const {
  const FineVec out = fineVec(fine, checkFine(*this, fine));
  const CoarseVec in = checkCoarse(*this, coarse);
  const WorkGroup w = workGroup(*this);
  if (w.threads > 512) errorQuda("aggregates of %d sites: the prolongator runs one work-group of at most 512 threads per aggregate", blockVol);
  const AggMap amap = aggMapOf(*this);
  const bool half = coarseHalfStorage() && V_h != nullptr;
  forShape(*this, [&](auto shape) {
    using S = decltype(shape);
    withV(*this, half, [&](auto h, const void *v) {
      constexpr bool HALF = decltype(h)::value;
      if (w.small) launch(prolong_small_kernel<S::NSF, S::NCF, S::NVEC, S::NV, HALF>, nAgg, 512, out, in, v, block_to_fine, blockVol, w.gs, spin_bs);
      else launch(prolong_kernel<S::NSF, S::NCF, S::NVEC, S::NV, HALF>, nAgg, w.threads, out, in, v, block_to_fine, blockVol, spin_bs, amap);
    });
  });
  if (g_acctOn) {
    char tag[48]; snprintf(tag, sizeof(tag), "coarse -> level %s%s", fineSpin == 4 ? "0" : "c", half ? " fp16 V" : "");
    acct(w.small ? "prolong_small_kernel" : "prolong_kernel", transferBytes(*this, vFraction(fine), 1, half ? 4 : 8), tag);
  }
  flops_ += 8ull * fineSpin * fineColor * Nvec * fineVol;  // reference lib/prolongator.cu:228
}

// ---- four sources per pass over V (fine level, fp32 V): see restrict_stream4_kernel / prolong4_kernel ----
bool Transfer::canQuad() const { return fineSpin == 4 && fineColor == 3 && spin_bs == 2 && blockVol > 32 && blockVol <= 256 && (Nvec == 8 || Nvec == 24 || Nvec == 32); }

// the operands of R4 / P4 (fine fields, all of one site subset) and of R4Block / P4Block (fine == nullptr: the fine side is a Blk4)
static Src4 src4(const Transfer &T, const ColorSpinorField *const *fine, const ColorSpinorField *const *coarse) {
  Src4 a;
  memset(&a, 0, sizeof(a));
  for (int s = 0; s < 4; s++) {
    a.c[s] = checkCoarse(T, *coarse[s]);
    if (!fine) continue;
    if (fine[s]->SiteSubset() != fine[0]->SiteSubset()) errorQuda("fine field does not match the transfer operator");
    a.f[s] = fineVec(*fine[s], checkFine(T, *fine[s]));
  }
  return a;
}
static Blk4 blk4(const Transfer &T, const float2 *panel, int nrhs, int col0, bool accumulate) {
  return {reinterpret_cast<float4 *>(const_cast<float2 *>(panel)), nrhs, col0, T.subset_parity == QUDA_ODD_PARITY ? 1 : 0, (int)(T.fineVol / 2), accumulate ? 1 : 0};
}
template <bool BLK> static void launchQuad(const Transfer &T, bool restrictor, const Src4 &a, const Blk4 &blk) {
  const int threads = workGroup(T).threads;
  const AggMap amap = aggMapOf(T);
  forShape(T, [&](auto shape) {
    using S = decltype(shape);
    if constexpr (S::stream) {   // canQuad
      if (restrictor) launch(restrict_stream4_kernel<S::NCF, S::NVEC, S::NV, BLK>, T.nAgg, threads, a, (const void *)T.V, T.block_to_fine, T.blockVol, maskArg(T, -1, 0), amap, blk);
      else launch(prolong4_kernel<S::NCF, S::NVEC, S::NV, BLK>, T.nAgg, threads, a, (const void *)T.V, T.block_to_fine, T.blockVol, amap, blk);
    }
  });
}

void Transfer::R4(ColorSpinorField *const coarse[4], const ColorSpinorField *const fine[4]) const {
  if (!canQuad()) errorQuda("four-source restrictor: fine level with 4^4-type aggregates only");
  launchQuad<false>(*this, true, src4(*this, fine, coarse), Blk4{});
  if (g_acctOn) acct("restrict_stream4_kernel", transferBytes(*this, vFraction(*fine[0]), 4, 8), "level 0 -> coarse, 4 sources");
  flops_ += 4 * 8ull * fineSpin * fineColor * Nvec * fineVol;
}
void Transfer::P4(ColorSpinorField *const fine[4], const ColorSpinorField *const coarse[4]) const {
  if (!canQuad()) errorQuda("four-source prolongator: fine level with 4^4-type aggregates only");
  launchQuad<false>(*this, false, src4(*this, fine, coarse), Blk4{});
  if (g_acctOn) acct("prolong4_kernel", transferBytes(*this, vFraction(*fine[0]), 4, 8), "coarse -> level 0, 4 sources");
  flops_ += 4 * 8ull * fineSpin * fineColor * Nvec * fineVol;
}

// ... with the fine vectors in four columns of a pair-major block field of one parity (block.h): the multi-source smoother's residuals in, its solutions out
void Transfer::R4Block(ColorSpinorField *const coarse[4], const float2 *panel, int nrhs, int col0) const {
  if (!canQuad() || site_subset != QUDA_PARITY_SITE_SUBSET) errorQuda("four-source restrictor on block fields: fine level, single-parity transfers");
  launchQuad<true>(*this, true, src4(*this, nullptr, coarse), blk4(*this, panel, nrhs, col0, false));
  if (g_acctOn) acct("restrict_stream4_kernel", transferBytes(*this, 0.5, 4, 8), "level 0 (block columns) -> coarse, 4 sources");
  flops_ += 4 * 8ull * fineSpin * fineColor * Nvec * fineVol / 2;
}
void Transfer::P4Block(float2 *panel, int nrhs, int col0, bool accumulate, const ColorSpinorField *const coarse[4]) const {
  if (!canQuad() || site_subset != QUDA_PARITY_SITE_SUBSET) errorQuda("four-source prolongator on block fields: fine level, single-parity transfers");
  launchQuad<true>(*this, false, src4(*this, nullptr, coarse), blk4(*this, panel, nrhs, col0, accumulate));
  if (g_acctOn) acct("prolong4_kernel", transferBytes(*this, 0.5, 4, 8, accumulate ? 4 : 0), "coarse -> level 0 (block columns), 4 sources");
  flops_ += 4 * 8ull * fineSpin * fineColor * Nvec * fineVol / 2;
}

// ---- the Galerkin split of four fine vectors, each with its own direction, in one pass over V (restrict4_kernel) ----
bool Transfer::canSplit4() const { return fineSpin == 4 && fineColor == 3 && blockVol > 32 && blockVol <= 256; }

void Transfer::RSplit4(ColorSpinorField *const leaving[4], ColorSpinorField *const staying[4], ColorSpinorField *const fine[4], const int dir[4]) const {
  if (!canSplit4()) errorQuda("the four-way split restriction is built for the fine level");
  Multi4 a;
  for (int q = 0; q < 4; q++) {
    a.in[q] = fineVec(*fine[q], checkFine(*this, *fine[q], true));
    a.out[q] = checkCoarse(*this, *leaving[q]); a.out2[q] = checkCoarse(*this, *staying[q]); a.dir[q] = dir[q];
  }
  forShape(*this, [&](auto shape) {
    using S = decltype(shape);
    if constexpr (S::NSF == 4)
      launch(restrict4_kernel<S::NSF, S::NCF, S::NVEC, S::NV>, nAgg, workGroup(*this).threads, a, (const float4 *)V, block_to_fine, blockVol, spin_bs, maskArg(*this, 0, 1), aggMapOf(*this));
  });
  flops_ += 4 * 8ull * fineSpin * fineColor * Nvec * fineVol;
}

}  // namespace quda
