// transfer_device.h — what transfer.hip (R and P of the solve phase) and transfer_setup.hip (building and inspecting V) share: the views of fine and coarse
// vectors, the order of the sites inside an aggregate with the masks of the Galerkin split, the work-group -> aggregate map, the loads of V (fp32 or fp16 mirror).
#pragma once

#include "transfer.h"

namespace quda {

constexpr int kMaxVec = 32;

// fine-vector element access: complex number sc of site x in one parity block of a planar field with NV reals per vector
template <int NV> __device__ __forceinline__ size_t fidx(int stride, int x, int sc) {
  const int r = 2 * sc;
  return ((size_t)(r / NV) * stride + x) * NV + (r % NV);
}

// the K complex components of fine site x into r[]: for the float4-plane order (NV = 4: components 2m, 2m + 1 share a plane entry)
// with one 16-byte load per pair — as 4-byte loads the gather of the four fine vectors of restrict4_kernel was 96 instructions per
// thread, each touching 32 cache lines per wave
template <int NV, int K> __device__ __forceinline__ void load_fine_site(float2 *r, const float *base, int stride, int x) {
  if (NV == 4 && K % 2 == 0) {
#pragma unroll
    for (int m = 0; m < K / 2; m++) {
      const float4 v = reinterpret_cast<const float4 *>(base)[(size_t)m * stride + x];
      r[2 * m] = make_float2(v.x, v.y); r[2 * m + 1] = make_float2(v.z, v.w);
    }
  } else {
#pragma unroll
    for (int k = 0; k < K; k++) { const size_t i = fidx<NV>(stride, x, k); r[k] = make_float2(base[i], base[i + 1]); }
  }
}

struct FineVec {
  float *v[2];  // even / odd parity block
  int stride, Vh;
};
struct CoarseVec {
  float *v[2];
  int stride, Vh;
};

// parity >= 0: `f` is a single-parity field holding that parity; the other parity is absent (nullptr): it restricts as zero
// and is not written by the prolongator (reference Transfer::setSiteSubset, lib/transfer.cpp:276-290)
static FineVec fineVec(const ColorSpinorField &f, int parity = -1) {
  if (f.Location() != QUDA_CUDA_FIELD_LOCATION || f.Precision() != QUDA_SINGLE_PRECISION)
    errorQuda("transfer operators work on fp32 device fields (precision %d)", f.Precision());
  ColorSpinorField &g = const_cast<ColorSpinorField &>(f);
  FineVec r;
  if (f.SiteSubset() == QUDA_FULL_SITE_SUBSET) {
    r.v[0] = (float *)g.Even().V(); r.v[1] = (float *)g.Odd().V();
  } else {
    if (parity != 0 && parity != 1) errorQuda("single-parity field without Transfer::setSiteSubset(QUDA_PARITY_SITE_SUBSET, parity)");
    r.v[parity] = (float *)g.V(); r.v[1 - parity] = nullptr;
  }
  r.stride = f.Stride(); r.Vh = f.VolumeCB();
  return r;
}

struct MaskArg {
  int dir;       // -1: no mask
  int boundary;  // 1: keep sites whose dir-neighbour is outside the aggregate, 0: inside
  int bs[4];
  int single[4]; // coarse extent 1 in that dimension: the neighbour always wraps into the same aggregate
  int pm;        // parity-major order of the sites inside an aggregate (Transfer::parityMajor), else lexicographic
};
// coordinates of site b of an aggregate.  Lexicographic (x fastest), or — parity-major, all block extents even — the even sites of the
// aggregate first, then the odd ones, each half in lexicographic order halved (the checkerboard numbering of the lattice applied to
// the block): a single-parity fine field (Transfer::setSiteSubset) then meets ONE contiguous half of every (component, vector pair)
// row of V, and the waves that own the absent parity issue no loads at all — half the V bytes for R and P of an even-odd cycle.
__device__ __forceinline__ void block_coords(int *y, const MaskArg &m, int b) {
  int l = b, p = 0;
  if (m.pm) {
    const int half = (m.bs[0] * m.bs[1] * m.bs[2] * m.bs[3]) >> 1;
    p = b >= half;
    l = 2 * (b - p * half);
  }
  y[0] = l % m.bs[0]; l /= m.bs[0];
  y[1] = l % m.bs[1]; l /= m.bs[1];
  y[2] = l % m.bs[2]; y[3] = l / m.bs[2];
  if (m.pm) y[0] += (p + y[1] + y[2] + y[3]) & 1;   // y[0] is even here: the site of the pair that has parity p
}

__device__ __forceinline__ bool mask_keep(const MaskArg &m, int b) {
  if (m.dir < 0) return true;
  const int mu = m.dir >> 1, fwd = !(m.dir & 1);
  int y[4];
  block_coords(y, m, b);
  const bool out = !m.single[mu] && (fwd ? y[mu] == m.bs[mu] - 1 : y[mu] == 0);
  return out == (m.boundary != 0);
}

// ---- block reduction of one float4 across the work-group (wave64 shuffles, then LDS across waves) ----
__device__ __forceinline__ float4 block_sum4(float4 v, float4 *lds) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    v.x += __shfl_down(v.x, off, 64); v.y += __shfl_down(v.y, off, 64);
    v.z += __shfl_down(v.z, off, 64); v.w += __shfl_down(v.w, off, 64);
  }
  const int wave = threadIdx.x >> 6, nw = (blockDim.x + 63) >> 6;
  __syncthreads();
  if ((threadIdx.x & 63) == 0) lds[wave] = v;
  __syncthreads();
  float4 r = lds[0];
  for (int w = 1; w < nw; w++) { r.x += lds[w].x; r.y += lds[w].y; r.z += lds[w].z; r.w += lds[w].w; }
  return r;
}

__device__ __forceinline__ bool mask_outside(const MaskArg &m, int b) {
  const int mu = m.dir >> 1, fwd = !(m.dir & 1);
  int y[4];
  block_coords(y, m, b);
  return !m.single[mu] && (fwd ? y[mu] == m.bs[mu] - 1 : y[mu] == 0);
}

typedef _Float16 vhalf4_t __attribute__((ext_vector_type(4)));
template <bool HALF> __device__ __forceinline__ float4 load_v(const void *V, size_t i) {
  if (HALF) {
    const vhalf4_t h = reinterpret_cast<const vhalf4_t *>(V)[i];
    return make_float4((float)h.x, (float)h.y, (float)h.z, (float)h.w);
  }
  // V is streamed once per kernel (24.5 GB at 48^3 x 96): non-temporal loads keep it from displacing the fine and coarse vectors the
  // same kernel reads and writes (prolongator 0.58 -> 0.76 of the HBM roofline at 32^4)
  typedef float f32x4_nt __attribute__((ext_vector_type(4)));
  const f32x4_nt t = __builtin_nontemporal_load(reinterpret_cast<const f32x4_nt *>(V) + i);
  return make_float4(t.x, t.y, t.z, t.w);
}

// work-group -> aggregate.  xgroup > 0: the four aggregates that are neighbours along x (xgroup = Xc[0] / 4 such groups per row) take
// four consecutive slots of ONE XCD (work-groups b, b + 8, b + 16, b + 24).  An aggregate 4 sites wide covers 2 consecutive
// checkerboard sites per row and parity, i.e. a 32-byte piece of every 128-byte line of the fine field; written a quarter at a
// time by work-groups far apart in the grid (neighbours along x differ in coarse parity: half a grid apart) every line went to
// memory in pieces once the field no longer fits the Infinity Cache — prolongator at 48^3 x 96: 0.56 of the HBM roofline against
// 0.76 at 32^4.  With the four quarters written from one L2 within microseconds the line leaves it whole.  The restrictors READ the
// fine vectors in the same 32-byte pieces (restrict4_kernel four of them at once): same order, so that three of the four pieces of a
// line are L2 hits.
struct AggMap { int xgroup, X0, X1, X2, Vh; };
__device__ __forceinline__ int aggregate_of_block(const AggMap &m) {
  const int b = blockIdx.x;
  if (!m.xgroup) return b;
  const int xcd = b & 7, within = b >> 3;
  int g = xcd + 8 * (within >> 2);
  const int r = within & 3;
  const int xg = g % m.xgroup; g /= m.xgroup;
  const int y = g % m.X1; g /= m.X1;
  const int z = g % m.X2; const int t = g / m.X2;
  const int x = 4 * xg + r;
  return ((x + y + z + t) & 1) * m.Vh + ((((t * m.X2 + z) * m.X1 + y) * m.X0 + x) >> 1);
}

typedef float f32x4_raw_t __attribute__((ext_vector_type(4)));
template <bool HALF> struct VRaw { typedef f32x4_raw_t type; };
template <> struct VRaw<true> { typedef vhalf4_t type; };
template <bool HALF> __device__ __forceinline__ typename VRaw<HALF>::type load_v_raw(const void *V, size_t i) {
  if constexpr (HALF) return reinterpret_cast<const vhalf4_t *>(V)[i];
  else return __builtin_nontemporal_load(reinterpret_cast<const f32x4_raw_t *>(V) + i);
}
__device__ __forceinline__ float4 v_unpack(const f32x4_raw_t &t) { return make_float4(t.x, t.y, t.z, t.w); }
__device__ __forceinline__ float4 v_unpack(const vhalf4_t &h) { return make_float4((float)h.x, (float)h.y, (float)h.z, (float)h.w); }

static CoarseVec coarseVec(const ColorSpinorField &c) {
  FineVec f = fineVec(c);
  CoarseVec r;
  r.v[0] = f.v[0]; r.v[1] = f.v[1]; r.stride = f.stride; r.Vh = f.Vh;
  return r;
}

}  // namespace quda
