// fine_block.hip — multi-right-hand-side fine operator on block fields for gfx950 (MI355X): fine_block_kernel and the reduction of its
// epilogue inner products, the dense clover-twist site matrices it applies, and their launchers (include/dslash.h applyFineBlock*).
// Shares only the spin algebra (dslash_arg.h) with the single-vector stencil of dslash.hip.
#include "dslash.h"

#include <cstring>
#include <type_traits>

#include "blas.h"
#include "block.h"
#include "device_io.h"
#include "dslash_arg.h"
#include "dslash_launch.h"

namespace quda {

// ================================================================================================
// Multi-right-hand-side full operator on block fields (block.h layout: [site][spin-colour j][rhs i] float2), fp32, recon 18:
//     out(x) = (1 + i a g5) in(x) - kappa sum_{8 hops} U P in(x + mu)          on the sites of ONE parity per launch
// for NRHS right-hand sides per link load — the operator behind the lockstep null-vector solves of the multigrid setup
// (multigrid.cpp; reference MG::generateNullVectors, lib/multigrid.cpp:693-779, where every one of the Nvec BiCGstab solves
// re-reads the links: 576 of the 768 B per site of the fp32 stencil).  One thread per (site, right-hand side); the links of the
// work-group's sites are staged once in LDS (full-line loads from the planar link blocks, broadcast reads), the spinor panels are
// read as 8-byte pairs, NRHS x 8 B contiguous per (site, component).  NRHS = 8 keeps the panel of a site at 768 B so that the
// neighbour re-use still fits the caches in the XCD-slab order of the single-vector kernel: 72 + ~110 + 96 + 96 B per site and
// right-hand side instead of 768 + 96.
// ================================================================================================
struct BlockOrder {   // the plane-tiled XCD mapping of dslash_kernel for work-groups of `bs` consecutive checkerboard sites
  int tiled, P, nxz, Zs, Ts, tz, tt, Z;
  FastDiv dNxz, dPerTile, dNtz, dPTt, dTt;
  __device__ __forceinline__ int map(int b) const {
    if (!tiled) return b;
    const int xcd = b & 7, within = b >> 3;
    const uint32_t xt = dNxz.div((uint32_t)xcd), xz = (uint32_t)xcd - xt * (uint32_t)nxz;
    const uint32_t tile = dPerTile.div((uint32_t)within), r = (uint32_t)within - tile * dPerTile.d;
    const uint32_t tile_t = dNtz.div(tile), tile_z = tile - tile_t * dNtz.d;
    const uint32_t zi = dPTt.div(r), r2 = r - zi * dPTt.d;
    const uint32_t yc = dTt.div(r2), ti = r2 - yc * dTt.d;
    const int z = (int)xz * Zs + (int)tile_z * tz + (int)zi, t = (int)xt * Ts + (int)tile_t * tt + (int)ti;
    return (t * Z + z) * P + (int)yc;
  }
};
static BlockOrder makeBlockOrder(const LatticeGeom &g, int bs) {
  BlockOrder o;
  memset(&o, 0, sizeof(o));
  const int plane = g.Xh * g.X[1];
  if (plane % bs || (g.Vh / bs) % 8) return o;
  const XcdSplit x = xcdPlaneSplit(g);
  if (!x.nxz) return o;
  const int nxz = x.nxz;
  o.tiled = 1; o.P = plane / bs; o.nxz = nxz; o.Zs = x.Zs; o.Ts = x.Ts; o.tz = o.Zs; o.tt = 1; o.Z = g.X[2];
  o.dNxz = FastDiv((uint32_t)nxz); o.dPerTile = FastDiv((uint32_t)(o.P * o.tz * o.tt)); o.dNtz = FastDiv((uint32_t)(o.Zs / o.tz));
  o.dPTt = FastDiv((uint32_t)(o.P * o.tt)); o.dTt = FastDiv((uint32_t)o.tt);
  return o;
}
static int fineBlockSitesPerGroup(int nrhs) { return nrhs == 24 ? 8 : 256 / nrhs; }   // SPB of fine_block_kernel
bool fineBlockOrderTiled(const LatticeGeom &g, int nrhs) { return makeBlockOrder(g, fineBlockSitesPerGroup(nrhs)).tiled != 0; }

struct FineBlockArg {
  float2 *out;             // panels of the output parity
  const float2 *in_same;   // panels of the same parity (twist term)
  const float2 *in_other;  // panels of the other parity (hops)
  const char *gauge;       // this parity's 8 direction blocks
  size_t link_bytes;
  int g_stride;
  int Vh, Xh, Y, Z, T, parity;
  FastDiv dXh, dY, dZ;
  // out = s0 (1 + i a0 g5) in_same + k1 (1 + i a1 g5) [sum of the 8 hops of in_other]; s0 = 0: in_same is not read
  float s0, a0, k1, a1;
  // twisted clover (kernel template CL): a dense site matrix [site][chirality][6 x 6 complex] of the OUTPUT parity replaces the factor
  // (1 + i a1 g5) of the hop sum (CL = 1: (A + i a g5)^-1 of the even-odd preconditioned operator) or (1 + i a0 g5) of in_same
  // (CL = 2: A + i a g5 of the full operator)
  const float *tmat;
  // grid-decomposed lattice: a hop across a partitioned face reads the neighbour rank's panel from the ghost zone of in_other (block.h
  // BlockGhost, parity field): ghostBase[d][k] = panel index, RELATIVE to in_other, of zone [d][k]
  int commMask;
  int ghostBase[4][2];
  BlockOrder order;
  // compact work-group tiles (NRHS = 8, 32 sites per work-group): 4 x 4 x 2 x 2 lattice sites = 32 sites of the output parity instead of 32
  // consecutive checkerboard sites.  The 256 neighbour panels a work-group reads are then only 128 distinct ones (every input site inside
  // the tile is the neighbour of up to 8 of its output sites), so half of the requests can be served by the CU's L1 instead of the L2:
  // the kernel is bound by the latency of its L2 requests (~100 KB in flight per CU), not by HBM.  tile = 0: the linear mapping.
  // MEASURED (round 3, 48^4, tools/fine_block_timing.py): 2278 us per parity launch with the tiles against 2027 us with the linear mapping
  // (twisted clover 2568 / 2281) — the scattered link staging and the lost XCD z-slab order cost more than the L1 hits gain; kept as an
  // opt-in (QUDA_AMD_BLOCK_FINE_TILE=1) for the record, the linear mapping stays the default.
  int tile, tilesX, tilesY, tilesZ;
  // inner products in the epilogue (NRHS = 8; dslash.h FineBlockDots): per right-hand side, summed over the work-group's sites in site order,
  // one row of partials per work-group.  dotMode 1: (a, out) [2 sums]; 2: (out, same) [2], |out|^2 [1], (a, same) [2], (a, out) [2]
  const float2 *dotA;
  double *dotPart;
  int dotMode;
  // 12-real links (recon-12): the third row is rebuilt while the links are staged; tsign_*: sign of the rebuilt row of the t links that carry the
  // folded antiperiodic boundary (forward links of the last time slice, backward links of the first), as in DslashArg
  int recon;
  float tsign_fwd, tsign_bwd;
};

// XY = 1 (NRHS = 8, CL = 0): the work-group is an 8 (x, checkerboard) x 4 (y) tile of one (z, t) plane and the panels its x and y hops need — 56 instead of
// 4 x 32 — are fetched ONCE into LDS (dynamic, 60 slots of 896 B); the z and t hops keep the register pipeline.  The kernel is bound by its L2 -> L1 requests
// (profiles/r03_fine_block_kernel_pmc.log): this takes a quarter of them out, at the price of two instead of four work-groups per CU (72.7 KB of LDS, 138 registers).
// MEASURED (48^4, tools/fine_block_timing.py): 2459 us per parity launch against 1874 us for the linear mapping — the lost occupancy costs more than the
// requests saved.  Correct under every partition mask (tools/fine_block_xy_check.py); kept as QUDA_AMD_BLOCK_FINE_XYTILE=1 for the record, off by default.
template <int NRHS, int CL = 0, int XY = 0> __global__ void __launch_bounds__(256) fine_block_kernel(const FineBlockArg arg) {
  constexpr int SPB = NRHS == 24 ? 8 : 256 / NRHS;   // sites per work-group (192 threads for 24 right-hand sides, else 256)
  constexpr int USTR = 8 * 18 + 4;                    // floats per site of staged links: 148 = 20 mod 32, the up to 8 sites of a wave start on 8 different banks
  constexpr int TSTR = 144 + 4;                       // the dense clover-twist matrices of a site: 2 x 36 complex, same bank spread
  __shared__ __attribute__((aligned(16))) float ulds[SPB * USTR];
  __shared__ __attribute__((aligned(16))) float tlds[CL ? SPB * TSTR : 4];
  const int s = threadIdx.x / NRHS, i = threadIdx.x - s * NRHS;
  extern __shared__ __attribute__((aligned(16))) float plds[];   // XY: staged x / y neighbour panels
  constexpr int PSTR = 224;   // floats per staged panel: 192 + 32 — consecutive slots start 128 B apart modulo the 256-byte bank row (two sites per 16-lane phase of a ds_read_b128)
  // site ss of this work-group -> checkerboard index
  int idx0 = 0, tbase = 0;
  int tX0 = 0, tY0 = 0, tZ = 0, tT = 0;
  if (XY) {
    const int m = arg.order.map(blockIdx.x), P = arg.tilesX * arg.tilesY;   // (t Z + z) P + tile of the plane, in the XCD-slab order of the linear mapping
    const int yc = m % P, zt = m / P;
    tZ = zt % arg.Z; tT = zt / arg.Z;
    tX0 = (yc % arg.tilesX) * 8; tY0 = (yc / arg.tilesX) * 4;
    tbase = ((tT * arg.Z + tZ) * arg.Y + tY0) * arg.Xh + tX0;
  } else if (NRHS == 8 && arg.tile) {
    // work-groups dealt to the XCDs in contiguous eighths of the tile list (t slowest), tile -> its corner
    const int nwg = (int)gridDim.x, b = (int)blockIdx.x;
    int tl = (nwg & 7) == 0 ? (b & 7) * (nwg >> 3) + (b >> 3) : b;
    const int tx = tl % arg.tilesX; tl /= arg.tilesX;
    const int ty = tl % arg.tilesY; tl /= arg.tilesY;
    const int tz = tl % arg.tilesZ; const int tt = tl / arg.tilesZ;
    tbase = ((2 * tt * arg.Z + 2 * tz) * arg.Y + 4 * ty) * arg.Xh + 2 * tx;
  } else {
    idx0 = arg.order.map(blockIdx.x) * SPB;
  }
  auto site_of = [&](int ss) -> int {
    if (XY) return tbase + (ss >> 3) * arg.Xh + (ss & 7);   // ss = y_l 8 + xh_l
    if (NRHS == 8 && arg.tile) {   // ss = ((t_l 2 + z_l) 4 + y_l) 2 + xh_l
      const int xl = ss & 1, yl = (ss >> 1) & 3, zl = (ss >> 3) & 1, tl = ss >> 4;
      return tbase + ((tl * arg.Z + zl) * arg.Y + yl) * arg.Xh + xl;
    }
    return idx0 + ss;
  };
  const int idx = site_of(s);
  if (CL) {   // 36 float4 per site, contiguous in memory
    for (int e = threadIdx.x; e < 36 * SPB; e += blockDim.x) {
      const int ss = e / 36, q = e - ss * 36;
      typedef float f32x4_t __attribute__((ext_vector_type(4)));
      const int sidx = site_of(ss);
      if (sidx < arg.Vh) *reinterpret_cast<f32x4_t *>(&tlds[ss * TSTR + 4 * q]) = __builtin_nontemporal_load(reinterpret_cast<const f32x4_t *>(arg.tmat) + (size_t)sidx * 36 + q);
    }
  }
  // ---- stage the links of the SPB sites: [site][dir][18]; planes 0..3 are float4, plane 4 the trailing float2 ----
  if (arg.recon == 12) {
    // one thread per (site, direction): two stored rows in three 16-byte planes, the third rebuilt here — once per work-group, for NRHS right-hand sides
    for (int e = threadIdx.x; e < 8 * SPB; e += blockDim.x) {
      const int ss = e % SPB, d = e / SPB;
      const int sidx = site_of(ss);
      if (sidx < arg.Vh) {
        float sign = 1.f;
        if (d >= 6) {
          const int tt = sidx / (arg.Xh * arg.Y * arg.Z);
          sign = d == 6 ? (tt == arg.T - 1 ? arg.tsign_fwd : 1.f) : (tt == 0 ? arg.tsign_bwd : 1.f);
        }
        float U[18];
        Link<float, 12>::load(U, arg.gauge + (size_t)d * arg.link_bytes, arg.g_stride, sidx, sign);
        float *dst = &ulds[ss * USTR + d * 18];
#pragma unroll
        for (int k = 0; k < 18; k++) dst[k] = U[k];
      }
    }
  } else
  for (int e = threadIdx.x; e < 8 * 5 * SPB; e += blockDim.x) {
    const int ss = e % SPB, pl = (e / SPB) % 5, d = e / (5 * SPB);
    const char *blk = arg.gauge + (size_t)d * arg.link_bytes;
    float *dst = &ulds[ss * USTR + d * 18 + pl * 4];
    const int sidx = site_of(ss);
    if (sidx < arg.Vh) {
      if (pl < 4) {
        const float4 v = reinterpret_cast<const float4 *>(blk)[(size_t)pl * arg.g_stride + sidx];
        dst[0] = v.x; dst[1] = v.y; dst[2] = v.z; dst[3] = v.w;
      } else {
        const float2 v = reinterpret_cast<const float2 *>(blk + (size_t)4 * arg.g_stride * 16)[sidx];
        dst[0] = v.x; dst[1] = v.y;
      }
    }
  }
  if (XY) {
    // slots (row r = 0..5: y0 - 1 .. y0 + 4, column c = 0..9: xh0 - 1 .. xh0 + 8), 48 sixteen-byte words each; the corner slots belong to no hop (they are
    // filled with a valid panel all the same: unconditional loads, issued back to back, then the LDS stores).  A slot outside the lattice wraps around or,
    // on a partitioned dimension, is the neighbour rank's panel in the ghost zone — column 0 only serves the -x hop, column 9 +x, row 0 -y, row 5 +y.
    float4 stg[12];
#pragma unroll
    for (int q = 0; q < 12; q++) {
      int e = (int)threadIdx.x + 256 * q;
      e = e < 2880 ? e : 2879;
      const int slot = e / 48, w = e - slot * 48, r = slot / 10, c = slot - r * 10;
      int yy = tY0 + r - 1, xx = tX0 + c - 1;
      long pn = -1;
      if (xx < 0) { if (arg.commMask & 1) pn = arg.ghostBase[0][0] + ((((tT * arg.Z + tZ) * arg.Y + (yy < 0 ? 0 : (yy >= arg.Y ? arg.Y - 1 : yy)))) >> 1); else xx = arg.Xh - 1; }
      else if (xx >= arg.Xh) { if (arg.commMask & 1) pn = arg.ghostBase[0][1] + ((((tT * arg.Z + tZ) * arg.Y + (yy < 0 ? 0 : (yy >= arg.Y ? arg.Y - 1 : yy)))) >> 1); else xx = 0; }
      if (pn < 0) {
        if (yy < 0) { if (arg.commMask & 2) pn = arg.ghostBase[1][0] + (tT * arg.Z + tZ) * arg.Xh + xx; else yy = arg.Y - 1; }
        else if (yy >= arg.Y) { if (arg.commMask & 2) pn = arg.ghostBase[1][1] + (tT * arg.Z + tZ) * arg.Xh + xx; else yy = 0; }
      }
      if (pn < 0) pn = ((long)(tT * arg.Z + tZ) * arg.Y + yy) * arg.Xh + xx;
      stg[q] = reinterpret_cast<const float4 *>(arg.in_other + pn * 12 * NRHS)[w];
    }
#pragma unroll
    for (int q = 0; q < 12; q++) {
      const int e = (int)threadIdx.x + 256 * q;
      if (e < 2880) { const int slot = e / 48, w = e - slot * 48; *reinterpret_cast<float4 *>(&plds[slot * PSTR + 4 * w]) = stg[q]; }
    }
  }
  __syncthreads();
  if (idx >= arg.Vh) return;
  // coordinates and neighbours (as stencil_site)
  const uint32_t za = arg.dXh.div((uint32_t)idx);
  const int xh = idx - (int)za * arg.Xh;
  const uint32_t zb = arg.dY.div(za);
  const int y = (int)za - (int)zb * arg.Y;
  const int t = (int)arg.dZ.div(zb);
  const int z = (int)zb - t * arg.Z;
  const int xodd = (y + z + t + arg.parity) & 1;
  const int Xh = arg.Xh, sy = Xh, sz = Xh * arg.Y, st = Xh * arg.Y * arg.Z;
  int nb[8];
  nb[0] = xodd ? (xh == Xh - 1 ? idx - (Xh - 1) : idx + 1) : idx;
  nb[1] = xodd ? idx : (xh == 0 ? idx + (Xh - 1) : idx - 1);
  nb[2] = y == arg.Y - 1 ? idx - (arg.Y - 1) * sy : idx + sy;
  nb[3] = y == 0 ? idx + (arg.Y - 1) * sy : idx - sy;
  nb[4] = z == arg.Z - 1 ? idx - (arg.Z - 1) * sz : idx + sz;
  nb[5] = z == 0 ? idx + (arg.Z - 1) * sz : idx - sz;
  nb[6] = t == arg.T - 1 ? idx - (arg.T - 1) * st : idx + st;
  nb[7] = t == 0 ? idx + (arg.T - 1) * st : idx - st;
  if (arg.commMask) {   // face index: the other three coordinates, lexicographic, halved (block.hip face_site_to_panel packs in this order)
    if (arg.commMask & 1) {
      const int f = ((t * arg.Z + z) * arg.Y + y) >> 1;
      if (xodd && xh == Xh - 1) nb[0] = arg.ghostBase[0][1] + f;
      if (!xodd && xh == 0) nb[1] = arg.ghostBase[0][0] + f;
    }
    if (arg.commMask & 2) {
      const int f = (t * arg.Z + z) * Xh + xh;
      if (y == arg.Y - 1) nb[2] = arg.ghostBase[1][1] + f;
      if (y == 0) nb[3] = arg.ghostBase[1][0] + f;
    }
    if (arg.commMask & 4) {
      const int f = (t * arg.Y + y) * Xh + xh;
      if (z == arg.Z - 1) nb[4] = arg.ghostBase[2][1] + f;
      if (z == 0) nb[5] = arg.ghostBase[2][0] + f;
    }
    if (arg.commMask & 8) {
      const int f = (z * arg.Y + y) * Xh + xh;
      if (t == arg.T - 1) nb[6] = arg.ghostBase[3][1] + f;
      if (t == 0) nb[7] = arg.ghostBase[3][0] + f;
    }
  }

  float acc[24];
#pragma unroll
  for (int k = 0; k < 24; k++) acc[k] = 0.f;
  const float *U0 = &ulds[s * USTR];
  // Same register discipline as stencil_site: two panel buffers, the loads of hop d + 1 issued before the arithmetic of hop d,
  // fenced so the compiler neither hoists all 108 loads to the top (256 registers, one wave per SIMD: 12.7 ms per launch at
  // 48^3 x 96, four times the bandwidth bound) nor serialises them.
  // The panels travel as 16-byte words, and the block field is PAIR-MAJOR (block.h): word ((site 6 + k) NRHS + i) holds components 2k, 2k + 1 of
  // right-hand side i, so a lane's six loads are its own 12 components and the NRHS lanes of a site still read whole 128-byte lines (8-byte
  // loads run at 0.54-0.70 of the 16-byte rate on gfx950, and the kernel is bound by its L2 -> L1 requests).  History: with the rhs-fastest
  // order the lane pair (i, i ^ 1) shared its loads and transposed 2 x 2 by DPP — 620 of the kernel's ~1950 vector instructions.
  float4 pA[6], pB[6];
#ifndef QA_FB_PANEL_POLICY
#define QA_FB_PANEL_POLICY 0   // 0 plain loads, 1 non-temporal (L1 bypassed), 2 sc1 raw buffer loads: measured, see DESIGN 3
#endif
  auto load_panel = [&](float4 *raw, const float2 *base, int site) {
    const float4 *p = reinterpret_cast<const float4 *>(base) + (long)site * 6 * NRHS + i;
#pragma unroll
    for (int k = 0; k < 6; k++) {
      if (QA_FB_PANEL_POLICY == 1) {
        typedef float f32x4_t __attribute__((ext_vector_type(4)));
        const f32x4_t v = __builtin_nontemporal_load(reinterpret_cast<const f32x4_t *>(p + k * NRHS));
        raw[k] = make_float4(v.x, v.y, v.z, v.w);
      } else {
        raw[k] = p[k * NRHS];
      }
    }
  };
  auto unpack_panel = [&](float *psi, const float4 *raw) {
#pragma unroll
    for (int k = 0; k < 6; k++) { psi[4 * k] = raw[k].x; psi[4 * k + 1] = raw[k].y; psi[4 * k + 2] = raw[k].z; psi[4 * k + 3] = raw[k].w; }
  };
  auto hop = [&](auto DIRC, const float4 *raw) {
    constexpr int DIR = decltype(DIRC)::value, MU = DIR / 2;
    float psi[24], h[12], g[12], U[18];
    unpack_panel(psi, raw);
#pragma unroll
    for (int k = 0; k < 18; k++) U[k] = U0[DIR * 18 + k];
    const float sgn = (DIR & 1) ? -1.f : 1.f;
    spin_project<MU>(h, psi, sgn);
    su3_mv(g, U, h);
    su3_mv(g + 6, U, h + 6);
    spin_reconstruct<MU>(acc, g, sgn);
  };
#define FB_FENCE() __builtin_amdgcn_sched_barrier(0)
#define FB_PIN() _Pragma("unroll") for (int k_ = 0; k_ < 24; k_++) asm volatile("" : "+v"(acc[k_]))
#define FB_LD(B, D) load_panel(p##B, arg.in_other, nb[D])
#define FB_CP(B, D) FB_FENCE(); hop(std::integral_constant<int, D>{}, p##B); FB_PIN(); FB_FENCE()
  if constexpr (XY) {
    // z / t panels requested first, the four x / y hops out of LDS while they travel
    float4 pC[6];
    const int r0 = (s >> 3) + 1, c0 = (s & 7) + 1;
    auto load_lds = [&](float4 *raw, int slot) {
      const float *b = &plds[slot * PSTR + 4 * i];
#pragma unroll
      for (int k = 0; k < 6; k++) raw[k] = *reinterpret_cast<const float4 *>(b + k * 4 * NRHS);   // word k NRHS + i of the panel
    };
    FB_LD(A, 4); FB_LD(B, 5);
    load_lds(pC, r0 * 10 + c0 + (xodd ? 1 : 0)); FB_CP(C, 0);
    load_lds(pC, r0 * 10 + c0 - (xodd ? 0 : 1)); FB_CP(C, 1);
    load_lds(pC, (r0 + 1) * 10 + c0); FB_CP(C, 2);
    load_lds(pC, (r0 - 1) * 10 + c0); FB_CP(C, 3);
    FB_CP(A, 4); FB_LD(A, 6); FB_CP(B, 5); FB_LD(B, 7);
    FB_CP(A, 6);
    if (arg.s0 != 0.f) load_panel(pA, arg.in_same, idx);
    FB_CP(B, 7);
  } else {
  FB_LD(A, 0); FB_LD(B, 1); FB_CP(A, 0); FB_LD(A, 2); FB_CP(B, 1); FB_LD(B, 3); FB_CP(A, 2);
  FB_LD(A, 4); FB_CP(B, 3); FB_LD(B, 5); FB_CP(A, 4); FB_LD(A, 6); FB_CP(B, 5); FB_LD(B, 7);
  FB_CP(A, 6);
  if (arg.s0 != 0.f) load_panel(pA, arg.in_same, idx);   // the site's own panel travels while the last hop is computed
  FB_CP(B, 7);
  }
#undef FB_FENCE
#undef FB_PIN
#undef FB_LD
#undef FB_CP
  float same[24];
  if (arg.s0 != 0.f) unpack_panel(same, pA);
  float outv[24];
  if (CL) {
    // dense 6 x 6 complex matrix per chirality on the hop sum (CL = 1) or on the site's own panel (CL = 2); rows read as three
    // 16-byte LDS words, the same address for the NRHS lanes of a site
    float *src = CL == 1 ? acc : same;
    float res[24];
    const float *T0 = &tlds[s * TSTR];
#pragma unroll
    for (int chi = 0; chi < 2; chi++)
#pragma unroll
      for (int r = 0; r < 6; r++) {
        float re = 0.f, im = 0.f;
#pragma unroll
        for (int q = 0; q < 3; q++) {
          const float4 m = *reinterpret_cast<const float4 *>(&T0[(chi * 6 + r) * 12 + 4 * q]);
          const float *v = &src[12 * chi + 4 * q];
          re += m.x * v[0] - m.y * v[1] + m.z * v[2] - m.w * v[3];
          im += m.x * v[1] + m.y * v[0] + m.z * v[3] + m.w * v[2];
        }
        res[12 * chi + 2 * r] = re; res[12 * chi + 2 * r + 1] = im;
      }
#pragma unroll
    for (int j = 0; j < 12; j++) {
      float re, im;
      if (CL == 1) {
        re = arg.k1 * res[2 * j]; im = arg.k1 * res[2 * j + 1];
        if (arg.s0 != 0.f) {
          const float a0 = (j < 6 ? 1.f : -1.f) * arg.a0;
          re += arg.s0 * (same[2 * j] - a0 * same[2 * j + 1]); im += arg.s0 * (same[2 * j + 1] + a0 * same[2 * j]);
        }
      } else {
        const float a1 = (j < 6 ? 1.f : -1.f) * arg.a1;
        re = arg.k1 * (acc[2 * j] - a1 * acc[2 * j + 1]) + arg.s0 * res[2 * j];
        im = arg.k1 * (acc[2 * j + 1] + a1 * acc[2 * j]) + arg.s0 * res[2 * j + 1];
      }
      outv[2 * j] = re; outv[2 * j + 1] = im;
    }
  } else {
#pragma unroll
    for (int j = 0; j < 12; j++) {
      const float sg = j < 6 ? 1.f : -1.f;   // g5 = diag(+,+,-,-): spins 0,1 are components 0..5
      const float a1 = sg * arg.a1;
      float re = arg.k1 * (acc[2 * j] - a1 * acc[2 * j + 1]), im = arg.k1 * (acc[2 * j + 1] + a1 * acc[2 * j]);
      if (arg.s0 != 0.f) {
        const float a0 = sg * arg.a0;
        re += arg.s0 * (same[2 * j] - a0 * same[2 * j + 1]); im += arg.s0 * (same[2 * j + 1] + a0 * same[2 * j]);
      }
      outv[2 * j] = re; outv[2 * j + 1] = im;
    }
  }
  if (NRHS <= 8 && arg.dotMode) {   // uniform
    // the two dot products of a BiCGstab half step where their operands already are: `out` and the site's own input panel in registers, one more
    // panel (a = r0) loaded — instead of separate passes over the fields (blockblas::cDot / bicgstabDots: 2 resp. 3 field reads); mode 3: the
    // two sums of a minimal-residual step, (out, same) and |out|^2, nothing loaded at all
    float av[24];
    if (arg.dotMode != 3) {
      float4 ra[6];
      load_panel(ra, arg.dotA, idx);
      unpack_panel(av, ra);
    }
    const int ns = arg.dotMode == 1 ? 2 : (arg.dotMode == 3 ? 3 : 7);
    // the products of two fp32 numbers are exact in fp64 and the site sums are taken in fp64: the sums carry only the rounding of their fp64
    // additions.  (Site sums in fp32 were off by ~2e-8 of the sum of the absolute values of their terms; the minimal-residual coefficients
    // formed from them then differ from the exact ones in BOTH parts by that much of |alpha|, which an element-wise comparison of the update
    // with its reference sees amplified by |alpha| / |Im alpha|.)
    double sm[7] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    // one component at a time, its operands taken through an opaque copy and fenced: the conversions to fp64 stay next to their use
    auto dbl = [](float v) -> double { asm volatile("" : "+v"(v)); return (double)v; };
#pragma unroll
    for (int j = 0; j < 12; j++) {
      const double orr = dbl(outv[2 * j]), oi = dbl(outv[2 * j + 1]);
      if (arg.dotMode != 1) {
        const double sr = dbl(same[2 * j]), si = dbl(same[2 * j + 1]);
        sm[0] += orr * sr + oi * si; sm[1] += orr * si - oi * sr;    // conj(out) same
        sm[2] += orr * orr + oi * oi;
        if (arg.dotMode == 2) {
          const double ar = dbl(av[2 * j]), ai = dbl(av[2 * j + 1]);
          sm[3] += ar * sr + ai * si; sm[4] += ar * si - ai * sr;      // conj(a) same
          sm[5] += ar * orr + ai * oi; sm[6] += ar * oi - ai * orr;    // conj(a) out
        }
      } else {
        const double ar = dbl(av[2 * j]), ai = dbl(av[2 * j + 1]);
        sm[0] += ar * orr + ai * oi; sm[1] += ar * oi - ai * orr;      // conj(a) out
      }
      __builtin_amdgcn_sched_barrier(0);
    }
    __syncthreads();   // every wave is through its hops: the staged links are dead, their LDS holds the partial sums now
    static_assert(NRHS > 8 || sizeof(ulds) >= 7 * 256 * sizeof(double), "the partial sums must fit the staged links' LDS");
    double *red = reinterpret_cast<double *>(ulds);   // 7 x 256 doubles = 14 KB of the >= 18.5 KB of staged links
    for (int k = 0; k < ns; k++) red[k * 256 + threadIdx.x] = sm[k];
    __syncthreads();
    if ((int)threadIdx.x < ns * NRHS) {
      const int k = threadIdx.x / NRHS, ii = threadIdx.x - k * NRHS;
      int nact = SPB;
      if (!arg.tile) { const int left = arg.Vh - idx0; nact = left < SPB ? left : SPB; }
      double t = 0.0;
      for (int ss = 0; ss < nact; ss++) t += red[k * 256 + ss * NRHS + ii];
      arg.dotPart[((size_t)blockIdx.x * ns + k) * NRHS + ii] = t;
    }
  }
  float4 *o = reinterpret_cast<float4 *>(arg.out) + (size_t)idx * 6 * NRHS + i;
#pragma unroll
  for (int k = 0; k < 6; k++) o[k * NRHS] = make_float4(outv[4 * k], outv[4 * k + 1], outv[4 * k + 2], outv[4 * k + 3]);
}

// Dense clover-twist matrices for fine_block_kernel: per site of one parity and chirality the 6 x 6 complex matrix
//     A + i a s      (s = +1 upper, -1 lower chirality; inverse = false)      or its inverse      (inverse = true)
// from the packed Hermitian clover blocks.  The inverse is a Gauss-Jordan elimination in fp64 on the matrix itself, not the
// stored (A^2 + mu2)^-1 field (reference lib/clover_invert.cu:56-85), so it is exact for the a it is given — the multigrid setup may
// run with a rescaled mu (delta_muPR, reference lib/interface_quda.cpp:2196-2211).  One thread per (site, chirality).
__global__ void __launch_bounds__(128) clover_twist_dense_kernel(float *out, const void *clA, int cl_stride, int Vh, double a, int inverse) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= 2 * Vh) return;
  const int idx = e >> 1, chi = e & 1;
  float C[36];
  Planar<float, 36>::load(C, (const char *)clA + (size_t)chi * 36 * sizeof(float) * cl_stride, cl_stride, idx, nullptr, 0);
  double mr[6][6], mi[6][6];
  for (int i = 0; i < 6; i++)
    for (int j = 0; j < 6; j++) {
      if (i == j) { mr[i][j] = C[i]; mi[i][j] = chi ? -a : a; }
      else if (j < i) { const int k = 15 - (6 - j) * (5 - j) / 2 + i - j - 1; mr[i][j] = C[6 + 2 * k]; mi[i][j] = C[6 + 2 * k + 1]; }
      else { const int k = 15 - (6 - i) * (5 - i) / 2 + j - i - 1; mr[i][j] = C[6 + 2 * k]; mi[i][j] = -C[6 + 2 * k + 1]; }
    }
  float *o = out + ((size_t)idx * 2 + chi) * 72;
  if (!inverse) {
    for (int i = 0; i < 6; i++) for (int j = 0; j < 6; j++) { o[(i * 6 + j) * 2] = (float)mr[i][j]; o[(i * 6 + j) * 2 + 1] = (float)mi[i][j]; }
    return;
  }
  // the Hermitian part A is positive definite on any sensible field and i a s only adds to the diagonal: no pivoting needed, but
  // the largest remaining diagonal element is taken anyway
  double vr[6][6], vi[6][6];
  for (int i = 0; i < 6; i++) for (int j = 0; j < 6; j++) { vr[i][j] = i == j ? 1.0 : 0.0; vi[i][j] = 0.0; }
  for (int c = 0; c < 6; c++) {
    int p = c;
    double best = mr[c][c] * mr[c][c] + mi[c][c] * mi[c][c];
    for (int r = c + 1; r < 6; r++) { const double m2 = mr[r][c] * mr[r][c] + mi[r][c] * mi[r][c]; if (m2 > best) { best = m2; p = r; } }
    if (p != c)
      for (int j = 0; j < 6; j++) {
        double t = mr[c][j]; mr[c][j] = mr[p][j]; mr[p][j] = t; t = mi[c][j]; mi[c][j] = mi[p][j]; mi[p][j] = t;
        t = vr[c][j]; vr[c][j] = vr[p][j]; vr[p][j] = t; t = vi[c][j]; vi[c][j] = vi[p][j]; vi[p][j] = t;
      }
    const double dr = mr[c][c] / best, di = -mi[c][c] / best;   // 1 / pivot
    for (int j = 0; j < 6; j++) {
      double xr = mr[c][j] * dr - mi[c][j] * di, xi = mr[c][j] * di + mi[c][j] * dr; mr[c][j] = xr; mi[c][j] = xi;
      xr = vr[c][j] * dr - vi[c][j] * di; xi = vr[c][j] * di + vi[c][j] * dr; vr[c][j] = xr; vi[c][j] = xi;
    }
    for (int r = 0; r < 6; r++) {
      if (r == c) continue;
      const double fr = mr[r][c], fi = mi[r][c];
      for (int j = 0; j < 6; j++) {
        mr[r][j] -= fr * mr[c][j] - fi * mi[c][j]; mi[r][j] -= fr * mi[c][j] + fi * mr[c][j];
        vr[r][j] -= fr * vr[c][j] - fi * vi[c][j]; vi[r][j] -= fr * vi[c][j] + fi * vr[c][j];
      }
    }
  }
  for (int i = 0; i < 6; i++) for (int j = 0; j < 6; j++) { o[(i * 6 + j) * 2] = (float)vr[i][j]; o[(i * 6 + j) * 2 + 1] = (float)vi[i][j]; }
}

void cloverTwistDense(float *out, const CloverField &C, int parity, double a, bool inverse) {
  if (C.precision != QUDA_SINGLE_PRECISION) errorQuda("dense clover-twist matrices are built from an fp32 clover field (got precision %d)", C.precision);
  const int Vh = C.geom.Vh;
  hipLaunchKernelGGL(clover_twist_dense_kernel, dim3((2 * Vh + 127) / 128), dim3(128), 0, computeStream(), out, C.A(parity), C.stride, Vh, a, inverse ? 1 : 0);
  HIP_CHECK(hipGetLastError());
}

bool fineBlockSupported(const GaugeField &U, int nrhs) {
  if (U.precision != QUDA_SINGLE_PRECISION || (U.reconstruct != QUDA_RECONSTRUCT_NO && U.reconstruct != QUDA_RECONSTRUCT_12)) return false;
  if (nrhs != 4 && nrhs != 8 && nrhs != 16 && nrhs != 24 && nrhs != 32) return false;
  static int off = -1;
  if (off < 0) { const char *e = getenv("QUDA_AMD_BLOCK_FINE"); off = (e && !atoi(e)) ? 1 : 0; }
  return !off;
}

// one parity of the generalised multi-right-hand-side stencil:
//   out(x) = s0 (1 + i a0 g5) in_same(x) + k1 (1 + i a1 g5) sum_{8 hops} U P in_other(x + mu)       x of parity `parity`
// all three fields are single-parity block panels [Vh][12][nrhs]; in_same may be nullptr when s0 = 0
// ---- epilogue inner products of fine_block_kernel: work-group partials -> 128 chunk sums -> pinned host memory, in a fixed order ----
static double *g_fbPart = nullptr, *g_fbPart2 = nullptr, *g_fbRes = nullptr, *g_fbResDev = nullptr;
static size_t g_fbPartBytes = 0;
static int g_fbBlocks = 0, g_fbVals = 0;
constexpr int kFbChunks = 128;
__global__ void __launch_bounds__(512) fine_block_dots_reduce(double *part2, const double *part, int nblocks, int nval) {
  // work-group g sums its contiguous range of partial rows; thread (row, val): flat, contiguous reads
  __shared__ double red[512];
  const int rows = blockDim.x / nval, row = threadIdx.x / nval, val = threadIdx.x - row * nval;
  const int per = (nblocks + gridDim.x - 1) / gridDim.x, b0 = blockIdx.x * per, b1 = min(nblocks, b0 + per);
  double t = 0.0;
  if (row < rows) for (int b = b0 + row; b < b1; b += rows) t += part[(size_t)b * nval + val];
  red[threadIdx.x] = row < rows ? t : 0.0;
  __syncthreads();
  if ((int)threadIdx.x < nval) {
    double u = 0.0;
    for (int r = 0; r < rows; r++) u += red[r * nval + threadIdx.x];
    part2[(size_t)blockIdx.x * nval + threadIdx.x] = u;
  }
}
__global__ void fine_block_dots_finish(double *res, const double *part2, int nchunks, int nval) {
  const int v = blockIdx.x, lane = threadIdx.x;
  double t = 0.0;
  for (int c = lane; c < nchunks; c += 64) t += part2[(size_t)c * nval + v];
  for (int off = 32; off > 0; off >>= 1) t += __shfl_down(t, off, 64);
  if (lane == 0) res[v] = t;
}
void freeFineBlockDots() {
  if (g_fbPart) { poolDeviceFree(g_fbPart, 0); g_fbPart = nullptr; g_fbPartBytes = 0; }
  if (g_fbPart2) { (void)hipFree(g_fbPart2); g_fbPart2 = nullptr; }
  if (g_fbRes) { (void)hipHostFree(g_fbRes); g_fbRes = nullptr; g_fbResDev = nullptr; }
}
bool fineBlockDotsSupported(int nrhs) {
  static int off = -1;
  if (off < 0) { const char *e = getenv("QUDA_AMD_BLOCK_FINE_DOTS"); off = (e && !atoi(e)) ? 1 : 0; }
  return !off && (nrhs == 8 || nrhs == 4);
}
static int fbDotSums(int mode) { return mode == 1 ? 2 : (mode == 3 ? 3 : 7); }
// after a launch with dots: sums[k * nrhs + i], k as in FineBlockArg::dotMode; a global sum on a grid-decomposed lattice
static void fbDotsReduce(double *dst, int nrhs, int mode) {
  const int ns = fbDotSums(mode), nval = ns * nrhs;
  if (!g_fbBlocks || g_fbVals != nval) errorQuda("no multi-right-hand-side stencil launch with inner products (mode %d) to finish", mode);
  const int threads = 512 / nval * nval;
  hipLaunchKernelGGL(fine_block_dots_reduce, dim3(kFbChunks), dim3(threads), 0, computeStream(), g_fbPart2, (const double *)g_fbPart, g_fbBlocks, nval);
  hipLaunchKernelGGL(fine_block_dots_finish, dim3(nval), dim3(64), 0, computeStream(), dst, (const double *)g_fbPart2, kFbChunks, nval);
  HIP_CHECK(hipGetLastError());
  g_fbBlocks = 0;
}
void fineBlockDotsFinish(double *sums, int nrhs, int mode) {
  const int nval = fbDotSums(mode) * nrhs;
  fbDotsReduce(g_fbResDev, nrhs, mode);
  HIP_CHECK(hipStreamSynchronize(computeStream()));
  for (int q = 0; q < nval; q++) sums[q] = g_fbRes[q];
  if (commReductionsNeeded()) comm_allreduce(sums, nval);
}
// the same into DEVICE memory, rank-local, no host round trip: the next kernel on the stream reads the sums (blockblas::mrUpdateDev)
void fineBlockDotsFinishDev(double *d_sums, int nrhs, int mode) { fbDotsReduce(d_sums, nrhs, mode); }

void applyFineBlockParity(float2 *out, const float2 *in_same, const float2 *in_other, int nrhs, const GaugeField &U, int parity, double s0, double a0, double k1,
                          double a1, const float *tmat, int tmode, float2 *ghost, const FineBlockDots *dots) {
  if (!fineBlockSupported(U, nrhs)) errorQuda("multi-right-hand-side fine operator: fp32 links (18 or 12 reals), 4/8/16/24/32 right-hand sides");
  if (s0 != 0.0 && !in_same) errorQuda("same-parity input missing");
  if (tmat && (tmode != 1 && tmode != 2)) errorQuda("site-matrix mode %d (1: on the hop sum, 2: on the same-parity input)", tmode);
  if (tmat && tmode == 2 && s0 == 0.0) errorQuda("site matrix on the same-parity input, but that input is switched off");
  const LatticeGeom &g = U.geom;
  const int spb = fineBlockSitesPerGroup(nrhs), threads = spb * nrhs;
  FineBlockArg arg;
  arg.link_bytes = U.link_bytes; arg.g_stride = U.stride;
  arg.Vh = g.Vh; arg.Xh = g.Xh; arg.Y = g.X[1]; arg.Z = g.X[2]; arg.T = g.X[3];
  arg.dXh = g.dXh; arg.dY = g.dY; arg.dZ = g.dZ;
  arg.s0 = (float)s0; arg.a0 = (float)a0; arg.k1 = (float)k1; arg.a1 = (float)a1;
  arg.order = makeBlockOrder(g, spb);
  int nb = (g.Vh + spb - 1) / spb;
  arg.tile = 0; arg.tilesX = arg.tilesY = arg.tilesZ = 1;
  {
    static int tileEnv = -1;
    if (tileEnv < 0) { const char *e = getenv("QUDA_AMD_BLOCK_FINE_TILE"); tileEnv = e ? atoi(e) : 0; }   // measured SLOWER (48^4: 2278 against 2027 us per launch): off
    if (tileEnv && nrhs == 8 && g.X[0] % 4 == 0 && g.X[1] % 4 == 0 && g.X[2] % 2 == 0 && g.X[3] % 2 == 0) {
      arg.tile = 1; arg.tilesX = g.X[0] / 4; arg.tilesY = g.X[1] / 4; arg.tilesZ = g.X[2] / 2;
      nb = arg.tilesX * arg.tilesY * arg.tilesZ * (g.X[3] / 2);   // = Vh / 32
    }
  }
  arg.parity = parity;
  arg.out = out; arg.in_same = in_same ? in_same : in_other; arg.in_other = in_other;
  arg.gauge = (const char *)U.parityBase(parity);
  arg.tmat = tmat;
  arg.recon = (int)U.reconstruct;
  {
    const bool first_t = commGrid().coords[3] == 0, last_t = commGrid().coords[3] == commGrid().dims[3] - 1;
    arg.tsign_fwd = (U.reconstruct == QUDA_RECONSTRUCT_12 && U.t_boundary == QUDA_ANTI_PERIODIC_T && last_t) ? -1.f : 1.f;
    arg.tsign_bwd = (U.reconstruct == QUDA_RECONSTRUCT_12 && U.t_boundary == QUDA_ANTI_PERIODIC_T && first_t) ? -1.f : 1.f;
  }
  arg.dotA = nullptr; arg.dotPart = nullptr; arg.dotMode = 0;
  if (dots) {
    if (!fineBlockDotsSupported(nrhs)) errorQuda("inner products in the stencil epilogue: 4 or 8 right-hand sides only");
    if (dots->mode < 1 || dots->mode > 3) errorQuda("inner-product mode %d", dots->mode);
    if (dots->mode >= 2 && s0 == 0.0) errorQuda("inner products with the same-parity input, but that input is switched off");
    const int ns = fbDotSums(dots->mode);
    // the first ns * nrhs threads of a work-group write its row of partial sums, and the threads of sites past Vh have left the kernel by
    // then: a last work-group with fewer than ns live sites would leave part of its row unwritten.  Vh of an even lattice is a multiple of 8 > ns.
    if (g.Vh % spb && g.Vh % spb < ns) errorQuda("inner products in the stencil epilogue: the last work-group holds %d sites, mode %d needs %d", g.Vh % spb, dots->mode, ns);
    const size_t need = (size_t)nb * ns * nrhs * sizeof(double);
    if (need > g_fbPartBytes) {
      if (g_fbPart) poolDeviceFree(g_fbPart, 0);
      g_fbPart = (double *)poolDeviceMalloc(need);
      g_fbPartBytes = need;
    }
    if (!g_fbPart2) {
      HIP_CHECK(qaMalloc((void **)&g_fbPart2, (size_t)kFbChunks * 7 * 8 * sizeof(double)));
      HIP_CHECK(hipHostMalloc((void **)&g_fbRes, 7 * 8 * sizeof(double), hipHostMallocMapped));
      HIP_CHECK(hipHostGetDevicePointer((void **)&g_fbResDev, g_fbRes, 0));
    }
    arg.dotA = dots->a; arg.dotPart = g_fbPart; arg.dotMode = dots->mode;
    g_fbBlocks = nb; g_fbVals = ns * nrhs;
  }
  // grid-decomposed lattice: the faces of in_other (parity 1 - parity) go to the neighbours' ghost zones first — one pack launch and one
  // grouped exchange on the compute stream (setup-time traffic; the solve-time stencil has its own overlapped transports, halo.h)
  arg.commMask = 0;
  for (int d = 0; d < 4; d++) arg.ghostBase[d][0] = arg.ghostBase[d][1] = 0;
  {
    const BlockGhost gh = blockGhost(g.X, true);
    if (gh.mask) {
      if (!ghost) errorQuda("multi-right-hand-side stencil on a grid-decomposed lattice: the input needs a ghost zone (block.h BlockGhost)");
      blockExchangeGhostRaw(in_other, ghost, 12, nrhs, gh, 1 - parity);
      const long panel = 12l * nrhs, rel = ghost - in_other;
      if (rel % panel) errorQuda("ghost zone not aligned with the panels of its field");
      arg.commMask = gh.mask;
      for (int d = 0; d < 4; d++) for (int k = 0; k < 2; k++) arg.ghostBase[d][k] = (int)(rel / panel) + gh.offset[d][k];
    }
  }
  {
    // the x / y tile variant (QUDA_AMD_BLOCK_FINE_XYTILE): 8 right-hand sides, no site matrices, planes that 8 x 4 tiles cover
    static int xyEnv = -1;
    if (xyEnv < 0) { const char *e = getenv("QUDA_AMD_BLOCK_FINE_XYTILE"); xyEnv = e ? atoi(e) : 0; }
    if (xyEnv && nrhs == 8 && !tmat && !arg.tile && g.Xh % 8 == 0 && g.X[1] % 4 == 0) {
      arg.tilesX = g.Xh / 8; arg.tilesY = g.X[1] / 4;
      constexpr size_t ldsXY = (size_t)60 * 224 * sizeof(float);
      static bool attr = false;
      if (!attr) { HIP_CHECK(hipFuncSetAttribute((const void *)fine_block_kernel<8, 0, 1>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)ldsXY)); attr = true; }
      hipLaunchKernelGGL((fine_block_kernel<8, 0, 1>), dim3(nb), dim3(threads), ldsXY, computeStream(), arg);
      HIP_CHECK(hipGetLastError());
      return;
    }
  }
  if (g_acctOn) {   // links once per site (+ the dense site matrices), per right-hand side: 8 neighbour panels at ideal re-use = 1 read, own panel, output
    char tag[64]; snprintf(tag, sizeof(tag), "level 0, %d rhs%s%s", nrhs, s0 != 0.0 ? " xpay" : "", dots ? " + sums" : "");
    acct("fine_block_kernel", (double)g.Vh * (8.0 * (U.reconstruct == QUDA_RECONSTRUCT_12 ? 48 : 72) + (tmat ? 576.0 : 0.0) + nrhs * 96.0 * (s0 != 0.0 ? 3 : 2)), tag);
  }
#define FB_LAUNCH(N) \
  if (!tmat) hipLaunchKernelGGL((fine_block_kernel<N, 0>), dim3(nb), dim3(threads), 0, computeStream(), arg); \
  else if (tmode == 1) hipLaunchKernelGGL((fine_block_kernel<N, 1>), dim3(nb), dim3(threads), 0, computeStream(), arg); \
  else hipLaunchKernelGGL((fine_block_kernel<N, 2>), dim3(nb), dim3(threads), 0, computeStream(), arg)
  switch (nrhs) {
    case 4: FB_LAUNCH(4); break;
    case 8: FB_LAUNCH(8); break;
    case 16: FB_LAUNCH(16); break;
    case 24: FB_LAUNCH(24); break;
    default: FB_LAUNCH(32); break;
  }
#undef FB_LAUNCH
  HIP_CHECK(hipGetLastError());
}

// out = (1 + i a g5) in - kappa D in on full block fields of 12 components (both parities, two launches)
// grid-decomposed lattice: `in` carries 2 x blockGhost(X, true).nGhost panels behind its V local ones — the ghost zone of the even
// half, then that of the odd half
void applyFineBlockM(float2 *out, float2 *in, int nrhs, const GaugeField &U, double kappa, double a, const float *const tmat[2]) {
  const size_t par = (size_t)U.geom.Vh * 12 * nrhs;
  const BlockGhost gh = blockGhost(U.geom.X, true);
  for (int p = 0; p < 2; p++)
    applyFineBlockParity(out + p * par, in + p * par, in + (1 - p) * par, nrhs, U, p, 1.0, a, -kappa, 0.0, tmat ? tmat[p] : nullptr, 2,
                         gh.mask ? in + 2 * par + (size_t)(1 - p) * gh.nGhost * 12 * nrhs : nullptr);
}

}  // namespace quda
