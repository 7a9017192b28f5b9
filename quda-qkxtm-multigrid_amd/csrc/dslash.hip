// dslash.hip — fine-grid even-odd Wilson / twisted-mass / twisted-clover stencil for gfx950 (MI355X).
//
// What it computes (reference semantics): tests/wilson_dslash_reference.cpp:106-133 (hop), :233-263 (twist),
// tests/clover_reference.cpp:19-64, :203-232 (clover, twisted clover); device-side behaviour of
// lib/dslash_core/tm_dslash_gt200_core.h / tmc_dslash_*_core.h (epilogues) — re-designed, not translated:
//
//  * one lane = one checkerboard site; every global access is a 16-byte (fp64/fp32) or 8-byte (16-bit)
//    per-lane, unit-stride stream, i.e. 1 KiB / 512 B per wave instruction;
//  * links come from the bidirectional pre-daggered layout (fields.h): no neighbour index and no dagger
//    branch on the link side, 8 perfectly aligned streams per site;
//  * spin basis is chiral (DeGrand-Rossi): each of the 8 projections keeps two independent colour vectors
//    (h0,h1), the other two rows are +-1/+-i multiples; the twist is a per-chirality complex scale and
//    the clover term two Hermitian 6x6 blocks — all fused into the epilogue, nothing is re-read;
//  * spinor neighbour re-use is left to L2/MALL: the block index is re-mapped so that each XCD (private
//    4 MiB L2) sweeps a contiguous slab of time slices instead of the default round-robin interleave;
//  * index arithmetic uses multiply-high fast division (no software integer divide on gfx950).
//
// Roofline: HBM-bound; algorithmic bytes per site = 8 R P + 24 P (in) + 24 P (out) [+ 24 P xpay]
// [+ 144 P clover & inverse] (+ norms for 16-bit), SURVEY.md section 8d.
#include "dslash.h"

#include <cstring>
#include <functional>
#include <vector>

#include "device_io.h"
#include "dslash_arg.h"
#include "dslash_launch.h"

namespace quda {

// ---- flag-in-data ghost transport (peer stores) ----
// A face site travels as NV 16-byte vectors {w0, flag, w1, flag}: two 4-byte payload words, each next to the exchange's flag
// (the cumulative use count of the (dimension, buffer) zone, never 0), plane-major [vector][faceCB].  Every 8-byte half is
// self-validating, so the receiver needs neither a counter nor any ordering between stores: it polls the very words it is
// about to use, and the sender just stores and leaves — no acknowledgement wait, no barrier, no atomic (those put the
// slowest pack block, 18 us under a saturated memory system, on the critical path of a 10-20 us kernel; the same idea as the
// LL protocol of the collective libraries).  Costs 2x the face bytes, which are a few hundred KB.
#ifndef QA_LL_STORE_AUX
#define QA_LL_STORE_AUX 17   // sc0 sc1: system scope, write-through
#endif
template <typename T> struct GhostLL;
template <> struct GhostLL<double> {
  static constexpr int NV = 12, NA = 8;
  static __device__ __forceinline__ void encode(unsigned *w, const double *h) {
#pragma unroll
    for (int k = 0; k < 12; k++) { const unsigned long long b = __builtin_bit_cast(unsigned long long, h[k]); w[2 * k] = (unsigned)b; w[2 * k + 1] = (unsigned)(b >> 32); }
  }
  static __device__ __forceinline__ void decode(double *h, const unsigned *w) {
#pragma unroll
    for (int k = 0; k < 12; k++) h[k] = __builtin_bit_cast(double, (unsigned long long)w[2 * k] | ((unsigned long long)w[2 * k + 1] << 32));
  }
};
template <> struct GhostLL<float> {
  static constexpr int NV = 6, NA = 4;
  static __device__ __forceinline__ void encode(unsigned *w, const float *h) {
#pragma unroll
    for (int k = 0; k < 12; k++) w[k] = __builtin_bit_cast(unsigned, h[k]);
  }
  static __device__ __forceinline__ void decode(float *h, const unsigned *w) {
#pragma unroll
    for (int k = 0; k < 12; k++) h[k] = __builtin_bit_cast(float, w[k]);
  }
};
template <> struct GhostLL<short> {   // 12 int16 + the fp32 scale of the site (same quantisation as Planar<short>::store)
  static constexpr int NV = 4, NA = 3;
  static __device__ __forceinline__ void encode(unsigned *w, const float *h) {
    float m = 0.f;
#pragma unroll
    for (int k = 0; k < 12; k++) m = fmaxf(m, fabsf(h[k]));
    const float sc = m > 0.f ? kShortMax / m : 0.f;
#pragma unroll
    for (int k = 0; k < 6; k++)
      w[k] = (unsigned)(unsigned short)Planar<short, 12>::q16(h[2 * k] * sc) | ((unsigned)(unsigned short)Planar<short, 12>::q16(h[2 * k + 1] * sc) << 16);
    w[6] = __builtin_bit_cast(unsigned, m);
    w[7] = 0u;
  }
  static __device__ __forceinline__ void decode(float *h, const unsigned *w) {
    const float sc = __builtin_bit_cast(float, w[6]) * kShortInv;
#pragma unroll
    for (int k = 0; k < 6; k++) { h[2 * k] = (float)(short)(w[k] & 0xffffu) * sc; h[2 * k + 1] = (float)(short)(w[k] >> 16) * sc; }
  }
};
template <typename T> __device__ __forceinline__ __amdgpu_buffer_rsrc_t ghost_ll_rsrc(const void *base, int faceCB) {
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<void *>(base), 0, (int)((unsigned)faceCB * (unsigned)(GhostLL<T>::NV * 16)), 0x00020000);
}
// sender: system-scope write-through stores into the neighbour's zone
template <typename T, typename real> __device__ __forceinline__ void ghost_ll_store(const real *h, void *zone, int faceCB, int f, unsigned flag) {
  constexpr int NV = GhostLL<T>::NV;
  unsigned w[2 * NV];
  GhostLL<T>::encode(w, h);
  const __amdgpu_buffer_rsrc_t rs = ghost_ll_rsrc<T>(zone, faceCB);
#pragma unroll
  for (int v = 0; v < NV; v++) {
    u32x4_t q; q.x = w[2 * v]; q.y = flag; q.z = w[2 * v + 1]; q.w = flag;
    __builtin_amdgcn_raw_buffer_store_b128(q, rs, f * 16, v * faceCB * 16, QA_LL_STORE_AUX);
  }
}
// receiver: poll the site's own vectors (system-scope loads) until every half carries this exchange's flag; bounded by `ticks`
// ---- the compact wire format: self-validating 16-byte atoms (QUDA_AMD_HALO_FORMAT=atom, tune key "halo_format" = 1) ----
// The flag-in-data vectors above spend half of every byte on the wire on flags (786 KB per fp64 face of the 8-GPU split of 32^3 x 64,
// two such faces sharing one xGMI link where a dimension has only two ranks).  Here a face site travels as NA atoms of 16 bytes =
// three 32-bit payload words + the exchange's 32-bit flag: fp64 24 words = 8 atoms = ONE 128-byte line per site, fp32 4 atoms = 64 bytes,
// 16-bit storage 6 packed words + the scale = 3 atoms = 48 bytes — 128 / 64 / 48 bytes per face site against 192 / 96 / 64.
// Plane-major [atom][faceCB].  Every atom is written by ONE 16-byte store of ONE lane and validates itself: the format assumes nothing
// about the order in which different stores, or different lanes of one store, become visible across xGMI — only that a naturally aligned
// 16-byte store of a lane is not torn, the granularity the collective libraries' 128-byte protocol builds on as well.  (Round 3 had
// 32-byte sectors written by two adjacent lanes with the flag in the second half: one assumption more, and an LDS transpose in the pack
// blocks to arrange it; replaced.)  The sender is pack_emit as for flag-in-data — no LDS, and the receiver needs 8 instead of 12
// sixteen-byte loads per fp64 site.
template <typename T> __device__ __forceinline__ __amdgpu_buffer_rsrc_t ghost_atom_rsrc(const void *base, int faceCB) {
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<void *>(base), 0, (int)((unsigned)faceCB * (unsigned)(GhostLL<T>::NA * 16)), 0x00020000);
}
template <typename T, typename real> __device__ __forceinline__ void ghost_atom_store(const real *h, void *zone, int faceCB, int f, unsigned flag) {
  constexpr int NV = GhostLL<T>::NV, NA = GhostLL<T>::NA;
  unsigned w[3 * NA > 2 * NV ? 3 * NA : 2 * NV];
  GhostLL<T>::encode(w, h);
#pragma unroll
  for (int k = 2 * NV; k < 3 * NA; k++) w[k] = 0u;
  const __amdgpu_buffer_rsrc_t rs = ghost_atom_rsrc<T>(zone, faceCB);
#pragma unroll
  for (int v = 0; v < NA; v++) {
    u32x4_t q; q.x = w[3 * v]; q.y = w[3 * v + 1]; q.z = w[3 * v + 2]; q.w = flag;
    __builtin_amdgcn_raw_buffer_store_b128(q, rs, f * 16, v * faceCB * 16, QA_LL_STORE_AUX);
  }
}
// one look at the atoms of face site f; false: some atom does not carry this exchange's flag yet (sy = the flag seen, sv = its atom)
template <typename T> __device__ __forceinline__ bool ghost_atom_read(unsigned *w, const __amdgpu_buffer_rsrc_t &rs, int faceCB, int f, unsigned flag, unsigned &sy, unsigned &sw, int &sv) {
  constexpr int NV = GhostLL<T>::NV, NA = GhostLL<T>::NA;
  bool ok = true;
#pragma unroll
  for (int v = 0; v < NA; v++) {
    const u32x4_t q = __builtin_amdgcn_raw_buffer_load_b128(rs, f * 16, v * faceCB * 16, 17);
    if (3 * v < 2 * NV) w[3 * v] = q.x;
    if (3 * v + 1 < 2 * NV) w[3 * v + 1] = q.y;
    if (3 * v + 2 < 2 * NV) w[3 * v + 2] = q.z;
    const bool good = q.w == flag;
    if (!good && ok) { sy = q.w; sw = q.w; sv = v; }
    ok = ok && good;
  }
  return ok;
}
template <typename T, typename real>
__device__ __forceinline__ void ghost_ll_load(real *h, const void *zone, int faceCB, int f, unsigned flag, unsigned long long ticks, int *errWord, int code, unsigned exSeq, int exBuf,
                                              int fmt) {
  constexpr int NV = GhostLL<T>::NV;
  unsigned w[2 * NV];
  if (fmt) {
    const __amdgpu_buffer_rsrc_t rs = ghost_atom_rsrc<T>(zone, faceCB);
    unsigned long long t0 = 0;
    for (;;) {
      unsigned sy = flag, sw = flag; int sv = -1;
      if (ghost_atom_read<T>(w, rs, faceCB, f, flag, sy, sw, sv)) break;
      if (!t0) t0 = wall_clock64();
      else if (__hip_atomic_load(errWord, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) break;
      else if (wall_clock64() - t0 > ticks) {
        if (atomicCAS(errWord, 0, code) == 0) { errWord[1] = f; errWord[2] = (int)flag; errWord[3] = (int)sy; errWord[4] = (int)sw; errWord[5] = (int)exSeq; errWord[6] = exBuf; errWord[7] = sv; }
        break;
      }
      __builtin_amdgcn_s_sleep(2);
    }
    GhostLL<T>::decode(h, w);
    return;
  }
  const __amdgpu_buffer_rsrc_t rs = ghost_ll_rsrc<T>(zone, faceCB);
  unsigned long long t0 = 0;
  for (;;) {
    bool ok = true;
#pragma unroll
    for (int v = 0; v < NV; v++) {
      const u32x4_t q = __builtin_amdgcn_raw_buffer_load_b128(rs, f * 16, v * faceCB * 16, 17);
      w[2 * v] = q.x; w[2 * v + 1] = q.z;
      ok = ok && q.y == flag && q.w == flag;
    }
    if (ok) break;
    if (!t0) t0 = wall_clock64();
    else if (__hip_atomic_load(errWord, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) break;   // another wait has given up already
    else if (wall_clock64() - t0 > ticks) {
      // give up: the host reports it (p2pCheck).  The first wait to get here claims the record and says what it was waiting for and
      // what it last saw there (one more look at the vectors: nothing of this is kept live in the polling loop)
      if (atomicCAS(errWord, 0, code) == 0) {
        unsigned sy = flag, sw = flag; int sv = -1;
        for (int v = NV - 1; v >= 0; v--) {
          const u32x4_t q = __builtin_amdgcn_raw_buffer_load_b128(rs, f * 16, v * faceCB * 16, 17);
          if (q.y != flag || q.w != flag) { sy = q.y; sw = q.w; sv = v; }
        }
        errWord[1] = f; errWord[2] = (int)flag; errWord[3] = (int)sy; errWord[4] = (int)sw; errWord[5] = (int)exSeq; errWord[6] = exBuf; errWord[7] = sv;
      }
      break;
    }
    __builtin_amdgcn_s_sleep(2);
  }
  GhostLL<T>::decode(h, w);
}
// One hop = load (neighbour spinor + this site's pre-daggered link) then project / multiply / reconstruct.
// The two phases are separate so the kernel can software-pipeline them: loads of direction d+1 are issued
// before the arithmetic of direction d (register double-buffering), fenced with sched_barrier so hipcc neither
// hoists all 8 directions' loads to the top (fp64: 512 registers + scratch spills, 1 wave/SIMD) nor serialises them.
// GAUX: cache policy of the link stream (0 default, 2 = nt: read-once data that should not displace the spinor
// working set from L2 / Infinity Cache).  QA_GAUX / QA_GAUX16 / QA_PAUX: build-time overrides for A/B timing (tools/build_variant.sh).
#ifndef QA_GAUX
#define QA_GAUX 2
#endif
#ifndef QA_GAUX16
#define QA_GAUX16 0
#endif
#ifndef QA_PAUX
#define QA_PAUX 0
#endif
// GH: 0 = every neighbour is local; 1 = off-node neighbours are read from the ghost zone (exterior pass); 2 = off-node hops are
// skipped here and done by ghost_hop() once the faces have arrived (single-launch peer-store path)
// hop_load only REQUESTS (raw register images, device_io.h RawBlock): the 16-bit -> fp32 conversion and the third row of a
// 12-real link are arithmetic on the loaded data and belong to hop_compute, behind the fence — inside the request phase they made
// the wave wait for the data of hop d + 1 before it started on hop d (16-bit and recon-12 kernels ran without any overlap).
template <typename T, int R, int DIR, int GAUX, int GH = 0, typename real>
__device__ __forceinline__ void hop_load(RawBlock<T, 24> &psi, typename Link<T, R>::Raw &U, const DslashArg<real> &arg, int idx, int nbr, bool off_node = false, int face = 0) {
  constexpr int MU = DIR / 2;
  // GH == 2: the load is issued for every lane (the periodic wrap makes the index valid) and the contribution of an off-node
  // lane is zeroed in hop_compute: a per-lane branch here splits the 8-hop pipeline into many basic blocks and costs the
  // fp64 kernel its second wave per SIMD (256 + 8 registers against 231 for the branch-free loop)
  if (GH == 1 && off_node) {
    // the neighbour lives on another rank: its (pre-twisted,) spin-projected half spinor was packed there with the same
    // projector sign; it goes into the first 12 slots of the buffer.  Issued here, with the other loads of the hop, so it
    // does not cost a dependent round trip in the compute phase.  sc0 sc1 (system-scope) loads: the zone may have been
    // written by another GPU while this kernel was running.
    const char *gb = arg.ghost[MU][(DIR & 1) ? 0 : 1];
    psi.template load12<17>(gb, arg.faceCB[MU], face, reinterpret_cast<const float *>(gb + arg.ghostNormOff[MU]), face);
  } else {
    psi.template load<QA_PAUX>(arg.in, arg.sp_stride, nbr, arg.inNorm, nbr);
  }
  Link<T, R>::template request<GAUX>(U, arg.gauge + (size_t)DIR * arg.link_bytes, arg.g_stride, idx);
}
template <typename T, int R, int DIR, bool PRETWIST, int GH, typename real>
__device__ __forceinline__ void hop_compute(real *acc, const RawBlock<T, 24> &psiRaw, const typename Link<T, R>::Raw &URaw, const DslashArg<real> &arg, real sign, bool off_node = false,
                                            int face = 0) {
  real psi[24], U[18];
  if constexpr (sizeof(T) == 2) {
    // 16-bit: the hop is linear in the neighbour and in the link, so the integers go through it as they are and the product of
    // the two scales is applied inside the reconstruction (conversion: one v_cvt per operand instead of v_cvt + v_mul)
    psiRaw.unpack_unscaled(psi);
    if constexpr (R == 8) {
      // 8-real links: the reconstruction is not linear in the stored values, so the link comes back in its own units and only the
      // neighbour's integers and scale go through the hop
      Link<T, R>::finish(U, URaw, sign);
      hop_arith<DIR, PRETWIST, GH, true>(acc, psi, U, arg, off_node, psiRaw.scale());
    } else {
      URaw.unpack_unscaled(U);
      if (R == 12) Link<T, R>::third_row(U, sign * kShortInv);   // row 3 = conj(row 1 x row 2): back to the units of the stored rows
      hop_arith<DIR, PRETWIST, GH, true>(acc, psi, U, arg, off_node, psiRaw.scale() * kShortInv);
    }
  } else {
    psiRaw.unpack(psi);
    Link<T, R>::finish(U, URaw, sign);
    hop_arith<DIR, PRETWIST, GH>(acc, psi, U, arg, off_node);
  }
}

// one off-node hop from the ghost zone (half spinor packed by the neighbour + this site's link), for the lanes that need it
template <typename T, int R, int DIR, int GAUX, typename real>
__device__ __forceinline__ void ghost_hop(real *acc, const DslashArg<real> &arg, int idx, bool off_node, int face, real sign) {
  constexpr int MU = DIR / 2;
  if (!off_node) return;
  real h[12], g[12], U[18];
  Link<T, R>::template load<GAUX>(U, arg.gauge + (size_t)DIR * arg.link_bytes, arg.g_stride, idx, sign);
  ghost_ll_load<T>(h, arg.ghost[MU][(DIR & 1) ? 0 : 1], arg.faceCB[MU], face, arg.waitCount[DIR], arg.waitTicks, arg.errWord, 1 + DIR, arg.exSeq, arg.exBuf, arg.pack.llFormat);
  const real s = (DIR & 1) ? -arg.sfwd : arg.sfwd;
  su3_mv(g, U, h);
  su3_mv(g + 6, U, h + 6);
  spin_reconstruct<MU>(acc, g, s);
}

// o = (chiral block held as a raw image) v.  16-bit: the block's integers go through the product unscaled and the 12 results take
// the block's scale (12 multiplications instead of 36)
template <typename T, typename real> __device__ __forceinline__ void clover_mv_raw(real *o, const RawBlock<T, 36> &raw, real *C, const real *v) {
  if constexpr (sizeof(T) == 2) {
    raw.unpack_unscaled(C);
    clover_block_mv(o, C, v);
    const real w = raw.scale();
#pragma unroll
    for (int k = 0; k < 12; k++) o[k] *= w;
  } else {
    raw.unpack(C);
    clover_block_mv(o, C, v);
  }
}

// fused epilogue of the stencil: twist / inverse twist / xpay / clover-twist (+ inverse), then the store of the site
template <typename T, int VARIANT, int GAUX, int SAUX, typename real>
__device__ __forceinline__ void dslash_epilogue(real *acc, const DslashArg<real> &arg, int idx) {
  constexpr bool CLOVER = VARIANT == 2;
  real xs[24];
  // (clover-twist inverse: x is only added at the very end; requested there, it does not sit in 24 registers through the four block products)
  RawBlock<T, 24> xsRaw;
  if (arg.xpay && !(CLOVER && arg.mode == DSLASH_CLOVER_TWIST_INV)) {
    xsRaw.load(arg.x, arg.sp_stride, idx, arg.xNorm, idx);
    if (!CLOVER) xsRaw.unpack(xs);
  }

  if (arg.mode == DSLASH_PLAIN) {
    if (arg.xpay) {
#pragma unroll
      for (int k = 0; k < 24; k++) acc[k] = xs[k] + arg.k * acc[k];
    }
  } else if (arg.mode == DSLASH_TWIST_INV || arg.mode == DSLASH_TWIST_INV_DSLASH) {
    if (arg.mode == DSLASH_TWIST_INV) twist_inplace(acc, arg.a);
    if (arg.xpay) {
#pragma unroll
      for (int k = 0; k < 24; k++) acc[k] = xs[k] + arg.b * acc[k];
    } else {
#pragma unroll
      for (int k = 0; k < 24; k++) acc[k] *= arg.b;
    }
  } else if (arg.mode == DSLASH_TWIST_XPAY) {
    twist_inplace(xs, arg.a);
#pragma unroll
    for (int k = 0; k < 24; k++) acc[k] = arg.k * acc[k] + xs[k];
  } else if (CLOVER) {
    real C[36], tmp[24];
    if (arg.mode == DSLASH_CLOVER_TWIST_INV) {
      // tmp = (A + i a g5) acc ; res = Ainv tmp, chirality by chirality (the two 6 x 6 blocks do not mix).  Four blocks of 36 reals
      // are read; left to itself the compiler requests all four up front and converts them at once (144 live registers on top of
      // acc: 176 VGPRs for the 16-bit kernel, 198 for fp32 — two waves per SIMD where the plain twisted-mass kernels run four).
      // Two raw images (RawBlock: 19 registers each in 16-bit), the next block requested before the product with the current
      // one, fenced like the hop pipeline.
      // (fp64: two images are 144 registers; its blocks are requested and used one after the other)
      if constexpr (sizeof(T) == 8) {
        const real sa[2] = {arg.a, -arg.a};
#pragma unroll
        for (int chi = 0; chi < 2; chi++) {
          real *t = tmp + 12 * chi, *v = acc + 12 * chi;
          Planar<T, 36>::template load<GAUX>(C, (const char *)arg.clA + (size_t)chi * 36 * sizeof(T) * arg.cl_stride, arg.cl_stride, idx, arg.clAn, chi * arg.cl_stride + idx);
          clover_block_mv(t, C, v);
#pragma unroll
          for (int k = 0; k < 6; k++) { t[2 * k] -= sa[chi] * v[2 * k + 1]; t[2 * k + 1] += sa[chi] * v[2 * k]; }
        }
#pragma unroll
        for (int chi = 0; chi < 2; chi++) {
          Planar<T, 36>::template load<GAUX>(C, (const char *)arg.clAinv + (size_t)chi * 36 * sizeof(T) * arg.cl_stride, arg.cl_stride, idx, arg.clAinvN, chi * arg.cl_stride + idx);
          clover_block_mv(acc + 12 * chi, C, tmp + 12 * chi);
        }
      } else {
        // one raw image at a time, each block requested after the product with the previous one (fenced): four exposed latencies,
        // but the kernel keeps the register count of the plain twisted-mass stencil and other waves cover them
        RawBlock<T, 36> Ca;
        const real sa[2] = {arg.a, -arg.a};
#pragma unroll
        for (int chi = 0; chi < 2; chi++) {
          real *t = tmp + 12 * chi, *v = acc + 12 * chi;
          Ca.template load<GAUX>((const char *)arg.clA + (size_t)chi * 36 * sizeof(T) * arg.cl_stride, arg.cl_stride, idx, arg.clAn, chi * arg.cl_stride + idx);
          __builtin_amdgcn_sched_barrier(0);
          clover_mv_raw<T>(t, Ca, C, v);
#pragma unroll
          for (int k = 0; k < 6; k++) { t[2 * k] -= sa[chi] * v[2 * k + 1]; t[2 * k + 1] += sa[chi] * v[2 * k]; }
          __builtin_amdgcn_sched_barrier(0);
          Ca.template load<GAUX>((const char *)arg.clAinv + (size_t)chi * 36 * sizeof(T) * arg.cl_stride, arg.cl_stride, idx, arg.clAinvN, chi * arg.cl_stride + idx);
          __builtin_amdgcn_sched_barrier(0);
          clover_mv_raw<T>(v, Ca, C, t);
          __builtin_amdgcn_sched_barrier(0);
        }
      }
      if (arg.xpay) {
        Planar<T, 24>::load(xs, arg.x, arg.sp_stride, idx, arg.xNorm, idx);
#pragma unroll
        for (int k = 0; k < 24; k++) acc[k] = xs[k] + arg.k * acc[k];
      }
    } else {  // DSLASH_CLOVER_TWIST_XPAY: out = k acc + (A + i a g5) x, chirality by chirality
      RawBlock<T, 36> Ca;
      const real sa[2] = {arg.a, -arg.a};
#pragma unroll
      for (int chi = 0; chi < 2; chi++) {
        real xv[24];
        xsRaw.unpack(xv);   // only the 12 values of this chirality survive: x stays a raw image (13 registers in 16-bit) until here
        real *t = tmp + 12 * chi, *v = xv + 12 * chi, *o = acc + 12 * chi;
        Ca.load((const char *)arg.clA + (size_t)chi * 36 * sizeof(T) * arg.cl_stride, arg.cl_stride, idx, arg.clAn, chi * arg.cl_stride + idx);
        __builtin_amdgcn_sched_barrier(0);
        clover_mv_raw<T>(t, Ca, C, v);
#pragma unroll
        for (int k = 0; k < 6; k++) { t[2 * k] -= sa[chi] * v[2 * k + 1]; t[2 * k + 1] += sa[chi] * v[2 * k]; }
#pragma unroll
        for (int k = 0; k < 12; k++) o[k] = arg.k * o[k] + t[k];
        __builtin_amdgcn_sched_barrier(0);
      }
    }
  }
  Planar<T, 24>::template store<SAUX>(acc, arg.out, arg.sp_stride, idx, arg.outNorm, idx);
}

// ---- fused doublet stencil: epilogue ----
// A wave of ndeg_dslash_kernel is 32 sites x 2 flavours: lane l < 32 holds flavour 1 of a site, lane l + 32 flavour 2 of the same site.
// The value the partner half-wave holds in the same register, by v_permlane32_swap (CDNA4): swap(v, v) returns {lower half in both
// halves, upper half in both halves}
__device__ __forceinline__ float half_swap(float v, bool upper) {
  const unsigned u = __builtin_bit_cast(unsigned, v);
  const auto r = __builtin_amdgcn_permlane32_swap(u, u, false, false);
  return __builtin_bit_cast(float, upper ? r[0] : r[1]);
}
__device__ __forceinline__ double half_swap(double v, bool upper) {
  const unsigned long long u = __builtin_bit_cast(unsigned long long, v);
  const unsigned lo = (unsigned)u, hi = (unsigned)(u >> 32);
  const auto rl = __builtin_amdgcn_permlane32_swap(lo, lo, false, false);
  const auto rh = __builtin_amdgcn_permlane32_swap(hi, hi, false, false);
  const unsigned long long w = ((unsigned long long)(upper ? rh[0] : rh[1]) << 32) | (upper ? rl[0] : rl[1]);
  return __builtin_bit_cast(double, w);
}
// acc: the hop sum of this lane's flavour; site: its index in the doublet's planes (f Vh + idx); upper: flavour 2 (a -> -a).
//   DSLASH_PLAIN      out = acc                                   [xpay: x + k acc]      both flavours of D in one launch
//   DSLASH_TWIST_INV  out = b (acc + i a g5 acc + nb acc')         [xpay: x + b (...)]    A^-1 D, b = d (times k), acc' the partner's
//   DSLASH_TWIST_XPAY out = k acc + (x + i a g5 x + nb x')                                k D + A x
template <typename T, int SAUX, typename real>
__device__ __forceinline__ void ndeg_epilogue(real *acc, const DslashArg<real> &arg, int site, bool upper) {
  real xs[24], o[24];
  if (arg.xpay) Planar<T, 24>::load(xs, arg.x, arg.sp_stride, site, arg.xNorm, site);
  const real a = upper ? -arg.a : arg.a;
  if (arg.mode == DSLASH_PLAIN) {
    if (arg.xpay) {
#pragma unroll
      for (int k = 0; k < 24; k++) acc[k] = xs[k] + arg.k * acc[k];
    }
  } else if (arg.mode == DSLASH_TWIST_INV) {
#pragma unroll
    for (int k = 0; k < 24; k++) o[k] = half_swap(acc[k], upper);
    twist_inplace(acc, a);
    if (arg.xpay) {
#pragma unroll
      for (int k = 0; k < 24; k++) acc[k] = xs[k] + arg.b * (acc[k] + arg.nb * o[k]);
    } else {
#pragma unroll
      for (int k = 0; k < 24; k++) acc[k] = arg.b * (acc[k] + arg.nb * o[k]);
    }
  } else {   // DSLASH_TWIST_XPAY
#pragma unroll
    for (int k = 0; k < 24; k++) o[k] = half_swap(xs[k], upper);
    twist_inplace(xs, a);
#pragma unroll
    for (int k = 0; k < 24; k++) acc[k] = arg.k * acc[k] + (xs[k] + arg.nb * o[k]);
  }
  Planar<T, 24>::template store<SAUX>(acc, arg.out, arg.sp_stride, site, arg.outNorm, site);
}

// ---- face packing (reference packFaceWilsonKernel / packTwistedFaceWilsonKernel, lib/dslash_pack.cu:272, :610) ----
// P2P: the send pointers are peer-mapped ghost zones — flag-in-data vectors, system-scope write-through stores (GhostLL)
// Block `bid` packs the face sites [bid * chunk, (bid + 1) * chunk) of the concatenated (dim, dir) ranges, chunk <= blockDim.
// The work of one face site in two steps, so that a caller can put other loads between the load and the stores:
// pack_locate: face item `tid` of the concatenated (dim, dir) ranges -> (slot = 2 dim + to_fwd, face index f, checkerboard index)
template <typename real> __device__ __forceinline__ int pack_locate(const PackArg<real> &arg, int tid, int &slot, int &f) {
  slot = 0;
#pragma unroll
  for (int k = 1; k < 8; k++) slot += tid >= arg.start[k];
  const int d = slot >> 1, to_fwd = slot & 1;
  f = tid - arg.start[slot];
  // other three coordinates from the face index (lexicographic, halved), then the site's full index
  int c[4], L[3], o[3], n = 0;
  for (int k = 0; k < 4; k++) if (k != d) { L[n] = arg.X[k]; o[n] = k; n++; }
  int l = 2 * f;
  const int c0 = l % L[0]; l /= L[0];
  const int c1 = l % L[1]; const int c2 = l / L[1];
  c[d] = to_fwd ? arg.X[d] - 1 : 0;
  c[o[0]] = c0; c[o[1]] = c1; c[o[2]] = c2;
  c[o[0]] += (arg.parity_in + c[0] + c[1] + c[2] + c[3]) & 1;  // pick the site of the pair that has the input parity
  return (((c[3] * arg.X[2] + c[2]) * arg.X[1] + c[1]) * arg.X[0] + c[0]) >> 1;
}
// pack_emit: (pre-twist,) project for the receiver's hop and store — flag-in-data vectors into the neighbour's zone (P2P) or planes
// of the send buffer
template <typename T, bool PRETWIST, bool P2P, typename real> __device__ __forceinline__ void pack_emit(const PackArg<real> &arg, real *psi, int slot, int f) {
  const int d = slot >> 1, to_fwd = slot & 1;
  real h[12];
  if (PRETWIST) twist_inplace(psi, arg.a);
  // the receiver uses this face for its hop in direction -d (if we send forward) / +d (if we send backward)
  const real s = to_fwd ? -arg.sfwd : arg.sfwd;
  switch (d) {
    case 0: spin_project<0>(h, psi, s); break;
    case 1: spin_project<1>(h, psi, s); break;
    case 2: spin_project<2>(h, psi, s); break;
    default: spin_project<3>(h, psi, s); break;
  }
  char *sb = arg.send[d][to_fwd];
  if (P2P) {   // straight into the neighbour's zone, flag in the data
    if (arg.llFormat) ghost_atom_store<T>(h, sb, arg.faceCB[d], f, arg.llFlag[d]);
    else ghost_ll_store<T>(h, sb, arg.faceCB[d], f, arg.llFlag[d]);
  }
  else Planar<T, 12>::store(h, sb, arg.faceCB[d], f, reinterpret_cast<float *>(sb + arg.normOff[d]), f);
}
template <typename T, bool PRETWIST, bool P2P, typename real> __device__ __forceinline__ void pack_body(const PackArg<real> &arg, int bid, int chunk) {
  const int tid = (int)threadIdx.x < chunk ? bid * chunk + (int)threadIdx.x : arg.start[8];
  if (P2P && arg.timeline && threadIdx.x == 0) {
    arg.timeline[bid] = wall_clock64();
    // where the block runs: HW_ID (cu_id 11:8, sh_id 12, se_id 15:13) and XCC_ID, for the placement statistics of the timeline
    arg.timeline[3072 + bid] = 0x100000000ull | ((unsigned long long)(__builtin_amdgcn_s_getreg(20 | (31 << 11)) & 0xf) << 16) | (__builtin_amdgcn_s_getreg(4 | (31 << 11)) & 0xff00u);
  }
  if (tid < arg.start[8]) {
    int slot, f;
    const int idx = pack_locate(arg, tid, slot, f);
    real psi[24];
    Planar<T, 24>::load(psi, arg.in, arg.sp_stride, idx, arg.inNorm, idx);
    if (P2P && arg.timeline) {
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      if (threadIdx.x == 0) arg.timeline[13312 + bid] = wall_clock64();
    }
    pack_emit<T, PRETWIST, P2P>(arg, psi, slot, f);
  }
  if (P2P && arg.timeline && threadIdx.x == 0) arg.timeline[1024 + bid] = wall_clock64();
}

// VARIANT: 0 = Wilson / twist epilogues, 1 = twist applied to the neighbours first (TWIST_INV_DSLASH), 2 = clover epilogues.
// Compile-time so the 8-hop pipeline below is one straight-line basic block (a wave-uniform runtime branch per hop
// made hipcc split it into ~80 blocks and shuttle the double buffers through AGPRs).
// All 8 hops + epilogue of one site.  KT: 0 = every neighbour is local (periodic wrap inside this rank); 1 = interior pass of a
// grid-decomposed lattice (sites that touch a partitioned boundary are skipped); 2 = exterior pass (boundary site, off-node
// neighbours from the ghost zone); 3 = single-launch peer-store path: local hops first, then the off-node hops once the
// neighbours' faces have arrived.
// ND = 1 (fused doublet stencil): the lane works on flavour fo / Vh of site idx — spinor indices are offset by fo inside the doublet's planes,
// the links are those of idx — and the epilogue mixes the flavours of the two half-waves (ndeg_epilogue)
template <typename T, int R, int VARIANT, int GAUX, int KT, int SAUX, int ND = 0, typename real>
__device__ __forceinline__ void stencil_site(const DslashArg<real> &arg, const int idx, const int fo = 0) {
  // checkerboard index -> coordinates (tests/test_util.cpp:419-443)
  const uint32_t za = arg.dXh.div((uint32_t)idx);
  const int xh = idx - (int)za * arg.Xh;
  const uint32_t zb = arg.dY.div(za);
  const int y = (int)za - (int)zb * arg.Y;
  const int t = (int)arg.dZ.div(zb);
  const int z = (int)zb - t * arg.Z;
  const int xodd = (y + z + t + arg.parity) & 1;
  const int xf = 2 * xh + xodd;  // full x coordinate
  // which hops leave this rank (KT != 0 only)
  const bool gx = (arg.commMask & 1) != 0, gy = (arg.commMask & 2) != 0, gz = (arg.commMask & 4) != 0, gt = (arg.commMask & 8) != 0;
  const bool o_xp = gx && xf == 2 * arg.Xh - 1, o_xm = gx && xf == 0, o_yp = gy && y == arg.Y - 1, o_ym = gy && y == 0;
  const bool o_zp = gz && z == arg.Z - 1, o_zm = gz && z == 0, o_tp = gt && t == arg.T - 1, o_tm = gt && t == 0;
  if (KT == 1 && (o_xp || o_xm || o_yp || o_ym || o_zp || o_zm || o_tp || o_tm)) return;
  // face (ghost-zone) indices: lexicographic over the three other coordinates, halved (reference tests/dslash_util.h:291-394)
  const int X1 = 2 * arg.Xh;
  const int f_x = ((t * arg.Z + z) * arg.Y + y) >> 1, f_y = ((t * arg.Z + z) * X1 + xf) >> 1;
  const int f_z = ((t * arg.Y + y) * X1 + xf) >> 1, f_t = ((z * arg.Y + y) * X1 + xf) >> 1;

  const int Xh = arg.Xh, sy = Xh, sz = Xh * arg.Y, st = Xh * arg.Y * arg.Z;
  const int n_xp = xodd ? (xh == Xh - 1 ? idx - (Xh - 1) : idx + 1) : idx;
  const int n_xm = xodd ? idx : (xh == 0 ? idx + (Xh - 1) : idx - 1);
  const int n_yp = y == arg.Y - 1 ? idx - (arg.Y - 1) * sy : idx + sy;
  const int n_ym = y == 0 ? idx + (arg.Y - 1) * sy : idx - sy;
  const int n_zp = z == arg.Z - 1 ? idx - (arg.Z - 1) * sz : idx + sz;
  const int n_zm = z == 0 ? idx + (arg.Z - 1) * sz : idx - sz;
  const int n_tp = t == arg.T - 1 ? idx - (arg.T - 1) * st : idx + st;
  const int n_tm = t == 0 ? idx + (arg.T - 1) * st : idx - st;

  real acc[24];
#pragma unroll
  for (int k = 0; k < 24; k++) acc[k] = 0;

  constexpr bool PT = VARIANT == 1;
  const real one = 1;
  const real sg_tp = t == arg.T - 1 ? arg.tsign_fwd : one, sg_tm = t == 0 ? arg.tsign_bwd : one;
  // direction order: dir = 2 mu + (0 forward, 1 backward), as the reference (tests/dslash_util.h:131-140)
  RawBlock<T, 24> pA, pB, pC;
  typename Link<T, R>::Raw uA, uB, uC;
  // QA_FENCE: nothing may be scheduled across (machine scheduler).  QA_PIN: an empty volatile asm that "modifies" the
  // accumulators, so LLVM's IR-level sinking cannot push a hop's arithmetic past the following loads either (without it
  // all 8 hops' FMAs sink below the last fence and every loaded register stays live: 390-512 registers, scratch spills).
#define QA_FENCE() __builtin_amdgcn_sched_barrier(0)
#define QA_PIN()                                                   \
  _Pragma("unroll") for (int k_ = 0; k_ < 24; k_++) asm volatile("" : "+v"(acc[k_]))
  // Hop order x+ x- y+ y- z+ z- t+ t- (the reference's direction numbering).  Measured and dropped: t- z- y- x- x+ y+ z+ t+
  // (aligned with an increasing sweep, so that the reads of one input site by different blocks fall closer together in time)
  // changed nothing at 32^4 or 48^3 x 96 in any precision (gpurun_out/sweep48b.log of round 2).
  constexpr int GH = KT == 2 ? 1 : (KT == 3 ? 2 : 0);
  const int nb[8] = {n_xp + fo, n_xm + fo, n_yp + fo, n_ym + fo, n_zp + fo, n_zm + fo, n_tp + fo, n_tm + fo};
  const real sg[8] = {one, one, one, one, one, one, sg_tp, sg_tm};
  const bool of[8] = {o_xp, o_xm, o_yp, o_ym, o_zp, o_zm, o_tp, o_tm};
  const int fc[8] = {f_x, f_x, f_y, f_y, f_z, f_z, f_t, f_t};
#define QA_LD(B, D) hop_load<T, R, D, GAUX, GH>(p##B, u##B, arg, idx, nb[D], of[D], fc[D])
#define QA_CP(B, D) QA_FENCE(); hop_compute<T, R, D, PT, GH>(acc, p##B, u##B, arg, sg[D], of[D], fc[D]); QA_PIN(); QA_FENCE()
#define QA_PIPE(d0, d1, d2, d3, d4, d5, d6, d7)                                                      \
  QA_LD(A, d0); QA_LD(B, d1); QA_CP(A, d0); QA_LD(A, d2); QA_CP(B, d1); QA_LD(B, d3); QA_CP(A, d2);  \
  QA_LD(A, d4); QA_CP(B, d3); QA_LD(B, d5); QA_CP(A, d4); QA_LD(A, d6); QA_CP(B, d5); QA_LD(B, d7);  \
  QA_CP(A, d6); QA_FENCE(); hop_compute<T, R, d7, PT, GH>(acc, pB, uB, arg, sg[d7], of[d7], fc[d7])
  // 16-bit storage: a hop in flight is 22 registers (raw image) and ~1.4 KB per wave, half of what the fp32 kernel keeps in flight at
  // the same depth — three hops deep instead of two
#define QA_PIPE3()                                                                                                     \
  QA_LD(A, 0); QA_LD(B, 1); QA_LD(C, 2); QA_CP(A, 0); QA_LD(A, 3); QA_CP(B, 1); QA_LD(B, 4); QA_CP(C, 2); QA_LD(C, 5); \
  QA_CP(A, 3); QA_LD(A, 6); QA_CP(B, 4); QA_LD(B, 7); QA_CP(C, 5); QA_CP(A, 6); QA_FENCE();                            \
  hop_compute<T, R, 7, PT, GH>(acc, pB, uB, arg, sg[7], of[7], fc[7])
  if (sizeof(T) == 2) { QA_PIPE3(); } else { QA_PIPE(0, 1, 2, 3, 4, 5, 6, 7); }
#undef QA_PIPE
#undef QA_PIPE3
#undef QA_LD
#undef QA_CP
#undef QA_FENCE
#undef QA_PIN

  if (KT == 3) {
    // the hops that leave this rank: wait (only the waves that own boundary sites) until the neighbours' faces are in, then add them
    const bool anyoff = o_xp || o_xm || o_yp || o_ym || o_zp || o_zm || o_tp || o_tm;
    if (__builtin_amdgcn_ballot_w64(anyoff) != 0) {
      if (arg.timeline && (threadIdx.x & 63) == 0) arg.timeline[4096 + (blockIdx.x * 4 + (threadIdx.x >> 6))] = wall_clock64();
      // (two directions in flight per wave — requests of the next while working on this one — measured slower: 26.6 against 25.2 us
      // fp64 on the 8-GPU sub-lattice, the exec-masked merges of the forward and backward lanes cost more than the overlap gains)
      ghost_hop<T, R, 0, GAUX>(acc, arg, idx, o_xp, f_x, one);
      ghost_hop<T, R, 1, GAUX>(acc, arg, idx, o_xm, f_x, one);
      ghost_hop<T, R, 2, GAUX>(acc, arg, idx, o_yp, f_y, one);
      ghost_hop<T, R, 3, GAUX>(acc, arg, idx, o_ym, f_y, one);
      ghost_hop<T, R, 4, GAUX>(acc, arg, idx, o_zp, f_z, one);
      ghost_hop<T, R, 5, GAUX>(acc, arg, idx, o_zm, f_z, one);
      ghost_hop<T, R, 6, GAUX>(acc, arg, idx, o_tp, f_t, sg_tp);
      ghost_hop<T, R, 7, GAUX>(acc, arg, idx, o_tm, f_t, sg_tm);
      if (arg.timeline && (threadIdx.x & 63) == 0) arg.timeline[8192 + (blockIdx.x * 4 + (threadIdx.x >> 6))] = wall_clock64();
    }
  }
  if constexpr (ND != 0) ndeg_epilogue<T, SAUX>(acc, arg, idx + fo, fo != 0);
  else dslash_epilogue<T, VARIANT, GAUX, SAUX>(acc, arg, idx);
}

// physical block b -> logical block (a run of consecutive checkerboard sites): XCD-aware remap, plane-tiled order, y groups, time-slab
// interleave (dslashBlockOrder sets the fields up for the number of SITES per block, which is blockDim.x in dslash_kernel and half of it
// in ndeg_dslash_kernel)
template <typename real> __device__ __forceinline__ int dslash_logical_block(const DslashArg<real> &arg, const int b) {
  const DslashOrder &o = arg.order;
  // XCD-aware block remap: blocks b, b+8, b+16, ... share an XCD (round-robin dispatch); give each XCD a
  // contiguous range of logical blocks (a slab of time slices) so t/z neighbours hit its own L2.
  const int xcd = b & 7, within = b >> 3;
  int lb;
  if (o.tiled) {
    const uint32_t xt = o.dNxz.div((uint32_t)xcd), xz = (uint32_t)xcd - xt * (uint32_t)o.nxz;
    const uint32_t tile = o.dPerTile.div((uint32_t)within), r = (uint32_t)within - tile * o.dPerTile.d;
    const uint32_t tile_t = o.dNtz.div(tile), tile_z = tile - tile_t * o.dNtz.d;
    uint32_t yc, zi, ti;
    if (o.tiled == 3) {
      // y groups: the XCD walks its whole (z-slab, t) range once per GROUP of plane chunks — group slowest, then t, z, chunk in the
      // group.  The set an XCD has to hold for the +-t re-use (three time slices of its slab) shrinks by the number of groups; fp64
      // at 48^3 x 96: 3 x 6 planes x 221 KB = 4 MB, the whole L2, without groups.  (tile = group here: dPerTile = Ts Zs Pg, dTzTt = Zs Pg,
      // dPTt = Pg, tz = Zs, tt = 1)
      const uint32_t tl3 = o.dTzTt.div(r), r2 = r - tl3 * o.dTzTt.d;
      zi = o.dPTt.div(r2);
      yc = tile * o.dPTt.d + (r2 - zi * o.dPTt.d);
      ti = tl3;
    } else if (o.tiled == 2) {   // inside a tile: z slowest, then the chunk of the plane, t fastest (lexicographic for tt = 1)
      zi = o.dPTt.div(r); const uint32_t r2 = r - zi * o.dPTt.d;
      yc = o.dTt.div(r2); ti = r2 - yc * o.dTt.d;
    } else {                // chunk slowest, then z, t fastest
      yc = o.dTzTt.div(r); const uint32_t r2 = r - yc * o.dTzTt.d;
      zi = o.dTt.div(r2); ti = r2 - zi * o.dTt.d;
    }
    int zl = (int)tile_z * o.tz + (int)zi, tl = (int)tile_t * o.tt + (int)ti;
    if (o.tiled == 3) { zl = (int)zi; tl = (int)ti; }
    if (arg.edgeFirst) {
      // partitioned launch: an XCD starts with the blocks that own boundary sites (they have the most to do: the off-node hops come
      // on top, after a wait), and the blocks dispatched last — the ones that share a CU with a pack block — are interior ones.
      // z: the upper half of the XCDs walks its slab downwards; t: a slab that spans the whole extent starts at T - 1 and wraps to
      // 0 (still a contiguous sweep on the periodic lattice), otherwise the upper half walks downwards as well.
      if (2 * (int)xz >= o.nxz) zl = o.Zs - 1 - zl;
      if (o.nxz == 8) tl = tl == 0 ? o.Ts - 1 : tl - 1;
      else if (xt) tl = o.Ts - 1 - tl;
    }
    const int z = (int)xz * o.Zs + zl, t = (int)xt * o.Ts + tl;
    lb = (t * arg.Z + z) * o.P + (int)yc;
  } else {
    lb = (xcd < o.xcd_r ? xcd * (o.xcd_q + 1) : o.xcd_r * (o.xcd_q + 1) + (xcd - o.xcd_r) * o.xcd_q) + within;
    if (o.xcd_q < 0) lb = b;   // remap off: consecutive blocks dealt round-robin over the XCDs (even spread of the boundary work)
    if (o.ts > 0) {
      // inside an XCD's slab of ts time slices walk t fastest: consecutive blocks are the same (y,z) chunk on ts successive
      // slices, so the +-t neighbours of a chunk are touched within a few blocks of each other (L2-resident) instead of a
      // whole slice apart
      const int per = o.bps * o.ts, s = lb / per, w = lb - s * per, c = w / o.ts, tt = w - c * o.ts;
      lb = (s * o.ts + tt) * o.bps + c;
    }
  }
  return lb;
}

template <typename T, int R, int VARIANT, int GAUX, int KT, int SAUX = 0>
__global__ void __launch_bounds__(256) dslash_kernel(const DslashArg<typename Store<T>::real> arg) {
  if (KT == 2) {
    const int tid = blockIdx.x * blockDim.x + threadIdx.x;
    if (tid >= arg.nboundary) return;
    stencil_site<T, R, VARIANT, GAUX, 2, SAUX>(arg, arg.blist[tid]);
    return;
  }
  int b = blockIdx.x;
  if (KT == 3) {
    // single-launch peer-store path: [pack blocks | every site]; boundary sites do their local hops first, then poll the
    // ghost words they need and add the off-node hops (stencil_site, KT == 3)
    if (b < arg.packBlocks) {
      if (arg.packPrio) __builtin_amdgcn_s_setprio(3);
      pack_body<T, VARIANT == 1, true>(arg.pack, b, arg.packChunk);
      return;
    }
    b -= arg.packBlocks;
    // the pack blocks' loads go first: a site wave keeps ~8 us worth of requests queued in its CU, and a pack wave that starts
    // together with it needs 12 (up to 18) us for its two round trips instead of 4
    for (int i = 0; i < arg.siteDelay; i++) __builtin_amdgcn_s_sleep(8);
  }
  const int lb = dslash_logical_block(arg, b);
  const int idx = lb * blockDim.x + threadIdx.x;
  if (idx >= arg.Vh) return;
  if (KT == 3 && arg.timeline && threadIdx.x == 0) {
    arg.timeline[2048 + blockIdx.x] = wall_clock64();
    arg.timeline[3072 + blockIdx.x] = 0x100000000ull | ((unsigned long long)(__builtin_amdgcn_s_getreg(20 | (31 << 11)) & 0xf) << 16) | (__builtin_amdgcn_s_getreg(4 | (31 << 11)) & 0xff00u);
  }
  stencil_site<T, R, VARIANT, GAUX, KT, SAUX>(arg, idx);
  if (KT == 3 && arg.timeline && threadIdx.x == 0) arg.timeline[12288 + blockIdx.x] = wall_clock64();
}

// Fused doublet stencil (unpartitioned launches): one launch computes both flavours of the non-degenerate twisted-mass doublet and
// requests every link once — the two half-waves of a wave run the hop pipeline of stencil_site on the same 32 sites, one flavour
// each, so they ask for the same link addresses, and the flavours meet in the epilogue through v_permlane32_swap.  A block of
// blockDim.x threads is blockDim.x / 2 consecutive sites; in, out and x are parity doublets (planes: flavour 1's Vh sites, then flavour 2's).
template <typename T, int R, int GAUX, int SAUX>
__global__ void __launch_bounds__(256) ndeg_dslash_kernel(const DslashArg<typename Store<T>::real> arg) {
  const int lb = dslash_logical_block(arg, (int)blockIdx.x);
  const int lane = threadIdx.x & 63;
  const int idx = lb * (int)(blockDim.x >> 1) + (int)(threadIdx.x >> 6) * 32 + (lane & 31);
  if (idx >= arg.Vh) return;   // both flavours of a site leave together: a live lane's partner is live
  stencil_site<T, R, 0, GAUX, 0, SAUX, 1>(arg, idx, (lane >> 5) * arg.Vh);
}

// ---- site-local kernel: twist / clover / twisted clover and inverse (reference lib/dslash_quda.cu:348-600) ----
template <typename real> struct SiteArg {
  void *out; float *outNorm;
  const void *in; const float *inNorm;
  const void *clA, *clAinv;
  const float *clAn, *clAinvN;
  int sp_stride, cl_stride, Vh, op;
  real a, b;
};

template <typename T, bool CLOVER>
__global__ void __launch_bounds__(256) site_kernel(const SiteArg<typename Store<T>::real> arg) {
  using real = typename Store<T>::real;
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= arg.Vh) return;
  real v[24];
  Planar<T, 24>::load(v, arg.in, arg.sp_stride, idx, arg.inNorm, idx);
  if (arg.op == SITE_TWIST) {
    twist_inplace(v, arg.a);
#pragma unroll
    for (int k = 0; k < 24; k++) v[k] *= arg.b;
  } else if (CLOVER) {
    real C[36], tmp[24];
#pragma unroll
    for (int chi = 0; chi < 2; chi++) {
      Planar<T, 36>::load(C, (const char *)arg.clA + (size_t)chi * 36 * sizeof(T) * arg.cl_stride, arg.cl_stride, idx, arg.clAn,
                          chi * arg.cl_stride + idx);
      clover_block_mv(tmp + 12 * chi, C, v + 12 * chi);
    }
    if (arg.op != SITE_CLOVER) {
#pragma unroll
      for (int k = 0; k < 6; k++) { tmp[2 * k] -= arg.a * v[2 * k + 1]; tmp[2 * k + 1] += arg.a * v[2 * k]; }
#pragma unroll
      for (int k = 6; k < 12; k++) { tmp[2 * k] += arg.a * v[2 * k + 1]; tmp[2 * k + 1] -= arg.a * v[2 * k]; }
    }
    if (arg.op == SITE_CLOVER_TWIST_INV) {
#pragma unroll
      for (int chi = 0; chi < 2; chi++) {
        Planar<T, 36>::load(C, (const char *)arg.clAinv + (size_t)chi * 36 * sizeof(T) * arg.cl_stride, arg.cl_stride, idx,
                            arg.clAinvN, chi * arg.cl_stride + idx);
        clover_block_mv(v + 12 * chi, C, tmp + 12 * chi);
      }
    } else {
#pragma unroll
      for (int k = 0; k < 24; k++) v[k] = tmp[k];
    }
  }
  Planar<T, 24>::store(v, arg.out, arg.sp_stride, idx, arg.outNorm, idx);
}

// ---- flavour-doublet twist (reference ndeg twistGamma5Cuda, lib/dslash_quda.cu; host tests/wilson_dslash_reference.cpp:411-440) ----
// t1 = d (in1 + i a g5 in1 + b in2), t2 = d (in2 - i a g5 in2 + b in1) on a parity doublet; out = t or, XPAY, out = x + k t.  One thread per
// 4-d site holds both flavours (planes: flavour 1's Vh sites, then flavour 2's) and reads them before it writes, so out may be in (or x)
template <typename real> struct NdegTwistArg {
  void *out; float *outNorm;
  const void *in; const float *inNorm;
  const void *x; const float *xNorm;
  int sp_stride, Vh;
  real a, b, d, k;
};

template <typename T, bool XPAY>
__global__ void __launch_bounds__(256) ndeg_twist_kernel(const NdegTwistArg<typename Store<T>::real> arg) {
  using real = typename Store<T>::real;
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= arg.Vh) return;
  real u[24], v[24], o[24];
  Planar<T, 24>::load(u, arg.in, arg.sp_stride, idx, arg.inNorm, idx);
  Planar<T, 24>::load(v, arg.in, arg.sp_stride, arg.Vh + idx, arg.inNorm, arg.Vh + idx);
#pragma unroll
  for (int f = 0; f < 2; f++) {
    const real *own = f ? v : u, *other = f ? u : v;
    const int site = f * arg.Vh + idx;
#pragma unroll
    for (int k = 0; k < 24; k++) o[k] = own[k];
    twist_inplace(o, f ? -arg.a : arg.a);
#pragma unroll
    for (int k = 0; k < 24; k++) o[k] = arg.d * (o[k] + arg.b * other[k]);
    if (XPAY) {
      real xv[24];
      Planar<T, 24>::load(xv, arg.x, arg.sp_stride, site, arg.xNorm, site);
#pragma unroll
      for (int k = 0; k < 24; k++) o[k] = xv[k] + arg.k * o[k];
    }
    Planar<T, 24>::store(o, arg.out, arg.sp_stride, site, arg.outNorm, site);
  }
}

template <typename T> static void launchNdegTwist(ColorSpinorField &out, const ColorSpinorField &in, double a, double b, double d, const ColorSpinorField *x, double k) {
  using real = typename Store<T>::real;
  NdegTwistArg<real> arg;
  arg.out = out.V(); arg.outNorm = (float *)out.Norm();
  arg.in = in.V(); arg.inNorm = (const float *)in.Norm();
  arg.x = x ? x->V() : nullptr; arg.xNorm = x ? (const float *)x->Norm() : nullptr;
  arg.sp_stride = in.Stride(); arg.Vh = in.VolumeCB4();
  arg.a = (real)a; arg.b = (real)b; arg.d = (real)d; arg.k = (real)k;
  const int bs = 256, nb = (arg.Vh + bs - 1) / bs;
  if (x) hipLaunchKernelGGL((ndeg_twist_kernel<T, true>), dim3(nb), dim3(bs), 0, computeStream(), arg);
  else hipLaunchKernelGGL((ndeg_twist_kernel<T, false>), dim3(nb), dim3(bs), 0, computeStream(), arg);
  HIP_CHECK(hipGetLastError());
}

void ndegTwistCoefficients(double kappa, double mu, double epsilon, bool inverse, bool dagger, double &a, double &b, double &d) {
  a = 2.0 * kappa * mu; b = -2.0 * kappa * epsilon; d = 1.0;
  if (inverse) {
    a = -a; b = -b;
    const double det = 1.0 + a * a - b * b;
    if (det <= 0.0) errorQuda("non-degenerate doublet: 1 + a^2 - b^2 = %g is not positive (kappa %g, mu %g, epsilon %g): the twist has no inverse", det, kappa, mu, epsilon);
    d = 1.0 / det;
  }
  if (dagger) a = -a;
}

void applyNdegTwist(ColorSpinorField &out, const ColorSpinorField &in, double a, double b, double d, const ColorSpinorField *x, double k) {
  if (out.Location() != QUDA_CUDA_FIELD_LOCATION || in.Location() != QUDA_CUDA_FIELD_LOCATION) errorQuda("device fields required");
  if (in.Nflavor() != 2 || out.Nflavor() != 2 || (x && x->Nflavor() != 2)) errorQuda("the doublet twist needs two-flavour fields (got %d, %d flavours)", in.Nflavor(), out.Nflavor());
  if (in.SiteSubset() != QUDA_PARITY_SITE_SUBSET || out.SiteSubset() != QUDA_PARITY_SITE_SUBSET) errorQuda("parity fields required");
  if (in.Precision() != out.Precision() || (x && x->Precision() != in.Precision())) errorQuda("precision mismatch");
  if (in.Nspin() != 4 || in.Ncolor() != 3) errorQuda("the doublet twist needs nSpin=4 nColor=3");
  if (out.Stride() != in.Stride() || out.VolumeCB() != in.VolumeCB()) errorQuda("doublet twist: output stride %d / volume %d against input %d / %d", out.Stride(), out.VolumeCB(), in.Stride(), in.VolumeCB());
  if (x && (x->Stride() != in.Stride() || x->VolumeCB() != in.VolumeCB() || x->SiteSubset() != QUDA_PARITY_SITE_SUBSET)) errorQuda("doublet twist: the xpay field does not match the input");
  if (g_acctOn) acct("ndeg_twist_kernel", (x ? 72.0 : 48.0) * in.Precision() * in.VolumeCB(), "level 0");
  switch (in.Precision()) {
    case QUDA_DOUBLE_PRECISION: launchNdegTwist<double>(out, in, a, b, d, x, k); break;
    case QUDA_SINGLE_PRECISION: launchNdegTwist<float>(out, in, a, b, d, x, k); break;
    case QUDA_HALF_PRECISION: launchNdegTwist<short>(out, in, a, b, d, x, k); break;
    default: errorQuda("bad precision %d", in.Precision());
  }
}

template <typename T, bool PRETWIST, bool P2P = false> __global__ void __launch_bounds__(256) pack_kernel(const PackArg<typename Store<T>::real> arg) {
  pack_body<T, PRETWIST, P2P>(arg, blockIdx.x, (int)blockDim.x);
}

static_assert(GhostLL<double>::NV == ghostLLVectors(8) && GhostLL<float>::NV == ghostLLVectors(4) && GhostLL<short>::NV == ghostLLVectors(2), "halo windows are sized by ghostLLVectors");

// link/clover stream cache policy: nt for the 16-byte-per-lane formats (measured on 32^4: fp64 4.67 -> 5.2 TB/s, fp32
// 4.68 -> 5.16 TB/s algorithmic; the read-once links no longer evict the re-used spinors), default for the 8-byte 16-bit format
// (nt there costs 18 %) — where it is a run-time choice between the build-time default and nt (dslashCachePolicy)
template <typename T> struct LinkPolicy {
  static constexpr int GAUX = sizeof(T) == 2 ? QA_GAUX16 : QA_GAUX;
  static constexpr bool knob = sizeof(T) == 2 && GAUX == 0;
  static constexpr int GNT = knob ? 2 : GAUX;
};

// all sites of an unpartitioned lattice: dslash_kernel or, for a doublet, ndeg_dslash_kernel, in the instantiation the cache policy selects
template <typename T, int R, int VARIANT, int GAUX, int SAUX, typename Arg> static void launchSites(const Arg &arg, bool ndeg, int nb, int threads, size_t lds) {
  if constexpr (VARIANT == 0) {
    if (ndeg) { hipLaunchKernelGGL((ndeg_dslash_kernel<T, R, GAUX, SAUX>), dim3(nb), dim3(threads), lds, computeStream(), arg); return; }
  }
  hipLaunchKernelGGL((dslash_kernel<T, R, VARIANT, GAUX, 0, SAUX>), dim3(nb), dim3(threads), lds, computeStream(), arg);
}

template <typename T, int R, int VARIANT, int GAUX, typename Arg> static void launchExterior(const Arg &arg, hipStream_t s) {
  if (arg.nboundary <= 0) return;
  static int eb = 0;
  if (!eb) { const char *e = getenv("QUDA_AMD_EXT_BLOCK"); eb = e ? atoi(e) : 64; }
  hipLaunchKernelGGL((dslash_kernel<T, R, VARIANT, GAUX, 2>), dim3((arg.nboundary + eb - 1) / eb), dim3(eb), 0, s, arg);
  HIP_CHECK(hipGetLastError());
}

// peer-store transport: ONE launch on ONE stream, [pack blocks | every site].  The pack blocks store the faces straight into
// the neighbours' ghost zones with the exchange's flag inside every word pair; a boundary site does its local hops first
// and then polls exactly the ghost words it needs (ghost_hop).
template <typename T, int R, int VARIANT, typename real>
static void launchPeerStore(DslashArg<real> &arg, PackArg<real> &pa, HaloBuffers &hb, const FacePlan &faces, const DslashTune &tune, int bs, int nb) {
  constexpr int GAUX = LinkPolicy<T>::GAUX;
  hipStream_t cs = computeStream();
  const PeerExchange ex = nextPeerExchange(hb, arg.commMask);
  arg.exSeq = ex.seq; arg.exBuf = ex.buf;
  for (int d = 0; d < 4; d++) {
    pa.send[d][0] = hb.peerGhost[d][0][ex.buf]; pa.send[d][1] = hb.peerGhost[d][1][ex.buf];
    if (!faces.on[d]) continue;
    arg.ghost[d][0] = hb.ghostBuf[d][0][ex.buf]; arg.ghost[d][1] = hb.ghostBuf[d][1][ex.buf];
    pa.llFlag[d] = ex.flag[d];
    arg.waitCount[2 * d] = arg.waitCount[2 * d + 1] = ex.flag[d];
  }
  pa.llFormat = haloWireFormat();
  arg.waitTicks = p2pTimeoutTicks(); arg.errWord = p2pErrorWord();
  arg.siteDelay = tune.site_delay; arg.packPrio = tune.pack_prio; arg.edgeFirst = p2pDeviceShared() ? 0 : tune.edge_first;   // ranks sharing a device: interior blocks first (p2p.h)
  // Full pack blocks (256 face sites each) in front of the grid.  They share CUs with site blocks, and the placement statistics of
  // the timeline show what that costs on the 8-GPU sub-lattice: a site block next to a pack block ends 4.3 us later than one
  // that has its CU to itself.  Spreading the packing thinly (one 96-thread pack block on EVERY CU) is far worse — 46 us
  // instead of 29, every site block ends late — so the system-scope write-through stores of a pack wave appear to hold up the
  // memory pipeline of the whole CU, and fewer CUs doing all of it is the better trade.
  // rounded up to a multiple of 8: blockIdx.x and the site-block number then agree mod 8, i.e. on the XCD (surplus pack blocks leave at once)
  arg.packBlocks = ((faces.start[8] + bs - 1) / bs + 7) / 8 * 8; arg.packChunk = bs;
  if (unsigned long long *tl = dslashTimelineBuffer()) {
    static int calls = 0;
    if (++calls == 60 && arg.packBlocks + nb <= 1024) {
      HIP_CHECK(hipStreamSynchronize(cs));
      memset(tl, 0, 16384 * sizeof(unsigned long long));
      pa.timeline = tl; arg.timeline = tl; arg.pack = pa;
      hipLaunchKernelGGL((dslash_kernel<T, R, VARIANT, GAUX, 3>), dim3(arg.packBlocks + nb), dim3(bs), 0, cs, arg);
      HIP_CHECK(hipStreamSynchronize(cs));
      dslashTimelineReport(tl, arg.packBlocks, nb);
      return;
    }
  }
  arg.pack = pa;
  hipLaunchKernelGGL((dslash_kernel<T, R, VARIANT, GAUX, 3>), dim3(arg.packBlocks + nb), dim3(bs), 0, cs, arg);
  HIP_CHECK(hipGetLastError());
}

static hipEvent_t g_evIn = nullptr, g_evHalo = nullptr;
// staged transport: pack + ONE grouped RCCL send/recv on the comms stream, interior stencil on the compute stream meanwhile,
// then the exterior pass over the boundary-site list
template <typename T, int R, int VARIANT, typename real>
static void launchStaged(DslashArg<real> &arg, PackArg<real> &pa, HaloBuffers &hb, const FacePlan &faces, int bs, int nb) {
  constexpr int GAUX = LinkPolicy<T>::GAUX;
  if (!g_evIn) { HIP_CHECK(hipEventCreateWithFlags(&g_evIn, hipEventDisableTiming)); HIP_CHECK(hipEventCreateWithFlags(&g_evHalo, hipEventDisableTiming)); }
  p2pStats()[1]++;
  hipStream_t cs = computeStream(), ms = commStream();
  HIP_CHECK(hipEventRecord(g_evIn, cs));            // `in` is complete and the previous exterior pass has released the ghost zone
  HIP_CHECK(hipStreamWaitEvent(ms, g_evIn, 0));
  std::vector<HaloMsg> msgs;
  for (int d = 0; d < 4; d++) {
    pa.normOff[d] = (int)hb.norm_offset[d];
    pa.send[d][0] = hb.send[d][0]; pa.send[d][1] = hb.send[d][1];
    if (!faces.on[d]) continue;
    // sent forward -> arrives in the +d neighbour's "from behind" zone; the matching receive fills ours from our -d neighbour
    msgs.push_back({d, +1, hb.send[d][1], hb.ghost[d][0], hb.face_bytes[d]});
    msgs.push_back({d, -1, hb.send[d][0], hb.ghost[d][1], hb.face_bytes[d]});
    arg.ghost[d][0] = hb.ghost[d][0]; arg.ghost[d][1] = hb.ghost[d][1];
    arg.ghostNormOff[d] = (int)hb.norm_offset[d];
  }
  hipLaunchKernelGGL((pack_kernel<T, VARIANT == 1>), dim3((faces.start[8] + 255) / 256), dim3(256), 0, ms, pa);
  HIP_CHECK(hipGetLastError());
  commExchange(msgs, ms);
  HIP_CHECK(hipEventRecord(g_evHalo, ms));

  hipLaunchKernelGGL((dslash_kernel<T, R, VARIANT, GAUX, 1>), dim3(nb), dim3(bs), 0, cs, arg);   // interior
  HIP_CHECK(hipGetLastError());
  HIP_CHECK(hipStreamWaitEvent(cs, g_evHalo, 0));
  launchExterior<T, R, VARIANT, GAUX>(arg, cs);
}

// Builds the kernel argument, asks dslash_launch.h for the plan of this launch and picks the instantiation.  candidate: knobs of a sweep
// candidate being timed; transport: which halo transport a partitioned launch takes (HALO_AUTO: peer stores once verified, else staged)
template <typename T, int R, int VARIANT>
static void launchDslash(ColorSpinorField &out, const ColorSpinorField &in, const GaugeField &U, const DslashParam &p, const DslashTune *candidate = nullptr,
                         HaloTransport transport = HALO_AUTO) {
  using real = typename Store<T>::real;
  const LatticeGeom &g = U.geom;
  const int mask = partitionMask();
  const auto applyWith = [&](const DslashTune *c) { launchDslash<T, R, VARIANT>(out, in, U, p, c, transport); };
  const DslashTune tune = effectiveDslashTune(g, in.Precision(), R, VARIANT, p, mask, candidate, transport, std::cref(applyWith));

  DslashArg<real> arg{};
  fillDslashFields(arg, &out, &in, U, p.parity);
  arg.x = p.x ? p.x->V() : nullptr; arg.xNorm = p.x ? (const float *)p.x->Norm() : nullptr;
  if (VARIANT == 2) {
    arg.clA = p.clover->A(p.parity); arg.clAinv = p.clover->Ainv(p.parity);
    arg.clAn = p.clover->Anorm(p.parity); arg.clAinvN = p.clover->AinvNorm(p.parity);
    arg.cl_stride = p.clover->stride;
  }
  arg.mode = p.mode; arg.xpay = p.x ? 1 : 0;
  arg.sfwd = p.dagger ? -1 : 1;
  arg.a = (real)p.a; arg.b = (real)p.b; arg.k = (real)p.k; arg.nb = (real)p.nb;
  for (int d = 0; d < 4; d++) arg.faceCB[d] = g.faceCB[d];

  const int fl = p.ndeg ? 2 : 1;   // fused doublet stencil: bs counts the SITES of a block, its threads are twice that
  const int bs = dslashBlockSites(g, tune.block, fl), nb = (g.Vh + bs - 1) / bs;
  setLastKernel(VARIANT == 2 ? "dslash_kernel (clover)" : "dslash_kernel", g.X, (int)sizeof(T), R, bs);
  arg.order = dslashBlockOrder(g, tune, bs, (int)sizeof(T));

  if (p.ndeg) {
    if (VARIANT != 0) errorQuda("fused doublet stencil: plain, twist-inverse and twist-xpay epilogues only (mode %d)", (int)p.mode);
    if (mask != 0) errorQuda("the fused doublet stencil has no halo path (partition mask %d): use the composed doublet operators", mask);
    setLastKernel("ndeg_dslash_kernel", g.X, (int)sizeof(T), R, bs * fl);
  }
  if (mask == 0) {
    const size_t lds = tune.lds_pad > 0 ? (size_t)tune.lds_pad : 0;   // measurement aid: dynamic LDS only to cap the blocks per CU
    const long long perSite = p.ndeg ? ndegDslashBytesPerSite(in.Precision(), R, p.x != nullptr) : dslashBytesPerSite(in.Precision(), R, p.mode, p.x != nullptr);
    const DslashCachePolicy c = dslashCachePolicy(tune, (long)fl * g.Vh, LinkPolicy<T>::knob, (size_t)g.Vh * (size_t)perSite);
    constexpr int G0 = LinkPolicy<T>::GAUX, G2 = LinkPolicy<T>::GNT;
    if (c.ntLinks) c.ntStore ? launchSites<T, R, VARIANT, G2, 2>(arg, p.ndeg, nb, bs * fl, lds) : launchSites<T, R, VARIANT, G2, 0>(arg, p.ndeg, nb, bs * fl, lds);
    else c.ntStore ? launchSites<T, R, VARIANT, G0, 2>(arg, p.ndeg, nb, bs * fl, lds) : launchSites<T, R, VARIANT, G0, 0>(arg, p.ndeg, nb, bs * fl, lds);
    HIP_CHECK(hipGetLastError());
    return;
  }

  // ---- grid-decomposed lattice (reference policies DslashCuda2 / DslashFusedExterior, lib/dslash_policy.cuh) ----
  HaloBuffers &hb = haloBuffers(g, in.Precision());
  if (transport == HALO_AUTO && hb.p2p && hb.verified == 0 && !p.x) {
    // first use of the peer-store transport for this precision (applications with an xpay field before that point go the staged
    // way: the check runs the kernel twice on `out`)
    const auto applyThrough = [&](HaloTransport t) { launchDslash<T, R, VARIANT>(out, in, U, p, nullptr, t); };
    verifyPeerStoreHalo(hb, out, sizeof(T) == 8 ? 1e-10 : (sizeof(T) == 4 ? 1e-4 : 3e-2), std::cref(applyThrough));
    return;
  }
  if (transport == HALO_AUTO) transport = hb.p2p && hb.verified == 1 ? HALO_PEER_STORE : HALO_STAGED;
  const BoundaryList &bl = boundaryList(g, mask);
  const FacePlan faces = dslashFacePlan(g, mask);
  PackArg<real> pa{};
  pa.in = in.V(); pa.inNorm = (const float *)in.Norm(); pa.sp_stride = in.Stride();
  for (int d = 0; d < 4; d++) { pa.X[d] = g.X[d]; pa.faceCB[d] = g.faceCB[d]; }
  pa.parity_in = 1 - p.parity; pa.sfwd = arg.sfwd; pa.a = arg.a;
  memcpy(pa.start, faces.start, sizeof(pa.start));
  arg.commMask = mask;
  arg.blist = bl.d_idx[p.parity]; arg.nboundary = bl.count[p.parity];
  if (transport == HALO_PEER_STORE) launchPeerStore<T, R, VARIANT>(arg, pa, hb, faces, tune, bs, nb);
  else launchStaged<T, R, VARIANT>(arg, pa, hb, faces, bs, nb);
}

template <typename T> static void dispatchRecon(ColorSpinorField &out, const ColorSpinorField &in, const GaugeField &U, const DslashParam &p) {
  const bool clover = p.mode == DSLASH_CLOVER_TWIST_INV || p.mode == DSLASH_CLOVER_TWIST_XPAY;
  if (clover && !p.clover) errorQuda("clover field required for dslash mode %d", p.mode);
  const int variant = clover ? 2 : (p.mode == DSLASH_TWIST_INV_DSLASH ? 1 : 0);
  if (U.reconstruct == QUDA_RECONSTRUCT_NO) {
    if (variant == 2) launchDslash<T, 18, 2>(out, in, U, p);
    else if (variant == 1) launchDslash<T, 18, 1>(out, in, U, p);
    else launchDslash<T, 18, 0>(out, in, U, p);
  } else if (U.reconstruct == QUDA_RECONSTRUCT_12) {
    if (variant == 2) launchDslash<T, 12, 2>(out, in, U, p);
    else if (variant == 1) launchDslash<T, 12, 1>(out, in, U, p);
    else launchDslash<T, 12, 0>(out, in, U, p);
  } else if (U.reconstruct == QUDA_RECONSTRUCT_8) {   // reference: the RECONSTRUCT_8 variants of every Wilson-type stencil, lib/dslash_quda.cuh:16-52
    if (variant == 2) launchDslash<T, 8, 2>(out, in, U, p);
    else if (variant == 1) launchDslash<T, 8, 1>(out, in, U, p);
    else launchDslash<T, 8, 0>(out, in, U, p);
  } else {
    errorQuda("reconstruct %d not supported (18, 12 and 8)", U.reconstruct);
  }
}

void applyDslash(ColorSpinorField &out, const ColorSpinorField &in, const GaugeField &U, const DslashParam &p) {
  if (out.Location() != QUDA_CUDA_FIELD_LOCATION || in.Location() != QUDA_CUDA_FIELD_LOCATION) errorQuda("device fields required");
  if (in.SiteSubset() != QUDA_PARITY_SITE_SUBSET || out.SiteSubset() != QUDA_PARITY_SITE_SUBSET) errorQuda("parity fields required");
  if (in.Precision() != out.Precision() || in.Precision() != U.precision) errorQuda("precision mismatch: spinor %d/%d gauge %d", in.Precision(), out.Precision(), U.precision);
  if (p.x && p.x->Precision() != in.Precision()) errorQuda("xpay precision mismatch");
  if (in.VolumeCB4() != U.geom.Vh || out.VolumeCB4() != U.geom.Vh) errorQuda("volume mismatch: spinor %d gauge %d", in.VolumeCB4(), U.geom.Vh);
  const int nfl = p.ndeg ? 2 : 1;   // the fused doublet stencil works on whole doublets, everything else on one flavour (Flavor() views of a doublet)
  if (in.Nflavor() != nfl || out.Nflavor() != nfl || (p.x && p.x->Nflavor() != nfl)) errorQuda("stencil on %d flavour(s): fields of %d / %d flavours", nfl, in.Nflavor(), out.Nflavor());
  if (p.ndeg && (p.mode != DSLASH_PLAIN && p.mode != DSLASH_TWIST_INV && p.mode != DSLASH_TWIST_XPAY)) errorQuda("fused doublet stencil: plain, twist-inverse and twist-xpay epilogues only (mode %d)", (int)p.mode);
  if (p.ndeg && p.mode == DSLASH_TWIST_XPAY && !p.x) errorQuda("fused doublet stencil: the twist-xpay epilogue needs x");
  if (in.Stride() != out.Stride() || (p.x && p.x->Stride() != in.Stride())) errorQuda("stencil: the fields' strides differ (%d, %d)", in.Stride(), out.Stride());
  if (in.V() == out.V()) errorQuda("in and out must not alias");
  if (in.Nspin() != 4 || in.Ncolor() != 3) errorQuda("fine-grid dslash needs nSpin=4 nColor=3");
  if (p.clover && p.clover->precision != in.Precision()) errorQuda("clover precision mismatch");
  if (g_acctOn) {   // one dslash_kernel launch on an unpartitioned lattice (the case the profile tool measures)
    char tag[48];
    snprintf(tag, sizeof(tag), "level 0 prec %d mode %d%s", (int)in.Precision(), (int)p.mode, p.x ? " xpay" : "");
    if (p.ndeg) acct("ndeg_dslash_kernel", (double)ndegDslashBytesPerSite(in.Precision(), (int)U.reconstruct, p.x != nullptr) * in.VolumeCB4(), tag);
    else acct("dslash_kernel", (double)dslashBytesPerSite(in.Precision(), (int)U.reconstruct, p.mode, p.x != nullptr) * in.VolumeCB(), tag);
  }
  switch (in.Precision()) {
    case QUDA_DOUBLE_PRECISION: dispatchRecon<double>(out, in, U, p); break;
    case QUDA_SINGLE_PRECISION: dispatchRecon<float>(out, in, U, p); break;
    case QUDA_HALF_PRECISION: dispatchRecon<short>(out, in, U, p); break;
    default: errorQuda("bad precision %d", in.Precision());
  }
}

template <typename T> static void launchSite(ColorSpinorField &out, const ColorSpinorField &in, SiteOp op, double a, double b,
                                             const CloverField *cl, int parity, bool inverse) {
  using real = typename Store<T>::real;
  SiteArg<real> arg;
  if (out.Stride() != in.Stride() || out.VolumeCB() != in.VolumeCB()) errorQuda("site operator: output stride %d / volume %d against input %d / %d", out.Stride(), out.VolumeCB(), in.Stride(), in.VolumeCB());
  arg.out = out.V(); arg.outNorm = (float *)out.Norm();
  arg.in = in.V(); arg.inNorm = (const float *)in.Norm();
  arg.sp_stride = in.Stride(); arg.Vh = in.VolumeCB(); arg.op = op;
  arg.a = (real)a; arg.b = (real)b;
  arg.clA = arg.clAinv = nullptr; arg.clAn = arg.clAinvN = nullptr; arg.cl_stride = 0;
  const int bs = 256, nb = (arg.Vh + bs - 1) / bs;
  if (op == SITE_TWIST) {
    hipLaunchKernelGGL((site_kernel<T, false>), dim3(nb), dim3(bs), 0, computeStream(), arg);
  } else {
    if (!cl) errorQuda("clover field required");
    if (op == SITE_CLOVER && inverse) { arg.clA = cl->Ainv(parity); arg.clAn = cl->AinvNorm(parity); }
    else { arg.clA = cl->A(parity); arg.clAn = cl->Anorm(parity); }
    arg.clAinv = cl->Ainv(parity); arg.clAinvN = cl->AinvNorm(parity);
    arg.cl_stride = cl->stride;
    hipLaunchKernelGGL((site_kernel<T, true>), dim3(nb), dim3(bs), 0, computeStream(), arg);
  }
  HIP_CHECK(hipGetLastError());
}

void applySite(ColorSpinorField &out, const ColorSpinorField &in, SiteOp op, double a, double b, const CloverField *clover,
               int parity, bool inverse) {
  if (in.Precision() != out.Precision()) errorQuda("precision mismatch");
  if (in.SiteSubset() != QUDA_PARITY_SITE_SUBSET) errorQuda("parity fields required");
  if (clover && clover->precision != in.Precision()) errorQuda("clover precision mismatch");
  if (g_acctOn) {
    const double P = in.Precision();
    acct("site_kernel", (48 * P + (op == SITE_TWIST ? 0 : (op == SITE_CLOVER_TWIST_INV ? 144 : 72) * P)) * in.VolumeCB(), "level 0");
  }
  switch (in.Precision()) {
    case QUDA_DOUBLE_PRECISION: launchSite<double>(out, in, op, a, b, clover, parity, inverse); break;
    case QUDA_SINGLE_PRECISION: launchSite<float>(out, in, op, a, b, clover, parity, inverse); break;
    case QUDA_HALF_PRECISION: launchSite<short>(out, in, op, a, b, clover, parity, inverse); break;
    default: errorQuda("bad precision %d", in.Precision());
  }
}

}  // namespace quda
