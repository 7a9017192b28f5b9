// dslash_arg.h — kernel arguments of the fine-grid stencil family (dslash.hip, hop.hip) and the spin algebra its kernels share
// (also used by fine_block.hip): spin projection / reconstruction in the chiral basis, the twist, one hop on unpacked operands.
#pragma once

#include "device_io.h"
#include "dslash.h"
#include "dslash_launch.h"

namespace quda {

// ---- face packing: spin-project the boundary sites of the INPUT field into the send buffers of every partitioned
// dimension in one launch (reference packFaceWilsonKernel / packTwistedFaceWilsonKernel, lib/dslash_pack.cu:272, :610) ----
template <typename real> struct PackArg {
  const void *in;
  const float *inNorm;
  int sp_stride;
  int X[4];         // full local extents
  int parity_in;    // parity of the input field
  real sfwd, a;
  char *send[4][2]; // [dim][0: to the -dim neighbour, 1: to the +dim neighbour]
  int faceCB[4];
  int normOff[4];
  int start[9];     // prefix offsets of the 8 (dim, dir) thread ranges
  // peer-store transport: send[][] point into the NEIGHBOURS' ghost zones; the last block to finish raises the flags there
  unsigned llFlag[4];      // flag-in-data value of this exchange per dimension (use count of the (dimension, buffer) zone)
  int llFormat;            // wire format of the peer-store ghost zones: 0 flag-in-data {word, flag, word, flag} vectors, 1 self-validating 16-byte atoms {3 words, flag} (GhostLL)
  unsigned long long *timeline;
};

template <typename real> struct DslashArg {
  void *out;
  float *outNorm;
  const void *in;
  const float *inNorm;
  const void *x;
  const float *xNorm;
  const char *gauge;  // base of this parity's 8 direction blocks
  size_t link_bytes;
  const void *clA, *clAinv;
  const float *clAn, *clAinvN;
  int sp_stride, g_stride, cl_stride;
  int Vh, Xh, Y, Z, T;
  FastDiv dXh, dY, dZ;
  int parity, mode, xpay;
  real sfwd;              // +1 no dagger, -1 dagger (selects P-/+ per reference :122)
  real a, b, k;
  real tsign_fwd, tsign_bwd;  // recon-12: sign of the reconstructed row of t-links on the boundary slices
  DslashOrder order;          // physical block -> logical block (dslash_launch.h dslashBlockOrder, dslash.hip dslash_logical_block)
  // grid-decomposed lattices (halo.h)
  int commMask;               // bit d set: dimension d is partitioned
  const int *blist;           // exterior kernel: checkerboard indices of the boundary sites
  int nboundary;
  const char *ghost[4][2];    // [dim][0: from the -dim neighbour, 1: from the +dim neighbour] spin-projected half spinors
  int faceCB[4];
  int ghostNormOff[4];        // byte offset of the fp32 scales inside a ghost block (16-bit storage)
  // peer-store transport (p2p.h): every ghost word carries the flag of its exchange (GhostLL); waitCount[dir] is the value the
  // off-node hop in direction dir expects, waitTicks bounds the polling, a time-out lands in *errWord
  unsigned waitCount[8];
  unsigned long long waitTicks;
  int siteDelay, packPrio;   // peer-store launch: site blocks start siteDelay x 64 x 8 cycles late; pack waves raise their issue priority
  int *errWord;              // error record (p2p.h kP2pErrInts)
  unsigned exSeq; int exBuf; // exchange number / buffer of this launch, for that record
  // peer-store transport: the first packBlocks blocks of the interior launch pack the faces (pack_body) while the rest of
  // the grid does the interior stencil — one launch, the faces leave at time zero and travel during the interior pass
  int packBlocks, packChunk;
  int edgeFirst;   // plane-tiled order of a partitioned launch: boundary planes first in every XCD (dslash_kernel)
  PackArg<real> pack;
  unsigned long long *timeline;   // QUDA_AMD_TIMELINE=1: per-block wall_clock64 stamps (measurement aid), else nullptr
  real nb;   // fused doublet stencil (ndeg_dslash_kernel): the flavour-mixing coefficient b of 1 + i a g5 tau3 + b tau1; a and the scale d travel in a, b
};

// ---- spin projection / reconstruction in the chiral basis; s = +1 selects projector[2 mu], -1 projector[2 mu + 1]
// of the reference table (tests/wilson_dslash_reference.cpp:21-70) ----
// fp32: one packed multiply-add per projected colour component (6 per hop instead of 12), pk:: of device_io.h
template <int MU> __device__ __forceinline__ void spin_project(float *h, const float *p, float s) {
  const pkf2 S = {s, s};
#pragma unroll
  for (int c = 0; c < 3; c++) {
    const pkf2 p0 = pk::ld(p, 2 * c), p1 = pk::ld(p, 6 + 2 * c), p2 = pk::ld(p, 12 + 2 * c), p3 = pk::ld(p, 18 + 2 * c);
    pkf2 h0, h1;
    if (MU == 0) { h0 = pk::aixmy(S, p3, p0); h1 = pk::aixmy(S, p2, p1); }        // h0 = p0 - s i p3, h1 = p1 - s i p2
    else if (MU == 1) { h0 = pk::axpy(S, p3, p0); h1 = pk::axmy(S, p2, p1); }     // h0 = p0 + s p3,   h1 = p1 - s p2
    else if (MU == 2) { h0 = pk::aixmy(S, p2, p0); h1 = pk::aixpy(S, p3, p1); }   // h0 = p0 - s i p2, h1 = p1 + s i p3
    else { h0 = pk::axmy(S, p2, p0); h1 = pk::axmy(S, p3, p1); }                  // h0 = p0 - s p2,   h1 = p1 - s p3
    pk::st(h, 2 * c, h0); pk::st(h, 6 + 2 * c, h1);
  }
}
template <int MU, typename real> __device__ __forceinline__ void spin_project(real *h, const real *p, real s) {
#pragma unroll
  for (int c = 0; c < 3; c++) {
    const real p0r = p[0 + 2 * c], p0i = p[1 + 2 * c], p1r = p[6 + 2 * c], p1i = p[7 + 2 * c];
    const real p2r = p[12 + 2 * c], p2i = p[13 + 2 * c], p3r = p[18 + 2 * c], p3i = p[19 + 2 * c];
    if (MU == 0) {  // h0 = p0 - s i p3, h1 = p1 - s i p2
      h[2 * c] = p0r + s * p3i; h[2 * c + 1] = p0i - s * p3r;
      h[6 + 2 * c] = p1r + s * p2i; h[7 + 2 * c] = p1i - s * p2r;
    } else if (MU == 1) {  // h0 = p0 + s p3, h1 = p1 - s p2
      h[2 * c] = p0r + s * p3r; h[2 * c + 1] = p0i + s * p3i;
      h[6 + 2 * c] = p1r - s * p2r; h[7 + 2 * c] = p1i - s * p2i;
    } else if (MU == 2) {  // h0 = p0 - s i p2, h1 = p1 + s i p3
      h[2 * c] = p0r + s * p2i; h[2 * c + 1] = p0i - s * p2r;
      h[6 + 2 * c] = p1r - s * p3i; h[7 + 2 * c] = p1i + s * p3r;
    } else {  // h0 = p0 - s p2, h1 = p1 - s p3
      h[2 * c] = p0r - s * p2r; h[2 * c + 1] = p0i - s * p2i;
      h[6 + 2 * c] = p1r - s * p3r; h[7 + 2 * c] = p1i - s * p3i;
    }
  }
}

// fp32: acc += w (reconstruction of g) in 12 packed instructions (w = 1: plain reconstruction)
template <int MU> __device__ __forceinline__ void spin_reconstruct_pk(float *acc, const float *g, float s, float w) {
  const pkf2 W = {w, w}, SW = {s * w, s * w};
#pragma unroll
  for (int c = 0; c < 3; c++) {
    const pkf2 g0 = pk::ld(g, 2 * c), g1 = pk::ld(g, 6 + 2 * c);
    pk::st(acc, 2 * c, pk::axpy(W, g0, pk::ld(acc, 2 * c)));
    pk::st(acc, 6 + 2 * c, pk::axpy(W, g1, pk::ld(acc, 6 + 2 * c)));
    pkf2 a2 = pk::ld(acc, 12 + 2 * c), a3 = pk::ld(acc, 18 + 2 * c);
    if (MU == 0) { a2 = pk::aixpy(SW, g1, a2); a3 = pk::aixpy(SW, g0, a3); }        // r2 = s i g1, r3 = s i g0
    else if (MU == 1) { a2 = pk::axmy(SW, g1, a2); a3 = pk::axpy(SW, g0, a3); }     // r2 = -s g1,  r3 = s g0
    else if (MU == 2) { a2 = pk::aixpy(SW, g0, a2); a3 = pk::aixmy(SW, g1, a3); }   // r2 = s i g0, r3 = -s i g1
    else { a2 = pk::axmy(SW, g0, a2); a3 = pk::axmy(SW, g1, a3); }                  // r2 = -s g0,  r3 = -s g1
    pk::st(acc, 12 + 2 * c, a2); pk::st(acc, 18 + 2 * c, a3);
  }
}
template <int MU> __device__ __forceinline__ void spin_reconstruct(float *acc, const float *g, float s) { spin_reconstruct_pk<MU>(acc, g, s, 1.0f); }
template <int MU, typename real> __device__ __forceinline__ void spin_reconstruct(real *acc, const real *g, real s) {
#pragma unroll
  for (int c = 0; c < 3; c++) {
    const real g0r = g[2 * c], g0i = g[2 * c + 1], g1r = g[6 + 2 * c], g1i = g[7 + 2 * c];
    acc[0 + 2 * c] += g0r; acc[1 + 2 * c] += g0i;
    acc[6 + 2 * c] += g1r; acc[7 + 2 * c] += g1i;
    if (MU == 0) {  // r2 = s i g1, r3 = s i g0
      acc[12 + 2 * c] -= s * g1i; acc[13 + 2 * c] += s * g1r;
      acc[18 + 2 * c] -= s * g0i; acc[19 + 2 * c] += s * g0r;
    } else if (MU == 1) {  // r2 = -s g1, r3 = s g0
      acc[12 + 2 * c] -= s * g1r; acc[13 + 2 * c] -= s * g1i;
      acc[18 + 2 * c] += s * g0r; acc[19 + 2 * c] += s * g0i;
    } else if (MU == 2) {  // r2 = s i g0, r3 = -s i g1
      acc[12 + 2 * c] -= s * g0i; acc[13 + 2 * c] += s * g0r;
      acc[18 + 2 * c] += s * g1i; acc[19 + 2 * c] -= s * g1r;
    } else {  // r2 = -s g0, r3 = -s g1
      acc[12 + 2 * c] -= s * g0r; acc[13 + 2 * c] -= s * g0i;
      acc[18 + 2 * c] -= s * g1r; acc[19 + 2 * c] -= s * g1i;
    }
  }
}

// acc += w (reconstruction of g): the same 24 instructions as above (12 adds become multiply-adds) — how the 16-bit kernels apply the
// scale of a neighbour's integers (site scale x link scale) for free, instead of to every one of the 24 + 18 converted operands
template <int MU> __device__ __forceinline__ void spin_reconstruct_scaled(float *acc, const float *g, float s, float w) { spin_reconstruct_pk<MU>(acc, g, s, w); }
template <int MU, typename real> __device__ __forceinline__ void spin_reconstruct_scaled(real *acc, const real *g, real s, real w) {
  const real sw = s * w;
#pragma unroll
  for (int c = 0; c < 3; c++) {
    const real g0r = g[2 * c], g0i = g[2 * c + 1], g1r = g[6 + 2 * c], g1i = g[7 + 2 * c];
    acc[0 + 2 * c] += w * g0r; acc[1 + 2 * c] += w * g0i;
    acc[6 + 2 * c] += w * g1r; acc[7 + 2 * c] += w * g1i;
    if (MU == 0) {
      acc[12 + 2 * c] -= sw * g1i; acc[13 + 2 * c] += sw * g1r;
      acc[18 + 2 * c] -= sw * g0i; acc[19 + 2 * c] += sw * g0r;
    } else if (MU == 1) {
      acc[12 + 2 * c] -= sw * g1r; acc[13 + 2 * c] -= sw * g1i;
      acc[18 + 2 * c] += sw * g0r; acc[19 + 2 * c] += sw * g0i;
    } else if (MU == 2) {
      acc[12 + 2 * c] -= sw * g0i; acc[13 + 2 * c] += sw * g0r;
      acc[18 + 2 * c] += sw * g1i; acc[19 + 2 * c] -= sw * g1r;
    } else {
      acc[12 + 2 * c] -= sw * g0r; acc[13 + 2 * c] -= sw * g0i;
      acc[18 + 2 * c] -= sw * g1r; acc[19 + 2 * c] -= sw * g1i;
    }
  }
}

// (1 + i a g5) in place; g5 = diag(+,+,-,-)
template <typename real> __device__ __forceinline__ void twist_inplace(real *p, real a) {
#pragma unroll
  for (int k = 0; k < 6; k++) {
    const real r = p[2 * k], i = p[2 * k + 1];
    p[2 * k] = r - a * i;
    p[2 * k + 1] = i + a * r;
  }
#pragma unroll
  for (int k = 6; k < 12; k++) {
    const real r = p[2 * k], i = p[2 * k + 1];
    p[2 * k] = r + a * i;
    p[2 * k + 1] = i - a * r;
  }
}

// project / multiply / reconstruct on unpacked operands
template <int DIR, bool PRETWIST, int GH, bool SCALED = false, typename real>
__device__ __forceinline__ void hop_arith(real *acc, real *psi, const real *U, const DslashArg<real> &arg, bool off_node = false, real w = 1) {
  constexpr int MU = DIR / 2;
  real h[12], g[12];
  const real s = (DIR & 1) ? -arg.sfwd : arg.sfwd;
  if (GH == 1 && off_node) {
#pragma unroll
    for (int k = 0; k < 12; k++) h[k] = psi[k];
  } else {
    if (PRETWIST) twist_inplace(psi, arg.a);  // QUDA_DEG_TWIST_INV_DSLASH: A^-1 applied to the neighbour before the hop
    spin_project<MU>(h, psi, s);
    if (GH == 2) {   // off-node hop: added later from the ghost zone (ghost_hop); select, not branch
#pragma unroll
      for (int k = 0; k < 12; k++) h[k] = off_node ? (real)0 : h[k];
    }
  }
  su3_mv(g, U, h);
  su3_mv(g + 6, U, h + 6);
  if (SCALED) spin_reconstruct_scaled<MU>(acc, g, s, w);
  else spin_reconstruct<MU>(acc, g, s);
}

// field, geometry and t-boundary-sign members of a DslashArg (everything else stays value-initialised); out / in may be nullptr
template <typename real>
inline void fillDslashFields(DslashArg<real> &arg, ColorSpinorField *out, const ColorSpinorField *in, const GaugeField &U, int parity) {
  const LatticeGeom &g = U.geom;
  if (out) { arg.out = out->V(); arg.outNorm = (float *)out->Norm(); }
  if (in) { arg.in = in->V(); arg.inNorm = (const float *)in->Norm(); arg.sp_stride = in->Stride(); }
  arg.gauge = (const char *)U.parityBase(parity);
  arg.link_bytes = U.link_bytes; arg.g_stride = U.stride;
  arg.Vh = g.Vh; arg.Xh = g.Xh; arg.Y = g.X[1]; arg.Z = g.X[2]; arg.T = g.X[3];
  arg.dXh = g.dXh; arg.dY = g.dY; arg.dZ = g.dZ;
  arg.parity = parity;
  // recon-12: the reconstructed row of boundary t-links carries the (folded) boundary sign; recon-8: u0 of the reconstruction is that sign
  const bool flip = U.reconstruct != QUDA_RECONSTRUCT_NO && U.t_boundary == QUDA_ANTI_PERIODIC_T;
  arg.tsign_fwd = (flip && commGrid().coords[3] == commGrid().dims[3] - 1) ? -1 : 1;
  arg.tsign_bwd = (flip && commGrid().coords[3] == 0) ? -1 : 1;
}

}  // namespace quda
