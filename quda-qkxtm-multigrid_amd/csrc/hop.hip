// hop.hip — set-up-time relatives of the fine-grid stencil for gfx950 (MI355X): the single-direction hop and covariant shift, the
// "UV" step of the direct Galerkin construction, the neighbour shift of a site field, and the full-face exchange they share.
// Kernel arguments and the hop arithmetic are those of the stencil (dslash_arg.h).
#include "dslash.h"

#include <vector>

#include "device_io.h"
#include "dslash_arg.h"
#include "halo.h"

namespace quda {

// ---- single-direction hop (setup-time helper for the multigrid coarse-operator construction) ----
template <typename T, int R>
__global__ void __launch_bounds__(256) hop_dir_kernel(const DslashArg<typename Store<T>::real> arg, int dir, typename Store<T>::real coef,
                                                      const void *ghost, int ghostFaceCB, int plain) {
  using real = typename Store<T>::real;
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= arg.Vh) return;
  const uint32_t za = arg.dXh.div((uint32_t)idx);
  const int xh = idx - (int)za * arg.Xh;
  const uint32_t zb = arg.dY.div(za);
  const int y = (int)za - (int)zb * arg.Y;
  const int t = (int)arg.dZ.div(zb);
  const int z = (int)zb - t * arg.Z;
  const int xodd = (y + z + t + arg.parity) & 1;
  const int Xh = arg.Xh, sy = Xh, sz = Xh * arg.Y, st = Xh * arg.Y * arg.Z;
  int nbr;
  real sign = 1;
  switch (dir) {
    case 0: nbr = xodd ? (xh == Xh - 1 ? idx - (Xh - 1) : idx + 1) : idx; break;
    case 1: nbr = xodd ? idx : (xh == 0 ? idx + (Xh - 1) : idx - 1); break;
    case 2: nbr = y == arg.Y - 1 ? idx - (arg.Y - 1) * sy : idx + sy; break;
    case 3: nbr = y == 0 ? idx + (arg.Y - 1) * sy : idx - sy; break;
    case 4: nbr = z == arg.Z - 1 ? idx - (arg.Z - 1) * sz : idx + sz; break;
    case 5: nbr = z == 0 ? idx + (arg.Z - 1) * sz : idx - sz; break;
    case 6: nbr = t == arg.T - 1 ? idx - (arg.T - 1) * st : idx + st; if (t == arg.T - 1) sign = arg.tsign_fwd; break;
    default: nbr = t == 0 ? idx + (arg.T - 1) * st : idx - st; if (t == 0) sign = arg.tsign_bwd; break;
  }
  real acc[24], psi[24], U[18];
#pragma unroll
  for (int k = 0; k < 24; k++) acc[k] = 0;
  // grid-decomposed direction: the neighbour of a face site lives on the adjacent rank; its full spinor was exchanged into
  // `ghost` (face index = lexicographic index of the other three coordinates, halved — same convention as pack_kernel)
  bool cross = false;
  int f = 0;
  if (ghost) {
    const int xf = 2 * xh + xodd, X0 = 2 * Xh;
    switch (dir >> 1) {
      case 0: cross = (dir & 1) ? xf == 0 : xf == X0 - 1; f = (y + arg.Y * (z + arg.Z * t)) >> 1; break;
      case 1: cross = (dir & 1) ? y == 0 : y == arg.Y - 1; f = (xf + X0 * (z + arg.Z * t)) >> 1; break;
      case 2: cross = (dir & 1) ? z == 0 : z == arg.Z - 1; f = (xf + X0 * (y + arg.Y * t)) >> 1; break;
      default: cross = (dir & 1) ? t == 0 : t == arg.T - 1; f = (xf + X0 * (y + arg.Y * z)) >> 1; break;
    }
  }
  if (cross) Planar<T, 24>::load(psi, ghost, ghostFaceCB, f, nullptr, f);
  else Planar<T, 24>::load(psi, arg.in, arg.sp_stride, nbr, arg.inNorm, nbr);
  Link<T, R>::load(U, arg.gauge + (size_t)dir * arg.link_bytes, arg.g_stride, idx, sign);
  if (plain) {
    // covariant shift without spin projection: acc = U psi on all four spins (the links of the backward directions are
    // stored daggered, so this is U_mu(x - mu)^dagger psi(x - mu) there)
#pragma unroll
    for (int sp = 0; sp < 4; sp++) su3_mv(acc + 6 * sp, U, psi + 6 * sp);
  } else
  switch (dir) {
    case 0: hop_arith<0, false, 0>(acc, psi, U, arg); break;
    case 1: hop_arith<1, false, 0>(acc, psi, U, arg); break;
    case 2: hop_arith<2, false, 0>(acc, psi, U, arg); break;
    case 3: hop_arith<3, false, 0>(acc, psi, U, arg); break;
    case 4: hop_arith<4, false, 0>(acc, psi, U, arg); break;
    case 5: hop_arith<5, false, 0>(acc, psi, U, arg); break;
    case 6: hop_arith<6, false, 0>(acc, psi, U, arg); break;
    default: hop_arith<7, false, 0>(acc, psi, U, arg); break;
  }
  if (arg.xpay) {   // out = k x + coef hop (x may be the output field itself: every thread reads its site before it writes it)
    real xs[24];
    Planar<T, 24>::load(xs, arg.x, arg.sp_stride, idx, arg.xNorm, idx);
#pragma unroll
    for (int k = 0; k < 24; k++) acc[k] = arg.k * xs[k] + coef * acc[k];
  } else {
#pragma unroll
    for (int k = 0; k < 24; k++) acc[k] *= coef;
  }
  Planar<T, 24>::store(acc, arg.out, arg.sp_stride, idx, arg.outNorm, idx);
}

// full (unprojected) spinors of the face x_d = face_coord of the parity_in checkerboard -> planar block of stride faceCB
template <typename T>
__global__ void __launch_bounds__(256) face_full_pack_kernel(void *dst, const void *in, const float *inNorm, int sp_stride, int X0, int X1, int X2, int X3,
                                                             int d, int face_coord, int parity_in, int faceCB) {
  using real = typename Store<T>::real;
  const int f = blockIdx.x * blockDim.x + threadIdx.x;
  if (f >= faceCB) return;
  const int X[4] = {X0, X1, X2, X3};
  int c[4], L[3], o[3], n = 0;
  for (int k = 0; k < 4; k++) if (k != d) { L[n] = X[k]; o[n] = k; n++; }
  int l = 2 * f;
  const int c0 = l % L[0]; l /= L[0];
  const int c1 = l % L[1]; const int c2 = l / L[1];
  c[d] = face_coord;
  c[o[0]] = c0; c[o[1]] = c1; c[o[2]] = c2;
  c[o[0]] += (parity_in + c[0] + c[1] + c[2] + c[3]) & 1;
  const int idx = (((c[3] * X[2] + c[2]) * X[1] + c[1]) * X[0] + c[0]) >> 1;
  real psi[24];
  Planar<T, 24>::load(psi, in, sp_stride, idx, inNorm, idx);
  Planar<T, 24>::store(psi, dst, faceCB, f, nullptr, f);
}

static char *g_ffSend = nullptr, *g_ffGhost = nullptr;
static size_t g_ffBytes = 0;
void freeFullFaceBuffers() {
  if (g_ffSend) (void)hipFree(g_ffSend);
  if (g_ffGhost) (void)hipFree(g_ffGhost);
  g_ffSend = g_ffGhost = nullptr; g_ffBytes = 0;
}

// The face a hop in direction `dir` to the sites of parity `parity` reads, fetched from the neighbour rank: a forward hop needs the
// x_mu = 0 face of the +mu neighbour (it sends it backward), a backward hop the x_mu = L-1 face of the -mu neighbour.  Full spinors
// of storage type T; setup-time path, so one blocking exchange on the compute stream.  Returns the ghost zone.
template <typename T> static const void *fetchFullFace(const void *in, const float *inNorm, int stride, const LatticeGeom &g, int parity, int dir) {
  const int mu = dir >> 1;
  const size_t bytes = (size_t)g.faceCB[mu] * 24 * sizeof(typename Store<T>::real);
  if (bytes > g_ffBytes) {
    freeFullFaceBuffers();
    HIP_CHECK(qaMalloc((void **)&g_ffSend, bytes));
    HIP_CHECK(qaMalloc((void **)&g_ffGhost, bytes));
    g_ffBytes = bytes;
  }
  const bool fwd = !(dir & 1);
  hipLaunchKernelGGL((face_full_pack_kernel<T>), dim3((g.faceCB[mu] + 255) / 256), dim3(256), 0, computeStream(), (void *)g_ffSend, in, inNorm, stride, g.X[0], g.X[1], g.X[2], g.X[3],
                     mu, fwd ? 0 : g.X[mu] - 1, 1 - parity, g.faceCB[mu]);
  HIP_CHECK(hipGetLastError());
  std::vector<HaloMsg> msgs;
  msgs.push_back({mu, fwd ? -1 : +1, g_ffSend, g_ffGhost, bytes});
  commExchange(msgs, computeStream());
  return g_ffGhost;
}

template <typename T, int R> static void launchHopDir(ColorSpinorField &out, const ColorSpinorField &in, const GaugeField &U, int parity, int dir, double coef,
                                                      bool plain = false, const ColorSpinorField *x = nullptr, double xcoef = 0) {
  using real = typename Store<T>::real;
  DslashArg<real> arg{};
  const LatticeGeom &g = U.geom;
  fillDslashFields(arg, &out, &in, U, parity);
  arg.sfwd = 1;
  if (x) { arg.x = x->V(); arg.xNorm = (const float *)x->Norm(); arg.xpay = 1; arg.k = (real)xcoef; }
  const int mu = dir >> 1;
  const void *ghost = commGrid().partitioned(mu) ? fetchFullFace<T>(in.V(), (const float *)in.Norm(), in.Stride(), g, parity, dir) : nullptr;
  hipLaunchKernelGGL((hop_dir_kernel<T, R>), dim3((g.Vh + 255) / 256), dim3(256), 0, computeStream(), arg, dir, (real)coef, ghost, g.faceCB[mu], plain ? 1 : 0);
  HIP_CHECK(hipGetLastError());
}

// out(parity) = xcoef x + coef U_dir psi(x + dhat(dir)) with NO spin projection (x may be nullptr or alias out); ghost-aware
void applyCovariantShift(ColorSpinorField &out, const ColorSpinorField &in, const GaugeField &U, int parity, int dir, double coef,
                         const ColorSpinorField *x, double xcoef) {
  if (in.Precision() != out.Precision() || in.Precision() != U.precision) errorQuda("precision mismatch");
  if (in.VolumeCB() != U.geom.Vh || out.VolumeCB() != U.geom.Vh) errorQuda("volume mismatch");
  if (x && (x->Precision() != out.Precision() || x->Stride() != out.Stride())) errorQuda("accumulation field does not match the output");
  if (in.Stride() != out.Stride()) errorQuda("stride mismatch");
  const int rr = (int)U.reconstruct;
  switch (in.Precision()) {
    case QUDA_DOUBLE_PRECISION: rr == 12 ? launchHopDir<double, 12>(out, in, U, parity, dir, coef, true, x, xcoef) : (rr == 8 ? launchHopDir<double, 8>(out, in, U, parity, dir, coef, true, x, xcoef) : launchHopDir<double, 18>(out, in, U, parity, dir, coef, true, x, xcoef)); break;
    case QUDA_SINGLE_PRECISION: rr == 12 ? launchHopDir<float, 12>(out, in, U, parity, dir, coef, true, x, xcoef) : (rr == 8 ? launchHopDir<float, 8>(out, in, U, parity, dir, coef, true, x, xcoef) : launchHopDir<float, 18>(out, in, U, parity, dir, coef, true, x, xcoef)); break;
    default: errorQuda("covariant shift: fp64/fp32 only");
  }
}

// ---- direct Galerkin construction, step 1 ("UV", reference ComputeUV lib/coarse_op.cuh:59-125): UV(x)[s, c; v] = coef U_mu(x) V(x + mu)[s, c; v]
// for ALL columns v of the transfer matrix at once — the link is read once per site instead of once per probe.  No spin projector here:
// (1 -+ gamma_mu) only permutes the spin rows of UV and multiplies them by +-1 / +-i, which galerkin_vuv_kernel does while it builds
// its operands (spin_partner_phase below) — half the bytes of a projected, chirality-split product.  V, UV in the aggregate-major order of
// the transfer operator, [aggregate][spin-colour][vector pair][site in aggregate] float4.  One work-group per aggregate, one thread per
// site of it (stores of a wave are 1 KiB contiguous), loop over the vector pairs.
__global__ void __launch_bounds__(256) galerkin_uv_kernel(const DslashArg<float> arg, const char *gaugeEven, const char *gaugeOdd, int dir, float coef, const float4 *V, float4 *UV,
                                                          const int *block_to_fine, const int *fine_to_block, int nvp, int aggOffset, int classMajor, int recon, float tsignFwd) {
  constexpr int BV = 256;
  const int A = blockIdx.x + aggOffset, Aloc = blockIdx.x, b = threadIdx.x;   // UV holds the aggregates [aggOffset, aggOffset + gridDim) only
  const int f = block_to_fine[(size_t)A * BV + b];
  const int parity = f >= arg.Vh, idx = f - parity * arg.Vh;
  const uint32_t za = arg.dXh.div((uint32_t)idx);
  const int xh = idx - (int)za * arg.Xh;
  const uint32_t zb = arg.dY.div(za);
  const int y = (int)za - (int)zb * arg.Y;
  const int tt = (int)arg.dZ.div(zb);
  const int z = (int)zb - tt * arg.Z;
  const int xodd = (y + z + tt + parity) & 1;
  const int Xh = arg.Xh, sy = Xh, sz = Xh * arg.Y, st = Xh * arg.Y * arg.Z;
  int nbr;
  switch (dir) {
    case 0: nbr = xodd ? (xh == Xh - 1 ? idx - (Xh - 1) : idx + 1) : idx; break;
    case 1: nbr = xodd ? idx : (xh == 0 ? idx + (Xh - 1) : idx - 1); break;
    case 2: nbr = y == arg.Y - 1 ? idx - (arg.Y - 1) * sy : idx + sy; break;
    case 3: nbr = y == 0 ? idx + (arg.Y - 1) * sy : idx - sy; break;
    case 4: nbr = z == arg.Z - 1 ? idx - (arg.Z - 1) * sz : idx + sz; break;
    case 5: nbr = z == 0 ? idx + (arg.Z - 1) * sz : idx - sz; break;
    case 6: nbr = tt == arg.T - 1 ? idx - (arg.T - 1) * st : idx + st; break;
    default: nbr = tt == 0 ? idx + (arg.T - 1) * st : idx - st; break;
  }
  const int posN = fine_to_block[(1 - parity) * arg.Vh + nbr];
  const int AN = posN / BV, bN = posN - AN * BV;
  // where this site's UV goes inside a (spin-colour, vector pair) row: classMajor — by its block coordinate along mu first (the class of sites one
  // wave of galerkin_vuv_kernel owns), then the other three coordinates: that wave then reads 64 consecutive entries of every row instead of
  // 16-byte pieces scattered over the whole row
  int bOut = b;
  if (classMajor) {
    const int c4[4] = {(2 * xh + xodd) & 3, y & 3, z & 3, tt & 3};
    const int mu = dir >> 1;
    int pos = 0, sh = 0;
#pragma unroll
    for (int d = 0; d < 4; d++) if (d != mu) { pos |= c4[d] << sh; sh += 2; }
    bOut = c4[mu] * 64 + pos;
  }
  float U[18];
  if (recon == 12) Link<float, 12>::load(U, (parity ? gaugeOdd : gaugeEven) + (size_t)dir * arg.link_bytes, arg.g_stride, idx, (dir == 6 && tt == arg.T - 1) ? tsignFwd : 1.f);
  else Link<float, 18>::load(U, (parity ? gaugeOdd : gaugeEven) + (size_t)dir * arg.link_bytes, arg.g_stride, idx, 1.f);
#pragma unroll
  for (int k = 0; k < 18; k++) U[k] *= coef;
  for (int vp = 0; vp < nvp; vp++) {
    float psi[2][24];
#pragma unroll
    for (int k = 0; k < 12; k++) {
      const float4 v = V[(((size_t)AN * 12 + k) * nvp + vp) * BV + bN];
      psi[0][2 * k] = v.x; psi[0][2 * k + 1] = v.y; psi[1][2 * k] = v.z; psi[1][2 * k + 1] = v.w;
    }
    float out[2][24];
#pragma unroll
    for (int vec = 0; vec < 2; vec++)
#pragma unroll
      for (int sp = 0; sp < 4; sp++) su3_mv(out[vec] + 6 * sp, U, psi[vec] + 6 * sp);
#pragma unroll
    for (int k = 0; k < 12; k++) UV[(((size_t)Aloc * 12 + k) * nvp + vp) * BV + bOut] = make_float4(out[0][2 * k], out[0][2 * k + 1], out[1][2 * k], out[1][2 * k + 1]);
  }
}
// fp32 recon-18 links (boundary condition inside the stored links), 4^4 aggregates, unpartitioned lattice (the neighbour's V would live on another rank)
void galerkinUV(float *UVout, const float *V, const GaugeField &U, int dir, double coef, const int *block_to_fine, const int *fine_to_block, int aggOffset, int nAgg, int blockVol, int nvec, bool classMajor) {
  if (U.precision != QUDA_SINGLE_PRECISION || (U.reconstruct != QUDA_RECONSTRUCT_NO && U.reconstruct != QUDA_RECONSTRUCT_12)) errorQuda("direct Galerkin construction: fp32 links (18 or 12 reals)");
  if (dir & 1) errorQuda("direct Galerkin construction: forward directions only");
  if (blockVol != 256) errorQuda("direct Galerkin construction: 4^4 aggregates");
  const LatticeGeom &g = U.geom;
  DslashArg<float> arg{};
  fillDslashFields<float>(arg, nullptr, nullptr, U, 0);   // geometry and link layout; the kernel takes both parities' link bases itself
  hipLaunchKernelGGL(galerkin_uv_kernel, dim3(nAgg), dim3(256), 0, computeStream(), arg, (const char *)U.parityBase(0), (const char *)U.parityBase(1), dir, (float)coef, (const float4 *)V,
                     (float4 *)UVout, block_to_fine, fine_to_block, nvec / 2, aggOffset, classMajor ? 1 : 0, (int)U.reconstruct,
                     arg.tsign_fwd);
  HIP_CHECK(hipGetLastError());
}

// the same for the site-diagonal term of the twisted-clover operator: L(x)[s, c; v] = (A_chi(s)(x) + i a s_chi) V(x)[s, c; v] — chirality-diagonal, so
// galerkin_vuv_kernel runs it in its "local" mode (no cross-chirality columns, every site belongs to the local matrix)
__global__ void __launch_bounds__(256) galerkin_local_uv_kernel(const float4 *V, float4 *L, const void *clEven, const void *clOdd, int cl_stride, int Vh, float a,
                                                                const int *block_to_fine, int nvp, int aggOffset) {
  constexpr int BV = 256;
  const int A = blockIdx.x + aggOffset, Aloc = blockIdx.x, b = threadIdx.x;
  const int f = block_to_fine[(size_t)A * BV + b];
  const int parity = f >= Vh, idx = f - parity * Vh;
  const void *clA = parity ? clOdd : clEven;
  float C[2][36];
#pragma unroll
  for (int chi = 0; chi < 2; chi++) Planar<float, 36>::load(C[chi], (const char *)clA + (size_t)chi * 36 * sizeof(float) * cl_stride, cl_stride, idx, nullptr, 0);
  for (int vp = 0; vp < nvp; vp++) {
    float psi[2][24], o[2][24];
#pragma unroll
    for (int k = 0; k < 12; k++) {
      const float4 v = V[(((size_t)A * 12 + k) * nvp + vp) * BV + b];
      psi[0][2 * k] = v.x; psi[0][2 * k + 1] = v.y; psi[1][2 * k] = v.z; psi[1][2 * k + 1] = v.w;
    }
#pragma unroll
    for (int vec = 0; vec < 2; vec++)
#pragma unroll
      for (int chi = 0; chi < 2; chi++) {
        const float *v = psi[vec] + 12 * chi;
        float *r = o[vec] + 12 * chi;
        clover_block_mv(r, C[chi], v);
        const float sa = chi ? -a : a;
#pragma unroll
        for (int k = 0; k < 6; k++) { r[2 * k] -= sa * v[2 * k + 1]; r[2 * k + 1] += sa * v[2 * k]; }
      }
#pragma unroll
    for (int k = 0; k < 12; k++) L[(((size_t)Aloc * 12 + k) * nvp + vp) * BV + b] = make_float4(o[0][2 * k], o[0][2 * k + 1], o[1][2 * k], o[1][2 * k + 1]);
  }
}
void galerkinLocalUV(float *Lout, const float *V, const CloverField &C, double a, const int *block_to_fine, int aggOffset, int nAgg, int blockVol, int nvec) {
  if (C.precision != QUDA_SINGLE_PRECISION) errorQuda("direct Galerkin construction: fp32 clover field");
  if (blockVol != 256) errorQuda("direct Galerkin construction: 4^4 aggregates");
  hipLaunchKernelGGL(galerkin_local_uv_kernel, dim3(nAgg), dim3(256), 0, computeStream(), (const float4 *)V, (float4 *)Lout, C.A(0), C.A(1), C.stride, C.geom.Vh, (float)a, block_to_fine, nvec / 2, aggOffset);
  HIP_CHECK(hipGetLastError());
}

void applyHopDir(ColorSpinorField &out, const ColorSpinorField &in, const GaugeField &U, int parity, int dir, double coef) {
  if (in.Precision() != out.Precision() || in.Precision() != U.precision) errorQuda("precision mismatch");
  if (in.VolumeCB() != U.geom.Vh) errorQuda("volume mismatch");
  const int rr = (int)U.reconstruct;
  switch (in.Precision()) {
    case QUDA_DOUBLE_PRECISION: rr == 12 ? launchHopDir<double, 12>(out, in, U, parity, dir, coef) : (rr == 8 ? launchHopDir<double, 8>(out, in, U, parity, dir, coef) : launchHopDir<double, 18>(out, in, U, parity, dir, coef)); break;
    case QUDA_SINGLE_PRECISION: rr == 12 ? launchHopDir<float, 12>(out, in, U, parity, dir, coef) : (rr == 8 ? launchHopDir<float, 8>(out, in, U, parity, dir, coef) : launchHopDir<float, 18>(out, in, U, parity, dir, coef)); break;
    default: errorQuda("single-direction hop: fp64/fp32 only");
  }
}

// ---- neighbour shift of a 24-real fp64 planar site field: out(x) = in(x + dhat(dir)), ghost-aware like the single-direction
// hop (full faces exchanged through commExchange).  Used by the grid-decomposed clover construction, which moves 3x3 matrix
// fields (18 of the 24 reals) between neighbouring sites; setup-time only. ----
__global__ void __launch_bounds__(256) shift_kernel(double *out, const double *in, int stride, int Vh, int Xh, int Y, int Z, int T, int parity, int dir,
                                                    const void *ghost, int ghostFaceCB) {
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= Vh) return;
  int l = idx;
  const int xh = l % Xh; l /= Xh;
  const int y = l % Y; l /= Y;
  const int z = l % Z, t = l / Z;
  const int xodd = (y + z + t + parity) & 1, xf = 2 * xh + xodd, X0 = 2 * Xh;
  const int sy = Xh, sz = Xh * Y, st = Xh * Y * Z;
  int nbr, f;
  bool cross;
  switch (dir) {
    case 0: nbr = xodd ? (xh == Xh - 1 ? idx - (Xh - 1) : idx + 1) : idx; cross = xf == X0 - 1; f = (y + Y * (z + Z * t)) >> 1; break;
    case 1: nbr = xodd ? idx : (xh == 0 ? idx + (Xh - 1) : idx - 1); cross = xf == 0; f = (y + Y * (z + Z * t)) >> 1; break;
    case 2: nbr = y == Y - 1 ? idx - (Y - 1) * sy : idx + sy; cross = y == Y - 1; f = (xf + X0 * (z + Z * t)) >> 1; break;
    case 3: nbr = y == 0 ? idx + (Y - 1) * sy : idx - sy; cross = y == 0; f = (xf + X0 * (z + Z * t)) >> 1; break;
    case 4: nbr = z == Z - 1 ? idx - (Z - 1) * sz : idx + sz; cross = z == Z - 1; f = (xf + X0 * (y + Y * t)) >> 1; break;
    case 5: nbr = z == 0 ? idx + (Z - 1) * sz : idx - sz; cross = z == 0; f = (xf + X0 * (y + Y * t)) >> 1; break;
    case 6: nbr = t == T - 1 ? idx - (T - 1) * st : idx + st; cross = t == T - 1; f = (xf + X0 * (y + Y * z)) >> 1; break;
    default: nbr = t == 0 ? idx + (T - 1) * st : idx - st; cross = t == 0; f = (xf + X0 * (y + Y * z)) >> 1; break;
  }
  double v[24];
  if (ghost && cross) Planar<double, 24>::load(v, ghost, ghostFaceCB, f, nullptr, f);
  else Planar<double, 24>::load(v, in, stride, nbr, nullptr, nbr);
  Planar<double, 24>::store(v, out, stride, idx, nullptr, idx);
}

// out: parity `parity` block, in: the other parity's block (both [12 double2 planes][stride])
void applyShift(double *out, const double *in, const LatticeGeom &g, int stride, int parity, int dir) {
  const int mu = dir >> 1;
  const void *ghost = commGrid().partitioned(mu) ? fetchFullFace<double>(in, nullptr, stride, g, parity, dir) : nullptr;
  hipLaunchKernelGGL(shift_kernel, dim3((g.Vh + 255) / 256), dim3(256), 0, computeStream(), out, in, stride, g.Vh, g.Xh, g.X[1], g.X[2], g.X[3], parity, dir, ghost,
                     g.faceCB[mu]);
  HIP_CHECK(hipGetLastError());
}

// the ghost zone a hop in direction `dir` to the sites of parity `parity` reads, copied into a buffer of the caller (faceCB[mu] x 24
// doubles, planar with stride faceCB[mu], face index as in hop_dir_kernel): `in` is the other parity's block of a 24-real fp64 planar
// field.  For kernels that need several ghost zones at once (the fused loop contraction, loop.hip).
void exchangeFullFace(void *ghostOut, const double *in, const LatticeGeom &g, int stride, int parity, int dir) {
  const int mu = dir >> 1;
  if (!commGrid().partitioned(mu)) errorQuda("exchangeFullFace: dimension %d is not partitioned", mu);
  const void *ghost = fetchFullFace<double>(in, nullptr, stride, g, parity, dir);
  HIP_CHECK(hipMemcpyAsync(ghostOut, ghost, (size_t)g.faceCB[mu] * 24 * sizeof(double), hipMemcpyDeviceToDevice, computeStream()));
}

}  // namespace quda
