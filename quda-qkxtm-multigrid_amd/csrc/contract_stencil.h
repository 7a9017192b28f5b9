// contract_stencil.h — the front half that the contractions (contract.hip, loop.hip, threep.hip) share: the neighbour arithmetic of a
// covariant hop, the site load from the interior or a ghost zone, the colour-summed building block, the geometry and link part of a
// stencil kernel's argument with the host code that fills it, the ghost zones' owner, the dispatch on the link reconstruction, and the
// small device helpers of the propagator contractions.  The shared tail (MomAccum, stageAndProject) is momproj.hip.
#pragma once

#include <vector>

#include "comm_quda.h"
#include "device_io.h"
#include "dslash.h"
#include "qa_core.h"

namespace quda {

// ---- propagator contractions (contract.hip, threep.hip) ----
__device__ __forceinline__ double2 cmul(double2 a, double2 b) { return make_double2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x); }

// the six permutations of three colours, the even ones first, and their signs
static __constant__ int c_eps[6][3] = {{0, 1, 2}, {1, 2, 0}, {2, 0, 1}, {0, 2, 1}, {2, 1, 0}, {1, 0, 2}};
static __constant__ double c_eps_sign[6] = {1, 1, 1, -1, -1, -1};

// P[(s * 4 + t) * 9 + c * 3 + d][site]: sink spin / colour s, c, source spin / colour t, d, V sites
__device__ __forceinline__ long prop_index(int s, int t, int c, int d, long V, long site) { return (((s * 4 + t) * 9 + c * 3 + d)) * V + site; }

// ---- the geometry and link part of a stencil kernel's argument ----
struct StencilGeom {
  int sp_stride;                 // of the 12 double2 planes of a spinor's parity block
  const char *gauge[2];          // parityBase of the links
  size_t link_bytes;
  int g_stride;
  int X0, Y, Z, T;               // local extents
  int t0;                        // first time slice of the chunk
  long S;                        // sites of the chunk
  double tsign_fwd, tsign_bwd;   // boundary sign where the links do not carry it
  // ghost zones of a partitioned direction mu: ghost + ghostOff[mu] + ((field * 2 + parity of the reading site) * 2 + fwd / bwd) * faceCB[mu] * 24
  const double *ghost;
  long ghostOff[4];              // -1: not partitioned
  int faceCB[4];
  double2 *cs;                   // [blocks][S][16]
};

// everything but the field pointers, the ghost zones, t0, S and cs; the one place for the boundary-sign rule among the contractions
inline void fillStencilGeom(StencilGeom &a, const GaugeField &U, const LatticeGeom &g, const CommGrid &cg) {
  a.gauge[0] = (const char *)U.parityBase(0); a.gauge[1] = (const char *)U.parityBase(1);
  a.link_bytes = U.link_bytes; a.g_stride = U.stride;
  a.X0 = g.X[0]; a.Y = g.X[1]; a.Z = g.X[2]; a.T = g.X[3];
  const bool anti = U.reconstruct != QUDA_RECONSTRUCT_NO && U.t_boundary == QUDA_ANTI_PERIODIC_T;
  a.tsign_fwd = (anti && cg.coords[3] == cg.dims[3] - 1) ? -1.0 : 1.0;
  a.tsign_bwd = (anti && cg.coords[3] == 0) ? -1.0 : 1.0;
  a.ghost = nullptr;
  for (int mu = 0; mu < 4; mu++) { a.faceCB[mu] = g.faceCB[mu]; a.ghostOff[mu] = -1; }
}

// the two parity blocks (even, odd) of one full 24-real fp64 planar field and their stride: a ColorSpinorField, or one flavour of a doublet
struct FullFieldView { const double *par[2]; int stride; };

// The ghost zones of n full fields in ONE buffer, exchanged for every (field, parity of the reading site, partitioned mu, fwd / bwd);
// fills ghost / ghostOff of the argument and frees the buffer when it goes out of scope.  Collective.
class GhostZones {
  double *buf = nullptr;

  void fill(StencilGeom &a, const std::vector<FullFieldView> &fields, const LatticeGeom &g, const CommGrid &cg) {
    const size_t n = fields.size();
    size_t doubles = 0;
    for (int mu = 0; mu < 4; mu++) {
      if (!cg.partitioned(mu)) continue;
      a.ghostOff[mu] = (long)doubles;
      doubles += n * 2 * 2 * g.faceCB[mu] * 24;
    }
    if (!doubles) return;
    HIP_CHECK(hipMalloc(&buf, doubles * sizeof(double)));
    a.ghost = buf;
    for (int mu = 0; mu < 4; mu++) {
      if (a.ghostOff[mu] < 0) continue;
      const size_t zone = (size_t)g.faceCB[mu] * 24;
      for (size_t f = 0; f < n; f++)
        for (int parity = 0; parity < 2; parity++)
          for (int d = 0; d < 2; d++)   // a site of `parity` reads the other parity's block
            exchangeFullFace(buf + a.ghostOff[mu] + ((f * 2 + parity) * 2 + d) * zone, fields[f].par[1 - parity], g, fields[f].stride, parity, 2 * mu + d);
    }
  }

public:
  GhostZones(StencilGeom &a, const std::vector<const ColorSpinorField *> &fields, const LatticeGeom &g, const CommGrid &cg) {
    std::vector<FullFieldView> views;
    for (const ColorSpinorField *f : fields) views.push_back({{(const double *)f->Even().V(), (const double *)f->Odd().V()}, f->Even().Stride()});
    fill(a, views, g, cg);
  }
  GhostZones(StencilGeom &a, const FullFieldView *fields, size_t n, const LatticeGeom &g, const CommGrid &cg) { fill(a, std::vector<FullFieldView>(fields, fields + n), g, cg); }
  ~GhostZones() { if (buf) (void)hipFree(buf); }
  GhostZones(const GhostZones &) = delete;
  GhostZones &operator=(const GhostZones &) = delete;
};

// kernel<18 | 12 | 8> by the reconstruction of the links
template <typename Arg> void launchByRecon(int recon, void (*k18)(Arg), void (*k12)(Arg), void (*k8)(Arg), dim3 grid, dim3 block, const Arg &arg) {
  hipLaunchKernelGGL(recon == 12 ? k12 : recon == 8 ? k8 : k18, grid, block, 0, computeStream(), arg);
  HIP_CHECK(hipGetLastError());
}

// ---- device side of a covariant hop ----
struct HopNeighbours {
  int idxF, idxB, face;     // checkerboard index of x + mu and x - mu, index on the face orthogonal to mu
  bool crossF, crossB;      // the hop leaves the local lattice
  double signF, signB;      // boundary sign of the link
};

__device__ __forceinline__ HopNeighbours hop_neighbours(int mu, int xc, int y, int z, int t, int X0, int Y, int Z, int T, double tsign_fwd, double tsign_bwd) {
  HopNeighbours h;
  int xf = xc, yf = y, zf = z, tf = t, xb = xc, yb = y, zb = z, tb = t;
  h.signF = 1.0; h.signB = 1.0;
  switch (mu) {
    case 0: h.crossF = xc == X0 - 1; h.crossB = xc == 0; xf = h.crossF ? 0 : xc + 1; xb = h.crossB ? X0 - 1 : xc - 1; h.face = (y + Y * (z + Z * t)) >> 1; break;
    case 1: h.crossF = y == Y - 1; h.crossB = y == 0; yf = h.crossF ? 0 : y + 1; yb = h.crossB ? Y - 1 : y - 1; h.face = (xc + X0 * (z + Z * t)) >> 1; break;
    case 2: h.crossF = z == Z - 1; h.crossB = z == 0; zf = h.crossF ? 0 : z + 1; zb = h.crossB ? Z - 1 : z - 1; h.face = (xc + X0 * (y + Y * t)) >> 1; break;
    default:
      h.crossF = t == T - 1; h.crossB = t == 0; tf = h.crossF ? 0 : t + 1; tb = h.crossB ? T - 1 : t - 1; h.face = (xc + X0 * (y + Y * z)) >> 1;
      if (h.crossF) h.signF = tsign_fwd;
      if (h.crossB) h.signB = tsign_bwd;
      break;
  }
  h.idxF = (((tf * Z + zf) * Y + yf) * X0 + xf) >> 1;
  h.idxB = (((tb * Z + zb) * Y + yb) * X0 + xb) >> 1;
  return h;
}

// the ghost zone that a site of the given parity reads field number `field` from in direction 2 mu + d, nullptr where mu is not partitioned
__device__ __forceinline__ const double *ghost_zone(const StencilGeom &a, int mu, int field, int parity, int d) {
  const long goff = a.ghostOff[mu];
  return goff >= 0 ? a.ghost + goff + (size_t)(((field * 2 + parity) * 2) + d) * ((size_t)a.faceCB[mu] * 24) : nullptr;
}

__device__ __forceinline__ void load_site(double *psi, const double *blk, int stride, int idx, const double *ghost, int faceCB, int face, bool cross) {
  if (ghost && cross) Planar<double, 24>::load(psi, ghost, faceCB, face, nullptr, face);
  else Planar<double, 24>::load(psi, blk, stride, idx, nullptr, idx);
}

// The building block C[u, v][4a + b] = sum_c conj(u[(a + 2) & 3, c]) v[b, c] (spinors as 24 reals) is 16 sums over the three colours of
// (re, im) += conj(p[c]) r[c], p and r one spin of each
__device__ __forceinline__ void colour_mac(double &re, double &im, const double *p, const double *r, int c) {
  re += p[2 * c] * r[2 * c] + p[2 * c + 1] * r[2 * c + 1];
  im += p[2 * c] * r[2 * c + 1] - p[2 * c + 1] * r[2 * c];
}
__device__ __forceinline__ void spin_dot(double &re, double &im, const double *p, const double *r) {
#pragma unroll
  for (int c = 0; c < 3; c++) colour_mac(re, im, p, r, c);
}

}  // namespace quda
