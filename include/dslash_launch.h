// dslash_launch.h — launch policy of the fine-grid stencil (csrc/dslash_launch.cpp): everything launchDslash decides that does not
// depend on the storage type, the link reconstruction or the kernel variant, as plain host functions.  Internal, like halo.h.
#pragma once

#include <functional>

#include "dslash.h"
#include "halo.h"
#include "tune.h"

namespace quda {

int partitionMask();   // bit d set: dimension d is grid-decomposed

// ---- block size and block order ----
// sites per block: the largest of 256 / 192 / 128 / 64 threads that cuts an (x, y) plane into whole blocks (needed by the plane-tiled
// order), 256 otherwise; `block` (threads, DslashTune::block) overrides.  flavours = 2 (fused doublet stencil): a block of n threads
// holds n / 2 sites — 128 / 96 / 64 / 32 sites
int dslashBlockSites(const LatticeGeom &g, int block, int flavours);

// how the 8 XCDs split the (z, t) lattice: nxz ways along z, 8 / nxz along t, slabs of Zs x Ts planes.  nxz = 0: no even split
struct XcdSplit { int nxz, Zs, Ts; };
XcdSplit xcdPlaneSplit(const LatticeGeom &g, int wantNxz = 0);   // wantNxz > 0: that split or none

// physical block b -> logical block (a run of consecutive checkerboard sites); read by dslash_logical_block (dslash.hip)
struct DslashOrder {
  int nblocks, xcd_q, xcd_r;  // XCD-aware remap: every XCD a contiguous range of logical blocks (xcd_q < 0: off)
  int ts, bps;                // time-slab interleave: ts slices per slab, bps blocks per time slice (ts = 0: off)
  // plane-tiled block order (tiled != 0): a block is chunk yc of the P chunks of one (z, t) plane; the 8 XCDs split the (z, t)
  // lattice nxz x (8 / nxz) ways and each walks its region tile by tile (tz x tt planes per tile, t fastest inside a tile)
  int tiled, P, nxz, Zs, Ts, tz, tt;
  FastDiv dNxz, dPerTile, dNtz, dTzTt, dTt, dPTt;
};
// bs: sites per block; elemBytes: storage bytes of one real of the spinor (the automatic y groups look at the working set)
DslashOrder dslashBlockOrder(const LatticeGeom &g, const DslashTune &tune, int bs, int elemBytes);

// ---- cache policy of one launch ----
struct DslashCachePolicy { bool ntStore, ntLinks; };
// sites: sites written by the launch; linkKnob: the kernel has a run-time link policy (16-bit storage); workingBytes: one application's working set
DslashCachePolicy dslashCachePolicy(const DslashTune &tune, long sites, bool linkKnob, size_t workingBytes);

// ---- launch-parameter cache and sweep (tune.h) ----
using DslashApply = std::function<void(const DslashTune *candidate)>;   // the caller's own application with a candidate's knobs
enum HaloTransport { HALO_AUTO, HALO_STAGED, HALO_PEER_STORE };
// The knobs of one launch: the user's (dslashTune), then — where left automatic — a sweep candidate's or the cached winner's for this
// (lattice, kernel, precision, reconstruct, epilogue, partition mask).  With tuning enabled the first launch of a key runs the sweep
// through `apply`; a partitioned launch that picks its own transport (HALO_AUTO) waits with that until the transport is verified.
DslashTune effectiveDslashTune(const LatticeGeom &g, QudaPrecision prec, int recon, int variant, const DslashParam &p, int pmask, const DslashTune *candidate,
                               HaloTransport transport, const DslashApply &apply);

// ---- faces of a partitioned launch ----
struct FacePlan {
  int start[9];   // prefix offsets of the 8 (dim, dir) thread ranges of the pack kernel; start[8] = all face sites
  bool on[4];     // dimension d is partitioned
};
FacePlan dslashFacePlan(const LatticeGeom &g, int mask);

// the next exchange of the peer-store transport: its number, its buffer and the flag its words carry per partitioned dimension
struct PeerExchange { unsigned seq; int buf; unsigned flag[4]; };
PeerExchange nextPeerExchange(HaloBuffers &hb, int mask);
// First use of the peer-store transport for a precision: the same application through the staged transport and through peer stores must agree
// (relative tolerance tol) on every rank, otherwise all ranks drop back to the staged transport for good; `out` holds the result either way.
void verifyPeerStoreHalo(HaloBuffers &hb, ColorSpinorField &out, double tol, const std::function<void(HaloTransport)> &applyThrough);

// QUDA_AMD_TIMELINE=1: the mapped stamp buffer of the peer-store kernel (16384 words, else nullptr), and the report over it
unsigned long long *dslashTimelineBuffer();
void dslashTimelineReport(const unsigned long long *tl, int packBlocks, int nb);

// 16-byte vectors per face site of the flag-in-data wire format (dslash.hip GhostLL<T>::NV)
constexpr int ghostLLVectors(int precBytes) { return precBytes == 8 ? 12 : (precBytes == 4 ? 6 : 4); }

}  // namespace quda
