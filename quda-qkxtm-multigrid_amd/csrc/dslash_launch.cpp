// dslash_launch.cpp — launch policy of the fine-grid stencil: tuning knobs, ghost-zone storage and boundary lists, and what a launch of
// dslash_kernel / ndeg_dslash_kernel decides apart from its template parameters (dslash_launch.h).  Host code only; the kernels and the
// launcher that picks an instantiation are in dslash.hip.
#include "dslash_launch.h"

#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "blas.h"

namespace quda {

// ------------------------------------------------------------------------------------------------
// launch-geometry knobs of the stencil (defaults from the environment, once; qudaAmdSetDslashTune changes them at run time so one
// process can sweep them — tools/dslash_sweep.py)
DslashTune &dslashTune() {
  static DslashTune t;
  static bool init = false;
  if (!init) {
    init = true;
    auto env = [](const char *n, int d) { const char *e = getenv(n); return e ? atoi(e) : d; };
    t.block = env("QUDA_AMD_DSLASH_BLOCK", 0);
    t.remap = env("QUDA_AMD_XCD_REMAP", 1);
    t.order = env("QUDA_AMD_DSLASH_ORDER", 1);
    t.store_aux = env("QUDA_AMD_STORE_AUX", -1);
    t.link_aux = env("QUDA_AMD_LINK_AUX", -1);
    t.tiled = env("QUDA_AMD_DSLASH_TILED", -1);
    t.nxz = env("QUDA_AMD_DSLASH_NXZ", 0);
    t.tz = env("QUDA_AMD_DSLASH_TZ", 0);
    t.tt = env("QUDA_AMD_DSLASH_TT", 0);
    t.lds_pad = env("QUDA_AMD_DSLASH_LDS", 0);
    t.ygroups = env("QUDA_AMD_DSLASH_YGROUPS", -1);
    t.edge_first = env("QUDA_AMD_EDGE_FIRST", 1);
    t.ndeg_fused = env("QUDA_AMD_NDEG_FUSED", -1);
    { const char *e = getenv("QUDA_AMD_HALO_FORMAT"); t.halo_format = !e ? -1 : ((!strcmp(e, "atom") || !strcmp(e, "atom16") || !strcmp(e, "sector") || !strcmp(e, "1")) ? 1 : 0); }
  }
  return t;
}
// automatic (-1): the compact atoms between DEVICES — two thirds of flag-in-data's bytes on the wire (fp64 / fp32; three quarters for 16-bit): in a
// 1 x 2 x 2 x 2 grid the +mu and -mu neighbour are the same GPU, so both faces of a dimension share one xGMI link, 1.57 MB per link and application in
// fp64 against 1.05 MB, ~26 against ~17 us at 60 GB/s next to a 20 us interior kernel — and flag-in-data where no link is crossed (ranks sharing a device in
// a rehearsal, the self-neighbour emulation on one rank).  Both formats validate every single store by itself (8-byte halves resp. 16-byte atoms), neither
// relies on the order in which stores become visible.  The same on every rank by construction.
int haloWireFormat() {
  const int f = dslashTune().halo_format;
  if (f >= 0) return f ? 1 : 0;
  return (commGrid().size > 1 && !p2pDeviceShared()) ? 1 : 0;
}
// the fused doublet stencil has no halo path: a partitioned lattice takes the composed operators whatever was asked for
bool ndegFusedSelected() {
  for (int d = 0; d < 4; d++) if (commGrid().partitioned(d)) return false;
  return dslashTune().ndeg_fused != 0;
}
void setDslashTune(const char *key, int value) {
  DslashTune &t = dslashTune();
  const std::string k(key);
  if (k == "block") t.block = value;
  else if (k == "remap") t.remap = value;
  else if (k == "order") t.order = value;
  else if (k == "store_aux") t.store_aux = value;
  else if (k == "link_aux") t.link_aux = value;
  else if (k == "tiled") t.tiled = value;
  else if (k == "nxz") t.nxz = value;
  else if (k == "tz") t.tz = value;
  else if (k == "tt") t.tt = value;
  else if (k == "lds_pad") t.lds_pad = value;
  else if (k == "ygroups") t.ygroups = value;
  else if (k == "site_delay") t.site_delay = value;
  else if (k == "pack_prio") t.pack_prio = value;
  else if (k == "edge_first") t.edge_first = value;
  else if (k == "halo_format") t.halo_format = value;
  else if (k == "ndeg_fused") t.ndeg_fused = value;
  else errorQuda("unknown stencil tuning key '%s'", key);
}

// ---- ghost-zone storage and the boundary-site lists ----
static HaloBuffers g_halo[3];
static std::vector<BoundaryList> g_blists;

static void releaseHalo(HaloBuffers &h) {
  if (h.window) {
    // neighbours may still be storing into / polling this window: drain the device and meet them before unmapping
    HIP_CHECK(hipDeviceSynchronize());
    commBarrier();
    commUnmapPeers(h.map);
    commBarrier();
    p2pFree(h.window);
  }
  if (h.pool) HIP_CHECK(hipFree(h.pool));
  h = HaloBuffers();
}

HaloBuffers &haloBuffers(const LatticeGeom &g, QudaPrecision prec) {
  HaloBuffers &h = g_halo[prec == QUDA_DOUBLE_PRECISION ? 0 : (prec == QUDA_SINGLE_PRECISION ? 1 : 2)];
  bool same = h.precision == prec;
  for (int d = 0; d < 4; d++) same = same && h.faceCB[d] == g.faceCB[d];
  if (same && h.pool) return h;
  releaseHalo(h);
  h.precision = prec;
  size_t total = 0;
  for (int d = 0; d < 4; d++) {
    h.faceCB[d] = g.faceCB[d];
    const size_t payload = ((size_t)g.faceCB[d] * 12 * (int)prec + 255) / 256 * 256;
    h.norm_offset[d] = payload;
    h.face_bytes[d] = payload + (prec == QUDA_HALF_PRECISION ? ((size_t)g.faceCB[d] * sizeof(float) + 255) / 256 * 256 : 0);
    total += 4 * h.face_bytes[d];
  }
  HIP_CHECK(qaMalloc((void **)&h.pool, total));
  // hipMemset on the null stream may still be in flight when it returns and does not order against the non-blocking
  // compute/comm streams: a late memset would wipe a freshly packed send buffer, so zero on the compute stream and drain
  HIP_CHECK(hipMemsetAsync(h.pool, 0, total, computeStream()));
  HIP_CHECK(hipStreamSynchronize(computeStream()));
  h.pool_bytes = total;
  char *p = h.pool;
  for (int d = 0; d < 4; d++)
    for (int dir = 0; dir < 2; dir++) { h.send[d][dir] = p; p += h.face_bytes[d]; h.ghost[d][dir] = p; p += h.face_bytes[d]; }

  // ---- peer-store transport: same offsets on every rank (same local lattice), so a neighbour address = its base + my offset
  h.p2p = p2pHaloEnabled();
  if (h.p2p) {
    // window = double-buffered flag-in-data zones [dim][k][buf], each NV 16-byte vectors per face site (GhostLL); zero-filled,
    // and the flag of an exchange is never 0
    const int nv = ghostLLVectors((int)prec);
    size_t wtotal = 0;
    size_t zone[4];
    for (int d = 0; d < 4; d++) { zone[d] = ((size_t)g.faceCB[d] * nv * 16 + 255) / 256 * 256; wtotal += 4 * zone[d]; }
    h.window = (char *)p2pAlloc(wtotal + 256);
    if (!commMapPeers(h.window, h.map)) errorQuda("peer mapping of a halo window failed after the transport probe succeeded");
    HIP_CHECK(hipDeviceSynchronize());
    size_t off = 0;
    for (int d = 0; d < 4; d++)
      for (int k = 0; k < 2; k++) {
        // k = 0: zone filled by the -d neighbour (it sent forward), k = 1: by the +d neighbour (it sent backward)
        const int to_fwd = k == 0 ? 1 : 0;                 // the sender's direction that fills zone k
        const int slot = 2 * d + (to_fwd ? 1 : 0);         // MY neighbour in that direction receives my (d, to_fwd) face in ITS zone k
        for (int buf = 0; buf < 2; buf++) {
          h.ghostBuf[d][k][buf] = h.window + off;
          h.peerGhost[d][to_fwd][buf] = (char *)h.map.peer[slot] + off;
          off += zone[d];
        }
      }
    h.seq = 0;
    for (int d = 0; d < 4; d++) h.uses[d][0] = h.uses[d][1] = 0;
    commBarrier();
  }
  return h;
}
void freeFullFaceBuffers();   // hop.hip
void freeCoarseGhosts();  // coarse.hip
void freeHaloBuffers() {
  for (HaloBuffers &h : g_halo) releaseHalo(h);
  freeBoundaryLists();
  freeFullFaceBuffers();
  freeCoarseGhosts();
}

const BoundaryList &boundaryList(const LatticeGeom &g, int mask) {
  for (const BoundaryList &b : g_blists)
    if (b.mask == mask && b.X[0] == g.X[0] && b.X[1] == g.X[1] && b.X[2] == g.X[2] && b.X[3] == g.X[3]) return b;
  BoundaryList b;
  b.mask = mask;
  for (int d = 0; d < 4; d++) b.X[d] = g.X[d];
  for (int parity = 0; parity < 2; parity++) {
    std::vector<int> list;
    for (int i = 0; i < g.Vh; i++) {
      const int za = i / g.Xh, xh = i - za * g.Xh, zb = za / g.X[1], y = za - zb * g.X[1], t = zb / g.X[2], z = zb - t * g.X[2];
      const int c[4] = {2 * xh + ((y + z + t + parity) & 1), y, z, t};
      bool bd = false;
      for (int d = 0; d < 4; d++) bd = bd || (((mask >> d) & 1) && (c[d] == 0 || c[d] == g.X[d] - 1));
      if (bd) list.push_back(i);
    }
    b.count[parity] = (int)list.size();
    if (!list.empty()) {
      HIP_CHECK(qaMalloc((void **)&b.d_idx[parity], list.size() * sizeof(int)));
      HIP_CHECK(hipMemcpy(b.d_idx[parity], list.data(), list.size() * sizeof(int), hipMemcpyHostToDevice));
    }
  }
  g_blists.push_back(b);
  return g_blists.back();
}
void freeBoundaryLists() {
  for (BoundaryList &b : g_blists)
    for (int p = 0; p < 2; p++) if (b.d_idx[p]) (void)hipFree(b.d_idx[p]);
  g_blists.clear();
}

int partitionMask() {
  int mask = 0;
  for (int d = 0; d < 4; d++) if (commGrid().partitioned(d)) mask |= 1 << d;
  return mask;
}

// ---- block size and block order ----
int dslashBlockSites(const LatticeGeom &g, int block, int flavours) {
  const int plane = g.Xh * g.X[1], fl = flavours;
  int bs = block / fl;
  if (bs * fl < 64 || bs * fl > 256 || (bs * fl) % 64) {
    bs = 256 / fl;
    for (int c : {256, 192, 128, 64}) if (plane % (c / fl) == 0) { bs = c / fl; break; }
  }
  return bs;
}

XcdSplit xcdPlaneSplit(const LatticeGeom &g, int wantNxz) {
  for (int c : {8, 4, 2, 1})
    if ((wantNxz <= 0 || wantNxz == c) && g.X[2] % c == 0 && g.X[3] % (8 / c) == 0) return {c, g.X[2] / c, g.X[3] / (8 / c)};
  return {0, 0, 0};
}

DslashOrder dslashBlockOrder(const LatticeGeom &g, const DslashTune &tune, int bs, int elemBytes) {
  DslashOrder o{};
  const int plane = g.Xh * g.X[1], nb = (g.Vh + bs - 1) / bs;
  // XCD-aware remap: blocks b, b + 8, ... share an XCD; every XCD gets a contiguous range of logical blocks
  o.nblocks = nb; o.xcd_q = nb / 8; o.xcd_r = nb % 8;
  if (!tune.remap) o.xcd_q = -1;
  // legacy slab order: t fastest inside an XCD's slab of ts time slices
  const int slice = g.Vh / g.X[3];
  if (tune.order > 0 && slice % bs == 0 && g.X[3] % 8 == 0 && nb % 8 == 0) {
    o.bps = slice / bs;
    o.ts = tune.order == 1 ? g.X[3] / 8 : tune.order;   // order > 1: explicit slab thickness (must divide T/8)
    if ((g.X[3] / 8) % o.ts != 0) o.ts = g.X[3] / 8;
  }
  if (o.xcd_q < 0) o.ts = 0;
  // plane-tiled order (see DslashOrder): needs whole blocks per plane and an even split of the (z, t) lattice over the 8 XCDs
  // Default since round 2: the 8 XCDs split z (or z x t where z has too few planes), every XCD walks its slab one time slice
  // after the other (tt = 1), all of them in the same time slices at the same time: 48^3 x 96 fp32 0.59 -> 0.61 of the
  // roofline, 32^4 fp32 0.70 -> 0.73 (with nt stores 0.64 / 0.73); tiles in t, t-slabs per XCD and deeper z tiles are all slower.
  if (tune.tiled == 0 || !tune.remap || plane % bs != 0 || g.Vh % bs != 0) return o;
  const XcdSplit x = xcdPlaneSplit(g, tune.nxz);
  if (!x.nxz) return o;
  const int Zs = x.Zs, Ts = x.Ts;
  int tz = tune.tz > 0 ? tune.tz : Zs, tt = tune.tt > 0 ? tune.tt : 1;
  if (tz > Zs || Zs % tz) tz = Zs;
  if (tt > Ts || Ts % tt) tt = 1;
  o.tiled = tune.tiled == 1 ? 1 : 2; o.P = plane / bs; o.nxz = x.nxz; o.Zs = Zs; o.Ts = Ts; o.tz = tz; o.tt = tt;
  o.dNxz = FastDiv((uint32_t)x.nxz); o.dPerTile = FastDiv((uint32_t)(o.P * tz * tt)); o.dNtz = FastDiv((uint32_t)(Zs / tz));
  o.dTzTt = FastDiv((uint32_t)(tz * tt)); o.dTt = FastDiv((uint32_t)tt); o.dPTt = FastDiv((uint32_t)(o.P * tt));
  // y groups (tune.ygroups > 1; automatic: fp64 fields whose three-slice working set per XCD exceeds the 4 MB L2)
  int yg = tune.ygroups;
  if (yg == 0) yg = 1;
  if (yg < 0) {
    yg = 1;
    const size_t slice3 = (size_t)3 * Zs * plane * 24 * elemBytes;
    if (elemBytes == 8) while (yg < o.P && o.P % (2 * yg) == 0 && slice3 / yg > ((size_t)5 << 19)) yg *= 2;
  }
  if (yg > 1 && o.P % yg == 0 && tz == Zs && tt == 1) {
    const int Pg = o.P / yg;
    o.tiled = 3;
    o.dPerTile = FastDiv((uint32_t)(Ts * Zs * Pg)); o.dTzTt = FastDiv((uint32_t)(Zs * Pg)); o.dPTt = FastDiv((uint32_t)Pg); o.dNtz = FastDiv(1u);
  }
  return o;
}

// ---- cache policy ----
// Output stores: nt from 2^18 sites up (measured +1...+5 % at 32^4 and 48^3 x 96 in every precision and action, +10 % for 16-bit twisted
// clover; on the 65k-site sub-lattice of an 8-GPU split it costs fp32 5 %), QUDA_AMD_STORE_AUX / "store_aux" = 0 | 2 overrides.
// 16-bit links: default policy while one application's working set fits the Infinity Cache (32^4: 205 MB of 256 MiB — the links are
// re-read from it by the next application, nt costs 13 % there), nt beyond it (48^3 x 96, 2.1 GB: 405 -> 381 us, measured twice).  The
// 16-byte-per-lane formats have their link policy fixed at build time (dslash.hip QA_GAUX).
DslashCachePolicy dslashCachePolicy(const DslashTune &tune, long sites, bool linkKnob, size_t workingBytes) {
  DslashCachePolicy c;
  c.ntStore = tune.store_aux >= 0 ? tune.store_aux == 2 : sites >= (1 << 18);
  c.ntLinks = linkKnob && (tune.link_aux >= 0 ? tune.link_aux == 2 : workingBytes > ((size_t)256 << 20));
  return c;
}

// ---- launch-parameter sweep (tune.h) ----
static TuneKey dslashTuneKey(const LatticeGeom &g, int precBytes, int recon, int variant, const DslashParam &p, int pmask) {
  char vol[32], aux[256];
  snprintf(vol, sizeof(vol), "%dx%dx%dx%d", g.X[0], g.X[1], g.X[2], g.X[3]);
  snprintf(aux, sizeof(aux), "prec=%d,recon=%d,mode=%d,xpay=%d,dagger=%d,comm=%d%d%d%d", precBytes, recon, (int)p.mode, p.x ? 1 : 0, p.dagger ? 1 : 0, pmask & 1, (pmask >> 1) & 1, (pmask >> 2) & 1,
           (pmask >> 3) & 1);
  return TuneKey(vol, variant == 2 ? "dslash_kernel<clover>" : (variant == 1 ? "dslash_kernel<twist-first>" : "dslash_kernel"), aux);
}
// Times the candidate knob settings of one key INTERLEAVED (A B C ... three rounds, minimum per candidate: consecutive runs of one candidate
// share the device's placement / clock state, tools/policy_interleaved.sh) with device events on the compute stream and stores the fastest.
// Every launch is the caller's own application (its output is simply produced several times); on a grid-decomposed lattice every rank runs the
// same number of launches, so the exchanges pair up.
static void sweepDslash(const TuneKey &key, const LatticeGeom &g, int precBytes, int pmask, const DslashApply &apply) {
  std::vector<DslashTune> cand;
  const DslashTune &user = dslashTune();
  const bool half = precBytes == 2;
  for (int yg : {1, 2})
    for (int st : {0, 2})
      for (int lk : {0, 2})
        for (int ef : {1, 0}) {
          if (user.ygroups >= 0 && yg != (user.ygroups > 1 ? user.ygroups : 1)) continue;
          if (user.store_aux >= 0 && st != user.store_aux) continue;
          if ((!half || pmask) && lk != 0) continue;                          // the link policy is a knob of the 16-bit unpartitioned kernel only
          if (half && user.link_aux >= 0 && lk != user.link_aux) continue;
          if (pmask && (st != 0 || yg != 1)) continue;                       // partitioned launch: boundary-first or interior-first order
          if (!pmask && ef != 1) continue;
          DslashTune t;
          t.ygroups = yg; t.store_aux = st; t.link_aux = half && !pmask ? lk : -1; t.edge_first = pmask ? ef : -1;
          cand.push_back(t);
        }
  if (cand.empty()) return;
  const int reps = 10, rounds = 3;
  std::vector<float> best(cand.size(), 1e30f);
  hipEvent_t e0, e1;
  HIP_CHECK(hipEventCreate(&e0)); HIP_CHECK(hipEventCreate(&e1));
  hipStream_t cs = computeStream();
  for (int round = 0; round < rounds; round++)
    for (size_t c = 0; c < cand.size(); c++) {
      apply(&cand[c]);   // warm-up of this candidate
      HIP_CHECK(hipEventRecord(e0, cs));
      for (int i = 0; i < reps; i++) apply(&cand[c]);
      HIP_CHECK(hipEventRecord(e1, cs));
      HIP_CHECK(hipEventSynchronize(e1));
      float ms = 0;
      HIP_CHECK(hipEventElapsedTime(&ms, e0, e1));
      best[c] = std::min(best[c], ms / reps);
    }
  HIP_CHECK(hipEventDestroy(e0)); HIP_CHECK(hipEventDestroy(e1));
  size_t w = 0;
  for (size_t c = 1; c < cand.size(); c++) if (best[c] < best[w]) w = c;
  TuneParam tp;
  const int bs = dslashBlockSites(g, 0, 1);
  tp.block[0] = bs; tp.grid[0] = (g.Vh + bs - 1) / bs;
  tp.aux[0] = cand[w].ygroups; tp.aux[1] = cand[w].link_aux < 0 ? 0 : cand[w].link_aux; tp.aux[2] = cand[w].store_aux; tp.aux[3] = cand[w].edge_first < 0 ? 1 : cand[w].edge_first;
  tp.time = 1e-3f * best[w];
  char text[160];
  int n = snprintf(text, sizeof(text), "# %.2f us;", 1e3 * best[w]);
  for (size_t c = 0; c < cand.size() && n < (int)sizeof(text) - 24; c++) n += snprintf(text + n, sizeof(text) - n, " yg%d st%d lk%d ef%d=%.2f", cand[c].ygroups, cand[c].store_aux, cand[c].link_aux, cand[c].edge_first, 1e3 * best[c]);
  tp.comment = text;
  tuneStore(key, tp);
  tuneCountSweep();
  saveTuneCache();
  if (getVerbosity() >= QUDA_SUMMARIZE) printfQuda("Tuned %s %s %s: y groups %d, link policy %d, store policy %d, boundary-first %d (%s)\n", key.volume, key.name, key.aux, tp.aux[0], tp.aux[1], tp.aux[2], tp.aux[3], text);
}

DslashTune effectiveDslashTune(const LatticeGeom &g, QudaPrecision prec, int recon, int variant, const DslashParam &p, int pmask, const DslashTune *candidate, HaloTransport transport,
                               const DslashApply &apply) {
  DslashTune tune = dslashTune();
  if (candidate) {   // a sweep's candidate being timed: its knobs, and the cache is left alone
    if (candidate->ygroups >= 0) tune.ygroups = candidate->ygroups;
    if (candidate->link_aux >= 0) tune.link_aux = candidate->link_aux;
    if (candidate->store_aux >= 0) tune.store_aux = candidate->store_aux;
    if (candidate->edge_first >= 0) tune.edge_first = candidate->edge_first;
  } else if (!p.ndeg && (tuningEnabled() || tuneCacheSize() > 0)) {
    const TuneKey key = dslashTuneKey(g, (int)prec, recon, variant, p, pmask);
    const TuneParam *tp = tuneLookup(key);
    // (a partitioned launch that picks its own transport is first verified, then tuned)
    if (!tp && tuningEnabled() && !(pmask && transport == HALO_AUTO && haloBuffers(g, prec).verified == 0)) {
      sweepDslash(key, g, (int)prec, pmask, apply);
      tp = tuneLookup(key);
    }
    if (tp) {
      if (tune.ygroups < 0) tune.ygroups = tp->aux[0];
      if (tune.link_aux < 0) tune.link_aux = tp->aux[1];
      if (tune.store_aux < 0) tune.store_aux = tp->aux[2];
      if (pmask) tune.edge_first = tp->aux[3];
    }
  }
  return tune;
}

// ---- partitioned launches ----
FacePlan dslashFacePlan(const LatticeGeom &g, int mask) {
  FacePlan f;
  int nt = 0;
  for (int d = 0; d < 4; d++) {
    f.on[d] = (mask >> d) & 1;
    for (int dir = 0; dir < 2; dir++) {
      f.start[2 * d + dir] = nt;
      if (f.on[d]) nt += g.faceCB[d];
    }
  }
  f.start[8] = nt;
  return f;
}

// Zones are double-buffered by the parity of the exchange counter: a neighbour can be at most one exchange ahead (to finish exchange k+1 it
// needs OUR face k+1, which is packed after our kernel k), and the flag — the use count of the (dimension, buffer) zone — tells this
// exchange's words from the ones two exchanges old.
PeerExchange nextPeerExchange(HaloBuffers &hb, int mask) {
  PeerExchange e{};
  e.seq = ++hb.seq;
  e.buf = e.seq & 1;
  p2pStats()[0]++;
  for (int d = 0; d < 4; d++)
    if ((mask >> d) & 1) {
      e.flag[d] = ++hb.uses[d][e.buf];
      if (e.flag[d] == 0) e.flag[d] = ++hb.uses[d][e.buf];   // 0 is the value of a never-written word
    }
  return e;
}

// The start-up probe has exercised the access patterns, this checks the production kernel itself.
void verifyPeerStoreHalo(HaloBuffers &hb, ColorSpinorField &out, double tol, const std::function<void(HaloTransport)> &applyThrough) {
  hipStream_t cs = computeStream();
  applyThrough(HALO_STAGED);
  HIP_CHECK(hipStreamSynchronize(cs));
  ColorSpinorField ref(out);
  applyThrough(HALO_PEER_STORE);
  HIP_CHECK(hipStreamSynchronize(cs));
  double fail = p2pTakeError() ? 1.0 : 0.0;
  const bool wasGlobal = blas::globalReduction();
  blas::setGlobalReduction(false);   // rank-local sums; the verdict is shared through the host collective below
  const double n2 = blas::norm2(out), d2 = blas::xmyNorm(out, ref);
  blas::setGlobalReduction(wasGlobal);
  if (!(d2 <= tol * tol * n2)) fail = 1.0;
  if (getenv("QUDA_AMD_P2P_VERIFY_FAIL")) fail = 1.0;   // test hook: exercise the fall-back
  comm_allreduce(&fail, 1);
  if (fail != 0.0) {
    if (commGrid().rank == 0) warningQuda("peer-store halo disagrees with the staged transport on its first use: staying with RCCL send/recv");
    p2pDisable();
    for (HaloBuffers &h : g_halo) { h.p2p = false; h.verified = 0; }
    applyThrough(HALO_AUTO);
    return;
  }
  hb.verified = 1;
}

// ---- QUDA_AMD_TIMELINE=1: per-block wall_clock64 stamps of one peer-store launch (measurement aid) ----
unsigned long long *dslashTimelineBuffer() {
  static unsigned long long *tl = nullptr;
  static int tlmode = -1;
  if (tlmode < 0) { const char *e = getenv("QUDA_AMD_TIMELINE"); tlmode = e ? atoi(e) : 0; if (tlmode) HIP_CHECK(hipHostMalloc((void **)&tl, 16384 * sizeof(unsigned long long), hipHostMallocMapped)); }
  return tl;
}
void dslashTimelineReport(const unsigned long long *tl, int packBlocks, int nb) {
  unsigned long long t0 = ~0ull;
  for (int i = 0; i < 16384; i++) if ((i < 3072 || i >= 4096) && tl[i] && tl[i] < t0) t0 = tl[i];   // 3072..4095 hold placement words
  auto stat = [&](int off, int n, const char *name) {
    double mn = 1e30, mx = 0, sum = 0; int c = 0;
    for (int i = 0; i < n; i++) if (tl[off + i]) { const double v = (tl[off + i] - t0) * 0.01; mn = v < mn ? v : mn; mx = v > mx ? v : mx; sum += v; c++; }
    if (c) printfQuda("timeline %-22s n=%4d  min %6.2f  mean %6.2f  max %6.2f us\n", name, c, mn, sum / c, mx);
  };
  stat(0, 1024, "pack block start"); stat(13312, 1024, "pack loads returned"); stat(1024, 1024, "pack block end"); stat(2048, 1024, "stencil block start");
  stat(4096, 4096, "boundary wave ghost beg"); stat(8192, 4096, "boundary wave ghost end"); stat(12288, 1024, "stencil block end");
  {   // placement: how many site / pack blocks share a CU, and when the site blocks of such CUs finish
    std::map<unsigned, std::pair<int, int>> cu;   // key -> (site blocks, pack blocks)
    const int npk = packBlocks, ntot = packBlocks + nb;
    for (int i = 0; i < ntot && i < 1024; i++) if (tl[3072 + i]) { auto &c = cu[(unsigned)tl[3072 + i]]; if (i < npk) c.second++; else c.first++; }
    double sum[4][2] = {}, mx[4][2] = {}; int cnt[4][2] = {};
    for (int i = npk; i < ntot && i < 1024; i++) if (tl[3072 + i] && tl[12288 + i]) {
      const auto &c = cu[(unsigned)tl[3072 + i]];
      const int a = c.first > 3 ? 3 : c.first, b = c.second > 0 ? 1 : 0;
      const double e = (tl[12288 + i] - t0) * 0.01;
      sum[a][b] += e; mx[a][b] = e > mx[a][b] ? e : mx[a][b]; cnt[a][b]++;
    }
    printfQuda("timeline placement: %zu CUs in use\n", cu.size());
    for (int a = 1; a < 4; a++) for (int b = 0; b < 2; b++)
      if (cnt[a][b]) printfQuda("timeline   site blocks on a CU with %d site block(s)%s: n=%3d  mean end %6.2f  max end %6.2f us\n", a, b ? " + pack block(s)" : "", cnt[a][b], sum[a][b] / cnt[a][b], mx[a][b]);
  }
  for (int x = 0; x < 8; x++) {   // per XCD (blocks are dealt round-robin): start / end of its stencil blocks
    double sb = 0, se = 0, mx = 0; int c = 0;
    for (int i = x; i < 1024; i += 8) if (tl[12288 + i]) { sb += (tl[2048 + i] - t0) * 0.01; const double e = (tl[12288 + i] - t0) * 0.01; se += e; mx = e > mx ? e : mx; c++; }
    if (c) printfQuda("timeline xcd %d: %3d stencil blocks, mean start %6.2f, mean end %6.2f, max end %6.2f us\n", x, c, sb / c, se / c, mx);
  }
}

long long dslashFlopsPerSite(DslashMode mode, bool xpay) {
  long long f = 1320;  // lib/dslash_quda.cuh:480-495
  switch (mode) {
    case DSLASH_PLAIN: f += xpay ? 48 : 0; break;
    case DSLASH_TWIST_INV: case DSLASH_TWIST_INV_DSLASH: case DSLASH_TWIST_XPAY: f += 48 + (xpay ? 48 : 0); break;  // lib/dslash_twisted_mass.cu:144-160
    case DSLASH_CLOVER_TWIST_INV: case DSLASH_CLOVER_TWIST_XPAY: f += 552 + (xpay ? 48 : 0); break;  // lib/dslash_twisted_clover.cu:213-230
  }
  return f;
}

// one fused doublet application per checkerboard site of the 4-d lattice: the 8 links once, in and out (and x) for both flavours
long long ndegDslashBytesPerSite(QudaPrecision prec, int recon, bool xpay) {
  const long long P = prec;
  long long b = 8LL * recon * P + 2 * (24 * P + 24 * P + (xpay ? 24 * P : 0));
  if (prec == QUDA_HALF_PRECISION) b += 2 * 4 * (2 + (xpay ? 1 : 0));
  return b;
}

long long dslashBytesPerSite(QudaPrecision prec, int recon, DslashMode mode, bool xpay) {
  const long long P = prec;
  long long b = 8LL * recon * P + 24 * P + 24 * P;
  const bool x = xpay || mode == DSLASH_TWIST_XPAY || mode == DSLASH_CLOVER_TWIST_XPAY;
  if (x) b += 24 * P;
  if (mode == DSLASH_CLOVER_TWIST_INV) b += 144 * P;
  if (mode == DSLASH_CLOVER_TWIST_XPAY) b += 72 * P;
  if (prec == QUDA_HALF_PRECISION) {
    b += 4 * (2 + (x ? 1 : 0));
    if (mode == DSLASH_CLOVER_TWIST_INV) b += 16;
    if (mode == DSLASH_CLOVER_TWIST_XPAY) b += 8;
  }
  return b;
}

}  // namespace quda
