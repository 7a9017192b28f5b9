// fields.h — lattice fields of the MI355X-native library.
//
// ColorSpinorField keeps the reference's layout contract (include/color_spinor_field.h:75-456,
// lib/color_spinor_field.cpp:129-216): parity fields with x[0] halved, stride = volumeCB + pad, planar
// FLOAT2 (fp64: nSpin*nColor double2 planes) / FLOAT4 (fp32: 6 float4 planes) / 16-bit (6 short4 planes +
// one fp32 norm per site, int16 fixed point as lib/io_spinor.h:49-62) device orders, full fields = even
// half then odd half, twistFlavor / gammaBasis attributes.  One deliberate difference, allowed by
// the device-internal spin basis of nSpin=4 fields is DeGrand-Rossi (chiral), not UKQCD,
// so gamma5, the twist and the clover term are spin-diagonal / chirality-block-diagonal in the kernels and
// the multigrid transfer needs no rotation; host fields in UKQCD basis are rotated on upload/download.
//
// GaugeField is re-designed for CDNA4 (the device link layout is not API-visible): for every parity p and
// checkerboard site x it stores the EIGHT matrices the stencil multiplies with at x,
//      W[p][2mu](x) = U_mu(x)        W[p][2mu+1](x) = U_mu(x - mu)^dagger,
// i.e. backward links are pre-gathered and pre-daggered once at load time.  Every link load of the Dslash
// is then a perfectly coalesced, aligned, unit-stride 16-byte-per-lane stream indexed by the thread's own
// site (no neighbour index arithmetic, no dagger variant, no ghost-link pad); HBM traffic per Dslash is
// unchanged (8 distinct links per site either way) at the price of 2x gauge capacity, which 288 GB absorbs.
#pragma once

#include "qa_core.h"

namespace quda {

// ------------------------------------------------------------------------------------------------
struct ColorSpinorParam {
  QudaFieldLocation location = QUDA_CUDA_FIELD_LOCATION;
  int nColor = 3, nSpin = 4, nDim = 4;
  int x[QUDA_MAX_DIM] = {0, 0, 0, 0, 0, 0};  // x[0] already halved for parity fields (reference convention)
  // non-degenerate twisted-mass doublet: nDim = 5 and x[4] = 2, the reference's flavour dimension (tests/invert_test.cpp:461-473)
  void setFlavors(int n) { if (n == 2) { nDim = 5; x[4] = 2; } else { nDim = 4; x[4] = 0; } }
  int flavors() const { return nDim == 5 && x[4] == 2 ? 2 : 1; }
  QudaPrecision precision = QUDA_DOUBLE_PRECISION;
  int pad = 0;
  bool planePad = true;  // device spin-4 fields: add the library's plane padding (fieldPadSites) to pad; false in the param() of an existing field, whose pad already holds it
  QudaTwistFlavorType twistFlavor = QUDA_TWIST_NO;
  QudaSiteSubset siteSubset = QUDA_PARITY_SITE_SUBSET;
  QudaSiteOrder siteOrder = QUDA_EVEN_ODD_SITE_ORDER;
  QudaFieldOrder fieldOrder = QUDA_INVALID_FIELD_ORDER;  // chosen from precision for device fields
  QudaGammaBasis gammaBasis = QUDA_DEGRAND_ROSSI_GAMMA_BASIS;
  QudaFieldCreate create = QUDA_ZERO_FIELD_CREATE;
  void *v = nullptr;     // for QUDA_REFERENCE_FIELD_CREATE
  void *norm = nullptr;
  ColorSpinorParam() {}
  // host field as described by the C ABI (reference include/color_spinor_field.h:118-160)
  ColorSpinorParam(void *V, const QudaInvertParam &inv, const int *X, bool pc_solution);
};

class ColorSpinorField {
 public:
  QudaFieldLocation location;
  int nColor, nSpin, nDim;
  int x[4];            // x[0] halved for parity fields
  int nFlavor;         // 2: flavour doublet (nDim = 5).  Every plane holds flavour 1's sites, then flavour 2's: checkerboard index f * Vh + i
  int volume, volumeCB, stride, pad;   // volume, volumeCB and stride count both flavours of a doublet: BLAS and the solvers see a longer parity field
  QudaPrecision precision;
  QudaSiteSubset siteSubset;
  QudaSiteOrder siteOrder;
  QudaFieldOrder fieldOrder;
  QudaGammaBasis gammaBasis;
  QudaTwistFlavorType twistFlavor;
  size_t bytes, norm_bytes;   // whole allocation (both parities for full fields)
  void *v_;
  void *norm_;
  bool owns;
  ColorSpinorField *even_, *odd_, *flavor_[2];

  explicit ColorSpinorField(const ColorSpinorParam &param);
  ColorSpinorField(const ColorSpinorField &src);  // deep copy, same location/layout
  virtual ~ColorSpinorField();
  ColorSpinorField &operator=(const ColorSpinorField &src);  // copy with reorder/precision/basis change

  void *V() { return v_; }
  const void *V() const { return v_; }
  void *Norm() { return norm_; }
  const void *Norm() const { return norm_; }
  int Nspin() const { return nSpin; }
  int Ncolor() const { return nColor; }
  int Volume() const { return volume; }
  int VolumeCB() const { return volumeCB; }
  int Stride() const { return stride; }
  int X(int d) const { return x[d]; }
  QudaPrecision Precision() const { return precision; }
  QudaSiteSubset SiteSubset() const { return siteSubset; }
  QudaTwistFlavorType TwistFlavor() const { return twistFlavor; }
  int Nflavor() const { return nFlavor; }
  int VolumeCB4() const { return volumeCB / nFlavor; }   // checkerboard sites of the 4-d lattice
  void changeTwist(QudaTwistFlavorType f);   // to or from the doublet: an error, the flavour count of a field is fixed
  QudaFieldLocation Location() const { return location; }
  size_t Bytes() const { return bytes; }
  long Length() const { return (long)(siteSubset == QUDA_FULL_SITE_SUBSET ? 2 : 1) * stride * nColor * nSpin * 2; }
  long RealLength() const { return (long)volume * nColor * nSpin * 2; }

  ColorSpinorField &Even();
  ColorSpinorField &Odd();
  const ColorSpinorField &Even() const { return const_cast<ColorSpinorField *>(this)->Even(); }
  const ColorSpinorField &Odd() const { return const_cast<ColorSpinorField *>(this)->Odd(); }
  // one flavour (0, 1) of a device parity doublet as a 4-d field of the same stride, twist flavour +1 / -1.  Stencil and site kernels
  // only: the flat BLAS kernels run over whole planes and must not see a view
  ColorSpinorField &Flavor(int f);
  const ColorSpinorField &Flavor(int f) const { return const_cast<ColorSpinorField *>(this)->Flavor(f); }

  void zero();
  // full local lattice dims (x[0] un-halved)
  void latticeDims(int X[4]) const {
    for (int d = 0; d < 4; d++) X[d] = x[d];
    if (siteSubset == QUDA_PARITY_SITE_SUBSET) X[0] *= 2;
  }
  static ColorSpinorField *Create(const ColorSpinorParam &p) { return new ColorSpinorField(p); }
  ColorSpinorParam param() const;

 private:
  void createViews();
};

// source-compatible names (reference include/color_spinor_field.h:458, :640)
class cudaColorSpinorField : public ColorSpinorField {
 public:
  explicit cudaColorSpinorField(const ColorSpinorParam &p);
  cudaColorSpinorField(const ColorSpinorField &src, const ColorSpinorParam &p);
  cudaColorSpinorField &operator=(const ColorSpinorField &src) { ColorSpinorField::operator=(src); return *this; }
};
class cpuColorSpinorField : public ColorSpinorField {
 public:
  explicit cpuColorSpinorField(const ColorSpinorParam &p);
  cpuColorSpinorField &operator=(const ColorSpinorField &src) { ColorSpinorField::operator=(src); return *this; }
};

void copyColorSpinor(ColorSpinorField &dst, const ColorSpinorField &src);
// uniform(0,1) random spinor from a counter-based generator keyed by (seed, global site, component): the same field for
// any process grid (reference uses a private rand48 clone, lib/color_spinor_util.cu:12-22)
void spinorRandom(ColorSpinorField &f, unsigned long long seed);

// ------------------------------------------------------------------------------------------------
// Fine-grid SU(3) gauge field in the bidirectional device layout described at the top of this file.
class GaugeField {
 public:
  LatticeGeom geom;
  QudaPrecision precision;
  QudaReconstructType reconstruct;  // 18 or 12
  QudaTboundary t_boundary;
  double anisotropy;
  int stride;               // = Vh
  size_t link_bytes;        // bytes of one (parity, direction) block
  size_t bytes;
  void *data;               // [parity][dir 0..7][link_bytes]
  bool tbc_folded;          // true: boundary sign is inside the stored links (recon 18)

  GaugeField(const LatticeGeom &g, QudaPrecision prec, QudaReconstructType recon, QudaTboundary tb, double aniso);
  ~GaugeField();
  // host QDP-order links (array of 4 pointers, even then odd, row-major 3x3; reference SURVEY section 9)
  void loadQDP(void *const h_gauge[4], QudaPrecision cpu_prec);
  void copyFrom(const GaugeField &src);   // device copy with precision change (fp32 -> 16-bit), same reconstruct
  const void *block(int parity, int dir) const { return (const char *)data + ((size_t)parity * 8 + dir) * link_bytes; }
  const void *parityBase(int parity) const { return block(parity, 0); }
  double GiB() const { return bytes / (double)(1 << 30); }
};

// Clover term A and its (twisted) inverse, two Hermitian 6x6 chiral blocks per site.  Host packed order
// as reference tests/clover_reference.cpp:25-53; device: planar 16-byte vectors per chiral block
// (fp64 18 double2, fp32 9 float4, 16-bit 9 short4 + one fp32 norm per block).  Values are stored
// un-halved (the reference's native order carries a factor 1/2, include/clover_field_order.h:425-429;
// an API-level replacement may drop it).
class CloverField {
 public:
  LatticeGeom geom;
  QudaPrecision precision;
  int stride;
  size_t parity_bytes, parity_norm_bytes, bytes;
  void *clover;      // [parity] A
  void *cloverInv;   // [parity] (A^2 + mu2)^-1 if twisted, else A^-1
  float *norm;       // [parity][2 blocks][stride] (16-bit only)
  float *invNorm;
  bool twisted;
  double mu2;
  double trlog[2];
  double coeff;      // the c of computeFromGauge; NAN: unknown (loaded from a host field)

  CloverField(const LatticeGeom &g, QudaPrecision prec);
  ~CloverField();
  void loadPacked(const void *h_clover, const void *h_inv, QudaPrecision cpu_prec);
  // A = 1 + i c sum_{mu>nu} sigma_mu_nu F_mu_nu from the resident links (reference createCloverQuda, lib/interface_quda.cpp:3950-4010:
  // computeFmunu + computeClover with c = clover_coeff); fp64 arithmetic, stored in this field's precision
  void computeFromGauge(const GaugeField &U, double coeff);
  void savePacked(void *h_clover, QudaPrecision cpu_prec) const;
  // compute cloverInv = (A^2 + mu2)^-1 on device (reference lib/clover_invert.cu:56-85); the plain inverse A^-1 if mu2 = 0 and the
  // field does not belong to a twisted operator (twisted clover at mu = 0 keeps the squared form A^-2 that its site kernels multiply
  // (A -+ i a g5) v with)
  void computeInverse(double mu2, bool twisted = false);
  void savePackedInverse(void *h_inv, QudaPrecision cpu_prec) const;
  const void *A(int parity) const { return (const char *)clover + (size_t)parity * parity_bytes; }
  const void *Ainv(int parity) const { return (const char *)cloverInv + (size_t)parity * parity_bytes; }
  const float *Anorm(int parity) const { return norm ? norm + (size_t)parity * 2 * stride : nullptr; }
  const float *AinvNorm(int parity) const { return invNorm ? invNorm + (size_t)parity * 2 * stride : nullptr; }
  double GiB() const { return 2.0 * bytes / (double)(1 << 30); }
};

// fp64 host links in QDP order: the four arrays of 18 V reals and the pointers to them, as loadQDP and saveGaugeQDP take them
struct HostLinks {
  std::vector<std::vector<double>> links;
  void *ptr[4];
  explicit HostLinks(size_t V) : links(4, std::vector<double>(V * 18)) { for (int d = 0; d < 4; d++) ptr[d] = links[d].data(); }
  HostLinks(const HostLinks &) = delete;
  HostLinks &operator=(const HostLinks &) = delete;
};

// gauge tools on the device (gauge_obs.hip): APE smearing of the spatial links (a new fp64 field), the plaquette averages, and the
// forward links back in host QDP order
GaugeField *apeSmear(const GaugeField &U, unsigned nSteps, double alpha);
// stout smearing of the first ndir directions (3: spatial links from spatial staples, 4: all links, all six planes); a new fp64 field
GaugeField *stoutSmear(const GaugeField &U, unsigned nSteps, double rho, int ndir);
// global topological charge from the clover-leaf field strength; h_density (may be NULL): this rank's q(x), even sites then odd
double topologicalCharge(const GaugeField &U, double *h_density);
// exp(i q[k]) of n traceless Hermitian 3x3 matrices (18 reals each) through the device function of the stout kernel (test hook)
void su3ExpIQ(int n, const double *h_q, double *h_out);
void plaquette(const GaugeField &U, double plq[3]);
void saveGaugeQDP(const GaugeField &U, void *const h_gauge[4], QudaPrecision cpu_prec);

// ---- gauge molecular dynamics (gauge_md.hip) ----
// The conjugate momentum of the links: ten fp64 per link in the reference's MILC order of a reconstruct-10 field,
// [site (even sites, then odd)][mu][10], on the device exactly as on the host
class MomField {
 public:
  LatticeGeom geom;
  size_t bytes;
  double *data;
  explicit MomField(const LatticeGeom &g);   // zeroed
  ~MomField();
  void zero();
  void load(const void *h_mom);
  void save(void *h_mom) const;
};
constexpr int kGaugeForceMaxLength = 8;    // links per path (plaquette 3, rectangle and chair 5, the Luescher-Weisz set fits)
constexpr int kGaugeForceMaxPaths = 64;    // paths per direction (Wilson 6, tree-level Symanzik 24, Luescher-Weisz 48)
// mom <- TA(mom - eb3 U V), V the coefficient-weighted sum of the path products (reference lib/gauge_force.cu:62-142); the direct
// gather on an unpartitioned lattice, the transport formulation on a partitioned one or under QUDA_AMD_GAUGE_FORCE_TRANSPORT=1
void gaugeForce(MomField &mom, const GaugeField &U, double eb3, int ***path, const int *length, const double *coeff, int num_paths, int max_length);
bool gaugeForceUsesTransport();
// exp(dt A) U (exact) or its eighth-order Taylor form, conj_mom: with the complex conjugate of A; the new links in host QDP order
void updateGaugeLinks(void *const h_out[4], const GaugeField &U, const MomField &mom, double dt, bool conj_mom, bool exact);
// the links projected onto SU(3), in host QDP order; returns the global number of links with max |U^dag U - 1| > tol
long projectSU3Links(void *const h_out[4], const GaugeField &U, double tol);
// sum over links of tr(A^dag A)/2 - 4, global, in a fixed order
double momAction(const MomField &mom);

// ---- gauge fixing (gauge_fix.hip; DESIGN section 3 "Gauge fixing") ----
struct GaugeFixResult { int iterations; double F, theta, delta; };   // delta: the last |F - F_prev|
// Overrelaxation towards the maximum of F = sum_x sum_{mu<D} Re tr U_mu(x) / (3 D V), D = 3 if gauge_dir == 3 (Coulomb) else 4 (Landau):
// at most nsteps iterations (even sites, then odd) with parameter omega, the links projected onto SU(3) when iteration % reunit_interval
// == reunit_interval - 1 and at the end; stops when theta (stop_theta) or |F - F_prev| falls below tolerance.  fp64 on matrix fields
// whatever the precision of U; the anti-periodic sign of the time links is taken off for the run and put back.  The direct sweep on
// an unpartitioned lattice, the transport formulation on a partitioned one or under QUDA_AMD_GAUGE_FIX_TRANSPORT=1.  h_out: the fixed
// links in host QDP order; h_transform (may be NULL): G(x), V x 18 reals, even sites then odd, with U^fixed_mu(x) = G(x) U_mu(x) G(x + mu)^dag;
// secs: {extracting the links, iterating, writing the result}
GaugeFixResult gaugeFixOVR(void *const h_out[4], double *h_transform, const GaugeField &U, int gauge_dir, int nsteps, int verbose_interval, double omega,
                           double tolerance, int reunit_interval, int stop_theta, double secs[3]);
bool gaugeFixUsesTransport();
// out = {F, theta} of the links of U (sign of the time boundary taken off), global, in a fixed summation order
void gaugeFixQuality(const GaugeField &U, int gauge_dir, double out[2]);

// ---- fermion force (ferm_force.hip) ----
constexpr int kFermForceMaxFields = 16;   // (X, Y) pairs of one launch, a doublet counting two: more are chunked on the host
// mom <- TA(mom - sum_i coeff[i] U O[X_i, Y_i]), O_mu[X, Y](x) = tr_spin[(1 - g_mu) X(x + mu) Y^dag(x) + (1 + g_mu) Y(x + mu) X^dag(x)]
// summed over the flavours; X_i, Y_i full fp64 device fields of one or two flavours.  Any partition mask (ghost zones of X and Y)
void fermionOprodForce(MomField &mom, const GaugeField &U, const std::vector<ColorSpinorField *> &X, const std::vector<ColorSpinorField *> &Y,
                       const std::vector<double> &coeff);
// mom <- mom + dt sum_i coeff[i] F[x_i], F the force of phi^dag (Mh^dag Mh)^-1 phi at the single-parity solutions x_i of the even-odd
// operator Mh of inv (Wilson, twisted mass +-1, the doublet; the four matpc types; the mass normalisations of the solves)
void tmForce(MomField &mom, const GaugeField &U, double dt, const std::vector<ColorSpinorField *> &x, const std::vector<double> &coeff, QudaInvertParam *inv);
// seconds the last fermionOprodForce spent in its kernel launches (device events), for tools/ferm_force_timing.py
double fermForceLastKernelSecs();
// the kernels of clover_force.hip count towards the same figure: reset starts a new call
void fermForceAddKernelSecs(double secs, bool reset);

// ---- twisted-clover force (clover_force.hip; DESIGN section 3 "Twisted-clover force") ----
// Six 3x3 colour matrices per site, one per plane f = mu (mu - 1) / 2 + nu, nu < mu (F10, F20, F21, F30, F31, F32): six fp64 matrix
// fields in one allocation.  Host order [site (even, odd)][f][3][3][re, im]
class TensorField {
 public:
  LatticeGeom geom;
  size_t bytes;
  double *data;
  explicit TensorField(const LatticeGeom &g);   // zeroed
  ~TensorField();
  TensorField(const TensorField &) = delete;
  TensorField &operator=(const TensorField &) = delete;
  void load(const double *h_tensor);
  void save(double *h_tensor) const;
};
// One (X, Y) pair of the sigma outer product: fp64 parity fields (even, odd) of one flavour and the complex coefficient of each parity
struct SigmaOprodPair { const ColorSpinorField *x[2], *y[2]; double cr[2], ci[2]; };
// T_f(x) (+)= sum_i c_i[parity(x)] S_f[X_i, Y_i](x), S_f[X, Y]_ba = sum_ss' (sigma_f)_ss' X_s'b conj(Y_sa).  Site-local: any partition mask
void cloverSigmaOprod(TensorField &T, const std::vector<SigmaOprodPair> &pairs, bool accumulate);
// T_f(x) (+)= c[parity(x)] sum_ss' (sigma_f)_ss' B(x)_(s'b)(sa), B = A (A^2 + mu2)^-1 from the fp64 blocks of a clover field and its
// resident (twisted) inverse; c = cr + i ci per parity.  Site-local: any partition mask
void cloverSigmaTrace(TensorField &T, const CloverField &clover, const double cr[2], const double ci[2], bool accumulate);
// mom <- mom + coeff G[T], G[T] the force of L_T(U) = sum_x sum_f Re tr(T_f(x) F_f(x; U)).  Unpartitioned lattices only
void cloverDerivativeForce(MomField &mom, const GaugeField &U, const TensorField &T, double coeff);
// stops with a message that names the partition if any direction is partitioned
void checkCloverDerivativeUnpartitioned(const char *fn);

}  // namespace quda
