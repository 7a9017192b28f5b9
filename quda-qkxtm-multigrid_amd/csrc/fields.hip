// fields.hip — spinor field allocation, host<->device reorder (+ precision / gamma-basis change), the staging buffer, and the gauge
// field: storage, upload into the CDNA4 device layout, precision change.  Reference behaviour restated:
// lib/color_spinor_field.cpp:129-216 (geometry), lib/copy_color_spinor.cuh:49-91 (basis rotation),
// lib/cuda_color_spinor_field.cu:513-590 (load/save).  The clover term: clover.hip; observables of the links: gauge_obs.hip.
#include "fields.h"
#include "p2p.h"

#include <cmath>
#include <cstring>
#include <vector>

#include "basis.h"
#include "device_io.h"
#include "dispatch.h"
#include "gauge_device.h"
#include "halo.h"

namespace quda {

// ================================================================================================
// ColorSpinorField
// ================================================================================================
ColorSpinorParam::ColorSpinorParam(void *V, const QudaInvertParam &inv, const int *X, bool pc_solution) {
  location = QUDA_CPU_FIELD_LOCATION;
  nColor = 3; nSpin = 4; nDim = 4;
  for (int d = 0; d < 4; d++) x[d] = X[d];
  siteSubset = pc_solution ? QUDA_PARITY_SITE_SUBSET : QUDA_FULL_SITE_SUBSET;
  if (pc_solution) x[0] /= 2;
  precision = inv.cpu_prec;
  pad = 0;
  twistFlavor = inv.twist_flavor;
  // the doublet: [flavour 1][flavour 2] per parity, the reference's fifth dimension.  Only the twisted-mass operator has one: elsewhere
  // (Wilson, where twist_flavor means nothing) the value does not make a two-flavour field
  if (inv.twist_flavor == QUDA_TWIST_NONDEG_DOUBLET) {
    if (inv.dslash_type == QUDA_TWISTED_MASS_DSLASH) setFlavors(2);
    else twistFlavor = QUDA_TWIST_NO;
  }
  siteOrder = QUDA_EVEN_ODD_SITE_ORDER;
  if (inv.dirac_order == QUDA_DIRAC_ORDER) fieldOrder = QUDA_SPACE_SPIN_COLOR_FIELD_ORDER;
  else if (inv.dirac_order == QUDA_QDP_DIRAC_ORDER) fieldOrder = QUDA_SPACE_COLOR_SPIN_FIELD_ORDER;
  else errorQuda("Dirac order %d not supported (QUDA_DIRAC_ORDER, QUDA_QDP_DIRAC_ORDER)", inv.dirac_order);
  gammaBasis = inv.gamma_basis;
  create = QUDA_REFERENCE_FIELD_CREATE;
  v = V;
}

// Plane padding (sites) of the device fields, QUDA_AMD_FIELD_PAD: the planes of a field are stride x 16 bytes apart, which is a multiple
// of 1 MiB on 32^4 and 48^3 x 96 — every plane of a site then falls into the same L2 set window (the reference pads for the same
// reason, "partition camping": sp_pad / ga_pad / cl_pad of QudaInvertParam / QudaGaugeParam).
int fieldPadSites() {
  static int v = [] { const char *e = getenv("QUDA_AMD_FIELD_PAD"); return e ? atoi(e) : 0; }();
  return v;
}
int gaugePadSites() {
  static int v = [] { const char *e = getenv("QUDA_AMD_GAUGE_PAD"); return e ? atoi(e) : fieldPadSites(); }();
  return v;
}

ColorSpinorField::ColorSpinorField(const ColorSpinorParam &p)
    : location(p.location), nColor(p.nColor), nSpin(p.nSpin), nDim(p.nDim), pad(p.pad), precision(p.precision),
      siteSubset(p.siteSubset), siteOrder(p.siteOrder), fieldOrder(p.fieldOrder), gammaBasis(p.gammaBasis),
      twistFlavor(p.twistFlavor), v_(nullptr), norm_(nullptr), owns(false), even_(nullptr), odd_(nullptr), flavor_{nullptr, nullptr} {
  nFlavor = p.flavors();
  nDim = nFlavor == 2 ? 5 : 4;
  if ((nFlavor == 2) != (twistFlavor == QUDA_TWIST_NONDEG_DOUBLET)) errorQuda("twist flavour %d on a field of %d flavour(s): the non-degenerate doublet is a two-flavour field", twistFlavor, nFlavor);
  volume = nFlavor;
  for (int d = 0; d < 4; d++) { x[d] = p.x[d]; volume *= p.x[d]; }
  if (volume <= 0) errorQuda("empty field: x = %d %d %d %d", x[0], x[1], x[2], x[3]);
  const int nsub = siteSubset == QUDA_FULL_SITE_SUBSET ? 2 : 1;
  volumeCB = volume / nsub;
  if (location == QUDA_CPU_FIELD_LOCATION) pad = 0;
  else if (p.planePad && p.create != QUDA_REFERENCE_FIELD_CREATE && nSpin == 4) pad += fieldPadSites();
  stride = volumeCB + pad;
  if (location == QUDA_CUDA_FIELD_LOCATION) {
    fieldOrder = (precision == QUDA_DOUBLE_PRECISION || nSpin != 4) ? QUDA_FLOAT2_FIELD_ORDER : QUDA_FLOAT4_FIELD_ORDER;
    if (nSpin == 4) gammaBasis = QUDA_DEGRAND_ROSSI_GAMMA_BASIS;  // device-internal basis (see fields.h)
    if (nSpin != 4 && precision == QUDA_HALF_PRECISION) errorQuda("16-bit coarse fields are not supported");
  } else {
    if (precision == QUDA_HALF_PRECISION) errorQuda("16-bit host fields are not supported");
    if (fieldOrder == QUDA_INVALID_FIELD_ORDER) fieldOrder = QUDA_SPACE_SPIN_COLOR_FIELD_ORDER;
  }
  const size_t per_parity = (size_t)stride * nColor * nSpin * 2 * precision;
  // keep each parity half 1 KiB aligned like the reference (TEX_ALIGN_REQ, include/quda_internal.h:32-33)
  const size_t half = location == QUDA_CUDA_FIELD_LOCATION ? alignUp(per_parity, 1024) : per_parity;
  bytes = nsub * half;
  norm_bytes = precision == QUDA_HALF_PRECISION ? nsub * alignUp((size_t)stride * sizeof(float), 1024) : 0;

  if (p.create == QUDA_REFERENCE_FIELD_CREATE) {
    v_ = p.v; norm_ = p.norm;
    if (!v_) errorQuda("reference field without data pointer");
  } else {
    owns = true;
    if (location == QUDA_CUDA_FIELD_LOCATION) {
      v_ = poolDeviceMalloc(bytes);
      if (norm_bytes) norm_ = poolDeviceMalloc(norm_bytes);
    } else {
      v_ = malloc(bytes);
      if (!v_) errorQuda("host allocation of %zu bytes failed", bytes);
    }
    if (p.create == QUDA_ZERO_FIELD_CREATE || (pad > 0 && location == QUDA_CUDA_FIELD_LOCATION)) zero();   // the flat BLAS kernels run over the pad too
  }
}

ColorSpinorParam ColorSpinorField::param() const {
  ColorSpinorParam p;
  p.location = location; p.nColor = nColor; p.nSpin = nSpin; p.nDim = nDim;
  for (int d = 0; d < 4; d++) p.x[d] = x[d];
  p.setFlavors(nFlavor);
  p.precision = precision; p.pad = pad; p.planePad = false; p.twistFlavor = twistFlavor; p.siteSubset = siteSubset; p.siteOrder = siteOrder;
  p.fieldOrder = fieldOrder; p.gammaBasis = gammaBasis; p.create = QUDA_NULL_FIELD_CREATE;
  return p;
}

ColorSpinorField::ColorSpinorField(const ColorSpinorField &src) : ColorSpinorField([&] { ColorSpinorParam p = src.param(); return p; }()) {
  copyColorSpinor(*this, src);
}

ColorSpinorField::~ColorSpinorField() {
  delete even_;
  delete odd_;
  delete flavor_[0];
  delete flavor_[1];
  if (owns) {
    if (location == QUDA_CUDA_FIELD_LOCATION) {
      poolDeviceFree(v_, bytes);
      poolDeviceFree(norm_, norm_bytes);
    } else {
      free(v_);
    }
  }
}

void ColorSpinorField::zero() {
  if (location == QUDA_CUDA_FIELD_LOCATION) {
    HIP_CHECK(hipMemsetAsync(v_, 0, bytes, computeStream()));
    if (norm_bytes) HIP_CHECK(hipMemsetAsync(norm_, 0, norm_bytes, computeStream()));
  } else {
    memset(v_, 0, bytes);
  }
}

void ColorSpinorField::createViews() {
  if (siteSubset != QUDA_FULL_SITE_SUBSET) errorQuda("Even()/Odd() need a full field");
  ColorSpinorParam p = param();
  p.siteSubset = QUDA_PARITY_SITE_SUBSET;
  p.x[0] = x[0] / 2;
  p.create = QUDA_REFERENCE_FIELD_CREATE;
  p.v = v_; p.norm = norm_;
  even_ = new ColorSpinorField(p);
  p.v = (char *)v_ + bytes / 2;  // reference lib/cpu_color_spinor_field.cpp:165
  p.norm = norm_ ? (char *)norm_ + norm_bytes / 2 : nullptr;
  odd_ = new ColorSpinorField(p);
}
ColorSpinorField &ColorSpinorField::Even() { if (!even_) createViews(); return *even_; }
ColorSpinorField &ColorSpinorField::Odd() { if (!odd_) createViews(); return *odd_; }

ColorSpinorField &ColorSpinorField::Flavor(int f) {
  if (nFlavor != 2 || f < 0 || f > 1) errorQuda("Flavor(%d) of a field of %d flavour(s)", f, nFlavor);
  if (siteSubset != QUDA_PARITY_SITE_SUBSET || location != QUDA_CUDA_FIELD_LOCATION || nSpin != 4) errorQuda("Flavor() needs a device parity doublet");
  if (!flavor_[f]) {
    const int Vh = VolumeCB4();
    ColorSpinorParam p = param();
    p.setFlavors(1);
    p.twistFlavor = f == 0 ? QUDA_TWIST_PLUS : QUDA_TWIST_MINUS;
    p.pad = stride - Vh;   // the planes of the view are the doublet's
    p.create = QUDA_REFERENCE_FIELD_CREATE;
    const size_t entry = 16;   // one plane entry of a site: double2, float4 or eight int16 (device_io.h)
    p.v = (char *)v_ + (size_t)f * Vh * entry;
    p.norm = norm_ ? (char *)norm_ + (size_t)f * Vh * sizeof(float) : nullptr;
    flavor_[f] = new ColorSpinorField(p);
  }
  return *flavor_[f];
}

void ColorSpinorField::changeTwist(QudaTwistFlavorType f) {
  if ((f == QUDA_TWIST_NONDEG_DOUBLET) != (nFlavor == 2)) errorQuda("changeTwist(%d) on a field of %d flavour(s): the non-degenerate doublet is fixed when the field is created", f, nFlavor);
  twistFlavor = f;
  if (even_) even_->twistFlavor = f;
  if (odd_) odd_->twistFlavor = f;
}

ColorSpinorField &ColorSpinorField::operator=(const ColorSpinorField &src) {
  if (&src != this) copyColorSpinor(*this, src);
  return *this;
}

static ColorSpinorParam deviceParamFrom(const ColorSpinorParam &p) { ColorSpinorParam q = p; q.location = QUDA_CUDA_FIELD_LOCATION; return q; }
static ColorSpinorParam hostParamFrom(const ColorSpinorParam &p) { ColorSpinorParam q = p; q.location = QUDA_CPU_FIELD_LOCATION; return q; }
cudaColorSpinorField::cudaColorSpinorField(const ColorSpinorParam &p) : ColorSpinorField(deviceParamFrom(p)) {}
cudaColorSpinorField::cudaColorSpinorField(const ColorSpinorField &src, const ColorSpinorParam &p) : ColorSpinorField(deviceParamFrom(p)) {
  twistFlavor = src.twistFlavor;
  copyColorSpinor(*this, src);
}
cpuColorSpinorField::cpuColorSpinorField(const ColorSpinorParam &p) : ColorSpinorField(hostParamFrom(p)) {}

// ---- reorder kernels -----------------------------------------------------------------------------
// host site-major record of NR reals: index (site*NR + (s*Nc + c)*2 + z)   [SPACE_SPIN_COLOR]
//                                       or   (site*NR + (c*Ns + s)*2 + z)   [SPACE_COLOR_SPIN]
template <typename TDev, typename THost>
__global__ void spinor_h2d_kernel(void *dev, float *norm, int stride, const THost *host, int Vh, int color_spin, int change) {
  using real = typename Store<TDev>::real;
  const int x = blockIdx.x * blockDim.x + threadIdx.x;
  if (x >= Vh) return;
  real r[24], q[24];
  const THost *h = host + (size_t)x * 24;
#pragma unroll
  for (int s = 0; s < 4; s++)
#pragma unroll
    for (int c = 0; c < 3; c++) {
      const int hi = color_spin ? (c * 4 + s) * 2 : (s * 3 + c) * 2;
      r[(s * 3 + c) * 2] = (real)h[hi];
      r[(s * 3 + c) * 2 + 1] = (real)h[hi + 1];
    }
  if (change) { rotate_basis(q, r, change); Planar<TDev, 24>::store(q, dev, stride, x, norm, x); }
  else Planar<TDev, 24>::store(r, dev, stride, x, norm, x);
}

template <typename TDev, typename THost>
__global__ void spinor_d2h_kernel(THost *host, const void *dev, const float *norm, int stride, int Vh, int color_spin, int change) {
  using real = typename Store<TDev>::real;
  const int x = blockIdx.x * blockDim.x + threadIdx.x;
  if (x >= Vh) return;
  real r[24], q[24];
  Planar<TDev, 24>::load(r, dev, stride, x, norm, x);
  if (change) rotate_basis(q, r, change);
  THost *h = host + (size_t)x * 24;
#pragma unroll
  for (int s = 0; s < 4; s++)
#pragma unroll
    for (int c = 0; c < 3; c++) {
      const int hi = color_spin ? (c * 4 + s) * 2 : (s * 3 + c) * 2;
      h[hi] = (THost)(change ? q[(s * 3 + c) * 2] : r[(s * 3 + c) * 2]);
      h[hi + 1] = (THost)(change ? q[(s * 3 + c) * 2 + 1] : r[(s * 3 + c) * 2 + 1]);
    }
}

template <typename TOut, typename TIn>
__global__ void spinor_d2d_kernel(void *out, float *onorm, int ostride, const void *in, const float *inorm, int istride, int Vh) {
  using rin = typename Store<TIn>::real;
  using rout = typename Store<TOut>::real;
  const int x = blockIdx.x * blockDim.x + threadIdx.x;
  if (x >= Vh) return;
  rin r[24];
  rout q[24];
  Planar<TIn, 24>::load(r, in, istride, x, inorm, x);
#pragma unroll
  for (int k = 0; k < 24; k++) q[k] = (rout)r[k];
  Planar<TOut, 24>::store(q, out, ostride, x, onorm, x);
}

// generic complex-plane fields (coarse grids: nSpin*nColor complex FLOAT2 planes), host site-major
template <typename TDev, typename THost>
__global__ void generic_h2d_kernel(TDev *dev, int stride, const THost *host, int Vh, int ncomplex) {
  const int x = blockIdx.x * blockDim.x + threadIdx.x;
  if (x >= Vh) return;
  for (int k = 0; k < ncomplex; k++) {
    dev[((size_t)k * stride + x) * 2] = (TDev)host[((size_t)x * ncomplex + k) * 2];
    dev[((size_t)k * stride + x) * 2 + 1] = (TDev)host[((size_t)x * ncomplex + k) * 2 + 1];
  }
}
template <typename TDev, typename THost>
__global__ void generic_d2h_kernel(THost *host, const TDev *dev, int stride, int Vh, int ncomplex) {
  const int x = blockIdx.x * blockDim.x + threadIdx.x;
  if (x >= Vh) return;
  for (int k = 0; k < ncomplex; k++) {
    host[((size_t)x * ncomplex + k) * 2] = (THost)dev[((size_t)k * stride + x) * 2];
    host[((size_t)x * ncomplex + k) * 2 + 1] = (THost)dev[((size_t)k * stride + x) * 2 + 1];
  }
}
template <typename TOut, typename TIn>
__global__ void generic_d2d_kernel(TOut *out, int ostride, const TIn *in, int istride, int Vh, int ncomplex) {
  const int x = blockIdx.x * blockDim.x + threadIdx.x;
  if (x >= Vh) return;
  for (int k = 0; k < ncomplex; k++) {
    out[((size_t)k * ostride + x) * 2] = (TOut)in[((size_t)k * istride + x) * 2];
    out[((size_t)k * ostride + x) * 2 + 1] = (TOut)in[((size_t)k * istride + x) * 2 + 1];
  }
}

// staging buffer for host<->device transfers (grows on demand, lives until endQuda)
static void *g_stage = nullptr;
static size_t g_stage_bytes = 0;
void *stagingBuffer(size_t bytes) {
  if (bytes > g_stage_bytes) {
    if (g_stage) HIP_CHECK(hipFree(g_stage));
    HIP_CHECK(qaMalloc(&g_stage, bytes));
    g_stage_bytes = bytes;
  }
  return g_stage;
}
void freeStagingBuffer() {
  if (g_stage) (void)hipFree(g_stage);
  g_stage = nullptr;
  g_stage_bytes = 0;
}

static int basisChange(QudaGammaBasis from, QudaGammaBasis to) {
  auto norm = [](QudaGammaBasis b) { return b == QUDA_CHIRAL_GAMMA_BASIS ? QUDA_DEGRAND_ROSSI_GAMMA_BASIS : b; };
  from = norm(from); to = norm(to);
  if (from == to) return BASIS_NONE;
  if (from == QUDA_UKQCD_GAMMA_BASIS && to == QUDA_DEGRAND_ROSSI_GAMMA_BASIS) return BASIS_UKQCD_TO_DR;
  if (from == QUDA_DEGRAND_ROSSI_GAMMA_BASIS && to == QUDA_UKQCD_GAMMA_BASIS) return BASIS_DR_TO_UKQCD;
  errorQuda("unsupported basis change %d -> %d", from, to);
  return 0;
}

template <typename TDev, typename THost> static void h2dParity(ColorSpinorField &dst, const ColorSpinorField &src) {
  const int Vh = dst.VolumeCB(), bs = 256, nb = (Vh + bs - 1) / bs;
  const size_t hbytes = (size_t)Vh * src.nSpin * src.nColor * 2 * sizeof(THost);
  void *stage = stagingBuffer(hbytes);
  HIP_CHECK(hipMemcpyAsync(stage, src.V(), hbytes, hipMemcpyHostToDevice, computeStream()));
  if (dst.nSpin == 4 && dst.nColor == 3) {
    const int cs = src.fieldOrder == QUDA_SPACE_COLOR_SPIN_FIELD_ORDER;
    hipLaunchKernelGGL((spinor_h2d_kernel<TDev, THost>), dim3(nb), dim3(bs), 0, computeStream(), dst.V(), (float *)dst.Norm(), dst.Stride(),
                       (const THost *)stage, Vh, cs, basisChange(src.gammaBasis, dst.gammaBasis));
  } else {
    if (sizeof(TDev) == 2) errorQuda("16-bit coarse fields unsupported");
    using D = typename Store<TDev>::real;
    hipLaunchKernelGGL((generic_h2d_kernel<D, THost>), dim3(nb), dim3(bs), 0, computeStream(), (D *)dst.V(), dst.Stride(), (const THost *)stage, Vh,
                       dst.nSpin * dst.nColor);
  }
  HIP_CHECK(hipGetLastError());
  HIP_CHECK(hipStreamSynchronize(computeStream()));  // staging buffer is reused by the next transfer
}

template <typename TDev, typename THost> static void d2hParity(ColorSpinorField &dst, const ColorSpinorField &src) {
  const int Vh = src.VolumeCB(), bs = 256, nb = (Vh + bs - 1) / bs;
  const size_t hbytes = (size_t)Vh * src.nSpin * src.nColor * 2 * sizeof(THost);
  void *stage = stagingBuffer(hbytes);
  if (src.nSpin == 4 && src.nColor == 3) {
    const int cs = dst.fieldOrder == QUDA_SPACE_COLOR_SPIN_FIELD_ORDER;
    hipLaunchKernelGGL((spinor_d2h_kernel<TDev, THost>), dim3(nb), dim3(bs), 0, computeStream(), (THost *)stage, src.V(), (const float *)src.Norm(),
                       src.Stride(), Vh, cs, basisChange(src.gammaBasis, dst.gammaBasis));
  } else {
    using D = typename Store<TDev>::real;
    hipLaunchKernelGGL((generic_d2h_kernel<D, THost>), dim3(nb), dim3(bs), 0, computeStream(), (THost *)stage, (const D *)src.V(), src.Stride(), Vh,
                       src.nSpin * src.nColor);
  }
  HIP_CHECK(hipGetLastError());
  HIP_CHECK(hipMemcpyAsync(dst.V(), stage, hbytes, hipMemcpyDeviceToHost, computeStream()));
  HIP_CHECK(hipStreamSynchronize(computeStream()));
  p2pCheck("download of a result field");
}

template <typename TOut, typename TIn> static void d2dParity(ColorSpinorField &dst, const ColorSpinorField &src) {
  const int Vh = src.VolumeCB(), bs = 256, nb = (Vh + bs - 1) / bs;
  acct(src.nSpin == 4 && src.nColor == 3 ? "spinor_d2d_kernel" : "generic_d2d_kernel", (double)Vh * src.nSpin * src.nColor * 2 * (sizeof(TOut) + sizeof(TIn)), src.nSpin == 4 ? "level 0" : "coarse");
  if (src.nSpin == 4 && src.nColor == 3) {
    hipLaunchKernelGGL((spinor_d2d_kernel<TOut, TIn>), dim3(nb), dim3(bs), 0, computeStream(), dst.V(), (float *)dst.Norm(), dst.Stride(), src.V(),
                       (const float *)src.Norm(), src.Stride(), Vh);
  } else {
    using O = typename Store<TOut>::real;
    using I = typename Store<TIn>::real;
    hipLaunchKernelGGL((generic_d2d_kernel<O, I>), dim3(nb), dim3(bs), 0, computeStream(), (O *)dst.V(), dst.Stride(), (const I *)src.V(), src.Stride(),
                       Vh, src.nSpin * src.nColor);
  }
  HIP_CHECK(hipGetLastError());
}

static void copyParity(ColorSpinorField &dst, const ColorSpinorField &src) {
  const bool dd = dst.Location() == QUDA_CUDA_FIELD_LOCATION, sd = src.Location() == QUDA_CUDA_FIELD_LOCATION;
  if (dd && !sd) {
    forPrecision(dst.Precision(), [&](auto td) {
      if (src.Precision() == QUDA_DOUBLE_PRECISION) h2dParity<decltype(td), double>(dst, src);
      else h2dParity<decltype(td), float>(dst, src);
    });
  } else if (!dd && sd) {
    forPrecision(src.Precision(), [&](auto td) {
      if (dst.Precision() == QUDA_DOUBLE_PRECISION) d2hParity<decltype(td), double>(dst, src);
      else d2hParity<decltype(td), float>(dst, src);
    });
  } else if (dd && sd) {
    if (dst.Precision() == src.Precision() && dst.Stride() == src.Stride()) {
      const size_t n = (size_t)src.Stride() * src.nSpin * src.nColor * 2 * src.Precision();
      HIP_CHECK(hipMemcpyAsync(dst.V(), src.V(), n, hipMemcpyDeviceToDevice, computeStream()));
      if (src.Precision() == QUDA_HALF_PRECISION)
        HIP_CHECK(hipMemcpyAsync(dst.Norm(), src.Norm(), (size_t)src.Stride() * sizeof(float), hipMemcpyDeviceToDevice, computeStream()));
    } else {
      forPrecision(src.Precision(), [&](auto ts) { forPrecision(dst.Precision(), [&](auto td) { d2dParity<decltype(td), decltype(ts)>(dst, src); }); });
    }
  } else {
    if (dst.Precision() != src.Precision() || dst.fieldOrder != src.fieldOrder || dst.gammaBasis != src.gammaBasis)
      errorQuda("host-to-host copies with layout change are not supported");
    memcpy(dst.V(), src.V(), (size_t)src.VolumeCB() * src.nSpin * src.nColor * 2 * src.Precision());
  }
}

void copyColorSpinor(ColorSpinorField &dst, const ColorSpinorField &src) {
  if (dst.nSpin != src.nSpin || dst.nColor != src.nColor) errorQuda("spin/colour mismatch %d,%d vs %d,%d", dst.nSpin, dst.nColor, src.nSpin, src.nColor);
  if (dst.SiteSubset() != src.SiteSubset()) errorQuda("site subset mismatch");
  if (dst.VolumeCB() != src.VolumeCB() || dst.Nflavor() != src.Nflavor()) errorQuda("volume mismatch %d (%d flavours) vs %d (%d)", dst.VolumeCB(), dst.Nflavor(), src.VolumeCB(), src.Nflavor());
  if (src.SiteSubset() == QUDA_FULL_SITE_SUBSET) {
    copyParity(dst.Even(), src.Even());
    copyParity(dst.Odd(), src.Odd());
  } else {
    copyParity(dst, src);
  }
  dst.twistFlavor = dst.twistFlavor == QUDA_TWIST_NO || dst.twistFlavor == QUDA_TWIST_INVALID ? src.twistFlavor : dst.twistFlavor;
}

// ---- random source ----
__device__ __forceinline__ float hash_uniform(unsigned long long seed, unsigned long long i) {
  unsigned long long z = seed + 0x9E3779B97F4A7C15ULL * (i + 1);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
  z ^= z >> 31;
  return (float)((z >> 40) * (1.0 / 16777216.0));
}
// vec reals per 16-byte (8-byte) plane element: the padding sites [Vh, stride) of every plane stay zero — the flat BLAS kernels run over them
template <typename real> __global__ void random_kernel(real *v, long n, unsigned long long seed, unsigned long long offset, int vec, int stride, int Vh) {
  const long i = blockIdx.x * (long)blockDim.x + threadIdx.x;
  if (i < n) v[i] = (int)((i / vec) % stride) < Vh ? (real)hash_uniform(seed, offset + i) : (real)0;
}
void spinorRandom(ColorSpinorField &f, unsigned long long seed) {
  if (f.Location() != QUDA_CUDA_FIELD_LOCATION) errorQuda("device field required");
  const int nseg = f.SiteSubset() == QUDA_FULL_SITE_SUBSET ? 2 : 1;
  const long n = (long)f.Stride() * f.Nspin() * f.Ncolor() * 2;
  const unsigned long long rank_off = (unsigned long long)commGrid().rank << 40;
  for (int s = 0; s < nseg; s++) {
    void *p = nseg == 2 ? (s ? f.Odd().V() : f.Even().V()) : f.V();
    const int bs = 256; const long nb = (n + bs - 1) / bs;
    const int vec = f.Nspin() == 4 && f.Precision() == QUDA_SINGLE_PRECISION ? 4 : 2;
    if (f.Precision() == QUDA_DOUBLE_PRECISION) hipLaunchKernelGGL((random_kernel<double>), dim3(nb), dim3(bs), 0, computeStream(), (double *)p, n, seed, rank_off + (unsigned long long)s * n, vec, f.Stride(), f.VolumeCB());
    else if (f.Precision() == QUDA_SINGLE_PRECISION) hipLaunchKernelGGL((random_kernel<float>), dim3(nb), dim3(bs), 0, computeStream(), (float *)p, n, seed, rank_off + (unsigned long long)s * n, vec, f.Stride(), f.VolumeCB());
    else errorQuda("random source needs fp64/fp32 storage");
  }
  HIP_CHECK(hipGetLastError());
}

// ================================================================================================
// GaugeField
// ================================================================================================
GaugeField::GaugeField(const LatticeGeom &g, QudaPrecision prec, QudaReconstructType recon, QudaTboundary tb, double aniso)
    : geom(g), precision(prec), reconstruct(recon), t_boundary(tb), anisotropy(aniso), stride(g.Vh + gaugePadSites()), data(nullptr), tbc_folded(true) {
  if (recon != QUDA_RECONSTRUCT_NO && recon != QUDA_RECONSTRUCT_12 && recon != QUDA_RECONSTRUCT_8) errorQuda("reconstruct %d not supported (18, 12, 8)", recon);
  if (prec == QUDA_HALF_PRECISION && aniso != 1.0) errorQuda("16-bit links need anisotropy 1 (fixed-point range)");
  link_bytes = alignUp((size_t)stride * (int)recon * (int)prec, 1024);
  bytes = 16 * link_bytes;
  HIP_CHECK(qaMalloc(&data, bytes));
}
GaugeField::~GaugeField() { if (data) (void)hipFree(data); }

// boundary slice x_d = L_d - 1 of U_d (both parities) -> contiguous [parity][face index][18] block for the +d neighbour
template <typename THost>
__global__ void gauge_face_pack_kernel(THost *out, const THost *h, LatticeGeom g, int d) {
  const int tid = blockIdx.x * blockDim.x + threadIdx.x;
  const int nf = g.faceCB[d];
  if (tid >= 2 * nf) return;
  const int q = tid >= nf, f = tid - q * nf;
  int c[4], L[3], o[3], n = 0;
  for (int k = 0; k < 4; k++) if (k != d) { L[n] = g.X[k]; o[n] = k; n++; }
  int l = 2 * f;
  const int c0 = l % L[0]; l /= L[0];
  const int c1 = l % L[1]; const int c2 = l / L[1];
  c[d] = g.X[d] - 1;
  c[o[0]] = c0; c[o[1]] = c1; c[o[2]] = c2;
  c[o[0]] += (q + c[0] + c[1] + c[2] + c[3]) & 1;
  const int idx = (((c[3] * g.X[2] + c[2]) * g.X[1] + c[1]) * g.X[0] + c[0]) >> 1;
  const THost *src = h + ((size_t)q * g.Vh + idx) * 18;
  THost *dst = out + (size_t)tid * 18;
  for (int k = 0; k < 18; k++) dst[k] = src[k];
}

// one thread per (parity, site): builds the 8 matrices the stencil needs at that site.  ghost[d] != nullptr: the
// backward link of a site on the x_d = 0 face lives on the -d neighbour rank and is taken from its packed last slice.
template <typename THost> struct GhostLinks { const THost *g[4]; };

// store one link in the device's reconstruct type: 18 / 12 the leading reals as they are, 8 the packed form of device_io.h su3_pack8
template <typename TDev, int R, typename real> __device__ __forceinline__ void store_link(const real *U, void *blk, int stride, int idx) {
  if constexpr (R == 8) {
    real o[8];
    su3_pack8(o, U, (real)(1.0 / PhaseUnit<TDev>::value));
    Planar<TDev, 8>::store(o, blk, stride, idx, nullptr, 0);
  } else {
    Planar<TDev, R>::store(U, blk, stride, idx, nullptr, 0);
  }
}

template <typename TDev, int R, typename THost>
__global__ void gauge_load_kernel(char *data, size_t link_bytes, int stride, const THost *h0, const THost *h1, const THost *h2, const THost *h3,
                                  LatticeGeom g, GhostLinks<THost> ghost) {
  using real = typename Store<TDev>::real;
  const int gid = blockIdx.x * blockDim.x + threadIdx.x;
  if (gid >= 2 * g.Vh) return;
  const int parity = gid >= g.Vh, idx = gid - parity * g.Vh;
  const uint32_t za = g.dXh.div((uint32_t)idx);
  const int xh = idx - (int)za * g.Xh;
  const uint32_t zb = g.dY.div(za);
  const int y = (int)za - (int)zb * g.X[1];
  const int t = (int)g.dZ.div(zb);
  const int z = (int)zb - t * g.X[2];
  const int xodd = (y + z + t + parity) & 1;
  const int xf = 2 * xh + xodd;
  const int Xh = g.Xh, sy = Xh, sz = Xh * g.X[1], st = Xh * g.X[1] * g.X[2];
  int nb[4], face[4];
  nb[0] = xodd ? idx : (xh == 0 ? idx + (Xh - 1) : idx - 1);
  nb[1] = y == 0 ? idx + (g.X[1] - 1) * sy : idx - sy;
  nb[2] = z == 0 ? idx + (g.X[2] - 1) * sz : idx - sz;
  nb[3] = t == 0 ? idx + (g.X[3] - 1) * st : idx - st;
  face[0] = ((t * g.X[2] + z) * g.X[1] + y) >> 1;
  face[1] = ((t * g.X[2] + z) * g.X[0] + xf) >> 1;
  face[2] = ((t * g.X[1] + y) * g.X[0] + xf) >> 1;
  face[3] = ((z * g.X[1] + y) * g.X[0] + xf) >> 1;
  const int coord[4] = {xf, y, z, t};
  const THost *h[4] = {h0, h1, h2, h3};
  char *base = data + (size_t)parity * 8 * link_bytes;
#pragma unroll
  for (int mu = 0; mu < 4; mu++) {
    real U[18];
    const THost *f = h[mu] + ((size_t)parity * g.Vh + idx) * 18;
#pragma unroll
    for (int k = 0; k < 18; k++) U[k] = (real)f[k];
    store_link<TDev, R>(U, base + (size_t)(2 * mu) * link_bytes, stride, idx);
    const THost *bk = (ghost.g[mu] && coord[mu] == 0) ? ghost.g[mu] + ((size_t)(1 - parity) * g.faceCB[mu] + face[mu]) * 18
                                                       : h[mu] + ((size_t)(1 - parity) * g.Vh + nb[mu]) * 18;
#pragma unroll
    for (int r = 0; r < 3; r++)
#pragma unroll
      for (int c = 0; c < 3; c++) {  // dagger
        U[r * 6 + c * 2] = (real)bk[c * 6 + r * 2];
        U[r * 6 + c * 2 + 1] = -(real)bk[c * 6 + r * 2 + 1];
      }
    store_link<TDev, R>(U, base + (size_t)(2 * mu + 1) * link_bytes, stride, idx);
  }
}

template <typename TDev, int R, typename THost> static void gaugeLoad(GaugeField &U, void *const h_gauge[4]) {
  const LatticeGeom &g = U.geom;
  const size_t n = (size_t)g.V * 18 * sizeof(THost);
  size_t ghost_bytes = 0;
  // links of the -d neighbour are needed wherever dimension d is split over ranks; QUDA_AMD_FORCE_GAUGE_HALO=1 also sends a
  // self-partitioned dimension (qudaAmdSetPartitionMask) through the same pack / exchange / ghost-index path, for testing
  static const bool force = getenv("QUDA_AMD_FORCE_GAUGE_HALO") != nullptr;
  auto split = [&](int d) { return commGrid().dims[d] > 1 || (force && commGrid().forced[d]); };
  for (int d = 0; d < 4; d++) if (split(d)) ghost_bytes += 2 * (size_t)2 * g.faceCB[d] * 18 * sizeof(THost);
  char *stage = (char *)stagingBuffer(4 * n + ghost_bytes);
  hipStream_t s = computeStream();
  for (int d = 0; d < 4; d++) HIP_CHECK(hipMemcpyAsync(stage + d * n, h_gauge[d], n, hipMemcpyHostToDevice, s));
  GhostLinks<THost> ghost;
  std::vector<HaloMsg> msgs;
  char *p = stage + 4 * n;
  for (int d = 0; d < 4; d++) {
    ghost.g[d] = nullptr;
    if (!split(d)) continue;
    const size_t fb = (size_t)2 * g.faceCB[d] * 18 * sizeof(THost);
    THost *sendb = (THost *)p; p += fb;
    THost *recvb = (THost *)p; p += fb;
    const int nt = 2 * g.faceCB[d];
    hipLaunchKernelGGL((gauge_face_pack_kernel<THost>), dim3((nt + 255) / 256), dim3(256), 0, s, sendb, (const THost *)(stage + d * n), g, d);
    HIP_CHECK(hipGetLastError());
    msgs.push_back({d, +1, sendb, recvb, fb});  // my last slice goes forward; I receive my -d neighbour's last slice
    ghost.g[d] = recvb;
  }
  if (!msgs.empty()) commExchange(msgs, s);
  const int bs = 256, nb = (2 * g.Vh + bs - 1) / bs;
  hipLaunchKernelGGL((gauge_load_kernel<TDev, R, THost>), dim3(nb), dim3(bs), 0, s, (char *)U.data, U.link_bytes, U.stride, (const THost *)stage,
                     (const THost *)(stage + n), (const THost *)(stage + 2 * n), (const THost *)(stage + 3 * n), g, ghost);
  HIP_CHECK(hipGetLastError());
  HIP_CHECK(hipStreamSynchronize(s));
}

void GaugeField::loadQDP(void *const h_gauge[4], QudaPrecision cpu_prec) {
  forLinkType(*this, [&](auto t, auto r) {
    if (cpu_prec == QUDA_DOUBLE_PRECISION) gaugeLoad<decltype(t), decltype(r)::value, double>(*this, h_gauge);
    else gaugeLoad<decltype(t), decltype(r)::value, float>(*this, h_gauge);
  });
}

// device-to-device copy of all 16 link blocks with precision change (same reconstruct): the 16-bit links of the multigrid's
// half-precision smoother are made from the resident fp32 field, the host copy is not kept
template <typename TOut, typename TIn, int R>
__global__ void gauge_convert_kernel(char *out, size_t out_link_bytes, const char *in, size_t in_link_bytes, int stride, int Vh) {
  const int gid = blockIdx.x * blockDim.x + threadIdx.x;
  if (gid >= 16 * Vh) return;
  const int blk = gid / Vh, idx = gid - blk * Vh;
  typename Store<TIn>::real u[R];
  Planar<TIn, R>::load(u, in + (size_t)blk * in_link_bytes, stride, idx, nullptr, 0);
  typename Store<TOut>::real v[R];
#pragma unroll
  for (int k = 0; k < R; k++) v[k] = (typename Store<TOut>::real)u[k];
  if (R == 8) {   // the two phases are stored in the unit of their precision (16-bit: phase / pi)
    const typename Store<TOut>::real f = (typename Store<TOut>::real)(PhaseUnit<TIn>::value / PhaseUnit<TOut>::value);
    v[0] *= f; v[1] *= f;
  }
  Planar<TOut, R>::store(v, out + (size_t)blk * out_link_bytes, stride, idx, nullptr, 0);
}
void GaugeField::copyFrom(const GaugeField &src) {
  if (!(src.geom == geom) || src.reconstruct != reconstruct) errorQuda("gauge copy: geometry / reconstruct mismatch");
  if (src.precision != QUDA_SINGLE_PRECISION || precision != QUDA_HALF_PRECISION) errorQuda("gauge copy: fp32 -> 16-bit only");
  const int bs = 256, nb = (16 * geom.Vh + bs - 1) / bs;
  forLinkType(*this, [&](auto, auto r) {   // the precisions are fixed above: only the reconstruct varies
    hipLaunchKernelGGL((gauge_convert_kernel<short, float, decltype(r)::value>), dim3(nb), dim3(bs), 0, computeStream(), (char *)data, link_bytes, (const char *)src.data, src.link_bytes, stride, geom.Vh);
  });
  HIP_CHECK(hipGetLastError());
}

}  // namespace quda
