// dispatch.h — run-time precision and link type to template arguments, and the launch of a site kernel: generic lambdas with tag
// arguments, as blas.hip's forShape / forAtLeast.  Host code; the stencil has its own (dslash.hip dispatchRecon).
#pragma once

#include <type_traits>

#include "fields.h"

namespace quda {

// fn(T()) with T the storage type of a device field of that precision: double, float or short
template <typename Fn> void forPrecision(QudaPrecision prec, Fn &&fn) {
  switch (prec) {
    case QUDA_DOUBLE_PRECISION: fn(double()); break;
    case QUDA_SINGLE_PRECISION: fn(float()); break;
    case QUDA_HALF_PRECISION: fn(short()); break;
    default: errorQuda("bad precision %d", prec);
  }
}

// fn(T(), std::integral_constant<int, R>()) with T the storage type of the links and R their stored reals: 18, 12 or 8
template <typename Fn> void forLinkType(const GaugeField &U, Fn &&fn) {
  const auto recon = [&](auto t) {
    if (U.reconstruct == QUDA_RECONSTRUCT_12) fn(t, std::integral_constant<int, 12>());
    else if (U.reconstruct == QUDA_RECONSTRUCT_8) fn(t, std::integral_constant<int, 8>());
    else fn(t, std::integral_constant<int, 18>());
  };
  switch (U.precision) {
    case QUDA_DOUBLE_PRECISION: recon(double()); break;
    case QUDA_SINGLE_PRECISION: recon(float()); break;
    case QUDA_HALF_PRECISION: recon(short()); break;
    default: errorQuda("bad gauge precision %d", U.precision);
  }
}

// one thread per site and parity: blocks of bs threads over 2 Vh sites on the compute stream, the launch checked
template <typename... Params, typename... Args> void launchSites(void (*kernel)(Params...), int Vh, int bs, Args &&...args) {
  hipLaunchKernelGGL(kernel, dim3((2 * Vh + bs - 1) / bs), dim3(bs), 0, computeStream(), static_cast<Params>(args)...);
  HIP_CHECK(hipGetLastError());
}

}  // namespace quda
