// lex_index.h — checkerboard (parity, index) -> lexicographic site index (x fastest) of the local lattice, shared by the QKXTM
// copy kernels (qkxtm.hip) and the two-point propagator packing (contract.hip).
#pragma once

#include <hip/hip_runtime.h>

namespace quda {

__device__ __forceinline__ long lex_of(int idx, int parity, int Xh, int Y, int Z) {
  int l = idx / Xh;
  const int y = l % Y; l /= Y;
  const int z = l % Z, t = l / Z;
  return 2l * idx + ((y + z + t + parity) & 1);   // checkerboard index = lexicographic index / 2
}

}  // namespace quda
