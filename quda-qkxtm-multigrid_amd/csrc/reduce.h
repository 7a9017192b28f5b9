// reduce.h — the hand-off that ends a grid-wide reduction: the work-group that arrives last adds what the others left in memory.
#pragma once
#include <hip/hip_runtime.h>

namespace quda {

// Called by every thread of every work-group, after the group has written its partial sums with agent-scope atomic stores.  Bumps the
// completion counter (zero between launches) and runs tail() — all threads of it — in the one group that finds every other group's
// bump before its own; that group puts the counter back to zero afterwards, so the next launch of the stream needs no memset.
//
// The partials are sc1 (write-through) stores.  The storing waves wait for their acknowledgement BEFORE the barrier, so the counter
// bump behind the barrier cannot overtake them on their way to memory (the last group may sit on another XCD with its own L2); a
// workgroup-scope fence emits nothing here, and a release on the bump would write back the whole dirty L2 (buffer_wbl2), which
// orders nothing these write-through stores need.  The wait is inline asm because the compiler may drop a builtin wait it believes
// redundant.  The last group then reads the partials with sc1 loads (agent-scope atomic loads in tail()) behind its own barrier —
// the drained-sc1 hand-off of MI355X_MICROARCH.md.
template <typename Tail> __device__ __forceinline__ void lastBlockFinishes(unsigned *count, Tail &&tail) {
  __shared__ int isLast;
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (threadIdx.x == 0) isLast = __hip_atomic_fetch_add(count, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == gridDim.x - 1;
  __syncthreads();
  if (isLast) {
    tail();
    if (threadIdx.x == 0) __hip_atomic_store(count, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

}  // namespace quda
