// Device helpers shared by component_kernels.hip and topology_kernels.hip: the lock-free union-find over int32 parents
// in which a parent is ALWAYS SMALLER than its child (the root of a set is its smallest index), and the wave scan both
// use for their per-block counts.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace vgt
{
__device__ __forceinline__ int32_t LoadLabel(const int32_t* label, int32_t i)
{
  return __atomic_load_n(label + i, __ATOMIC_RELAXED);
}

__device__ __forceinline__ int32_t FindRoot(const int32_t* label, int32_t a)
{
  // parents are smaller than their children: the walk strictly descends and ends at the set's smallest index.  A stale
  // read yields an earlier parent -- still an ancestor
  for (int32_t p = LoadLabel(label, a); p != a; p = LoadLabel(label, a)) a = p;
  return a;
}

__device__ __forceinline__ void Union(int32_t* label, int32_t a, int32_t b)
{
  for (;;)
  {
    a = FindRoot(label, a);
    b = FindRoot(label, b);
    if (a == b) return;
    if (a < b)
    {
      const int32_t t = a;
      a = b;
      b = t;
    }
    // a > b: hang a below b.  If a was no root any more, label[a] is now min(old, b) and old (< a) still has to be
    // joined with b: go on with it.
    const int32_t old = atomicMin(label + a, b);
    if (old == a) return;
    a = old;
  }
}

// Inclusive prefix sum over the lanes of a wave.
__device__ __forceinline__ int WaveInclusiveScan(int value, int lane)
{
  for (int d = 1; d < 64; d <<= 1)
  {
    const int other = __shfl_up(value, d);
    if (lane >= d) value += other;
  }
  return value;
}
}  // namespace vgt
