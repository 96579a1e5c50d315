// The small pieces of the reference's voxel walk that more than one translation unit restates: the index conversion, the
// per-axis boundary parameter, the in-grid test and the linear index.  Shared by the raycast voxelizer
// (voxelizer_kernels.hip) and the segment queries (segment_kernels.hip), so that both walk the same cells bit for bit.
// Both translation units are compiled with -ffp-contract=off and correctly rounded division and sqrt.
#pragma once

#include "vgt_internal.hpp"

#include <cmath>

namespace vgt
{
namespace
{
template <typename Real>
struct RaycastTraits;
// ToIndex: what `static_cast<integer>(std::floor(x))` of the reference gives where IT runs.  The float walk restates
// the device kernels (cuda_voxelization_helpers.cu:140-144, :229-240): on the device the cast saturates and turns NaN
// into 0, which is what v_cvt_i32_f32 does as well.  The double walk restates the CPU voxelizer
// (cpu_pointcloud_voxelization.cpp:107, :181, :294-297), whose cast on x86-64 answers "indefinite" (the most negative
// integer) to NaN: never a voxel of the grid.  It matters for a ray of length zero seen from outside the grid (its
// direction is 0 / 0 and its entry point NaN): the device kernels start it in voxel (0, 0, 0), the CPU voxelizer drops it.
template <>
struct RaycastTraits<float>
{
  using Grid = RaycastGridF32;
  static constexpr float kFlat = 1e-10f;
  static constexpr float kNudge = 1e-10f;
  // (spelled out: a bare float -> int cast of NaN or of an out-of-range value is undefined in C++, whatever v_cvt_i32_f32
  // does with it; the compiler folds this back into the one conversion instruction -- the same contract as the oracle's
  // device_index_f32)
  static __device__ __forceinline__ int32_t ToIndex(float floored)
  {
    if (isnan(floored)) return 0;
    if (floored >= 2147483648.0f) return INT32_MAX;
    if (floored <= -2147483648.0f) return INT32_MIN;
    return static_cast<int32_t>(floored);
  }
};
template <>
struct RaycastTraits<double>
{
  using Grid = RaycastGridF64;
  static constexpr double kFlat = 1e-10;
  static constexpr double kNudge = 1e-10;
  static __device__ __forceinline__ int32_t ToIndex(double floored)
  {
    // The CPU voxelizer's index is 64 bits wide (the oracle's host_index_f64): NaN and everything outside int64 is x86's
    // "indefinite", the most negative integer; a value inside int64 but outside int32 keeps its sign -- all that matters
    // about an index that far outside the grid is which way the walk steps away from it.
    if (!(floored > -9223372036854775808.0 && floored < 9223372036854775808.0)) return INT32_MIN;
    if (floored >= 2147483648.0) return INT32_MAX;
    if (floored <= -2147483648.0) return INT32_MIN;
    return static_cast<int32_t>(floored);
  }
};

template <typename Real>
__device__ __forceinline__ Real AxisT(Real point, Real ray, Real lo, Real hi)
{
  // GetAxisTValue, cuda_voxelization_helpers.cu:52-71
  if (ray > Real(0)) return fabs((hi - point) / ray);
  if (ray < -Real(0)) return fabs((point - lo) / ray);
  return static_cast<Real>(INFINITY);
}

__device__ __forceinline__ bool InGrid(const int32_t idx[3], const int32_t counts[3])
{
  return idx[0] >= 0 && idx[0] < counts[0] && idx[1] >= 0 && idx[1] < counts[1] && idx[2] >= 0 &&
         idx[2] < counts[2];
}

__device__ __forceinline__ int64_t CellIndex(const int32_t idx[3], const int32_t counts[3])
{
  return (static_cast<int64_t>(idx[0]) * counts[1] + idx[1]) * counts[2] + idx[2];
}
}  // namespace
}  // namespace vgt
