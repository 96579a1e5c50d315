// Device code shared by the kernels that check a sphere model against an SDF (body_kernels.hip: configurations given as
// link poses; motion_kernels.hip: the samples of motions, poses in LDS): one sphere's clearance at its world centre, the
// order of the spheres of a configuration, its reduction over a lane segment and the status rule -- each the one
// definition of include/vgt_hip.h, vgt_hip_check_spheres, so that both kernels give the same bits.  The kernels keep their
// own loops: where the sphere and its pose come from differs.
#pragma once

#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Wunused-function"
#include "sdf_sampling.hpp"
#pragma clang diagnostic pop
#include "vgt_internal.hpp"

namespace vgt
{
namespace
{
constexpr uint8_t kBodyClear = 0, kBodyCollision = 1, kBodyNoValue = 2;

// (clearance, index) of a better than of b: smaller clearance, then smaller index; index < 0 = no candidate
__device__ __forceinline__ bool BetterSphere(double ca, int ia, double cb, int ib)
{
  return ia >= 0 && (ib < 0 || ca < cb || (ca == cb && ia < ib));
}

// The world centre of a sphere at (x, y, z) in the frame of a link whose pose has its element (column c, row r) at
// m[c * column_stride + r * row_stride].
__device__ __forceinline__ void SphereCentre(const double* m, int column_stride, int row_stride, double x, double y, double z,
                                             double (&w)[3])
{
#pragma unroll
  for (int r = 0; r < 3; r++)
    w[r] = ((m[r * row_stride] * x + m[column_stride + r * row_stride] * y) + m[2 * column_stride + r * row_stride] * z) +
           m[3 * column_stride + r * row_stride];
}

// The clearance of a sphere of `radius` around w, and the cell of w; false: w is not in the grid, no value.
__device__ __forceinline__ bool SphereClearance(const float* __restrict__ sdf, int nx, int ny, int nz, double resolution,
                                                const GridFromWorld& xf, const double (&w)[3], double radius,
                                                CellOfLocation& c, double& clearance)
{
  if (!LocateCell(nx, ny, nz, resolution, xf, w[0], w[1], w[2], c)) return false;
  const double d = InterpolateCorners(c, LoadCorners(sdf, ny, nz, resolution, c), resolution);
  clearance = d - radius;
  return true;
}

// The best (clearance, sphere) of the `width` lanes of a segment (a power of two, segments aligned), on every lane of it.
__device__ __forceinline__ void BestSphereOfSegment(int width, double& winner, int& winner_sphere)
{
  for (int offset = width >> 1; offset > 0; offset >>= 1)
  {
    const double other = __shfl_xor(winner, offset);
    const int other_sphere = __shfl_xor(winner_sphere, offset);
    if (BetterSphere(other, other_sphere, winner, winner_sphere))
    {
      winner = other;
      winner_sphere = other_sphere;
    }
  }
}

// The status of a configuration from its counts and its worst sphere (-1: none).
__device__ __forceinline__ uint8_t SphereModelStatus(int num_below, int num_outside, int outside_is_collision,
                                                     int winner_sphere)
{
  uint8_t status = kBodyNoValue;
  if (num_below > 0 || (outside_is_collision && num_outside > 0))
    status = kBodyCollision;
  else if (winner_sphere >= 0)
    status = kBodyClear;
  return status;
}
}  // namespace
}  // namespace vgt
