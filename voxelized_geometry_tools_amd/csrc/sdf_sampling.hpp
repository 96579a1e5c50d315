// Device code shared by the SDF consumers (cell_kernels.hip: estimate, gradients, projection; body_kernels.hip: sphere
// models): the trilinear distance estimate of SignedDistanceField::EstimateLocationDistance in its three steps and the
// coarse gradient of one voxel, each in the one operation order the oracle restates (cell_kernels.hip's header comments
// give the order and the reference lines).  Every translation unit that includes this is built without contraction.
#pragma once

#include "vgt_internal.hpp"

namespace vgt
{
namespace
{
struct Rotation
{
  double m[9];
  int enabled;
};

struct GridFromWorld
{
  double m[16];
  int enabled;
};

// The per-voxel rule, shared by the whole-field kernel and the projection loop (voxel i = x*sx + y*sy + z).  Returns
// false, with NaN in all three components, where the reference's GradientQuery is empty.
__device__ __forceinline__ bool CoarseGradientAt(const float* __restrict__ sdf, int nx, int ny, int nz, int64_t sx,
                                                 int64_t sy, double resolution, int enable_edge_gradients,
                                                 const Rotation& rot, int64_t i, int x, int y, int z, double& gx,
                                                 double& gy, double& gz)
{
  gx = 0.0;
  gy = 0.0;
  gz = 0.0;
  if (x > 0 && y > 0 && z > 0 && x < nx - 1 && y < ny - 1 && z < nz - 1)
  {
    const double inv_twice_resolution = 1.0 / (2.0 * resolution);
    gx = static_cast<double>(sdf[i + sx] - sdf[i - sx]) * inv_twice_resolution;
    gy = static_cast<double>(sdf[i + sy] - sdf[i - sy]) * inv_twice_resolution;
    gz = static_cast<double>(sdf[i + 1] - sdf[i - 1]) * inv_twice_resolution;
  }
  else if (enable_edge_gradients)
  {
    const int lx = max(0, x - 1), hx = min(nx - 1, x + 1);
    const int ly = max(0, y - 1), hy = min(ny - 1, y + 1);
    const int lz = max(0, z - 1), hz = min(nz - 1, z + 1);
    const double x_increment = static_cast<double>(hx - lx) * resolution;
    const double y_increment = static_cast<double>(hy - ly) * resolution;
    const double z_increment = static_cast<double>(hz - lz) * resolution;
    if (x_increment > 0.0)
      gx = (static_cast<double>(sdf[i + (hx - x) * sx]) - static_cast<double>(sdf[i - (x - lx) * sx])) *
           (1.0 / x_increment);
    if (y_increment > 0.0)
      gy = (static_cast<double>(sdf[i + (hy - y) * sy]) - static_cast<double>(sdf[i - (y - ly) * sy])) *
           (1.0 / y_increment);
    if (z_increment > 0.0)
      gz = (static_cast<double>(sdf[i + (hz - z)]) - static_cast<double>(sdf[i - (z - lz)])) * (1.0 / z_increment);
  }
  else
  {
    gx = gy = gz = __longlong_as_double(0x7ff8000000000000ll);
    return false;
  }
  if (rot.enabled)
  {
    const double wx = rot.m[0] * gx + rot.m[1] * gy + rot.m[2] * gz;
    const double wy = rot.m[3] * gx + rot.m[4] * gy + rot.m[5] * gz;
    const double wz = rot.m[6] * gx + rot.m[7] * gy + rot.m[8] * gz;
    gx = wx;
    gy = wy;
    gz = wz;
  }
  return true;
}

struct EstimateResult
{
  double value;
  bool has_value;
};

__device__ __forceinline__ void AxisInterpolationIndices(int initial, int size, double offset, int& lower, int& upper)
{
  lower = initial;
  upper = initial;
  if (offset >= 0.0)
  {
    upper = initial + 1;
    if (upper >= size)
    {
      upper = initial;
      lower = initial - 1;
      if (lower < 0) lower = initial;
    }
  }
  else
  {
    lower = initial - 1;
    if (lower < 0)
    {
      upper = initial + 1;
      lower = initial;
      if (upper >= size) upper = initial;
    }
  }
}

__device__ __forceinline__ double CorrectedCenterDistance(const float* __restrict__ sdf, int64_t index, double resolution)
{
  const double nominal = static_cast<double>(sdf[index]);
  const double offset = resolution * 0.5;
  return (nominal >= 0.0) ? nominal - offset : nominal + offset;
}

__device__ __forceinline__ double Lerp(double a, double b, double t) { return a * (1.0 - t) + b * t; }

// EstimateDistance in its three steps, so that a caller that evaluates it again and again near one place (the
// projection loop) can keep the loaded corners while their indices stay the same.
struct CellOfLocation
{
  double g[3];                 // the location in the grid frame
  int ix, iy, iz;              // the cell it lies in
  int lx, ux, ly, uy, lz, uz;  // GetAxisInterpolationIndices per axis
};

struct CornerDistances
{
  double mmm, mmp, mpm, mpp, pmm, pmp, ppm, ppp;  // GetCorrectedCenterDistance at (x, y, z) in {lower, upper}^3
};

// false: the location is not in the grid (also for NaN and infinite coordinates)
__device__ __forceinline__ bool LocateCell(int nx, int ny, int nz, double resolution, const GridFromWorld& xf, double x,
                                           double y, double z, CellOfLocation& c)
{
  c.g[0] = x;
  c.g[1] = y;
  c.g[2] = z;
  if (xf.enabled)
  {
    const double* M = xf.m;
    c.g[0] = M[0] * x + M[4] * y + M[8] * z + M[12];
    c.g[1] = M[1] * x + M[5] * y + M[9] * z + M[13];
    c.g[2] = M[2] * x + M[6] * y + M[10] * z + M[14];
  }
  const double inv = 1.0 / resolution;
  const double fx = floor(c.g[0] * inv), fy = floor(c.g[1] * inv), fz = floor(c.g[2] * inv);
  if (!(fx >= 0.0 && fx < nx && fy >= 0.0 && fy < ny && fz >= 0.0 && fz < nz)) return false;  // also rejects NaN
  c.ix = static_cast<int>(fx);
  c.iy = static_cast<int>(fy);
  c.iz = static_cast<int>(fz);
  const double cx = (static_cast<double>(c.ix) + 0.5) * resolution;
  const double cy = (static_cast<double>(c.iy) + 0.5) * resolution;
  const double cz = (static_cast<double>(c.iz) + 0.5) * resolution;
  AxisInterpolationIndices(c.ix, nx, c.g[0] - cx, c.lx, c.ux);
  AxisInterpolationIndices(c.iy, ny, c.g[1] - cy, c.ly, c.uy);
  AxisInterpolationIndices(c.iz, nz, c.g[2] - cz, c.lz, c.uz);
  return true;
}

__device__ __forceinline__ CornerDistances LoadCorners(const float* __restrict__ sdf, int ny, int nz, double resolution,
                                                       const CellOfLocation& c)
{
  const int64_t sx = static_cast<int64_t>(ny) * nz, sy = nz;
  auto at = [&](int a, int b, int d) { return CorrectedCenterDistance(sdf, a * sx + b * sy + d, resolution); };
  CornerDistances k;
  k.mmm = at(c.lx, c.ly, c.lz), k.mmp = at(c.lx, c.ly, c.uz), k.mpm = at(c.lx, c.uy, c.lz), k.mpp = at(c.lx, c.uy, c.uz);
  k.pmm = at(c.ux, c.ly, c.lz), k.pmp = at(c.ux, c.ly, c.uz), k.ppm = at(c.ux, c.uy, c.lz), k.ppp = at(c.ux, c.uy, c.uz);
  return k;
}

__device__ __forceinline__ double InterpolateCorners(const CellOfLocation& c, const CornerDistances& k, double resolution)
{
  const double low_x = (static_cast<double>(c.lx) + 0.5) * resolution;
  const double low_y = (static_cast<double>(c.ly) + 0.5) * resolution;
  const double low_z = (static_cast<double>(c.lz) + 0.5) * resolution;
  const double tx = (c.g[0] - low_x) / ((low_x + resolution) - low_x);
  const double ty = (c.g[1] - low_y) / ((low_y + resolution) - low_y);
  const double tz = (c.g[2] - low_z) / ((low_z + resolution) - low_z);
  const double mm = Lerp(k.mmm, k.pmm, tx), mp = Lerp(k.mmp, k.pmp, tx), pm = Lerp(k.mpm, k.ppm, tx),
               pp = Lerp(k.mpp, k.ppp, tx);
  const double lo = Lerp(mm, pm, ty), hi = Lerp(mp, pp, ty);
  return Lerp(lo, hi, tz);
}

__device__ EstimateResult EstimateDistance(const float* __restrict__ sdf, int nx, int ny, int nz, double resolution,
                                           const GridFromWorld& xf, double x, double y, double z)
{
  EstimateResult r{0.0, false};
  CellOfLocation c;
  if (!LocateCell(nx, ny, nz, resolution, xf, x, y, z, c)) return r;
  r.value = InterpolateCorners(c, LoadCorners(sdf, ny, nz, resolution, c), resolution);
  r.has_value = true;
  return r;
}

inline GridFromWorld MakeGridFromWorld(const double* grid_from_world_host)
{
  GridFromWorld xf;
  xf.enabled = grid_from_world_host ? 1 : 0;
  for (int k = 0; k < 16; k++) xf.m[k] = grid_from_world_host ? grid_from_world_host[k] : 0.0;
  return xf;
}

inline Rotation MakeRotation(const double* rotation_host)
{
  Rotation rot;
  rot.enabled = rotation_host ? 1 : 0;
  for (int k = 0; k < 9; k++) rot.m[k] = rotation_host ? rotation_host[k] : 0.0;
  return rot;
}
}  // namespace
}  // namespace vgt
