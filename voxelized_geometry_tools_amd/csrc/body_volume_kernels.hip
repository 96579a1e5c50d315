// Sphere models into voxel grids and onto point clouds for gfx950: which cells, or which points, the spheres of B
// configurations cover, and the least configuration that does.  Rules and every output: include/vgt_hip.h,
// vgt_hip_rasterize_spheres and vgt_hip_spheres_cover_points.  Both answers are minima over a set, so neither depends on
// the order of the work or on where an atomic lands.
//
// RasterizeSpheresKernel, a scatter.  Persistent waves (at most kVolumeMaxWorkgroups workgroups of 4); wave v of the
// launch takes the pairs k = b * S + s = v, v + waves, ... in ascending order, so that low configurations tend to claim
// cells first.  Every lane computes the pair's centre c in the grid frame and R (wave-uniform).  Per axis the wave
// derives a range of cell indices that contains every cell the rule can cover,
//     [floor(((c_a - R) / resolution - 0.5) - slack), floor(((c_a + R) / resolution - 0.5) + slack)],
//     slack = 1 + ((|c_a| + R) / resolution) * 2^-48,
// i.e. the exact range widened by one cell, plus a term that stays below one cell until the sphere is 2^48 cells away or
// wide: it bounds, 32 times over, the rounding of the few operations of the range and of `covers` itself (each relative
// 2^-53 of magnitudes <= (|c_a| + R) / resolution + n_a), so a huge sphere whose surface crosses the grid is not pruned
// wrongly.  The range is clamped to [0, n_a - 1] in double BEFORE any conversion to int (a NaN from inf - inf falls to
// the full range); a range that lies outside the grid is empty.  The 64 lanes walk the box with Z fastest, every lane
// evaluates the literal `covers` for its cell -- the box only prunes, the comparison decides -- and lowers the entry
// with an unsigned atomicMin.
// A plain load comes first and the atomic is skipped when the entry is already <= the key.  Entries only ever fall
// during a launch, so a stale read (this CU's L1 and this XCD's L2 are not refreshed by other CUs' atomics) can only
// show a value that is too HIGH and cause a redundant atomic, never a skipped one that was needed, never a wrong result.
// That is what keeps a long motion through the same space from issuing one atomic per (cell, configuration).
// A whole box stays on one wave (no split of large boxes: DESIGN.md 4k, Not built).
//
// CoverPointsKernel, a gather.  One lane per point, 256 points per workgroup, grid-stride trips.  For b ascending the
// workgroup computes the world centres and R of configuration b's spheres cooperatively, 256 at a time, into LDS
// (4 doubles per sphere, 8 KiB; R = -1 marks a sphere that is not usable); every lane that is not settled scans the chunk
// in ascending s -- all lanes read the same LDS address, a broadcast -- records the first sphere that covers its point
// and is then settled for good: ascending b, then s, makes the first found the least.  The workgroup leaves the loops
// when __syncthreads_and says all of its points are settled; every barrier is reached by the whole workgroup (trip,
// configuration and chunk counts depend on blockIdx and the arguments alone).
//
// In bounds by construction: a link outside [0, L) makes the sphere not usable before any pose address is formed; the
// grid is addressed only through indices clamped into it, by usable spheres; a lane with i >= N forms no address.
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Wunused-function"
#include "sdf_sampling.hpp"
#pragma clang diagnostic pop
#include "vgt_internal.hpp"

#include <cmath>

namespace vgt
{
namespace
{
constexpr int kVolumeThreads = 256;
constexpr int kVolumeWaves = kVolumeThreads / 64;
constexpr int kVolumeTableMax = 256;  // spheres of the rasterizer's LDS table, 36 B each: 9 KiB
constexpr int kVolumeChunk = 256;     // spheres per LDS chunk of the point kernel, 32 B each: 8 KiB
// Workgroups of a launch: eight per CU on 256 CUs, about what is resident; the rest by striding.
constexpr int kVolumeMaxWorkgroups = 2048;

__device__ __forceinline__ bool Finite(double v) { return fabs(v) < __longlong_as_double(0x7ff0000000000000ll); }

// The world centre and R of sphere (x, y, z, radius) on `link` in configuration b; false: not usable (then no pose
// address was formed for a link out of range).
__device__ __forceinline__ bool WorldSphere(const SphereVolumeModel& model, int64_t b, double x, double y, double z,
                                            double radius, int32_t link, double w[3], double& R)
{
  if (link < 0 || link >= model.num_links) return false;
  const double* m = model.poses + (b * model.num_links + link) * 16;
  for (int r = 0; r < 3; r++) w[r] = ((m[r] * x + m[4 + r] * y) + m[8 + r] * z) + m[12 + r];
  R = radius + model.padding;
  return Finite(w[0]) && Finite(w[1]) && Finite(w[2]) && Finite(R) && R >= 0.0;
}

// The clamped range of one axis as doubles; false: empty.
__device__ __forceinline__ bool AxisRange(double c, double R, double resolution, int n, double& lo, double& hi)
{
  const double slack = 1.0 + ((fabs(c) + R) / resolution) * 0x1p-48;
  lo = floor(((c - R) / resolution - 0.5) - slack);
  hi = floor(((c + R) / resolution - 0.5) + slack);
  const double last = static_cast<double>(n - 1);
  lo = (lo >= 0.0) ? lo : 0.0;    // (NaN: the whole axis)
  hi = (hi <= last) ? hi : last;  // (NaN: the whole axis)
  return lo <= hi;
}

// kCount (the testing library's counting runs only): also adds the (cell, sphere) tests made, those that covered and the
// atomics issued to counters[0 .. 2], one atomicAdd each per wave.
template <bool kCount>
__global__ __launch_bounds__(kVolumeThreads) void RasterizeSpheresKernel(unsigned* first, int nx, int ny,
                                                                         int nz, double resolution,
                                                                         const GridFromWorld xf,
                                                                         const SphereVolumeModel model, unsigned base,
                                                                         unsigned long long* counters)
{
  __shared__ double table_xyzr[kVolumeTableMax * 4];
  __shared__ int32_t table_link[kVolumeTableMax];

  const int S = model.num_spheres;
  const int lane = static_cast<int>(threadIdx.x) & 63, wave = static_cast<int>(threadIdx.x) >> 6;
  const bool table_in_lds = S <= kVolumeTableMax;
  if (table_in_lds)
  {
    for (int i = static_cast<int>(threadIdx.x); i < S * 4; i += kVolumeThreads) table_xyzr[i] = model.xyzr[i];
    for (int i = static_cast<int>(threadIdx.x); i < S; i += kVolumeThreads) table_link[i] = model.link[i];
    __syncthreads();
  }
  // (no barrier below this line: the waves of a workgroup may make different numbers of trips)
  const int64_t pairs = static_cast<int64_t>(model.num_configurations) * S;
  const int64_t waves = static_cast<int64_t>(gridDim.x) * kVolumeWaves;
  const int64_t sx = static_cast<int64_t>(ny) * nz;
  unsigned long long tests = 0, covering = 0, atomics = 0;  // (kCount: this lane's)
  for (int64_t k = static_cast<int64_t>(blockIdx.x) * kVolumeWaves + wave; k < pairs; k += waves)
  {
    const int64_t b = k / S;
    const int s = static_cast<int>(k - b * S);
    double x, y, z, radius;
    int32_t link;
    if (table_in_lds)
    {
      x = table_xyzr[4 * s], y = table_xyzr[4 * s + 1], z = table_xyzr[4 * s + 2], radius = table_xyzr[4 * s + 3];
      link = table_link[s];
    }
    else
    {
      const double* p = model.xyzr + 4 * static_cast<int64_t>(s);
      x = p[0], y = p[1], z = p[2], radius = p[3];
      link = model.link[s];
    }
    double w[3], R;
    if (!WorldSphere(model, b, x, y, z, radius, link, w, R)) continue;
    double c[3] = {w[0], w[1], w[2]};
    if (xf.enabled)
    {
      const double* M = xf.m;
      c[0] = M[0] * w[0] + M[4] * w[1] + M[8] * w[2] + M[12];
      c[1] = M[1] * w[0] + M[5] * w[1] + M[9] * w[2] + M[13];
      c[2] = M[2] * w[0] + M[6] * w[1] + M[10] * w[2] + M[14];
      if (!(Finite(c[0]) && Finite(c[1]) && Finite(c[2]))) continue;
    }
    double lo_x, hi_x, lo_y, hi_y, lo_z, hi_z;
    if (!AxisRange(c[0], R, resolution, nx, lo_x, hi_x) || !AxisRange(c[1], R, resolution, ny, lo_y, hi_y) ||
        !AxisRange(c[2], R, resolution, nz, lo_z, hi_z))
      continue;
    // (0 <= lo <= hi <= n - 1 holds in double: the conversions are exact and in the grid)
    const int x0 = static_cast<int>(lo_x), y0 = static_cast<int>(lo_y), z0 = static_cast<int>(lo_z);
    const unsigned bx = static_cast<unsigned>(static_cast<int>(hi_x) - x0 + 1);
    const unsigned by = static_cast<unsigned>(static_cast<int>(hi_y) - y0 + 1);
    const unsigned bz = static_cast<unsigned>(static_cast<int>(hi_z) - z0 + 1);
    const unsigned total = bx * by * bz;  // <= the cells of the grid < 2^31
    const double RR = R * R;
    const unsigned key = base + static_cast<unsigned>(b);
    // The lane's cell of the box, Z fastest, and the step of 64 cells as (step_x, step_y, step_z) with carries: one
    // set of divisions per pair, none per cell.
    const unsigned row = by * bz;
    unsigned ix = static_cast<unsigned>(lane) / row;
    unsigned rest = static_cast<unsigned>(lane) - ix * row;
    unsigned iy = rest / bz;
    unsigned iz = rest - iy * bz;
    const unsigned step_x = 64u / row;
    const unsigned step_rest = 64u - step_x * row;
    const unsigned step_y = step_rest / bz;
    const unsigned step_z = step_rest - step_y * bz;
    for (unsigned t = static_cast<unsigned>(lane); t < total; t += 64u)
    {
      const int cx = x0 + static_cast<int>(ix), cy = y0 + static_cast<int>(iy), cz = z0 + static_cast<int>(iz);
      const double dx = (static_cast<double>(cx) + 0.5) * resolution - c[0];
      const double dy = (static_cast<double>(cy) + 0.5) * resolution - c[1];
      const double dz = (static_cast<double>(cz) + 0.5) * resolution - c[2];
      if (kCount) tests++;
      if (((dx * dx + dy * dy) + dz * dz) <= RR)
      {
        unsigned* entry = first + (cx * sx + static_cast<int64_t>(cy) * nz + cz);
        if (kCount) covering++;
        // entries only fall: a stale value here is too high at worst, which costs a redundant atomic and nothing else
        if (*entry > key)
        {
          atomicMin(entry, key);
          if (kCount) atomics++;
        }
      }
      iz += step_z;
      if (iz >= bz) iz -= bz, iy++;
      iy += step_y;
      if (iy >= by) iy -= by, ix++;
      ix += step_x;
    }
  }
  if (kCount)
  {
    for (int offset = 32; offset > 0; offset >>= 1)
    {
      tests += __shfl_xor(tests, offset);
      covering += __shfl_xor(covering, offset);
      atomics += __shfl_xor(atomics, offset);
    }
    if (lane == 0)
    {
      atomicAdd(counters, tests);
      atomicAdd(counters + 1, covering);
      atomicAdd(counters + 2, atomics);
    }
  }
}

struct PointsFromWorld
{
  double m[16];
  int enabled;
};

__global__ __launch_bounds__(kVolumeThreads) void CoverPointsKernel(const unsigned* points, int64_t num_points,
                                                                    const PointsFromWorld xf,
                                                                    const SphereVolumeModel model,
                                                                    int32_t* first_configuration, int32_t* first_sphere,
                                                                    unsigned* filtered)
{
  __shared__ double chunk_wr[kVolumeChunk * 4];  // world centre and R; R = -1: not usable

  const int S = model.num_spheres, B = S > 0 ? model.num_configurations : 0;
  const int tid = static_cast<int>(threadIdx.x);
  const int64_t stride = static_cast<int64_t>(gridDim.x) * kVolumeThreads;
  for (int64_t first_point = static_cast<int64_t>(blockIdx.x) * kVolumeThreads; first_point < num_points;
       first_point += stride)
  {
    const int64_t i = first_point + tid;
    const bool live = i < num_points;
    unsigned bits[3] = {0u, 0u, 0u};
    double q[3] = {0.0, 0.0, 0.0};
    bool settled = true;  // nothing can cover it: no point, or a non-finite one
    if (live)
    {
      for (int a = 0; a < 3; a++) bits[a] = points[3 * i + a];
      const double px = static_cast<double>(__uint_as_float(bits[0]));
      const double py = static_cast<double>(__uint_as_float(bits[1]));
      const double pz = static_cast<double>(__uint_as_float(bits[2]));
      q[0] = px, q[1] = py, q[2] = pz;
      if (xf.enabled)
        for (int r = 0; r < 3; r++) q[r] = ((xf.m[r] * px + xf.m[4 + r] * py) + xf.m[8 + r] * pz) + xf.m[12 + r];
      settled = !(Finite(px) && Finite(py) && Finite(pz) && Finite(q[0]) && Finite(q[1]) && Finite(q[2]));
    }
    int found_b = -1, found_s = -1;
    bool all_settled = false;
    for (int b = 0; b < B && !all_settled; b++)
    {
      for (int chunk = 0; chunk < S && !all_settled; chunk += kVolumeChunk)
      {
        const int s = chunk + tid;
        if (s < S)
        {
          const double* p = model.xyzr + 4 * static_cast<int64_t>(s);
          double w[3] = {0.0, 0.0, 0.0}, R = -1.0;
          if (!WorldSphere(model, b, p[0], p[1], p[2], p[3], model.link[s], w, R)) R = -1.0;
          chunk_wr[4 * tid] = w[0];
          chunk_wr[4 * tid + 1] = w[1];
          chunk_wr[4 * tid + 2] = w[2];
          chunk_wr[4 * tid + 3] = R;
        }
        __syncthreads();
        if (!settled)
        {
          const int count = min(kVolumeChunk, S - chunk);
          for (int j = 0; j < count; j++)
          {
            const double R = chunk_wr[4 * j + 3];
            const double dx = q[0] - chunk_wr[4 * j], dy = q[1] - chunk_wr[4 * j + 1], dz = q[2] - chunk_wr[4 * j + 2];
            if (R >= 0.0 && ((dx * dx + dy * dy) + dz * dz) <= R * R)
            {
              found_b = b;
              found_s = chunk + j;
              settled = true;
              break;
            }
          }
        }
        // (also the barrier between this chunk's reads and the next chunk's writes)
        all_settled = __syncthreads_and(settled) != 0;
      }
    }
    if (live)
    {
      if (first_configuration) first_configuration[i] = found_b;
      if (first_sphere) first_sphere[i] = found_s;
      if (filtered)
        for (int a = 0; a < 3; a++) filtered[3 * i + a] = found_b >= 0 ? 0x7fc00000u : bits[a];
    }
  }
}

int64_t VolumeWorkgroups(int64_t wanted, int max_workgroups)
{
  const int64_t most = max_workgroups > 0 ? max_workgroups : kVolumeMaxWorkgroups;
  return wanted < most ? wanted : most;
}
}  // namespace

hipError_t LaunchRasterizeSpheres(int64_t nx, int64_t ny, int64_t nz, double resolution,
                                  const double* grid_from_world_host, const SphereVolumeModel& model, int64_t base,
                                  bool keep, int32_t* first_configuration_dev, int max_workgroups,
                                  unsigned long long* counters_dev, hipStream_t stream)
{
  const int64_t cells = nx * ny * nz;
  if (cells <= 0) return hipSuccess;
  if (!keep)
  {
    const hipError_t err = hipMemsetAsync(first_configuration_dev, 0xff, static_cast<size_t>(cells) * 4, stream);
    if (err != hipSuccess) return err;
  }
  const int64_t pairs = static_cast<int64_t>(model.num_configurations) * model.num_spheres;
  if (pairs <= 0) return hipSuccess;
  const int64_t workgroups = VolumeWorkgroups((pairs + kVolumeWaves - 1) / kVolumeWaves, max_workgroups);
  const auto kernel = counters_dev ? RasterizeSpheresKernel<true> : RasterizeSpheresKernel<false>;
  hipLaunchKernelGGL(kernel, dim3(static_cast<unsigned>(workgroups)), dim3(kVolumeThreads), 0, stream,
                     reinterpret_cast<unsigned*>(first_configuration_dev), static_cast<int>(nx), static_cast<int>(ny),
                     static_cast<int>(nz), resolution, MakeGridFromWorld(grid_from_world_host), model,
                     static_cast<unsigned>(base), counters_dev);
  return hipGetLastError();
}

hipError_t LaunchCoverPoints(const float* points_xyz_dev, int64_t num_points, const double* world_from_points_host,
                             const SphereVolumeModel& model, int32_t* first_configuration_dev,
                             int32_t* first_sphere_dev, float* filtered_xyz_dev, int max_workgroups,
                             hipStream_t stream)
{
  if (num_points <= 0) return hipSuccess;
  PointsFromWorld xf;
  xf.enabled = world_from_points_host ? 1 : 0;
  for (int k = 0; k < 16; k++) xf.m[k] = world_from_points_host ? world_from_points_host[k] : 0.0;
  const int64_t workgroups = VolumeWorkgroups((num_points + kVolumeThreads - 1) / kVolumeThreads, max_workgroups);
  hipLaunchKernelGGL(CoverPointsKernel, dim3(static_cast<unsigned>(workgroups)), dim3(kVolumeThreads), 0, stream,
                     reinterpret_cast<const unsigned*>(points_xyz_dev), num_points, xf, model, first_configuration_dev,
                     first_sphere_dev, reinterpret_cast<unsigned*>(filtered_xyz_dev));
  return hipGetLastError();
}
}  // namespace vgt
