// Sphere-model checks for gfx950: B configurations of a body of S spheres attached to L links, against a float SDF.
// Semantics and every output: include/vgt_hip.h, vgt_hip_check_spheres.  A gather (the trilinear estimate at each
// transformed sphere centre) plus a segmented reduction (the worst sphere per configuration).
//
// Work mapping.  One lane per (configuration, sphere).  W is the least power of two >= min(S, 64) (1 for S == 0); a
// wave works on a GROUP of 64 / W consecutive configurations at a time, one segment of W lanes each, and for S > 64 --
// one configuration per wave -- loops over ceil(S / 64) slices, every lane keeping its running (clearance, index).
// Waves are persistent: wave w of the launch takes the groups w, w + waves, w + 2 waves, ...  Every wave of a workgroup
// makes the same number of trips (a wave without a group idles through its last one), so the workgroup barriers around
// the LDS staging are uniform.
//
// Staging.  The sphere table (x, y, z, r and the link: 36 bytes per sphere) is copied into LDS once per workgroup when
// S <= kSphereTableMax; larger models are read through the cache.  Every lane gathers the 12 used doubles of its own
// link's pose.  The alternative -- the poses of a wave's group copied into LDS cooperatively (consecutive lanes,
// consecutive doubles) when they fit kPoseDoublesPerWave, the gather otherwise -- was built and measured:
// equal within the run-to-run spread from 64 spheres on, 8 % slower at 16, with 8 more VGPRs and 16 KiB more LDS.  It
// stays in the source as VGT_BODY_STAGE_POSES=1 so that the A/B can be repeated (tools/ab_bodies.sh).
//
// Reduction.  Within a segment by __shfl_xor over the pair (clearance, sphere index), ordered "smaller clearance, then
// smaller index, no candidate last": a total order on distinct indices, so the result does not depend on the shape of
// the reduction.  Counts by __ballot + __popcll under the segment's mask.  The lane that holds the winning sphere still
// has its cell in registers: it evaluates the gradient there and writes the configuration's outputs (lane 0 of the
// segment when there is no winner).
//
// In bounds by construction: a lane with s >= S or b >= B forms no address; a link outside [0, L) (possible in the
// device form only) makes its sphere "without a value" before any pose address is formed; the field is read only through
// LocateCell's in-grid indices (never for an empty grid, where LocateCell has no cell).
// (EstimateDistance itself is not called here: the kernel needs the cell between its steps)
#include "body_check.hpp"
#include "vgt_internal.hpp"

#include <cmath>

#ifndef VGT_BODY_STAGE_POSES
#define VGT_BODY_STAGE_POSES 0
#endif

namespace vgt
{
namespace
{
constexpr int kBodyThreads = 256;
constexpr int kBodyWaves = kBodyThreads / 64;
// LDS per workgroup: the sphere table, 256 * 36 B = 9 KiB.  (With VGT_BODY_STAGE_POSES=1 also 4 waves * 4 KiB of
// poses, 42 link poses per wave: 25 KiB in all.)
constexpr int kSphereTableMax = 256;
constexpr int kPoseDoublesPerWave = 512;
// Workgroups of a launch: eight per CU on 256 CUs, about what is resident; the groups beyond that by striding.
constexpr int kBodyMaxWorkgroups = 2048;

struct BodyModel
{
  const double* xyzr;   // [S][4]
  const int32_t* link;  // [S]
  const double* poses;  // [B][L][16], column-major
  int num_spheres, num_links;
  int64_t num_configurations;
};

struct BodyQuery
{
  double minimum_clearance;
  int outside_is_collision;
};

template <bool kStagePoses>
__global__ __launch_bounds__(kBodyThreads) void CheckSpheresKernel(const float* __restrict__ sdf, int nx, int ny, int nz,
                                                                   double resolution, const GridFromWorld xf,
                                                                   const Rotation rot, const BodyModel model,
                                                                   const BodyQuery query, int log2_width,
                                                                   const BodyOutputs out)
{
  __shared__ double table_xyzr[kSphereTableMax * 4];
  __shared__ int32_t table_link[kSphereTableMax];
  __shared__ double staged_poses[kStagePoses ? kBodyWaves * kPoseDoublesPerWave : 1];

  const double nan = __longlong_as_double(0x7ff8000000000000ll);
  const int S = model.num_spheres, L = model.num_links;
  const int64_t B = model.num_configurations;
  const int lane = static_cast<int>(threadIdx.x) & 63, wave = static_cast<int>(threadIdx.x) >> 6;
  const int width = 1 << log2_width;
  const int per_wave = 64 >> log2_width;  // configurations of a group
  const int slices = static_cast<int>((static_cast<int64_t>(S) + width - 1) >> log2_width);  // 1 for 1 <= S <= 64, 0 for S == 0
  const int segment = lane >> log2_width, in_segment = lane & (width - 1);
  const unsigned long long segment_mask = (width == 64 ? ~0ull : ((1ull << width) - 1ull)) << (segment * width);
  const int64_t sx = static_cast<int64_t>(ny) * nz, sy = nz;

  const bool table_in_lds = S <= kSphereTableMax;
  if (table_in_lds)
  {
    for (int i = static_cast<int>(threadIdx.x); i < S * 4; i += kBodyThreads) table_xyzr[i] = model.xyzr[i];
    for (int i = static_cast<int>(threadIdx.x); i < S; i += kBodyThreads) table_link[i] = model.link[i];
    __syncthreads();
  }
  const int64_t group_poses = static_cast<int64_t>(per_wave) * L;  // link poses of a group
  const bool poses_in_lds = kStagePoses && group_poses * 12 <= kPoseDoublesPerWave;
  double* const my_poses = staged_poses + (kStagePoses ? wave * kPoseDoublesPerWave : 0);

  const int64_t groups = (B + per_wave - 1) / per_wave;
  const int64_t waves = static_cast<int64_t>(gridDim.x) * kBodyWaves;
  const int64_t trips = (groups + waves - 1) / waves;  // the same for every wave
  int64_t group = static_cast<int64_t>(blockIdx.x) * kBodyWaves + wave;
  for (int64_t trip = 0; trip < trips; trip++, group += waves)
  {
    const int64_t b = group * per_wave + segment;
    const bool live = group < groups && b < B;
    if (kStagePoses && poses_in_lds)
    {
      __syncthreads();  // (the previous trip's reads are done)
      if (group < groups)
      {
        const int64_t first_pose = group * group_poses, all_poses = B * L;
        for (int i = lane; i < static_cast<int>(group_poses) * 12; i += 64)
        {
          const int64_t pose = first_pose + i / 12;
          const int e = i % 12;  // column e / 3, row e % 3
          if (pose < all_poses) my_poses[i] = model.poses[pose * 16 + (e / 3) * 4 + (e % 3)];
        }
      }
      __syncthreads();
    }

    double best = nan;
    int best_sphere = -1, best_ix = 0, best_iy = 0, best_iz = 0;
    int num_below = 0, num_outside = 0;
    for (int slice = 0; slice < slices; slice++)
    {
      const int s = (slice << log2_width) + in_segment;
      const bool active = live && s < S;
      bool has_value = false;
      double clearance = nan;
      CellOfLocation c;
      c.ix = c.iy = c.iz = 0;
      if (active)
      {
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
        if (link >= 0 && link < L)
        {
          double w[3];
          if (kStagePoses && poses_in_lds)
            SphereCentre(my_poses + (segment * L + link) * 12, 3, 1, x, y, z, w);
          else
            SphereCentre(model.poses + (b * L + link) * 16, 4, 1, x, y, z, w);
          has_value = SphereClearance(sdf, nx, ny, nz, resolution, xf, w, radius, c, clearance);
        }
      }
      if (out.sphere_clearance && active) out.sphere_clearance[b * S + s] = clearance;
      if (out.sphere_gradient && active)
      {
        double gx = nan, gy = nan, gz = nan;
        if (has_value)
          CoarseGradientAt(sdf, nx, ny, nz, sx, sy, resolution, 1, rot, c.ix * sx + c.iy * sy + c.iz, c.ix, c.iy, c.iz, gx,
                           gy, gz);
        double* g = out.sphere_gradient + 3 * (b * S + s);
        g[0] = gx;
        g[1] = gy;
        g[2] = gz;
      }
      num_outside += __popcll(__ballot(active && !has_value) & segment_mask);
      num_below += __popcll(__ballot(has_value && clearance <= query.minimum_clearance) & segment_mask);
      // (NaN compares false: a NaN clearance is no candidate.  A later slice's index is larger: `<` keeps the first.)
      if (has_value && (best_sphere < 0 ? clearance == clearance : clearance < best))
      {
        best = clearance;
        best_sphere = s;
        best_ix = c.ix, best_iy = c.iy, best_iz = c.iz;
      }
    }

    double winner = best;
    int winner_sphere = best_sphere;
    BestSphereOfSegment(width, winner, winner_sphere);

    const bool writer = live && (winner_sphere >= 0 ? best_sphere == winner_sphere : in_segment == 0);
    if (writer)
    {
      const uint8_t status = SphereModelStatus(num_below, num_outside, query.outside_is_collision, winner_sphere);
      out.status[b] = status;
      if (out.min_clearance) out.min_clearance[b] = winner_sphere >= 0 ? winner : nan;
      if (out.min_sphere) out.min_sphere[b] = winner_sphere;
      if (out.num_below) out.num_below[b] = num_below;
      if (out.num_outside) out.num_outside[b] = num_outside;
      if (out.min_gradient)
      {
        double gx = nan, gy = nan, gz = nan;
        if (winner_sphere >= 0)
          CoarseGradientAt(sdf, nx, ny, nz, sx, sy, resolution, 1, rot, best_ix * sx + best_iy * sy + best_iz, best_ix,
                           best_iy, best_iz, gx, gy, gz);
        out.min_gradient[3 * b] = gx;
        out.min_gradient[3 * b + 1] = gy;
        out.min_gradient[3 * b + 2] = gz;
      }
    }
  }
}
}  // namespace

int CheckSpheresWidthLog2(int64_t num_spheres)
{
  int log2_width = 0;
  while (log2_width < 6 && (int64_t{1} << log2_width) < num_spheres) log2_width++;
  return log2_width;
}

hipError_t LaunchCheckSpheres(const float* sdf_dev, int64_t nx, int64_t ny, int64_t nz, double resolution,
                              const double* grid_from_world_host, const double* rotation_host,
                              const double* sphere_xyzr_dev, const int32_t* sphere_link_dev, int64_t num_spheres,
                              const double* link_poses_dev, int64_t num_links, int64_t num_configurations,
                              double minimum_clearance, int outside_is_collision, const BodyOutputs& out,
                              int max_workgroups, hipStream_t stream)
{
  if (num_configurations <= 0) return hipSuccess;
  const int log2_width = CheckSpheresWidthLog2(num_spheres);
  const int64_t per_wave = 64 >> log2_width;
  const int64_t groups = (num_configurations + per_wave - 1) / per_wave;
  int64_t workgroups = (groups + kBodyWaves - 1) / kBodyWaves;
  const int64_t most = max_workgroups > 0 ? max_workgroups : kBodyMaxWorkgroups;
  if (workgroups > most) workgroups = most;
  const BodyModel model{sphere_xyzr_dev,
                        sphere_link_dev,
                        link_poses_dev,
                        static_cast<int>(num_spheres),
                        static_cast<int>(num_links),
                        num_configurations};
  const BodyQuery query{minimum_clearance, outside_is_collision ? 1 : 0};
  hipLaunchKernelGGL(CheckSpheresKernel<VGT_BODY_STAGE_POSES != 0>, dim3(static_cast<unsigned>(workgroups)),
                     dim3(kBodyThreads), 0, stream, sdf_dev, static_cast<int>(nx), static_cast<int>(ny),
                     static_cast<int>(nz), resolution, MakeGridFromWorld(grid_from_world_host),
                     MakeRotation(rotation_host), model, query, log2_width, out);
  return hipGetLastError();
}
}  // namespace vgt
