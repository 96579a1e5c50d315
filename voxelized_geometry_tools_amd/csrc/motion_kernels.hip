// Motions between joint configurations checked against a float SDF, for gfx950: E straight joint-space motions of a
// kinematic tree of L links carrying S spheres, n + 1 samples each, one verdict per motion.  Semantics and every output:
// include/vgt_hip.h, vgt_hip_check_motions.  Per sample the kernel computes what vgt_hip_check_spheres_from_joints
// computes, with the same code: the limit test, the frame and the link step of kinematics_math.hpp
// (ForwardKinematicsKernel's) and the sphere's clearance, order, segment reduction and status of body_check.hpp
// (CheckSpheresKernel's).  The poses live in LDS between the two and are
// never written to memory.
//
// Work mapping.  A workgroup is one wave; waves are persistent over motions: workgroup w takes the motions w,
// w + workgroups, ...  A wave walks its motion in tiles of T samples, ascending (T a power of two <= 64: the launcher's,
// MotionTileSamples):
//   phase A   lane i < T with k = tile * T + i <= n interpolates the joint values (a value is computed where a link or
//             the limit test reads it, from the motion's two rows, whose addresses are wave-uniform: nothing is kept) and
//             walks the links, writing each pose to LDS as pose[link][element][i] -- doubles, consecutive lanes on
//             consecutive 8-byte words.  A parent's pose comes from registers when it is the link before, from that LDS
//             array otherwise: every link has a slot.  The lane keeps its sample's fk_status.
//   barrier   reached by all 64 lanes: a lane without a sample idles through both phases.
//   phase B   one lane per (sample, sphere) in CheckSpheresKernel's segment scheme: W the least power of two >=
//             min(S, 64), 64 / W samples per pass in ascending k, slices of 64 spheres for S > 64.  Poses from LDS, the
//             sphere table from LDS when it fits (below).  Per sample the check's ballot counts and its __shfl_xor
//             reduction under "smaller clearance, then smaller sphere index"; the lane that holds the winning sphere
//             keeps its cell.  Across samples every lane keeps a running best under "smaller clearance, then smaller k"
//             and a running least colliding k; both are total orders on distinct k and are combined once per motion by
//             __shfl_xor, so the result does not depend on T, W or the launch geometry.
//   barrier   before the next tile overwrites the poses.
// Under VGT_HIP_MOTION_STOP_AT_COLLISION the samples of a pass beyond the pass's first collision are masked out before
// they enter anything, the later passes and tiles are not run (a wave-uniform branch from a ballot), and phase A's lanes
// add their fk_status only up to that k.
// One lane -- the one that holds the motion's winning sample, lane 0 when there is none -- evaluates min_gradient once,
// at the kept cell, and writes the motion's outputs.
//
// LDS.  Dynamic: the poses, 96 L T bytes, at most 60 KiB (T: MotionTileSamples, which stays well below that where it
// can: occupancy is worth more than full tiles); behind them the sphere table (36 B per sphere) when
// S <= kMotionTableMax and both fit the 64 KiB a launch gets without an attribute; a larger model, or one next to a
// full 60 KiB of poses, is read through the cache.
//
// In bounds by construction: a lane with k > n, e >= E or s >= S forms no address; n < 0 (possible in the device form
// only) is handled before anything is read from the joint arrays; a sphere's link from device memory is compared against
// [0, L) before an LDS or global address is formed from it; parent, joint_type and joint_index were validated on the host
// when the tree was made; the field is read only through LocateCell's in-grid indices.
#include "body_check.hpp"
#include "kinematics_math.hpp"
#include "vgt_internal.hpp"

#include <cmath>

// What the launcher takes for the samples of a tile below what fits the LDS budget (DESIGN.md 4n has the A/B): at most
// VGT_MOTION_MAX_TILE samples, and poses of at most VGT_MOTION_TILE_BYTES where more than one sample would exceed them.
// 12 KiB: with the kernel's registers a CU holds twelve of these waves, and 160 KiB / 12 is what each may take of its LDS.
#ifndef VGT_MOTION_MAX_TILE
#define VGT_MOTION_MAX_TILE 64
#endif
#ifndef VGT_MOTION_TILE_BYTES
#define VGT_MOTION_TILE_BYTES (12 * 1024)
#endif

namespace vgt
{
namespace
{
constexpr int kMotionThreads = 64;  // one wave per workgroup
constexpr uint8_t kMotionClear = 0, kMotionCollision = 1, kMotionNoValue = 2, kMotionInvalid = 3;
constexpr int kMotionTableMax = 256;
constexpr size_t kMotionLdsLimit = 64 * 1024;  // (the poses' share: kMotionPoseBudget, vgt_internal.hpp)
// Workgroups of a launch: 32 waves per CU on 256 CUs; the motions beyond that by striding.
constexpr int kMotionMaxWorkgroups = 8192;
static_assert(VGT_MOTION_MAX_TILE >= 1 && VGT_MOTION_MAX_TILE <= 64 && (VGT_MOTION_MAX_TILE & (VGT_MOTION_MAX_TILE - 1)) == 0,
              "VGT_MOTION_MAX_TILE is a power of two in [1, 64]");

struct MotionTree
{
  const KinematicLink* links;
  const double* limits;  // [J][2] or nullptr
  int num_links, num_joints;
};

struct MotionModel
{
  const double* xyzr;   // [S][4]
  const int32_t* link;  // [S]
  int num_spheres;
};

struct MotionBatch
{
  const double* from;    // [E][J]
  const double* to;      // [E][J]
  const int32_t* steps;  // [E] or nullptr
  int uniform_steps;
  int64_t num_motions;
};

struct MotionQuery
{
  double minimum_clearance;
  int outside_is_collision, stop_at_collision;
};

// Joint j of sample k of n: include/vgt_hip.h.  `to` is not read for k == 0.
__device__ __forceinline__ double SampleJoint(const double* __restrict__ from, const double* __restrict__ to, int j, int k,
                                              int n)
{
  const double a = from[j];
  if (k == 0) return a;
  const double b = to[j];
  if (k == n) return b;
  const double t = static_cast<double>(k) / static_cast<double>(n);
  return a + t * (b - a);
}

__global__ __launch_bounds__(kMotionThreads) void CheckMotionsKernel(const float* __restrict__ sdf, int nx, int ny, int nz,
                                                                     double resolution, const GridFromWorld xf,
                                                                     const Rotation rot, const MotionTree tree,
                                                                     const KinematicsBase base, const MotionModel model,
                                                                     const MotionBatch batch, const MotionQuery query,
                                                                     int log2_width, int log2_tile, int table_in_lds,
                                                                     const MotionOutputs out)
{
  extern __shared__ __attribute__((aligned(16))) double lds[];  // poses [L][12][T], then the table: xyzr [S][4], link [S]

  const double nan = __longlong_as_double(0x7ff8000000000000ll);
  const int S = model.num_spheres, L = tree.num_links, J = tree.num_joints;
  const int lane = static_cast<int>(threadIdx.x);
  const int T = 1 << log2_tile;
  const int width = 1 << log2_width;
  const int per_pass = 64 >> log2_width;  // samples of a pass
  const int slices = static_cast<int>((static_cast<int64_t>(S) + width - 1) >> log2_width);
  const int segment = lane >> log2_width, in_segment = lane & (width - 1);
  const unsigned long long segment_mask = (width == 64 ? ~0ull : ((1ull << width) - 1ull)) << (segment * width);
  const int64_t sx = static_cast<int64_t>(ny) * nz, sy = nz;

  double* const poses = lds;
  double* const table_xyzr = lds + static_cast<size_t>(L) * 12 * T;
  int32_t* const table_link = reinterpret_cast<int32_t*>(table_xyzr + static_cast<size_t>(S) * 4);
  if (table_in_lds)
  {
    for (int i = lane; i < S * 4; i += kMotionThreads) table_xyzr[i] = model.xyzr[i];
    for (int i = lane; i < S; i += kMotionThreads) table_link[i] = model.link[i];
    __syncthreads();
  }

  for (int64_t e = blockIdx.x; e < batch.num_motions; e += gridDim.x)
  {
    const int n = batch.steps ? batch.steps[e] : batch.uniform_steps;  // (wave-uniform, as everything derived from it)
    if (n < 0)
    {
      if (lane == 0)
      {
        out.status[e] = kMotionInvalid;
        if (out.first_collision) out.first_collision[e] = -1;
        if (out.min_clearance) out.min_clearance[e] = nan;
        if (out.min_sample) out.min_sample[e] = -1;
        if (out.min_sphere) out.min_sphere[e] = -1;
        if (out.min_gradient) out.min_gradient[3 * e] = out.min_gradient[3 * e + 1] = out.min_gradient[3 * e + 2] = nan;
        if (out.fk_status) out.fk_status[e] = 0;
      }
      continue;
    }
    // (J == 0: no link and no limit reads a joint, and the arrays may be null)
    const double* const from = J > 0 ? batch.from + e * J : nullptr;
    const double* const to = J > 0 ? batch.to + e * J : nullptr;

    // what this lane has seen of the motion so far
    double run_clearance = nan;
    int run_sample = -1, run_sphere = -1, run_ix = 0, run_iy = 0, run_iz = 0;
    int run_collision = -1;  // the least colliding k
    bool run_no_value = false;
    uint8_t run_bits = 0;

    for (int64_t first = 0; first <= n; first += T)
    {
      // ---- phase A: the poses of the tile's samples into LDS ----
      const bool alive = lane < T && first + lane <= n;
      const int my_k = static_cast<int>(alive ? first + lane : 0);
      uint8_t bits = 0;
      if (alive)
      {
        const auto joint = [&](int j) { return SampleJoint(from, to, j, my_k, n); };
        if (tree.limits) bits = LimitBits(tree.limits, J, joint);
        LinkPose previous;  // the pose of link i - 1
#pragma unroll
        for (int c = 0; c < 12; c++) previous.m[c] = 0.0;
        for (int i = 0; i < L; i++)
        {
          const KinematicLink& link = tree.links[i];
          const LinkPose frame = LinkFrame(link, i, base, previous, [&](int parent) {
            LinkPose kept;  // this lane's own earlier pose
            const double* at = poses + (static_cast<size_t>(parent) * 12) * T + lane;
#pragma unroll
            for (int c = 0; c < 12; c++) kept.m[c] = at[c * T];
            return kept;
          });
          const LinkPose pose = LinkPoseFromFrame(link, frame, joint, bits);
          double* keep = poses + (static_cast<size_t>(i) * 12) * T + lane;
#pragma unroll
          for (int c = 0; c < 12; c++) keep[c * T] = pose.m[c];
          previous = pose;
        }
      }
      __syncthreads();

      // ---- phase B: the check of every sample of the tile, 64 / W samples per pass ----
      const int in_tile = static_cast<int>(n - first + 1 < T ? n - first + 1 : T);
      int stop_k = -1;  // under the stop flag: the tile's first collision
      for (int pass_first = 0; pass_first < in_tile; pass_first += per_pass)
      {
        const int slot = pass_first + segment;  // the sample's place in the tile
        const bool live = slot < in_tile;
        const int k = static_cast<int>(first) + slot;
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
              SphereCentre(poses + (static_cast<size_t>(link) * 12) * T + slot, 3 * T, T, x, y, z, w);
              has_value = SphereClearance(sdf, nx, ny, nz, resolution, xf, w, radius, c, clearance);
            }
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

        // the sample's status, the same on every lane of its segment
        const uint8_t status = SphereModelStatus(num_below, num_outside, query.outside_is_collision, winner_sphere);
        const bool collides = live && status == kBodyCollision;
        bool considered = live;
        if (query.stop_at_collision)
        {
          const unsigned long long hits = __ballot(collides);
          if (hits)
          {
            const int first_segment = (__ffsll(hits) - 1) >> log2_width;
            stop_k = static_cast<int>(first) + pass_first + first_segment;
            considered = live && segment <= first_segment;  // (the later samples do not exist)
          }
        }
        if (considered)
        {
          if (collides && (run_collision < 0 || k < run_collision)) run_collision = k;
          if (status == kBodyNoValue) run_no_value = true;
          // (one lane per sample: the one whose own sphere won, which has the cell.  This lane's k only grow: `<` keeps
          // the first.)
          if (winner_sphere >= 0 && best_sphere == winner_sphere && (run_sample < 0 || winner < run_clearance))
          {
            run_clearance = winner;
            run_sample = k;
            run_sphere = winner_sphere;
            run_ix = best_ix, run_iy = best_iy, run_iz = best_iz;
          }
        }
        if (stop_k >= 0) break;
      }
      if (alive && (stop_k < 0 || my_k <= stop_k)) run_bits |= bits;
      __syncthreads();  // (the tile's reads are done)
      if (stop_k >= 0) break;
    }

    // ---- the motion's verdict: the lanes' records combined ----
    double winner = run_clearance;
    int winner_sample = run_sample, winner_sphere = run_sphere;
    int first_collision = run_collision;
    for (int offset = 32; offset > 0; offset >>= 1)
    {
      const double other = __shfl_xor(winner, offset);
      const int other_sample = __shfl_xor(winner_sample, offset);
      const int other_sphere = __shfl_xor(winner_sphere, offset);
      if (BetterSphere(other, other_sample, winner, winner_sample))
      {
        winner = other;
        winner_sample = other_sample;
        winner_sphere = other_sphere;
      }
      const int other_collision = __shfl_xor(first_collision, offset);
      if (other_collision >= 0 && (first_collision < 0 || other_collision < first_collision))
        first_collision = other_collision;
    }
    const bool any_no_value = __ballot(run_no_value) != 0;
    const uint8_t fk_status = static_cast<uint8_t>((__ballot((run_bits & 1) != 0) ? 1 : 0) | (__ballot((run_bits & 2) != 0) ? 2 : 0));
    const bool writer = winner_sample >= 0 ? run_sample == winner_sample : lane == 0;
    if (writer)
    {
      out.status[e] = first_collision >= 0 ? kMotionCollision : any_no_value ? kMotionNoValue : kMotionClear;
      if (out.first_collision) out.first_collision[e] = first_collision;
      if (out.min_clearance) out.min_clearance[e] = winner_sample >= 0 ? winner : nan;
      if (out.min_sample) out.min_sample[e] = winner_sample;
      if (out.min_sphere) out.min_sphere[e] = winner_sample >= 0 ? winner_sphere : -1;
      if (out.min_gradient)
      {
        double gx = nan, gy = nan, gz = nan;
        if (winner_sample >= 0)
          CoarseGradientAt(sdf, nx, ny, nz, sx, sy, resolution, 1, rot, run_ix * sx + run_iy * sy + run_iz, run_ix, run_iy,
                           run_iz, gx, gy, gz);
        out.min_gradient[3 * e] = gx;
        out.min_gradient[3 * e + 1] = gy;
        out.min_gradient[3 * e + 2] = gz;
      }
      if (out.fk_status) out.fk_status[e] = fk_status;
    }
  }
}
}  // namespace

int MotionTileSamples(int64_t num_links)
{
  if (num_links <= 0 || num_links > kMotionMaxLinks) return 0;
  const size_t per_sample = static_cast<size_t>(num_links) * kMotionPoseBytesPerLink;
  const size_t budget = VGT_MOTION_TILE_BYTES < kMotionPoseBudget ? VGT_MOTION_TILE_BYTES : kMotionPoseBudget;
  int tile = VGT_MOTION_MAX_TILE;
  while (tile > 1 && per_sample * static_cast<size_t>(tile) > budget) tile >>= 1;  // (one sample always fits the 60 KiB)
  return tile;
}

MotionLaunchGeometry SelectMotionGeometry(int64_t num_links, int64_t num_spheres)
{
  MotionLaunchGeometry geometry{0, 0, 0, 0, 0};
  const int tile = MotionTileSamples(num_links);
  if (tile <= 0) return geometry;
  geometry.tile = tile;
  while ((1 << geometry.log2_tile) < tile) geometry.log2_tile++;
  geometry.log2_width = CheckSpheresWidthLog2(num_spheres);
  const size_t pose_bytes = static_cast<size_t>(num_links) * kMotionPoseBytesPerLink * static_cast<size_t>(tile);
  const size_t table_bytes = static_cast<size_t>(num_spheres) * 36;
  geometry.table_in_lds = num_spheres <= kMotionTableMax && pose_bytes + table_bytes <= kMotionLdsLimit ? 1 : 0;
  geometry.lds_bytes = pose_bytes + (geometry.table_in_lds ? table_bytes : 0);
  return geometry;
}

hipError_t LaunchCheckMotions(const float* sdf_dev, int64_t nx, int64_t ny, int64_t nz, double resolution,
                              const double* grid_from_world_host, const double* rotation_host,
                              const double* sphere_xyzr_dev, const int32_t* sphere_link_dev, int64_t num_spheres,
                              const KinematicLink* links_dev, int64_t num_links, int64_t num_joints,
                              const double* joint_from_dev, const double* joint_to_dev, const int32_t* num_steps_dev,
                              int32_t uniform_steps, int64_t num_motions, const double* world_from_base_host,
                              const double* limits_dev, double minimum_clearance, int outside_is_collision,
                              int stop_at_collision, const MotionOutputs& out, int max_workgroups, hipStream_t stream)
{
  if (num_motions <= 0) return hipSuccess;
  const MotionLaunchGeometry geometry = SelectMotionGeometry(num_links, num_spheres);
  if (geometry.tile <= 0) return hipErrorInvalidValue;
  const int64_t most = max_workgroups > 0 ? max_workgroups : kMotionMaxWorkgroups;
  const int64_t workgroups = num_motions < most ? num_motions : most;
  const MotionTree tree{links_dev, limits_dev, static_cast<int>(num_links), static_cast<int>(num_joints)};
  const MotionModel model{sphere_xyzr_dev, sphere_link_dev, static_cast<int>(num_spheres)};
  const MotionBatch batch{joint_from_dev, joint_to_dev, num_steps_dev, uniform_steps, num_motions};
  const MotionQuery query{minimum_clearance, outside_is_collision ? 1 : 0, stop_at_collision ? 1 : 0};
  hipLaunchKernelGGL(CheckMotionsKernel, dim3(static_cast<unsigned>(workgroups)), dim3(kMotionThreads),
                     geometry.lds_bytes, stream, sdf_dev, static_cast<int>(nx), static_cast<int>(ny), static_cast<int>(nz),
                     resolution, MakeGridFromWorld(grid_from_world_host), MakeRotation(rotation_host), tree,
                     MakeKinematicsBase(world_from_base_host), model, batch, query, geometry.log2_width, geometry.log2_tile,
                     geometry.table_in_lds, out);
  return hipGetLastError();
}
}  // namespace vgt
