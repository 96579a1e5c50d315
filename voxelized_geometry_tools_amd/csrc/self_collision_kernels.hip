// Self-collision of a sphere model, for gfx950: B configurations of a kinematic tree of L links and J joint columns
// carrying S spheres, and a list of P sphere pairs; per configuration the clearance of every pair, the worst pair, its
// direction and that clearance's gradient with respect to the joints.  Semantics and every output: include/vgt_hip.h,
// vgt_hip_check_self_collision.  The poses come from the limit test, the frame and the link step of kinematics_math.hpp
// (the joint-value form) or from the caller's link poses (the poses form: the same kernel template with another phase A),
// the centres from SphereCentre of body_check.hpp, the order of the pairs from its BetterSphere and the status from its
// SphereModelStatus.  The pair arithmetic is plain double arithmetic (the build's -ffp-contract=off keeps every operator on
// its own; sqrt and / are the correctly rounded ones).  The term of the joint gradient is restated here from
// kinematics_kernels.hip (WalkSphere) as cost_kernels.hip restates it, on poses in LDS: the same operations in the same
// order, held together by tests/test_gpu_self.py.  Poses and centres live in LDS and are never written to memory.
//
// Work mapping.  A workgroup is one wave; waves are persistent over tiles of T consecutive configurations (T a power of
// two <= 64: the launcher's, SelfCollisionTileSamples): workgroup w takes the tiles w, w + workgroups, ...
//   phase A   joint values: lane i < T with b = tile * T + i < B walks the links, writing each pose to LDS as
//             pose[link][element][i]; a parent's pose comes from registers when it is the link before, from that array
//             otherwise; the lane writes its configuration's fk_status.  Link poses: the 64 lanes copy the tile's
//             [T][L][16] doubles, coalesced, leaving the twelve used elements of each in the same layout.
//   phase B   one lane per (configuration, sphere), striding: the world centre to LDS as centre[sphere][row][i]; NaN x3
//             for a sphere whose link is outside [0, L).  (The radii went to an LDS table once, before the first tile.)
//   phase C   lane = k * T + i: the 64 / T lanes k of configuration i stride over the pairs p = k, k + 64 / T, ...; the
//             lanes of one k read the same pair (one address), the wave reads 64 / T consecutive pairs.  Each lane keeps
//             its best (clearance, p) and two counts; a butterfly of __shfl_xor over the offsets 32 ... T leaves the
//             configuration's on every one of its lanes.  Lane k == 0 writes the per-configuration outputs and leaves
//             min_pair in LDS.
//   phase D   one lane per (configuration, joint column), one more per configuration for min_direction: the direction
//             of min_pair from the centres in LDS, then the two walks, sphere a with n and sphere b with -n.
// The best pair is a total order ((clearance, p), p distinct) and the counts are integer sums: no output depends on T or
// on the launch geometry.
//
// LDS.  Dynamic: the poses, 96 L T bytes; the centres, 24 S T bytes; the radii, 8 S bytes; min_pair, 256 bytes.  T is the
// largest power of two <= VGT_SELF_MAX_TILE whose poses and centres take at most VGT_SELF_TILE_BYTES (one configuration
// where two would exceed them), and a model whose one configuration does not fit 64 KiB together with the rest is refused
// (SelfCollisionTileSamples gives 0): centres are never recomputed per pair.
//
// In bounds by construction: a lane with b >= B forms no address; a sphere's link and a pair's two indices from device
// memory are compared against [0, L) and [0, S) before an LDS or global address is formed from them, in every phase;
// parent, joint_type and joint_index were validated on the host when the tree was made; min_pair in LDS is -1 or an index
// this tile's phase C read.
#include "body_check.hpp"
#include "kinematics_math.hpp"
#include "vgt_internal.hpp"

#include <cmath>

// The launcher's choices: tiles of at most VGT_SELF_MAX_TILE configurations whose poses and centres take
// at most VGT_SELF_TILE_BYTES where more than one configuration would exceed them.
#ifndef VGT_SELF_MAX_TILE
#define VGT_SELF_MAX_TILE 64
#endif
#ifndef VGT_SELF_TILE_BYTES
#define VGT_SELF_TILE_BYTES (16 * 1024)
#endif

namespace vgt
{
namespace
{
constexpr int kSelfThreads = 64;  // one wave per workgroup
// Workgroups of a launch: 32 waves per CU on 256 CUs; the tiles beyond that by striding.
constexpr int kSelfMaxWorkgroups = 8192;
static_assert(VGT_SELF_MAX_TILE >= 1 && VGT_SELF_MAX_TILE <= 64 && (VGT_SELF_MAX_TILE & (VGT_SELF_MAX_TILE - 1)) == 0,
              "VGT_SELF_MAX_TILE is a power of two in [1, 64]");

struct SelfTree
{
  const KinematicLink* links;  // nullptr: the poses form without a gradient
  const double* limits;        // [J][2] or nullptr
  int num_links, num_joints;
};

struct SelfModel
{
  const double* xyzr;   // [S][4]
  const int32_t* link;  // [S]
  int num_spheres;
};

struct SelfPairs
{
  const int32_t* pairs;  // [P][2]
  int64_t num_pairs;
};

// The clearance of the pair (a, b) of the configuration at `slot` of the tile, from centres [S][3][T] and radii [S]; e
// and dist are left for the direction.  a and b are in [0, S).
__device__ __forceinline__ double PairClearance(const double* centres, const double* radii, int T, int slot, int a, int b,
                                                double (&e)[3], double& dist)
{
  const double* const ca = centres + (static_cast<size_t>(a) * 3) * T + slot;
  const double* const cb = centres + (static_cast<size_t>(b) * 3) * T + slot;
#pragma unroll
  for (int r = 0; r < 3; r++) e[r] = ca[r * T] - cb[r * T];
  const double d2 = (e[0] * e[0] + e[1] * e[1]) + e[2] * e[2];
  dist = sqrt(d2);
  return (dist - radii[a]) - radii[b];
}

// kFromJoints: `source` is joint_values [B][J]; otherwise link_poses [B][L][16].
template <bool kFromJoints>
__global__ __launch_bounds__(kSelfThreads) void SelfCollisionKernel(const SelfTree tree, const KinematicsBase base,
                                                                    const SelfModel model, const SelfPairs list,
                                                                    const double* __restrict__ source,
                                                                    int64_t num_configurations, double minimum_clearance,
                                                                    int no_value_is_collision, int log2_tile,
                                                                    const SelfCollisionOutputs out)
{
  // poses [L][12][T]; centres [S][3][T]; radii [S]; then the ints: min_pair [64]
  extern __shared__ __attribute__((aligned(16))) double lds[];

  const double nan = __longlong_as_double(0x7ff8000000000000ll);
  const int S = model.num_spheres, L = tree.num_links, J = tree.num_joints;
  const int64_t B = num_configurations, P = list.num_pairs;
  const int lane = static_cast<int>(threadIdx.x);
  const int T = 1 << log2_tile;
  const int slot_of_lane = lane & (T - 1), k_of_lane = lane >> log2_tile;
  const int per_slot = kSelfThreads >> log2_tile;  // phase C's lanes per configuration

  double* const poses = lds;
  double* const centres = poses + static_cast<size_t>(L) * 12 * T;
  double* const radii = centres + static_cast<size_t>(S) * 3 * T;
  int32_t* const min_pairs = reinterpret_cast<int32_t*>(radii + S);
  for (int s = lane; s < S; s += kSelfThreads) radii[s] = model.xyzr[4 * static_cast<int64_t>(s) + 3];
  __syncthreads();

  const int64_t tiles = (B + T - 1) >> log2_tile;
  for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x)
  {
    const int64_t first = tile << log2_tile;
    const int in_tile = static_cast<int>(B - first < T ? B - first : T);

    // ---- phase A: the poses of the tile's configurations into LDS ----
    if (kFromJoints)
    {
      if (lane < in_tile)
      {
        const int64_t b = first + lane;
        // (J == 0: no link and no limit reads a joint, and the array may be null)
        const double* const q = J > 0 ? source + b * J : nullptr;
        const auto joint = [&](int j) { return q[j]; };
        uint8_t bits = 0;
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
        if (out.fk_status) out.fk_status[b] = bits;
      }
    }
    else
    {
      const int per_configuration = L * 16;
      const int count = in_tile * per_configuration;  // (at most 64 * 16 L)
      const double* const from = source + first * per_configuration;
      for (int i = lane; i < count; i += kSelfThreads)
      {
        const int slot = i / per_configuration;
        const int within = i - slot * per_configuration;
        const int link = within >> 4, column = (within >> 2) & 3, row = within & 3;
        const double value = from[i];
        if (row < 3) poses[(static_cast<size_t>(link) * 12 + 3 * column + row) * T + slot] = value;
      }
    }
    __syncthreads();

    // ---- phase B: the world centres, one lane per (configuration, sphere) ----
    for (int item = lane; item < (S << log2_tile); item += kSelfThreads)
    {
      const int slot = item & (T - 1), s = item >> log2_tile;
      if (slot >= in_tile) continue;
      double centre[3] = {nan, nan, nan};
      const int32_t link = model.link[s];
      if (link >= 0 && link < L)
      {
        const double* p = model.xyzr + 4 * static_cast<int64_t>(s);
        SphereCentre(poses + (static_cast<size_t>(link) * 12) * T + slot, 3 * T, T, p[0], p[1], p[2], centre);
      }
      double* const keep = centres + (static_cast<size_t>(s) * 3) * T + slot;
#pragma unroll
      for (int r = 0; r < 3; r++) keep[r * T] = centre[r];
    }
    __syncthreads();

    // ---- phase C: the pairs; the 64 / T lanes of a configuration stride over the list ----
    {
      double best = nan;
      int best_pair = -1, num_below = 0, num_without_value = 0;
      const int64_t b = first + slot_of_lane;
      if (slot_of_lane < in_tile)
        for (int64_t p = k_of_lane; p < P; p += per_slot)
        {
          const int32_t sphere_a = list.pairs[2 * p], sphere_b = list.pairs[2 * p + 1];
          double clearance = nan;
          if (sphere_a >= 0 && sphere_a < S && sphere_b >= 0 && sphere_b < S)
          {
            double e[3], dist;
            clearance = PairClearance(centres, radii, T, slot_of_lane, sphere_a, sphere_b, e, dist);
          }
          if (out.pair_clearance) out.pair_clearance[b * P + p] = clearance;
          if (clearance == clearance)
          {
            if (clearance <= minimum_clearance) num_below++;
            if (BetterSphere(clearance, static_cast<int>(p), best, best_pair))
            {
              best = clearance;
              best_pair = static_cast<int>(p);
            }
          }
          else
            num_without_value++;
        }
      for (int offset = kSelfThreads >> 1; offset >= T; offset >>= 1)
      {
        const double other = __shfl_xor(best, offset);
        const int other_pair = __shfl_xor(best_pair, offset);
        if (BetterSphere(other, other_pair, best, best_pair))
        {
          best = other;
          best_pair = other_pair;
        }
        num_below += __shfl_xor(num_below, offset);
        num_without_value += __shfl_xor(num_without_value, offset);
      }
      if (k_of_lane == 0 && slot_of_lane < in_tile)
      {
        min_pairs[slot_of_lane] = best_pair;
        out.status[b] = SphereModelStatus(num_below, num_without_value, no_value_is_collision, best_pair);
        if (out.num_below) out.num_below[b] = num_below;
        if (out.num_without_value) out.num_without_value[b] = num_without_value;
        if (out.min_clearance) out.min_clearance[b] = best;  // (NaN without a candidate: it was never replaced)
        if (out.min_pair) out.min_pair[b] = best_pair;
      }
    }
    __syncthreads();

    // ---- phase D: one lane per (configuration, joint column), one more per configuration for the direction ----
    {
      const int columns = out.joint_gradient ? J : 0;
      const int per_configuration = columns + (out.min_direction ? 1 : 0);
      const int items = in_tile * per_configuration;
      for (int item = lane; item < items; item += kSelfThreads)
      {
        const int slot = item / per_configuration;
        const int column = item - slot * per_configuration;
        const int64_t b = first + slot;
        const int pair = min_pairs[slot];
        int sphere_a = -1, sphere_b = -1, link_a = -1, link_b = -1;
        double n[3] = {nan, nan, nan};
        if (pair >= 0)
        {
          sphere_a = list.pairs[2 * static_cast<int64_t>(pair)];
          sphere_b = list.pairs[2 * static_cast<int64_t>(pair) + 1];
        }
        // (the pair had a clearance, so both are spheres on links of the tree; what is compared forms the addresses)
        if (sphere_a >= 0 && sphere_a < S && sphere_b >= 0 && sphere_b < S)
        {
          double e[3], dist;
          PairClearance(centres, radii, T, slot, sphere_a, sphere_b, e, dist);
#pragma unroll
          for (int r = 0; r < 3; r++) n[r] = e[r] / dist;
          link_a = model.link[sphere_a];
          link_b = model.link[sphere_b];
        }
        if (column == columns)
        {
#pragma unroll
          for (int r = 0; r < 3; r++) out.min_direction[b * 3 + r] = n[r];
          continue;
        }
        double acc = nan;
        if (link_a >= 0 && link_a < L && link_b >= 0 && link_b < L)
        {
          acc = 0.0;
          const double* const own = poses + slot;  // element e of link i: own[(i * 12 + e) * T]
          // the summed form's terms of one sphere for this column, in walk order (its weight is 1.0)
          const auto walk = [&](int k, int sphere, double g0, double g1, double g2) {
            const double* const centre = centres + (static_cast<size_t>(sphere) * 3) * T + slot;
            const double p0 = centre[0], p1 = centre[T], p2 = centre[2 * T];
            int parent;
            for (int i = k; i >= 0; i = parent)
            {
              const KinematicLink& link = tree.links[i];
              parent = link.parent;
              const int joint_type = link.joint_type;
              if (joint_type == kJointFixed || link.joint_index != column) continue;
              const double x = link.axis[0], y = link.axis[1], z = link.axis[2];
              const double* m = own + (static_cast<size_t>(i) * 12) * T;
              double a[3];
#pragma unroll
              for (int r = 0; r < 3; r++) a[r] = (m[r * T] * x + m[(3 + r) * T] * y) + m[(6 + r) * T] * z;
              double term;
              if (joint_type == kJointRevolute)
              {
                const double d0 = p0 - m[9 * T], d1 = p1 - m[10 * T], d2 = p2 - m[11 * T];
                const double u0 = a[1] * d2 - a[2] * d1, u1 = a[2] * d0 - a[0] * d2, u2 = a[0] * d1 - a[1] * d0;
                term = (g0 * u0 + g1 * u1) + g2 * u2;
              }
              else
                term = (g0 * a[0] + g1 * a[1]) + g2 * a[2];
              acc = acc + 1.0 * term;
            }
          };
          walk(link_a, sphere_a, n[0], n[1], n[2]);
          walk(link_b, sphere_b, -n[0], -n[1], -n[2]);
        }
        out.joint_gradient[b * J + column] = acc;
      }
    }
    __syncthreads();  // (the poses', the centres' and min_pair's reads are done)
  }
}

// The bytes of dynamic LDS of a launch.
size_t SelfLdsBytes(int64_t num_links, int64_t num_spheres, int tile)
{
  return (static_cast<size_t>(num_links) * kSelfPoseBytesPerLink + static_cast<size_t>(num_spheres) * kSelfCentreBytes) *
             static_cast<size_t>(tile) +
         static_cast<size_t>(num_spheres) * 8 + kSelfThreads * 4;
}
}  // namespace

int SelfCollisionTileSamples(int64_t num_links, int64_t num_spheres)
{
  if (num_links <= 0 || num_spheres < 0) return 0;
  // (before any product: neither alone may fill the LDS)
  if (num_links > static_cast<int64_t>(kSelfLdsLimit / kSelfPoseBytesPerLink) ||
      num_spheres > static_cast<int64_t>(kSelfLdsLimit / kSelfCentreBytes))
    return 0;
  if (SelfLdsBytes(num_links, num_spheres, 1) > kSelfLdsLimit) return 0;
  const size_t per_sample =
      static_cast<size_t>(num_links) * kSelfPoseBytesPerLink + static_cast<size_t>(num_spheres) * kSelfCentreBytes;
  int tile = VGT_SELF_MAX_TILE;
  while (tile > 1 && (per_sample * static_cast<size_t>(tile) > VGT_SELF_TILE_BYTES ||
                      SelfLdsBytes(num_links, num_spheres, tile) > kSelfLdsLimit))
    tile >>= 1;
  return tile;
}

hipError_t LaunchSelfCollision(const double* sphere_xyzr_dev, const int32_t* sphere_link_dev, int64_t num_spheres,
                               const int32_t* pairs_dev, int64_t num_pairs, const KinematicLink* links_dev,
                               int64_t num_links, int64_t num_joints, const double* joint_values_dev,
                               const double* link_poses_dev, int64_t num_configurations,
                               const double* world_from_base_host, const double* limits_dev, double minimum_clearance,
                               int no_value_is_collision, const SelfCollisionOutputs& out, int max_workgroups,
                               hipStream_t stream)
{
  if (num_configurations <= 0) return hipSuccess;
  const int tile = SelfCollisionTileSamples(num_links, num_spheres);
  if (tile <= 0) return hipErrorInvalidValue;
  if (!link_poses_dev && !links_dev) return hipErrorInvalidValue;
  int log2_tile = 0;
  while ((1 << log2_tile) < tile) log2_tile++;
  const size_t lds_bytes = SelfLdsBytes(num_links, num_spheres, tile);
  const int64_t tiles = (num_configurations + tile - 1) / tile;
  const int64_t most = max_workgroups > 0 ? max_workgroups : kSelfMaxWorkgroups;
  const int64_t workgroups = tiles < most ? tiles : most;
  const SelfTree tree{links_dev, limits_dev, static_cast<int>(num_links), static_cast<int>(num_joints)};
  const SelfModel model{sphere_xyzr_dev, sphere_link_dev, static_cast<int>(num_spheres)};
  // (a model without spheres has no pair with a value and none without: the list is not read)
  const SelfPairs list{pairs_dev, num_spheres > 0 ? num_pairs : 0};
  if (link_poses_dev)
    hipLaunchKernelGGL(SelfCollisionKernel<false>, dim3(static_cast<unsigned>(workgroups)), dim3(kSelfThreads), lds_bytes,
                       stream, tree, MakeKinematicsBase(nullptr), model, list, link_poses_dev, num_configurations,
                       minimum_clearance, no_value_is_collision, log2_tile, out);
  else
    hipLaunchKernelGGL(SelfCollisionKernel<true>, dim3(static_cast<unsigned>(workgroups)), dim3(kSelfThreads), lds_bytes,
                       stream, tree, MakeKinematicsBase(world_from_base_host), model, list, joint_values_dev,
                       num_configurations, minimum_clearance, no_value_is_collision, log2_tile, out);
  return hipGetLastError();
}
}  // namespace vgt
