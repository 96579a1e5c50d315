// The obstacle cost of configurations given as joint values, and its gradient with respect to the joints, for gfx950: B
// configurations of a kinematic tree of L links and J joint columns carrying S spheres, against a float SDF.  Semantics
// and every output: include/vgt_hip.h, vgt_hip_clearance_cost.  Per (configuration, sphere) the kernel computes what
// vgt_hip_check_spheres computes on the poses of vgt_hip_forward_kinematics, with the same code: the limit test, the frame
// and the link step of kinematics_math.hpp and the sphere's centre and clearance of body_check.hpp, the coarse gradient
// as CheckSpheresKernel calls it.  The hinge and the ordered sums are plain double arithmetic (the build's
// -ffp-contract=off keeps every operator on its own).  The term of the joint gradient is restated here from
// kinematics_kernels.hip (WalkSphere), on poses in LDS instead of memory: the same operations in the same order, held
// together by tests/test_gpu_cost.py.  Poses and per-sphere values live in LDS and are never written to memory.
//
// Work mapping.  A workgroup is one wave; waves are persistent over tiles of T consecutive configurations (T a power of
// two <= 64: the launcher's, CostTileSamples): workgroup w takes the tiles w, w + workgroups, ...
//   phase A   lane i < T with b = tile * T + i < B walks the links, writing each pose to LDS as pose[link][element][i];
//             a parent's pose comes from registers when it is the link before, from that array otherwise.  The lane writes
//             its configuration's fk_status.
//   Then, per GROUP of P * (64 / W) configurations of the tile (W the check's segment width, the least power of two >=
//   min(S, 64); P the passes buffered, VGT_COST_BUFFER_PASSES at most) and per slice of W spheres, ascending:
//   phase B   P passes, one lane per (configuration, sphere) in CheckSpheresKernel's segment scheme: centre, clearance,
//             hinge, and -- in the gradient form, for a sphere with a weight -- the coarse gradient.  Each lane leaves its
//             c, flags and (gradient form) w, g and centre in the buffer of its pass.
//   phase C   one lane per (configuration of the group, joint column) walks the slice's spheres of its configuration in
//             ascending s over what phase B left and adds the summed form's terms from the poses in LDS; one more lane
//             per configuration adds the c_s in that order and counts.  Accumulators are registers; for S > 64 (several
//             slices, 64 / W = 1) they rest between the slices: the cost and the counts in LDS, a column's sum in its own
//             output element, which the same lane wrote.
// Every sum is one lane's, in ascending s: no output depends on T, W, P or the launch geometry.
//
// LDS.  Dynamic: the poses, 96 L T bytes (T: CostTileSamples, within VGT_COST_TILE_BYTES where more than one
// configuration fits them, 48 KiB at the most); the buffer, P * 64 entries of 8 B (cost only) or 64 B (gradient form) plus
// 4 B of flags; for S > 64 the resting cost and counts, 20 P B; in the gradient form what the walk reads of every link
// (parent, joint type and index, axis: 36 B per link) when it fits; the sphere table (36 B per sphere) when
// S <= kCostTableMax and all of it fits the 64 KiB a launch gets without an attribute, otherwise links and model are
// read through the cache.  The launcher halves P until the rest fits.
//
// In bounds by construction: a lane with b >= B or s >= S forms no address; a sphere's link from device memory is
// compared against [0, L) before an LDS or global address is formed from it, in both phases; parent, joint_type and
// joint_index were validated on the host when the tree was made; the field is read only through LocateCell's in-grid
// indices; buffer indices are below P * 64 and the resting indices below P by the loops' own limits.
#include "body_check.hpp"
#include "kinematics_math.hpp"
#include "vgt_internal.hpp"

#include <cmath>

// The launcher's choices (DESIGN.md 4o has the A/B): tiles of at most VGT_COST_MAX_TILE configurations whose poses take at
// most VGT_COST_TILE_BYTES where more than one configuration would exceed them, and at most VGT_COST_BUFFER_PASSES
// passes of phase B buffered in front of phase C.
#ifndef VGT_COST_MAX_TILE
#define VGT_COST_MAX_TILE 64
#endif
#ifndef VGT_COST_TILE_BYTES
#define VGT_COST_TILE_BYTES (6 * 1024)
#endif
#ifndef VGT_COST_BUFFER_PASSES
#define VGT_COST_BUFFER_PASSES 4
#endif

namespace vgt
{
namespace
{
constexpr int kCostThreads = 64;  // one wave per workgroup
constexpr int kCostTableMax = 256;
constexpr size_t kCostLdsLimit = 64 * 1024;
// Workgroups of a launch: 32 waves per CU on 256 CUs; the tiles beyond that by striding.
constexpr int kCostMaxWorkgroups = 8192;
constexpr int kCostHasValue = 1, kCostActive = 2, kCostWithoutGradient = 4;  // an entry's flags
// doubles per buffered entry: c; then w, g[3], centre[3]
constexpr int kCostEntryCostOnly = 1, kCostEntryGradient = 8;
static_assert(VGT_COST_MAX_TILE >= 1 && VGT_COST_MAX_TILE <= 64 && (VGT_COST_MAX_TILE & (VGT_COST_MAX_TILE - 1)) == 0,
              "VGT_COST_MAX_TILE is a power of two in [1, 64]");
static_assert(VGT_COST_BUFFER_PASSES >= 1 && VGT_COST_BUFFER_PASSES <= 64 &&
                  (VGT_COST_BUFFER_PASSES & (VGT_COST_BUFFER_PASSES - 1)) == 0,
              "VGT_COST_BUFFER_PASSES is a power of two in [1, 64]");

struct CostTree
{
  const KinematicLink* links;
  const double* limits;  // [J][2] or nullptr
  int num_links, num_joints;
};

struct CostModel
{
  const double* xyzr;   // [S][4]
  const int32_t* link;  // [S]
  int num_spheres;
};

struct CostGeometry
{
  int log2_width, log2_tile, passes, table_in_lds, links_in_lds;
};

// The hinge of include/vgt_hip.h on a clearance that is not NaN: c and w = dc/dd.
__device__ __forceinline__ void Hinge(double d, double margin, double& c, double& w)
{
  if (d < 0.0)
  {
    c = (margin * 0.5) - d;
    w = -1.0;
  }
  else if (d <= margin)
  {
    const double t = d - margin;
    c = ((t * t) * 0.5) / margin;
    w = t / margin;
  }
  else
  {
    c = 0.0;
    w = 0.0;
  }
}

template <bool kGradient>
__global__ __launch_bounds__(kCostThreads) void ClearanceCostKernel(const float* __restrict__ sdf, int nx, int ny, int nz,
                                                                    double resolution, const GridFromWorld xf,
                                                                    const Rotation rot, const CostTree tree,
                                                                    const KinematicsBase base, const CostModel model,
                                                                    const double* __restrict__ joint_values,
                                                                    int64_t num_configurations, double margin,
                                                                    const CostGeometry geometry, const CostOutputs out)
{
  // poses [L][12][T]; buffer [P][entry][64]; resting costs [P] (S > 64); table xyzr [S][4]; the links' axes [L][3];
  // then the ints: flags [P][64], resting counts [P][3] (S > 64), table link [S], the links' parent, joint_type and
  // joint_index [L][3]
  extern __shared__ __attribute__((aligned(16))) double lds[];

  constexpr int kEntry = kGradient ? kCostEntryGradient : kCostEntryCostOnly;
  const double nan = __longlong_as_double(0x7ff8000000000000ll);
  const int S = model.num_spheres, L = tree.num_links, J = tree.num_joints;
  const int64_t B = num_configurations;
  const int lane = static_cast<int>(threadIdx.x);
  const int log2_width = geometry.log2_width;
  const int T = 1 << geometry.log2_tile;
  const int P = geometry.passes;
  const int table_in_lds = geometry.table_in_lds;
  const int width = 1 << log2_width;
  const int log2_per_pass = 6 - log2_width;
  const int per_pass = 1 << log2_per_pass;  // configurations of a pass
  const int slices = static_cast<int>((static_cast<int64_t>(S) + width - 1) >> log2_width);
  const int rounds = slices > 0 ? slices : 1;  // (S == 0: one round over no spheres writes the outputs)
  const bool resting = slices > 1;             // (then per_pass == 1)
  const int group = P << log2_per_pass;        // configurations of a group
  const int segment = lane >> log2_width, in_segment = lane & (width - 1);
  const int64_t sx = static_cast<int64_t>(ny) * nz, sy = nz;
  // phase C's lanes per configuration; the last one has the cost
  const int per_configuration = kGradient && out.joint_gradient ? J + 1 : 1;

  double* const poses = lds;
  double* const buffer = poses + static_cast<size_t>(L) * 12 * T;
  double* const rest = buffer + static_cast<size_t>(P) * kEntry * 64;
  double* const table_xyzr = rest + (resting ? static_cast<size_t>(P) : 0);
  const int links_in_lds = kGradient ? geometry.links_in_lds : 0;
  double* const link_axis = table_xyzr + (table_in_lds ? static_cast<size_t>(S) * 4 : 0);
  int32_t* const flags = reinterpret_cast<int32_t*>(link_axis + (links_in_lds ? static_cast<size_t>(L) * 3 : 0));
  int32_t* const rest_counts = flags + static_cast<size_t>(P) * 64;
  int32_t* const table_link = rest_counts + (resting ? static_cast<size_t>(P) * 3 : 0);
  int32_t* const link_ints = table_link + (table_in_lds ? S : 0);
  if (table_in_lds)
  {
    for (int i = lane; i < S * 4; i += kCostThreads) table_xyzr[i] = model.xyzr[i];
    for (int i = lane; i < S; i += kCostThreads) table_link[i] = model.link[i];
  }
  if (links_in_lds)
    for (int i = lane; i < L; i += kCostThreads)
    {
      const KinematicLink& link = tree.links[i];
      link_ints[3 * i] = link.parent, link_ints[3 * i + 1] = link.joint_type, link_ints[3 * i + 2] = link.joint_index;
      link_axis[3 * i] = link.axis[0], link_axis[3 * i + 1] = link.axis[1], link_axis[3 * i + 2] = link.axis[2];
    }
  __syncthreads();

  const int64_t tiles = (B + T - 1) >> geometry.log2_tile;
  for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x)
  {
    const int64_t first = tile << geometry.log2_tile;
    const int in_tile = static_cast<int>(B - first < T ? B - first : T);

    // ---- phase A: the poses of the tile's configurations into LDS ----
    if (lane < in_tile)
    {
      const int64_t b = first + lane;
      // (J == 0: no link and no limit reads a joint, and the array may be null)
      const double* const q = J > 0 ? joint_values + b * J : nullptr;
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
    __syncthreads();

    for (int group_first = 0; group_first < in_tile; group_first += group)
    {
      const int in_group = in_tile - group_first < group ? in_tile - group_first : group;
      for (int round = 0; round < rounds; round++)
      {
        const int slice_first = round << log2_width;
        // ---- phase B: the passes of the group, one lane per (configuration, sphere of the slice) ----
        for (int pass = 0; (pass << log2_per_pass) < in_group; pass++)
        {
          const int slot = group_first + (pass << log2_per_pass) + segment;  // the configuration's place in the tile
          const int s = slice_first + in_segment;
          const bool active = slot < in_tile && s < S;
          double c = nan, w = 0.0, gx = nan, gy = nan, gz = nan;
          double centre[3] = {nan, nan, nan};
          int entry_flags = 0;
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
              CellOfLocation cell;
              cell.ix = cell.iy = cell.iz = 0;
              double clearance = nan;
              SphereCentre(poses + (static_cast<size_t>(link) * 12) * T + slot, 3 * T, T, x, y, z, centre);
              const bool has_value = SphereClearance(sdf, nx, ny, nz, resolution, xf, centre, radius, cell, clearance);
              if (has_value && clearance == clearance)
              {
                Hinge(clearance, margin, c, w);
                entry_flags = kCostHasValue;
                if (w != 0.0)
                {
                  entry_flags |= kCostActive;
                  if (kGradient)
                  {
                    CoarseGradientAt(sdf, nx, ny, nz, sx, sy, resolution, 1, rot, cell.ix * sx + cell.iy * sy + cell.iz,
                                     cell.ix, cell.iy, cell.iz, gx, gy, gz);
                    if (gx != gx || gy != gy || gz != gz)
                    {
                      entry_flags |= kCostWithoutGradient;
                      w = 0.0;
                    }
                  }
                }
              }
            }
          }
          double* const entry = buffer + static_cast<size_t>(pass) * kEntry * 64 + lane;
          entry[0] = c;
          if (kGradient)
          {
            entry[1 * 64] = w;
            entry[2 * 64] = gx, entry[3 * 64] = gy, entry[4 * 64] = gz;
            entry[5 * 64] = centre[0], entry[6 * 64] = centre[1], entry[7 * 64] = centre[2];
          }
          flags[pass * 64 + lane] = entry_flags;
        }
        __syncthreads();

        // ---- phase C: one lane per (configuration of the group, joint column), one more for the cost ----
        const int in_slice = S - slice_first < width ? (S - slice_first > 0 ? S - slice_first : 0) : width;
        const bool last = round == rounds - 1;
        const int64_t items = static_cast<int64_t>(in_group) * per_configuration;
        for (int64_t item = lane; item < items; item += kCostThreads)
        {
          const int configuration = static_cast<int>(item / per_configuration);
          const int column = static_cast<int>(item - static_cast<int64_t>(configuration) * per_configuration);
          const int slot = group_first + configuration;
          const int64_t b = first + slot;
          const int pass = configuration >> log2_per_pass;
          const int at = (configuration & (per_pass - 1)) << log2_width;  // the configuration's segment in its pass
          const double* const entries = buffer + static_cast<size_t>(pass) * kEntry * 64 + at;
          if (column == per_configuration - 1)
          {
            double acc = 0.0;
            int num_active = 0, num_outside = 0, num_without_gradient = 0;
            if (resting && round > 0)
            {
              acc = rest[configuration];
              num_active = rest_counts[3 * configuration];
              num_outside = rest_counts[3 * configuration + 1];
              num_without_gradient = rest_counts[3 * configuration + 2];
            }
            for (int i = 0; i < in_slice; i++)
            {
              const int f = flags[pass * 64 + at + i];
              if (f & kCostHasValue)
                acc = acc + entries[i];
              else
                num_outside++;
              if (f & kCostActive) num_active++;
              if (f & kCostWithoutGradient) num_without_gradient++;
            }
            if (!last)
            {
              rest[configuration] = acc;
              rest_counts[3 * configuration] = num_active;
              rest_counts[3 * configuration + 1] = num_outside;
              rest_counts[3 * configuration + 2] = num_without_gradient;
            }
            else
            {
              out.cost[b] = acc;
              if (out.num_active) out.num_active[b] = num_active;
              if (out.num_outside) out.num_outside[b] = num_outside;
              if (out.num_without_gradient) out.num_without_gradient[b] = num_without_gradient;
            }
          }
          else if (kGradient)
          {
            // (between the slices the sum rests in its own output element: this lane's earlier store, program order)
            double* const sum = out.joint_gradient + (b * J + column);
            double acc = round > 0 ? *sum : 0.0;
            const double* const own = poses + slot;  // element e of link i: own[(i * 12 + e) * T]
            for (int i = 0; i < in_slice; i++)
            {
              const double weight = entries[1 * 64 + i];
              if (weight == 0.0) continue;
              const int s = slice_first + i;
              const int32_t k = table_in_lds ? table_link[s] : model.link[s];
              if (k < 0 || k >= L) continue;
              const double g0 = entries[2 * 64 + i], g1 = entries[3 * 64 + i], g2 = entries[4 * 64 + i];
              const double p0 = entries[5 * 64 + i], p1 = entries[6 * 64 + i], p2 = entries[7 * 64 + i];
              // the summed form's terms of this sphere for this column, in walk order
              int parent;
              for (int n = k; n >= 0; n = parent)
              {
                int joint_type, joint_index;
                double x, y, z;
                if (links_in_lds)
                {
                  parent = link_ints[3 * n], joint_type = link_ints[3 * n + 1], joint_index = link_ints[3 * n + 2];
                  if (joint_type == kJointFixed || joint_index != column) continue;
                  x = link_axis[3 * n], y = link_axis[3 * n + 1], z = link_axis[3 * n + 2];
                }
                else
                {
                  const KinematicLink& link = tree.links[n];
                  parent = link.parent, joint_type = link.joint_type, joint_index = link.joint_index;
                  if (joint_type == kJointFixed || joint_index != column) continue;
                  x = link.axis[0], y = link.axis[1], z = link.axis[2];
                }
                const double* m = own + (static_cast<size_t>(n) * 12) * T;
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
                acc = acc + weight * term;
              }
            }
            *sum = acc;
          }
        }
        __syncthreads();  // (the buffer's and, after the last group, the poses' reads are done)
      }
    }
  }
}

// The bytes of dynamic LDS of a launch.
size_t CostLdsBytes(int64_t num_links, int64_t num_spheres, int tile, int passes, bool gradient, bool table_in_lds,
                    bool links_in_lds)
{
  const size_t entry = gradient ? kCostEntryGradient : kCostEntryCostOnly;
  const bool resting = num_spheres > 64;
  size_t bytes = static_cast<size_t>(num_links) * kCostPoseBytesPerLink * static_cast<size_t>(tile);
  bytes += static_cast<size_t>(passes) * 64 * (entry * 8 + 4);
  if (resting) bytes += static_cast<size_t>(passes) * (8 + 12);
  if (table_in_lds) bytes += static_cast<size_t>(num_spheres) * 36;
  if (links_in_lds) bytes += static_cast<size_t>(num_links) * 36;
  return bytes;
}
}  // namespace

int CostTileSamples(int64_t num_links)
{
  if (num_links <= 0 || num_links > kCostMaxLinks) return 0;
  const size_t per_sample = static_cast<size_t>(num_links) * kCostPoseBytesPerLink;
  const size_t budget = VGT_COST_TILE_BYTES < kCostPoseBudget ? VGT_COST_TILE_BYTES : kCostPoseBudget;
  int tile = VGT_COST_MAX_TILE;
  while (tile > 1 && per_sample * static_cast<size_t>(tile) > budget) tile >>= 1;  // (one always fits the 48 KiB)
  return tile;
}

CostLaunchGeometry SelectCostGeometry(int64_t num_links, int64_t num_spheres, bool gradient)
{
  CostLaunchGeometry geometry{0, 0, 0, 0, 0, 0, 0};
  const int tile = CostTileSamples(num_links);
  if (tile <= 0) return geometry;
  int log2_tile = 0;
  while ((1 << log2_tile) < tile) log2_tile++;
  const int log2_width = CheckSpheresWidthLog2(num_spheres);
  const int per_pass = 64 >> log2_width;
  // the passes a tile has at the most; of those, what fits
  int passes = VGT_COST_BUFFER_PASSES;
  while (passes > 1 && (passes >> 1) * per_pass >= tile) passes >>= 1;
  while (passes > 1 && CostLdsBytes(num_links, num_spheres, tile, passes, gradient, false, false) > kCostLdsLimit)
    passes >>= 1;
  if (CostLdsBytes(num_links, num_spheres, tile, passes, gradient, false, false) > kCostLdsLimit)
    return geometry;  // (not with kCostMaxLinks: vgt_internal.hpp has the sum)
  // what the walk reads of the links first (every step of phase C's inner loop), then the sphere table
  const bool links_in_lds =
      gradient && CostLdsBytes(num_links, num_spheres, tile, passes, gradient, false, true) <= kCostLdsLimit;
  const bool table_in_lds =
      num_spheres <= kCostTableMax &&
      CostLdsBytes(num_links, num_spheres, tile, passes, gradient, true, links_in_lds) <= kCostLdsLimit;
  geometry.tile = tile;
  geometry.log2_tile = log2_tile;
  geometry.log2_width = log2_width;
  geometry.passes = passes;
  geometry.table_in_lds = table_in_lds ? 1 : 0;
  geometry.links_in_lds = links_in_lds ? 1 : 0;
  geometry.lds_bytes = CostLdsBytes(num_links, num_spheres, tile, passes, gradient, table_in_lds, links_in_lds);
  return geometry;
}

hipError_t LaunchClearanceCost(const float* sdf_dev, int64_t nx, int64_t ny, int64_t nz, double resolution,
                               const double* grid_from_world_host, const double* rotation_host,
                               const double* sphere_xyzr_dev, const int32_t* sphere_link_dev, int64_t num_spheres,
                               const KinematicLink* links_dev, int64_t num_links, int64_t num_joints,
                               const double* joint_values_dev, int64_t num_configurations,
                               const double* world_from_base_host, const double* limits_dev, double margin,
                               const CostOutputs& out, int max_workgroups, hipStream_t stream)
{
  if (num_configurations <= 0) return hipSuccess;
  // (the count of skipped gradients needs the gradients: only without both does the cost-only kernel run)
  const bool gradient = out.joint_gradient != nullptr || out.num_without_gradient != nullptr;
  const CostLaunchGeometry selected = SelectCostGeometry(num_links, num_spheres, gradient);
  if (selected.tile <= 0) return hipErrorInvalidValue;
  const int tile = selected.tile;
  const size_t lds_bytes = selected.lds_bytes;
  const int64_t tiles = (num_configurations + tile - 1) / tile;
  const int64_t most = max_workgroups > 0 ? max_workgroups : kCostMaxWorkgroups;
  const int64_t workgroups = tiles < most ? tiles : most;
  const CostTree tree{links_dev, limits_dev, static_cast<int>(num_links), static_cast<int>(num_joints)};
  const CostModel model{sphere_xyzr_dev, sphere_link_dev, static_cast<int>(num_spheres)};
  const CostGeometry geometry{selected.log2_width, selected.log2_tile, selected.passes, selected.table_in_lds,
                              selected.links_in_lds};
  if (gradient)
    hipLaunchKernelGGL(ClearanceCostKernel<true>, dim3(static_cast<unsigned>(workgroups)), dim3(kCostThreads), lds_bytes,
                       stream, sdf_dev, static_cast<int>(nx), static_cast<int>(ny), static_cast<int>(nz), resolution,
                       MakeGridFromWorld(grid_from_world_host), MakeRotation(rotation_host), tree,
                       MakeKinematicsBase(world_from_base_host), model, joint_values_dev, num_configurations, margin,
                       geometry, out);
  else
    hipLaunchKernelGGL(ClearanceCostKernel<false>, dim3(static_cast<unsigned>(workgroups)), dim3(kCostThreads), lds_bytes,
                       stream, sdf_dev, static_cast<int>(nx), static_cast<int>(ny), static_cast<int>(nz), resolution,
                       MakeGridFromWorld(grid_from_world_host), MakeRotation(rotation_host), tree,
                       MakeKinematicsBase(world_from_base_host), model, joint_values_dev, num_configurations, margin,
                       geometry, out);
  return hipGetLastError();
}
}  // namespace vgt
