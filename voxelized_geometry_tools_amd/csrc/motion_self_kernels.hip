// Motions between joint configurations checked against a float SDF and against the robot itself in one walk, for gfx950:
// E straight joint-space motions of a kinematic tree of L links carrying S spheres with a list of P sphere pairs, n + 1
// samples each, one verdict per motion.  Semantics and every output: include/vgt_hip.h, vgt_hip_check_motions_with_self.
// Per sample the kernel computes what vgt_hip_check_spheres_from_joints and vgt_hip_check_self_collision compute, with the
// same code: the limit test, the frame and the link step of kinematics_math.hpp, the sphere's centre, clearance, order,
// segment reduction and status of body_check.hpp.  The pair arithmetic is restated here from self_collision_kernels.hip
// (PairClearance) as that file restates the gradient term: the same operations in the same order, held together by
// tests/test_gpu_motion_self.py.  Poses and centres live in LDS and are never written to memory.
//
// Work mapping.  A workgroup is one wave; waves are persistent over motions: workgroup w takes the motions w,
// w + workgroups, ...  A wave walks its motion in tiles of T samples, ascending (T a power of two <= 64: the launcher's,
// MotionSelfTileSamples):
//   phase A   CheckMotionsKernel's: lane i < T with k = tile * T + i <= n interpolates the joint values and walks the
//             links, writing each pose to LDS as pose[link][element][i].  The lane keeps its sample's fk_status.
//   phase B   one lane per (sample, sphere) in CheckSpheresKernel's segment scheme: W the least power of two >=
//             min(S, 64), 64 / W samples per pass in ascending k, slices of 64 spheres for S > 64.  The world centre once,
//             kept in LDS as centre[sphere][row][slot] (NaN x3 for a link outside [0, L)); with a field the sphere's
//             clearance, the check's ballot counts and its __shfl_xor reduction; the sample's status, worst sphere and
//             that sphere's cell go to a record per slot in LDS.
//   phase C   with pairs: lane = j * T + i: the 64 / T lanes j of sample i stride over the pairs p = j, j + 64 / T, ...;
//             each lane keeps its best (clearance, p) and two counts; a butterfly of __shfl_xor over the offsets
//             32 ... T leaves the sample's on every one of its lanes, lane i among them.
//   verdict   lane i < T -- the lane of phase A -- has its sample's self part in registers and reads its environment
//             record: whether the sample collides, why, whether it is without a value.  Across tiles the lane keeps a
//             running least colliding k with its cause and two running bests (environment, self) under "smaller value,
//             then smaller k"; its k only grow.  All three are total orders on distinct k and are combined once per motion
//             by __shfl_xor, so the result does not depend on T, W or the launch geometry.
// Under VGT_HIP_MOTION_STOP_AT_COLLISION phase B stops behind the pass that holds the tile's first environment hit (the
// later slots get no centre and phase C leaves them out: they lie behind a combined hit), the samples behind the tile's
// first combined collision are masked out before they enter anything, the later tiles are not run (a wave-uniform branch
// from a ballot), and the lanes add their fk_status only up to that k.
// The lane that holds the motion's closest environment sample evaluates min_gradient once, at the kept cell, and writes
// the environment's outputs; lane 0 writes the others.
//
// LDS.  Dynamic: the poses, 96 L T bytes; the centres, 24 S T bytes; the radii, 8 S bytes; the per-slot records, 1792
// bytes.  T is the largest power of two <= 64 whose poses and centres take at most VGT_MOTION_SELF_TILE_BYTES (one sample
// where two would exceed them), and a model whose one sample does not fit 64 KiB together with the rest is refused
// (MotionSelfTileSamples gives 0): centres are never recomputed per pair.
//
// In bounds by construction: a lane with k > n, e >= E or s >= S forms no address; n < 0 (possible in the device form
// only) is handled before anything is read from the joint arrays; a sphere's link and a pair's two indices from device
// memory are compared against [0, L) and [0, S) before an LDS or global address is formed from them; parent, joint_type
// and joint_index were validated on the host when the tree was made; the field is read only through LocateCell's in-grid
// indices; a slot's record is read only by a lane whose slot phase B wrote in this tile.
#include "body_check.hpp"
#include "kinematics_math.hpp"
#include "vgt_internal.hpp"

#include <cmath>

// What the launcher takes for the samples of a tile: the poses and centres of a tile take at most
// VGT_MOTION_SELF_TILE_BYTES where more than one sample would exceed them.
#ifndef VGT_MOTION_SELF_TILE_BYTES
#define VGT_MOTION_SELF_TILE_BYTES (16 * 1024)
#endif

namespace vgt
{
namespace
{
constexpr int kMotionSelfThreads = 64;  // one wave per workgroup
constexpr uint8_t kMotionSelfClear = 0, kMotionSelfCollision = 1, kMotionSelfNoValue = 2, kMotionSelfInvalid = 3;
constexpr uint8_t kCauseEnvironment = 1, kCauseSelf = 2;
// Workgroups of a launch: 32 waves per CU on 256 CUs; the motions beyond that by striding.
constexpr int kMotionSelfMaxWorkgroups = 8192;

struct MotionSelfTree
{
  const KinematicLink* links;
  const double* limits;  // [J][2] or nullptr
  int num_links, num_joints;
};

struct MotionSelfModel
{
  const double* xyzr;    // [S][4]
  const int32_t* link;   // [S]
  const int32_t* pairs;  // [P][2]
  int num_spheres;
  int64_t num_pairs;  // (0 for a model without spheres: the list is not read)
  int with_self;      // the self part is there
};

struct MotionSelfBatch
{
  const double* from;    // [E][J]
  const double* to;      // [E][J]
  const int32_t* steps;  // [E] or nullptr
  int uniform_steps;
  int64_t num_motions;
};

struct MotionSelfQuery
{
  double minimum_clearance, self_minimum_clearance;
  int outside_is_collision, no_value_is_collision, stop_at_collision;
};

// Joint j of sample k of n: include/vgt_hip.h, vgt_hip_check_motions.  `to` is not read for k == 0.
__device__ __forceinline__ double SampleJointOfMotion(const double* __restrict__ from, const double* __restrict__ to, int j,
                                                      int k, int n)
{
  const double a = from[j];
  if (k == 0) return a;
  const double b = to[j];
  if (k == n) return b;
  const double t = static_cast<double>(k) / static_cast<double>(n);
  return a + t * (b - a);
}

// The clearance of the pair (a, b) of the sample at `slot` of the tile, from centres [S][3][T] and radii [S]: restated
// from self_collision_kernels.hip.  a and b are in [0, S).
__device__ __forceinline__ double PairClearanceOfSample(const double* centres, const double* radii, int T, int slot, int a,
                                                        int b)
{
  const double* const ca = centres + (static_cast<size_t>(a) * 3) * T + slot;
  const double* const cb = centres + (static_cast<size_t>(b) * 3) * T + slot;
  double e[3];
#pragma unroll
  for (int r = 0; r < 3; r++) e[r] = ca[r * T] - cb[r * T];
  const double d2 = (e[0] * e[0] + e[1] * e[1]) + e[2] * e[2];
  const double dist = sqrt(d2);
  return (dist - radii[a]) - radii[b];
}

// kField: there is an environment part; without it nothing is loaded from the grid.
template <bool kField>
__global__ __launch_bounds__(kMotionSelfThreads) void CheckMotionsWithSelfKernel(
    const float* __restrict__ sdf, int nx, int ny, int nz, double resolution, const GridFromWorld xf, const Rotation rot,
    const MotionSelfTree tree, const KinematicsBase base, const MotionSelfModel model, const MotionSelfBatch batch,
    const MotionSelfQuery query, int log2_width, int log2_tile, const MotionSelfOutputs out)
{
  // poses [L][12][T]; centres [S][3][T]; radii [S]; the records of the slots: clearance [64], then the ints sphere [64],
  // status [64], ix [64], iy [64], iz [64]
  extern __shared__ __attribute__((aligned(16))) double lds[];

  const double nan = __longlong_as_double(0x7ff8000000000000ll);
  const int S = model.num_spheres, L = tree.num_links, J = tree.num_joints;
  const int64_t P = model.num_pairs;
  const bool with_self = model.with_self != 0;
  const int lane = static_cast<int>(threadIdx.x);
  const int T = 1 << log2_tile;
  const int width = 1 << log2_width;
  const int per_pass = 64 >> log2_width;  // samples of a pass of phase B
  const int slices = static_cast<int>((static_cast<int64_t>(S) + width - 1) >> log2_width);
  const int segment = lane >> log2_width, in_segment = lane & (width - 1);
  const unsigned long long segment_mask = (width == 64 ? ~0ull : ((1ull << width) - 1ull)) << (segment * width);
  const int slot_of_lane = lane & (T - 1), j_of_lane = lane >> log2_tile;
  const int per_slot = kMotionSelfThreads >> log2_tile;  // phase C's lanes per sample
  const int64_t sx = static_cast<int64_t>(ny) * nz, sy = nz;

  double* const poses = lds;
  double* const centres = poses + static_cast<size_t>(L) * 12 * T;
  double* const radii = centres + static_cast<size_t>(S) * 3 * T;
  double* const record_clearance = radii + S;
  int32_t* const record_sphere = reinterpret_cast<int32_t*>(record_clearance + kMotionSelfThreads);
  int32_t* const record_status = record_sphere + kMotionSelfThreads;
  int32_t* const record_ix = record_status + kMotionSelfThreads;
  int32_t* const record_iy = record_ix + kMotionSelfThreads;
  int32_t* const record_iz = record_iy + kMotionSelfThreads;
  for (int s = lane; s < S; s += kMotionSelfThreads) radii[s] = model.xyzr[4 * static_cast<int64_t>(s) + 3];
  __syncthreads();

  for (int64_t e = blockIdx.x; e < batch.num_motions; e += gridDim.x)
  {
    const int n = batch.steps ? batch.steps[e] : batch.uniform_steps;  // (wave-uniform, as everything derived from it)
    if (n < 0)
    {
      if (lane == 0)
      {
        out.status[e] = kMotionSelfInvalid;
        if (out.first_collision) out.first_collision[e] = -1;
        if (out.collision_cause) out.collision_cause[e] = 0;
        if (out.min_clearance) out.min_clearance[e] = nan;
        if (out.min_sample) out.min_sample[e] = -1;
        if (out.min_sphere) out.min_sphere[e] = -1;
        if (out.min_gradient) out.min_gradient[3 * e] = out.min_gradient[3 * e + 1] = out.min_gradient[3 * e + 2] = nan;
        if (out.self_min_clearance) out.self_min_clearance[e] = nan;
        if (out.self_min_sample) out.self_min_sample[e] = -1;
        if (out.self_min_pair) out.self_min_pair[e] = -1;
        if (out.fk_status) out.fk_status[e] = 0;
      }
      continue;
    }
    // (J == 0: no link and no limit reads a joint, and the arrays may be null)
    const double* const from = J > 0 ? batch.from + e * J : nullptr;
    const double* const to = J > 0 ? batch.to + e * J : nullptr;

    // what this lane has seen of the motion so far: its own samples, whose k only grow
    double run_clearance = nan, run_self = nan;
    int run_sample = -1, run_sphere = -1, run_ix = 0, run_iy = 0, run_iz = 0;
    int run_self_sample = -1, run_self_pair = -1;
    int run_collision = -1;  // the least colliding k
    uint8_t run_cause = 0;
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
        const auto joint = [&](int j) { return SampleJointOfMotion(from, to, j, my_k, n); };
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

      // ---- phase B: the centres and the environment part of every sample of the tile, 64 / W samples per pass ----
      const int in_tile = static_cast<int>(n - first + 1 < T ? n - first + 1 : T);
      int slots_done = in_tile;  // the slots that have centres and a record
      for (int pass_first = 0; pass_first < in_tile; pass_first += per_pass)
      {
        const int slot = pass_first + segment;  // the sample's place in the tile
        const bool live = slot < in_tile;
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
            const double* p = model.xyzr + 4 * static_cast<int64_t>(s);
            const int32_t link = model.link[s];
            double w[3] = {nan, nan, nan};
            if (link >= 0 && link < L)
            {
              SphereCentre(poses + (static_cast<size_t>(link) * 12) * T + slot, 3 * T, T, p[0], p[1], p[2], w);
              if (kField) has_value = SphereClearance(sdf, nx, ny, nz, resolution, xf, w, p[3], c, clearance);
            }
            if (with_self)
            {
              double* const keep = centres + (static_cast<size_t>(s) * 3) * T + slot;
#pragma unroll
              for (int r = 0; r < 3; r++) keep[r * T] = w[r];
            }
          }
          if (kField)
          {
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
        }
        if (kField)
        {
          double winner = best;
          int winner_sphere = best_sphere;
          BestSphereOfSegment(width, winner, winner_sphere);
          // the sample's status, the same on every lane of its segment
          const uint8_t status = SphereModelStatus(num_below, num_outside, query.outside_is_collision, winner_sphere);
          if (live && in_segment == 0)
          {
            record_status[slot] = status;
            if (winner_sphere < 0) record_sphere[slot] = -1;
          }
          // (one lane per sample: the one whose own sphere won, which has the cell)
          if (live && winner_sphere >= 0 && best_sphere == winner_sphere)
          {
            record_clearance[slot] = winner;
            record_sphere[slot] = winner_sphere;
            record_ix[slot] = best_ix, record_iy[slot] = best_iy, record_iz[slot] = best_iz;
          }
          if (query.stop_at_collision)
          {
            const unsigned long long hits = __ballot(live && status == kBodyCollision);
            if (hits)
            {
              // (the samples behind the first of them do not exist)
              slots_done = pass_first + ((__ffsll(hits) - 1) >> log2_width) + 1;
              break;
            }
          }
        }
      }
      __syncthreads();

      // ---- phase C: the pairs; the 64 / T lanes of a sample stride over the list ----
      double self_best = nan;
      int self_pair = -1;
      uint8_t self_status = kBodyNoValue;
      if (with_self)
      {
        int num_below = 0, num_without_value = 0;
        if (slot_of_lane < slots_done)
          for (int64_t p = j_of_lane; p < P; p += per_slot)
          {
            const int32_t sphere_a = model.pairs[2 * p], sphere_b = model.pairs[2 * p + 1];
            double clearance = nan;
            if (sphere_a >= 0 && sphere_a < S && sphere_b >= 0 && sphere_b < S)
              clearance = PairClearanceOfSample(centres, radii, T, slot_of_lane, sphere_a, sphere_b);
            if (clearance == clearance)
            {
              if (clearance <= query.self_minimum_clearance) num_below++;
              if (BetterSphere(clearance, static_cast<int>(p), self_best, self_pair))
              {
                self_best = clearance;
                self_pair = static_cast<int>(p);
              }
            }
            else
              num_without_value++;
          }
        for (int offset = kMotionSelfThreads >> 1; offset >= T; offset >>= 1)
        {
          const double other = __shfl_xor(self_best, offset);
          const int other_pair = __shfl_xor(self_pair, offset);
          if (BetterSphere(other, other_pair, self_best, self_pair))
          {
            self_best = other;
            self_pair = other_pair;
          }
          num_below += __shfl_xor(num_below, offset);
          num_without_value += __shfl_xor(num_without_value, offset);
        }
        self_status = SphereModelStatus(num_below, num_without_value, query.no_value_is_collision, self_pair);
      }

      // ---- the verdict of the tile's samples: lane i has sample i's two parts ----
      const bool valid = alive && lane < slots_done;
      uint8_t cause = 0;
      bool without_value = false;
      if (valid)
      {
        if (kField)
        {
          const uint8_t status = static_cast<uint8_t>(record_status[lane]);
          if (status == kBodyCollision) cause |= kCauseEnvironment;
          if (status == kBodyNoValue) without_value = true;
        }
        if (with_self)
        {
          if (self_status == kBodyCollision) cause |= kCauseSelf;
          if (self_status == kBodyNoValue) without_value = true;
        }
      }
      bool considered = valid;
      int stop_k = -1;  // under the stop flag: the tile's first collision
      if (query.stop_at_collision)
      {
        const unsigned long long hits = __ballot(cause != 0);
        if (hits)
        {
          const int first_slot = __ffsll(hits) - 1;
          stop_k = static_cast<int>(first) + first_slot;
          considered = valid && lane <= first_slot;  // (the later samples do not exist)
        }
      }
      if (considered)
      {
        // (this lane's k only grow: `<` keeps the first)
        if (cause != 0 && run_collision < 0)
        {
          run_collision = my_k;
          run_cause = cause;
        }
        if (cause == 0 && without_value) run_no_value = true;
        if (kField)
        {
          const int sphere = record_sphere[lane];
          if (sphere >= 0)
          {
            const double clearance = record_clearance[lane];
            if (run_sample < 0 || clearance < run_clearance)
            {
              run_clearance = clearance;
              run_sample = my_k;
              run_sphere = sphere;
              run_ix = record_ix[lane], run_iy = record_iy[lane], run_iz = record_iz[lane];
            }
          }
        }
        if (self_pair >= 0 && (run_self_sample < 0 || self_best < run_self))
        {
          run_self = self_best;
          run_self_sample = my_k;
          run_self_pair = self_pair;
        }
        run_bits |= bits;
      }
      __syncthreads();  // (the tile's reads are done)
      if (stop_k >= 0) break;
    }

    // ---- the motion's verdict: the lanes' records combined ----
    double winner = run_clearance, self_winner = run_self;
    int winner_sample = run_sample, winner_sphere = run_sphere;
    int self_winner_sample = run_self_sample, self_winner_pair = run_self_pair;
    int first_collision = run_collision, first_cause = run_cause;
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
      const double self_other = __shfl_xor(self_winner, offset);
      const int self_other_sample = __shfl_xor(self_winner_sample, offset);
      const int self_other_pair = __shfl_xor(self_winner_pair, offset);
      if (BetterSphere(self_other, self_other_sample, self_winner, self_winner_sample))
      {
        self_winner = self_other;
        self_winner_sample = self_other_sample;
        self_winner_pair = self_other_pair;
      }
      const int other_collision = __shfl_xor(first_collision, offset);
      const int other_cause = __shfl_xor(first_cause, offset);
      if (other_collision >= 0 && (first_collision < 0 || other_collision < first_collision))
      {
        first_collision = other_collision;
        first_cause = other_cause;
      }
    }
    const bool any_no_value = __ballot(run_no_value) != 0;
    const uint8_t fk_status =
        static_cast<uint8_t>((__ballot((run_bits & 1) != 0) ? 1 : 0) | (__ballot((run_bits & 2) != 0) ? 2 : 0));
    if (lane == 0)
    {
      out.status[e] = first_collision >= 0 ? kMotionSelfCollision : any_no_value ? kMotionSelfNoValue : kMotionSelfClear;
      if (out.first_collision) out.first_collision[e] = first_collision;
      if (out.collision_cause) out.collision_cause[e] = first_collision >= 0 ? static_cast<uint8_t>(first_cause) : 0;
      if (out.self_min_clearance) out.self_min_clearance[e] = self_winner_sample >= 0 ? self_winner : nan;
      if (out.self_min_sample) out.self_min_sample[e] = self_winner_sample;
      if (out.self_min_pair) out.self_min_pair[e] = self_winner_sample >= 0 ? self_winner_pair : -1;
      if (out.fk_status) out.fk_status[e] = fk_status;
    }
    const bool writer = winner_sample >= 0 ? run_sample == winner_sample : lane == 0;
    if (writer)
    {
      if (out.min_clearance) out.min_clearance[e] = winner_sample >= 0 ? winner : nan;
      if (out.min_sample) out.min_sample[e] = winner_sample;
      if (out.min_sphere) out.min_sphere[e] = winner_sample >= 0 ? winner_sphere : -1;
      if (out.min_gradient)
      {
        double gx = nan, gy = nan, gz = nan;
        if (kField && winner_sample >= 0)
          CoarseGradientAt(sdf, nx, ny, nz, sx, sy, resolution, 1, rot, run_ix * sx + run_iy * sy + run_iz, run_ix, run_iy,
                           run_iz, gx, gy, gz);
        out.min_gradient[3 * e] = gx;
        out.min_gradient[3 * e + 1] = gy;
        out.min_gradient[3 * e + 2] = gz;
      }
    }
  }
}

// The bytes of dynamic LDS of a launch.
size_t MotionSelfLdsBytes(int64_t num_links, int64_t num_spheres, int tile)
{
  return (static_cast<size_t>(num_links) * kMotionSelfPoseBytesPerLink +
          static_cast<size_t>(num_spheres) * kMotionSelfCentreBytes) *
             static_cast<size_t>(tile) +
         static_cast<size_t>(num_spheres) * 8 + kMotionSelfRecordBytes;
}
}  // namespace

int MotionSelfTileSamples(int64_t num_links, int64_t num_spheres)
{
  if (num_links <= 0 || num_spheres < 0) return 0;
  // (before any product: neither alone may fill the LDS)
  if (num_links > static_cast<int64_t>(kMotionSelfLdsLimit / kMotionSelfPoseBytesPerLink) ||
      num_spheres > static_cast<int64_t>(kMotionSelfLdsLimit / kMotionSelfCentreBytes))
    return 0;
  if (MotionSelfLdsBytes(num_links, num_spheres, 1) > kMotionSelfLdsLimit) return 0;
  const size_t per_sample = static_cast<size_t>(num_links) * kMotionSelfPoseBytesPerLink +
                            static_cast<size_t>(num_spheres) * kMotionSelfCentreBytes;
  int tile = 64;
  while (tile > 1 && (per_sample * static_cast<size_t>(tile) > VGT_MOTION_SELF_TILE_BYTES ||
                      MotionSelfLdsBytes(num_links, num_spheres, tile) > kMotionSelfLdsLimit))
    tile >>= 1;
  return tile;
}

hipError_t LaunchCheckMotionsWithSelf(const float* sdf_dev, int64_t nx, int64_t ny, int64_t nz, double resolution,
                                      const double* grid_from_world_host, const double* rotation_host,
                                      const double* sphere_xyzr_dev, const int32_t* sphere_link_dev, int64_t num_spheres,
                                      const int32_t* pairs_dev, int64_t num_pairs, const KinematicLink* links_dev,
                                      int64_t num_links, int64_t num_joints, const double* joint_from_dev,
                                      const double* joint_to_dev, const int32_t* num_steps_dev, int32_t uniform_steps,
                                      int64_t num_motions, const double* world_from_base_host, const double* limits_dev,
                                      double minimum_clearance, double self_minimum_clearance, int outside_is_collision,
                                      int no_value_is_collision, int stop_at_collision, const MotionSelfOutputs& out,
                                      int max_workgroups, hipStream_t stream)
{
  if (num_motions <= 0) return hipSuccess;
  if (!sdf_dev && num_pairs <= 0) return hipErrorInvalidValue;
  const int tile = MotionSelfTileSamples(num_links, num_spheres);
  if (tile <= 0) return hipErrorInvalidValue;
  int log2_tile = 0;
  while ((1 << log2_tile) < tile) log2_tile++;
  const int log2_width = CheckSpheresWidthLog2(num_spheres);
  const size_t lds_bytes = MotionSelfLdsBytes(num_links, num_spheres, tile);
  const int64_t most = max_workgroups > 0 ? max_workgroups : kMotionSelfMaxWorkgroups;
  const int64_t workgroups = num_motions < most ? num_motions : most;
  const MotionSelfTree tree{links_dev, limits_dev, static_cast<int>(num_links), static_cast<int>(num_joints)};
  // (a model without spheres has no pair with a value and none without: the list is not read)
  const MotionSelfModel model{sphere_xyzr_dev,
                              sphere_link_dev,
                              pairs_dev,
                              static_cast<int>(num_spheres),
                              num_spheres > 0 ? num_pairs : 0,
                              num_pairs > 0 ? 1 : 0};
  const MotionSelfBatch batch{joint_from_dev, joint_to_dev, num_steps_dev, uniform_steps, num_motions};
  const MotionSelfQuery query{minimum_clearance, self_minimum_clearance, outside_is_collision ? 1 : 0,
                              no_value_is_collision ? 1 : 0, stop_at_collision ? 1 : 0};
  const KinematicsBase base = MakeKinematicsBase(world_from_base_host);
  if (sdf_dev)
    hipLaunchKernelGGL(CheckMotionsWithSelfKernel<true>, dim3(static_cast<unsigned>(workgroups)),
                       dim3(kMotionSelfThreads), lds_bytes, stream, sdf_dev, static_cast<int>(nx), static_cast<int>(ny),
                       static_cast<int>(nz), resolution, MakeGridFromWorld(grid_from_world_host),
                       MakeRotation(rotation_host), tree, base, model, batch, query, log2_width, log2_tile, out);
  else
    hipLaunchKernelGGL(CheckMotionsWithSelfKernel<false>, dim3(static_cast<unsigned>(workgroups)),
                       dim3(kMotionSelfThreads), lds_bytes, stream, static_cast<const float*>(nullptr), 0, 0, 0, 1.0,
                       MakeGridFromWorld(nullptr), MakeRotation(nullptr), tree, base, model, batch, query, log2_width,
                       log2_tile, out);
  return hipGetLastError();
}
}  // namespace vgt
