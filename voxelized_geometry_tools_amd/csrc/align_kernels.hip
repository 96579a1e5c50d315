// Point clouds aligned to an SDF for gfx950: B pose hypotheses of a cloud of N points, scored and refined by damped
// Gauss-Newton steps on the trilinear distance estimate.  The definition -- the evaluation, the one summation tree, the
// solve, the update, the loop -- and every output: include/vgt_hip.h, vgt_hip_align_points.  Four kernels, and nothing
// between them but kernel boundaries (no flags polled, no floating-point atomics, no host round trip):
//
//   AlignStartKernel     copies the poses into the workspace and marks every pose as running.
//   AlignEvaluateKernel  the hot path: the eight gathers of the estimate per (pose, point), the gradient of the
//                        interpolant from those corners, the 28 terms, and the first two levels of the tree.
//   AlignReduceKernel    one further level of the tree (64 partial records -> 1), launched while a pose has more than
//                        64 records left.
//   AlignSolveKernel     the last level, then per pose on one lane: bookkeeping, the 6 x 6 solve and the update.
//
// Work mapping of the evaluation.  One lane per (pose, point); a wave owns a GROUP of 64 consecutive points of one pose
// and reduces each term over it by the halving tree (lane i adds lane i + h: two ds_bpermute steps across the rows of
// 16 lanes, four DPP row shifts inside them); a workgroup owns a BLOCK of 4096 consecutive points, its 64 groups dealt
// evenly to its waves (4 waves of 16 groups, or 16 waves of 4: kAlignWideItems); the 64 group sums per term go to LDS
// ([term][group], 14 KiB) and are reduced there by the same tree, the terms dealt to the waves.  One record of 32
// doubles per (pose, block) goes to the workspace: the 28 sums and the three counts (as doubles: they are below 2^31 and
// their sums exact in any order).  Workgroups are persistent and stride over the (pose, block) items; the pose is read
// once per item; an item of a pose that has stopped is skipped on the flag the solve kernel wrote in an earlier launch.
//
// In bounds by construction: a lane with point index >= N forms no address; the field is read only through LocateCell's
// in-grid indices; record and pose addresses come from item < B * blocks.
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Wunused-function"
#include "sdf_sampling.hpp"
#pragma clang diagnostic pop
#include "vgt_internal.hpp"
#include "../../include/vgt_hip.h"

#include <cmath>

namespace vgt
{
namespace
{
constexpr int kAlignThreads = 256;  // of the small kernels, and of the evaluation when there are many items
constexpr int kAlignWaves = kAlignThreads / 64;
constexpr int kAlignBlockPoints = 64 * 64;  // a block: 64 groups of 64 points
// The evaluation with 16 waves per workgroup instead of 4 (4 groups per wave instead of 16): the same sums, a quarter of
// the dependent trips per item, one workgroup per CU instead of four.  Taken while the items are fewer than the narrow
// form keeps busy at once (four workgroups on each of 256 CUs): at 1024 items the two take the same number of rounds.
constexpr int kAlignWideThreads = 1024;
constexpr int64_t kAlignWideItems = 768;
constexpr int kAlignTerms = 28;   // H (21), b (6), e (1)
constexpr int kAlignSlots = 31;   // the terms, then num_used, num_outside, num_rejected
constexpr int kAlignRecord = 32;  // doubles per record (one slot of padding)
// Workgroups of an evaluation launch: eight per CU on 256 CUs; the items beyond that by striding.
constexpr int kAlignMaxWorkgroups = 2048;
constexpr int32_t kPoseStopped = 0, kPoseRunning = 1, kPoseLastEvaluation = 2;

struct AlignWorkspace
{
  double* poses;     // [B][16], the poses in progress
  int32_t* state;    // [B] kPose*
  int32_t* evaluations;  // [B]
  double* records[2];    // [B][blocks][32] and [B][ceil(blocks / 64)][32]
  size_t bytes;
};

inline size_t AlignUp(size_t bytes) { return (bytes + 255) / 256 * 256; }

AlignWorkspace CarveAlignWorkspace(void* base, int64_t num_points, int64_t num_poses)
{
  const size_t b = static_cast<size_t>(num_poses);
  const size_t blocks = static_cast<size_t>((num_points + kAlignBlockPoints - 1) / kAlignBlockPoints);
  const size_t second = (blocks + 63) / 64;
  char* p = static_cast<char*>(base);
  size_t offset = 0;
  AlignWorkspace w;
  w.poses = reinterpret_cast<double*>(p + offset);
  offset += AlignUp(b * 16 * sizeof(double));
  w.state = reinterpret_cast<int32_t*>(p + offset);
  offset += AlignUp(b * sizeof(int32_t));
  w.evaluations = reinterpret_cast<int32_t*>(p + offset);
  offset += AlignUp(b * sizeof(int32_t));
  w.records[0] = reinterpret_cast<double*>(p + offset);
  offset += AlignUp(b * blocks * kAlignRecord * sizeof(double));
  w.records[1] = reinterpret_cast<double*>(p + offset);
  offset += AlignUp(b * second * kAlignRecord * sizeof(double));
  w.bytes = offset;
  return w;
}

// Lane i reads lane i + kShift of its row of 16 lanes (DPP row_shl); a lane without such a lane reads 0.
template <int kShift>
__device__ __forceinline__ double RowShiftLeft(double v)
{
  const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(v), 0x100 + kShift, 0xf, 0xf, false);
  const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(v), 0x100 + kShift, 0xf, 0xf, false);
  return __hiloint2double(hi, lo);
}

// The halving tree over the 64 lanes: for h in 32 ... 1, lane i < h becomes v[i] + v[i + h].  Lane 0 holds the sum; the
// other lanes hold what the tree does not use.  Every lane of the wave must be here.
__device__ __forceinline__ double WaveTreeSum(double v)
{
  v = v + __shfl_down(v, 32);
  v = v + __shfl_down(v, 16);
  v = v + RowShiftLeft<8>(v);
  v = v + RowShiftLeft<4>(v);
  v = v + RowShiftLeft<2>(v);
  v = v + RowShiftLeft<1>(v);
  return v;
}

__device__ __forceinline__ bool Finite(double v) { return fabs(v) <= 1.7976931348623157e308; }  // false for NaN

struct AlignResidual
{
  double target_distance, max_residual;
  double pivot[3];
};

__global__ __launch_bounds__(kAlignThreads) void AlignStartKernel(const double* __restrict__ poses_in, int64_t num_poses,
                                                                  double* __restrict__ poses, int32_t* __restrict__ state,
                                                                  int32_t* __restrict__ evaluations)
{
  const int64_t i = static_cast<int64_t>(blockIdx.x) * kAlignThreads + threadIdx.x;
  if (i >= num_poses * 16) return;
  poses[i] = poses_in[i];
  if ((i & 15) == 0)
  {
    state[i >> 4] = kPoseRunning;
    evaluations[i >> 4] = 0;
  }
}

template <int kThreads>
__global__ __launch_bounds__(kThreads) void AlignEvaluateKernel(
    const float* __restrict__ sdf, int nx, int ny, int nz, double resolution, const GridFromWorld xf, const Rotation rot,
    const float* __restrict__ points, int64_t num_points, int64_t num_poses, int64_t num_blocks,
    const double* __restrict__ poses, const int32_t* __restrict__ state, const AlignResidual residual,
    double* __restrict__ records)
{
  constexpr int kWaves = kThreads / 64, kGroupsPerWave = 64 / kWaves;
  __shared__ double group_sums[kAlignTerms * 64];  // [term][group of the block]
  __shared__ int wave_counts[kWaves * 3];

  const int lane = static_cast<int>(threadIdx.x) & 63, wave = static_cast<int>(threadIdx.x) >> 6;
  const int64_t items = num_poses * num_blocks;
  for (int64_t item = blockIdx.x; item < items; item += gridDim.x)
  {
    const int64_t b = item / num_blocks, block = item - b * num_blocks;
    if (state[b] == kPoseStopped) continue;  // (the same for the whole workgroup)
    const double* m = poses + b * 16;
    const double m0 = m[0], m1 = m[1], m2 = m[2], m4 = m[4], m5 = m[5], m6 = m[6], m8 = m[8], m9 = m[9], m10 = m[10],
                 m12 = m[12], m13 = m[13], m14 = m[14];
    int num_used = 0, num_outside = 0, num_rejected = 0;
    for (int j = 0; j < kGroupsPerWave; j++)
    {
      const int group = wave * kGroupsPerWave + j;
      const int64_t first = block * kAlignBlockPoints + static_cast<int64_t>(group) * 64;
      if (first >= num_points)
      {
        // a group of padding alone: its tree sums +0.0 to +0.0
        if (lane < kAlignTerms) group_sums[lane * 64 + group] = 0.0;
        continue;
      }
      const int64_t i = first + lane;
      double term[kAlignTerms];
#pragma unroll
      for (int t = 0; t < kAlignTerms; t++) term[t] = 0.0;
      bool finite_point = false, has_value = false, used = false;
      if (i < num_points)
      {
        const double x = static_cast<double>(points[3 * i]), y = static_cast<double>(points[3 * i + 1]),
                     z = static_cast<double>(points[3 * i + 2]);
        finite_point = Finite(x) && Finite(y) && Finite(z);
        if (finite_point)
        {
          const double w0 = ((m0 * x + m4 * y) + m8 * z) + m12;
          const double w1 = ((m1 * x + m5 * y) + m9 * z) + m13;
          const double w2 = ((m2 * x + m6 * y) + m10 * z) + m14;
          CellOfLocation c;
          if (LocateCell(nx, ny, nz, resolution, xf, w0, w1, w2, c))
          {
            has_value = true;
            const CornerDistances k = LoadCorners(sdf, ny, nz, resolution, c);
            const double d = InterpolateCorners(c, k, resolution);
            // the weights and spans, as InterpolateCorners forms them
            const double low_x = (static_cast<double>(c.lx) + 0.5) * resolution;
            const double low_y = (static_cast<double>(c.ly) + 0.5) * resolution;
            const double low_z = (static_cast<double>(c.lz) + 0.5) * resolution;
            const double ex = (low_x + resolution) - low_x, ey = (low_y + resolution) - low_y,
                         ez = (low_z + resolution) - low_z;
            const double tx = (c.g[0] - low_x) / ex, ty = (c.g[1] - low_y) / ey, tz = (c.g[2] - low_z) / ez;
            double gx = Lerp(Lerp(k.pmm - k.mmm, k.ppm - k.mpm, ty), Lerp(k.pmp - k.mmp, k.ppp - k.mpp, ty), tz) / ex;
            double gy = Lerp(Lerp(k.mpm - k.mmm, k.ppm - k.pmm, tx), Lerp(k.mpp - k.mmp, k.ppp - k.pmp, tx), tz) / ey;
            double gz = Lerp(Lerp(k.mmp - k.mmm, k.pmp - k.pmm, tx), Lerp(k.mpp - k.mpm, k.ppp - k.ppm, tx), ty) / ez;
            if (rot.enabled)
            {
              const double rx = rot.m[0] * gx + rot.m[1] * gy + rot.m[2] * gz;
              const double ry = rot.m[3] * gx + rot.m[4] * gy + rot.m[5] * gz;
              const double rz = rot.m[6] * gx + rot.m[7] * gy + rot.m[8] * gz;
              gx = rx, gy = ry, gz = rz;
            }
            const double r = d - residual.target_distance;
            used = Finite(r) && Finite(gx) && Finite(gy) && Finite(gz) && fabs(r) <= residual.max_residual;
            if (used)
            {
              const double q0 = w0 - residual.pivot[0], q1 = w1 - residual.pivot[1], q2 = w2 - residual.pivot[2];
              double J[6];
              J[0] = gx, J[1] = gy, J[2] = gz;
              J[3] = q1 * gz - q2 * gy;
              J[4] = q2 * gx - q0 * gz;
              J[5] = q0 * gy - q1 * gx;
              int t = 0;
#pragma unroll
              for (int a = 0; a < 6; a++)
#pragma unroll
                for (int e = a; e < 6; e++) term[t++] = J[a] * J[e];
#pragma unroll
              for (int a = 0; a < 6; a++) term[21 + a] = J[a] * r;
              term[27] = r * r;
            }
          }
        }
      }
      num_used += __popcll(__ballot(used));
      num_outside += __popcll(__ballot(finite_point && !has_value));
      num_rejected += __popcll(__ballot(has_value && !used));
#pragma unroll
      for (int t = 0; t < kAlignTerms; t++)
      {
        const double sum = WaveTreeSum(term[t]);
        if (lane == 0) group_sums[t * 64 + group] = sum;
      }
    }
    if (lane == 0)
    {
      wave_counts[wave * 3] = num_used;
      wave_counts[wave * 3 + 1] = num_outside;
      wave_counts[wave * 3 + 2] = num_rejected;
    }
    __syncthreads();
    double* record = records + item * kAlignRecord;
    // the second level: the 64 group sums of a term; a cloud of one group is that group's sum as it stands
    const bool one_group = num_points <= 64;
    for (int t = wave; t < kAlignTerms; t += kWaves)
    {
      const double sum = one_group ? group_sums[t * 64] : WaveTreeSum(group_sums[t * 64 + lane]);
      if (lane == 0) record[t] = sum;
    }
    if (threadIdx.x < 3)
    {
      int count = 0;
      for (int w = 0; w < kWaves; w++) count += wave_counts[w * 3 + static_cast<int>(threadIdx.x)];
      record[kAlignTerms + threadIdx.x] = static_cast<double>(count);
    }
    __syncthreads();  // (the next item writes the two arrays again)
  }
}

// One level of the tree above the blocks: record g of a pose's output list is the tree sum of its input records
// 64 g ... 64 g + 63, slot by slot, the list padded with +0.0.  One wave per (pose, output record).
__global__ __launch_bounds__(kAlignThreads) void AlignReduceKernel(const double* __restrict__ in, int64_t num_in,
                                                                   double* __restrict__ out, int64_t num_out,
                                                                   int64_t num_poses, const int32_t* __restrict__ state)
{
  const int lane = static_cast<int>(threadIdx.x) & 63, wave = static_cast<int>(threadIdx.x) >> 6;
  const int64_t items = num_poses * num_out, waves = static_cast<int64_t>(gridDim.x) * kAlignWaves;
  for (int64_t item = static_cast<int64_t>(blockIdx.x) * kAlignWaves + wave; item < items; item += waves)
  {
    const int64_t b = item / num_out, g = item - b * num_out;
    if (state[b] == kPoseStopped) continue;
    const int64_t entry = g * 64 + lane;
    const double* source = in + (b * num_in + (entry < num_in ? entry : 0)) * kAlignRecord;
    for (int slot = 0; slot < kAlignSlots; slot++)
    {
      const double sum = WaveTreeSum(entry < num_in ? source[slot] : 0.0);
      if (lane == 0) out[item * kAlignRecord + slot] = sum;
    }
  }
}

// The last level (num_in <= 64 records per pose), then everything that happens once per pose and evaluation, on lane 0
// of the pose's wave.  `iteration`: how many steps the poses still running have taken (0 after the first evaluation).
__global__ __launch_bounds__(kAlignThreads) void AlignSolveKernel(const double* __restrict__ records, int64_t num_in,
                                                                  int64_t num_poses, int iteration,
                                                                  const AlignOptions options, double* __restrict__ poses,
                                                                  int32_t* __restrict__ state,
                                                                  int32_t* __restrict__ evaluations,
                                                                  const AlignOutputs out)
{
  const int lane = static_cast<int>(threadIdx.x) & 63, wave = static_cast<int>(threadIdx.x) >> 6;
  const int64_t b = static_cast<int64_t>(blockIdx.x) * kAlignWaves + wave;
  if (b >= num_poses) return;  // (the whole wave)
  const int32_t running = state[b];
  if (running == kPoseStopped) return;

  double sums[kAlignSlots];
  const double* source = records + (b * num_in + (lane < num_in ? lane : 0)) * kAlignRecord;
#pragma unroll
  for (int slot = 0; slot < kAlignSlots; slot++)
    sums[slot] = num_in == 1 ? source[slot] : WaveTreeSum(lane < num_in ? source[slot] : 0.0);
  if (lane != 0) return;

  const int num_used = static_cast<int>(sums[28]);
  const int count = evaluations[b] + 1;
  evaluations[b] = count;
  if (out.num_used) out.num_used[b] = num_used;
  if (out.num_outside) out.num_outside[b] = static_cast<int>(sums[29]);
  if (out.num_rejected) out.num_rejected[b] = static_cast<int>(sums[30]);
  if (out.sum_squared) out.sum_squared[b] = sums[27];
  if (out.evaluations) out.evaluations[b] = count;
  if (out.normal_equations)
    for (int t = 0; t < 27; t++) out.normal_equations[b * 27 + t] = sums[t];
  if (out.last_step && iteration == 0)
    for (int r = 0; r < 6; r++) out.last_step[b * 6 + r] = 0.0;

  double* m = poses + b * 16;
  int status = -1;
  if (num_used < options.min_points)
    status = VGT_HIP_ALIGN_TOO_FEW;
  else if (running == kPoseLastEvaluation)
    status = VGT_HIP_ALIGN_CONVERGED;
  else if (iteration >= options.max_iterations)
    status = VGT_HIP_ALIGN_ITERATION_LIMIT;
  else
  {
    // A = L D L^T, column by column
    double A[6][6], L[6][6], D[6];
    {
      int t = 0;
#pragma unroll
      for (int j = 0; j < 6; j++)
#pragma unroll
        for (int k = j; k < 6; k++)
        {
          A[j][k] = sums[t];
          A[k][j] = sums[t];
          t++;
        }
    }
    const double scale = 1.0 + options.damping;
#pragma unroll
    for (int j = 0; j < 6; j++) A[j][j] = A[j][j] * scale;
    bool degenerate = false;
#pragma unroll
    for (int j = 0; j < 6; j++)
    {
      double d = A[j][j];
#pragma unroll
      for (int k = 0; k < j; k++) d = d - (L[j][k] * L[j][k]) * D[k];
      D[j] = d;
      if (!(d > 0.0)) degenerate = true;
#pragma unroll
      for (int i = j + 1; i < 6; i++)
      {
        double l = A[i][j];
#pragma unroll
        for (int k = 0; k < j; k++) l = l - (L[i][k] * L[j][k]) * D[k];
        L[i][j] = l / d;
      }
    }
    double step[6];
    {
      double y[6], x[6];
#pragma unroll
      for (int i = 0; i < 6; i++)
      {
        double v = sums[21 + i];
#pragma unroll
        for (int k = 0; k < i; k++) v = v - L[i][k] * y[k];
        y[i] = v;
      }
#pragma unroll
      for (int i = 5; i >= 0; i--)
      {
        double v = y[i] / D[i];
#pragma unroll
        for (int k = i + 1; k < 6; k++) v = v - L[k][i] * x[k];
        x[i] = v;
      }
#pragma unroll
      for (int i = 0; i < 6; i++)
      {
        step[i] = -x[i];
        if (!Finite(step[i])) degenerate = true;
      }
    }
    if (degenerate)
      status = VGT_HIP_ALIGN_DEGENERATE;
    else
    {
      const double ax = step[3] * 0.5, ay = step[4] * 0.5, az = step[5] * 0.5;
      const double s = 1.0 + ((ax * ax + ay * ay) + az * az);
      const double f = 2.0 / s;
      double R[3][3];
      R[0][0] = 1.0 - f * (ay * ay + az * az), R[0][1] = f * (ax * ay - az), R[0][2] = f * (ax * az + ay);
      R[1][0] = f * (ax * ay + az), R[1][1] = 1.0 - f * (ax * ax + az * az), R[1][2] = f * (ay * az - ax);
      R[2][0] = f * (ax * az - ay), R[2][1] = f * (ay * az + ax), R[2][2] = 1.0 - f * (ax * ax + ay * ay);
      double next[12];
#pragma unroll
      for (int c = 0; c < 3; c++)
#pragma unroll
        for (int r = 0; r < 3; r++)
          next[c * 3 + r] = (R[r][0] * m[4 * c] + R[r][1] * m[4 * c + 1]) + R[r][2] * m[4 * c + 2];
      const double u0 = m[12] - options.pivot[0], u1 = m[13] - options.pivot[1], u2 = m[14] - options.pivot[2];
#pragma unroll
      for (int r = 0; r < 3; r++)
        next[9 + r] = (((R[r][0] * u0 + R[r][1] * u1) + R[r][2] * u2) + options.pivot[r]) + step[r];
#pragma unroll
      for (int c = 0; c < 4; c++)
#pragma unroll
        for (int r = 0; r < 3; r++) m[4 * c + r] = next[c * 3 + r];
      if (out.last_step)
        for (int r = 0; r < 6; r++) out.last_step[b * 6 + r] = step[r];
      const double most_v = fmax(fmax(fabs(step[0]), fabs(step[1])), fabs(step[2]));
      const double most_w = fmax(fmax(fabs(step[3]), fabs(step[4])), fabs(step[5]));
      if (most_v <= options.translation_tolerance && most_w <= options.rotation_tolerance) state[b] = kPoseLastEvaluation;
    }
  }
  if (status >= 0)
  {
    state[b] = kPoseStopped;
    out.status[b] = static_cast<uint8_t>(status);
    if (out.poses)
      for (int k = 0; k < 16; k++) out.poses[b * 16 + k] = m[k];
  }
}
}  // namespace

size_t AlignWorkspaceBytes(int64_t num_points, int64_t num_poses)
{
  const int64_t most = 0x7fffffffLL;
  if (num_points <= 0 || num_poses <= 0 || num_points > most || num_poses > most) return 0;
  const int64_t blocks = (num_points + kAlignBlockPoints - 1) / kAlignBlockPoints;
  if (num_poses * blocks > most) return 0;
  return CarveAlignWorkspace(nullptr, num_points, num_poses).bytes;
}

hipError_t LaunchAlignPoints(const float* sdf_dev, int64_t nx, int64_t ny, int64_t nz, double resolution,
                             const double* grid_from_world_host, const double* rotation_host,
                             const float* points_xyz_dev, int64_t num_points, const double* poses_dev,
                             int64_t num_poses, const AlignOptions& options, const AlignOutputs& out,
                             void* workspace_dev, int max_workgroups, hipStream_t stream)
{
  if (AlignWorkspaceBytes(num_points, num_poses) == 0 || !workspace_dev) return hipErrorInvalidValue;
  const AlignWorkspace ws = CarveAlignWorkspace(workspace_dev, num_points, num_poses);
  const int64_t blocks = (num_points + kAlignBlockPoints - 1) / kAlignBlockPoints;
  const int64_t items = num_poses * blocks;
  const int64_t most = max_workgroups > 0 ? max_workgroups : kAlignMaxWorkgroups;
  const unsigned evaluate_grid = static_cast<unsigned>(items < most ? items : most);
  const unsigned solve_grid = static_cast<unsigned>((num_poses + kAlignWaves - 1) / kAlignWaves);
  const GridFromWorld xf = MakeGridFromWorld(grid_from_world_host);
  const Rotation rot = MakeRotation(rotation_host);
  const AlignResidual residual{options.target_distance, options.max_residual,
                               {options.pivot[0], options.pivot[1], options.pivot[2]}};

  hipLaunchKernelGGL(AlignStartKernel, dim3(static_cast<unsigned>((num_poses * 16 + kAlignThreads - 1) / kAlignThreads)),
                     dim3(kAlignThreads), 0, stream, poses_dev, num_poses, ws.poses, ws.state, ws.evaluations);
  hipError_t err = hipGetLastError();
  for (int iteration = 0; iteration <= options.max_iterations && err == hipSuccess; iteration++)
  {
    if (items <= kAlignWideItems)
      hipLaunchKernelGGL(AlignEvaluateKernel<kAlignWideThreads>, dim3(evaluate_grid), dim3(kAlignWideThreads), 0, stream,
                         sdf_dev, static_cast<int>(nx), static_cast<int>(ny), static_cast<int>(nz), resolution, xf, rot,
                         points_xyz_dev, num_points, num_poses, blocks, ws.poses, ws.state, residual, ws.records[0]);
    else
      hipLaunchKernelGGL(AlignEvaluateKernel<kAlignThreads>, dim3(evaluate_grid), dim3(kAlignThreads), 0, stream, sdf_dev,
                         static_cast<int>(nx), static_cast<int>(ny), static_cast<int>(nz), resolution, xf, rot,
                         points_xyz_dev, num_points, num_poses, blocks, ws.poses, ws.state, residual, ws.records[0]);
    err = hipGetLastError();
    int from = 0;
    int64_t num_in = blocks;
    while (num_in > 64 && err == hipSuccess)
    {
      const int64_t num_out = (num_in + 63) / 64;
      const int64_t groups = (num_poses * num_out + kAlignWaves - 1) / kAlignWaves;
      hipLaunchKernelGGL(AlignReduceKernel, dim3(static_cast<unsigned>(groups < most ? groups : most)),
                         dim3(kAlignThreads), 0, stream, ws.records[from], num_in, ws.records[1 - from], num_out,
                         num_poses, ws.state);
      err = hipGetLastError();
      from = 1 - from;
      num_in = num_out;
    }
    if (err != hipSuccess) break;
    hipLaunchKernelGGL(AlignSolveKernel, dim3(solve_grid), dim3(kAlignThreads), 0, stream, ws.records[from], num_in,
                       num_poses, iteration, options, ws.poses, ws.state, ws.evaluations, out);
    err = hipGetLastError();
  }
  return err;
}
}  // namespace vgt
