// Inverse kinematics for gfx950: tip poses to joint values by damped least-squares steps.  Semantics and every output:
// include/vgt_hip.h, vgt_hip_solve_ik.  Everything is plain double arithmetic in the header's order (the build's
// -ffp-contract=off keeps every operator on its own); the chain's poses are made by the link steps of
// kinematics_math.hpp, so they are the forward kinematics' bits by construction.
//
// One lane per problem, a workgroup is one wave: nothing here needs a barrier, and the lanes may diverge.  A lane whose
// problem has stopped idles until the wave's last one stops.  The chain (its links, base first) and the link table are
// the same for every lane: the indices are wave-uniform, the loads are scalar.
//
// Where things live:
//   registers   the pose being walked, the target, e, A and the solve;
//   LDS         per moving chain link the six doubles (a, o) that its column needs -- the axis in the world and the
//               link's origin --, written by the walk from the base to the tip and read by the walk back:
//               tile[slot][component][lane], doubles, so consecutive lanes touch consecutive 8-byte words (no bank
//               conflicts); 3 KiB per slot, sized by the chain's moving links, 48 KiB at kIkMaxChainJoints.  Once a
//               link's dq is known its slot's first word holds it (the column is not needed again);
//   the output  the lane's working row of joint values is its own row of `joints`: same lane, same address, program
//               order, as the forward kinematics reads back its own poses.
//
// Waves are persistent: workgroup w takes the groups of 64 problems w, w + workgroups, ...
//
// In bounds by construction: a lane with b >= B forms no address; the chain's links are in [0, L) and joint_index in
// [0, J) on links that are not fixed (validated on the host); a slot index stays below the chain's moving links, which
// sized the LDS.
#include "kinematics_math.hpp"
#include "vgt_internal.hpp"

#include "../../include/vgt_hip.h"

#include <cmath>

namespace vgt
{
namespace
{
constexpr int kIkThreads = 64;  // one wave per workgroup
// Workgroups of a launch: three per CU by the LDS of a full chain, on 256 CUs, a few rounds of them.
constexpr int kIkMaxWorkgroups = 4096;

struct IkChain
{
  const KinematicLink* links;
  const int32_t* chain;  // [chain_links], base first
  int chain_links, moving_links, num_joints;
};

__device__ __forceinline__ bool IkFinite(double v) { return fabs(v) <= 0x1.fffffffffffffp+1023; }

// The weighted column of a moving link from its (a, o) in LDS and the tip's translation p.
__device__ __forceinline__ void IkColumn(const double* kept, int joint_type, const double* p, const double* w, double* c)
{
  const double a0 = kept[0], a1 = kept[kIkThreads], a2 = kept[2 * kIkThreads];
  if (joint_type == kJointRevolute)
  {
    const double d0 = p[0] - kept[3 * kIkThreads], d1 = p[1] - kept[4 * kIkThreads], d2 = p[2] - kept[5 * kIkThreads];
    c[0] = a1 * d2 - a2 * d1, c[1] = a2 * d0 - a0 * d2, c[2] = a0 * d1 - a1 * d0;
    c[3] = a0, c[4] = a1, c[5] = a2;
  }
  else
  {
    c[0] = a0, c[1] = a1, c[2] = a2;
    c[3] = c[4] = c[5] = 0.0;
  }
#pragma unroll
  for (int k = 0; k < 6; k++) c[k] = w[k] * c[k];
}

__global__ __launch_bounds__(kIkThreads) void SolveIkKernel(const IkChain tree, const double* __restrict__ targets,
                                                            int64_t seeds_per_target, const double* seeds,
                                                            int64_t num_problems, const KinematicsBase base,
                                                            const double* __restrict__ limits, const IkOptions options,
                                                            const IkOutputs out)
{
  extern __shared__ __attribute__((aligned(16))) double tile[];  // [moving_links][6][64]
  const int lane = static_cast<int>(threadIdx.x);
  const int J = tree.num_joints;
  const int64_t groups = (num_problems + kIkThreads - 1) / kIkThreads;
  double w[6];
#pragma unroll
  for (int k = 0; k < 6; k++) w[k] = options.weights[k];
  const bool whole_rotation = w[3] != 0.0 && w[4] != 0.0 && w[5] != 0.0;
  for (int64_t group = blockIdx.x; group < groups; group += gridDim.x)
  {
    const int64_t b = group * kIkThreads + lane;
    if (b >= num_problems) continue;  // (no barrier anywhere below)
    double* q = out.joints + b * J;
    if (q != seeds + b * J)
      for (int j = 0; j < J; j++) q[j] = seeds[b * J + j];
    const auto joint = [&](int j) { return q[j]; };
    const double* target = targets + (b / seeds_per_target) * 16;
    double aim[12];  // aim[3 c + r]
#pragma unroll
    for (int c = 0; c < 4; c++)
#pragma unroll
      for (int r = 0; r < 3; r++) aim[3 * c + r] = target[4 * c + r];

    int steps = 0;
    uint8_t status, bits;
    LinkPose tip;
    double e[6];
    for (;;)
    {
      // evaluate: the chain's poses from the base to the tip; (a, o) of the moving links into LDS
      bits = 0;
      tip = LinkPose{};
      int slot = 0;
      for (int at = 0; at < tree.chain_links; at++)
      {
        const int i = tree.chain[at];
        const KinematicLink& link = tree.links[i];
        // (the parent of a chain link is the chain link before it: the pose in `tip`)
        const LinkPose previous = tip;
        const LinkPose frame = LinkFrame(link, i, base, previous, [&](int) { return previous; });
        tip = LinkPoseFromFrame(link, frame, joint, bits);
        if (link.joint_type != kJointFixed)
        {
          const double* m = tip.m;
          const double x = link.axis[0], y = link.axis[1], z = link.axis[2];
          double* kept = tile + (slot * 6) * kIkThreads + lane;
#pragma unroll
          for (int r = 0; r < 3; r++)
          {
            kept[r * kIkThreads] = (m[r] * x + m[3 + r] * y) + m[6 + r] * z;
            kept[(3 + r) * kIkThreads] = m[9 + r];
          }
          slot++;
        }
      }
      const double* m = tip.m;
#pragma unroll
      for (int r = 0; r < 3; r++) e[r] = aim[9 + r] - m[9 + r];
      double turn[3] = {0.0, 0.0, 0.0}, trace = 0.0;
#pragma unroll
      for (int c = 0; c < 3; c++)
      {
        const double a0 = m[3 * c], a1 = m[3 * c + 1], a2 = m[3 * c + 2];
        const double b0 = aim[3 * c], b1 = aim[3 * c + 1], b2 = aim[3 * c + 2];
        const double x0 = a1 * b2 - a2 * b1, x1 = a2 * b0 - a0 * b2, x2 = a0 * b1 - a1 * b0;
        const double dot = (a0 * b0 + a1 * b1) + a2 * b2;
        // (the sums start with their first terms: (x_0 + x_1) + x_2)
        turn[0] = c == 0 ? x0 : turn[0] + x0;
        turn[1] = c == 0 ? x1 : turn[1] + x1;
        turn[2] = c == 0 ? x2 : turn[2] + x2;
        trace = c == 0 ? dot : trace + dot;
      }
#pragma unroll
      for (int r = 0; r < 3; r++) e[3 + r] = turn[r] * 0.5;

      if (bits & 1)
      {
        status = VGT_HIP_IK_NOT_COMPUTABLE;
        break;
      }
      bool converged = true;
#pragma unroll
      for (int k = 0; k < 6; k++)
        if (w[k] != 0.0 && !(fabs(e[k]) <= (k < 3 ? options.position_tolerance : options.rotation_tolerance)))
          converged = false;
      if (whole_rotation && !(trace > 1.0)) converged = false;
      if (converged)
      {
        status = VGT_HIP_IK_CONVERGED;
        break;
      }
      if (steps >= options.max_iterations)
      {
        status = VGT_HIP_IK_ITERATION_LIMIT;
        break;
      }

      // step: A = sum c c^T over the chain from the tip to the base, damped; A y = the weighted e
      double A[6][6];
#pragma unroll
      for (int j = 0; j < 6; j++)
#pragma unroll
        for (int k = j; k < 6; k++) A[j][k] = 0.0;
      const double p[3] = {m[9], m[10], m[11]};
      slot = tree.moving_links;
      for (int at = tree.chain_links - 1; at >= 0; at--)
      {
        const KinematicLink& link = tree.links[tree.chain[at]];
        if (link.joint_type == kJointFixed) continue;
        slot--;
        double c[6];
        IkColumn(tile + (slot * 6) * kIkThreads + lane, link.joint_type, p, w, c);
#pragma unroll
        for (int j = 0; j < 6; j++)
#pragma unroll
          for (int k = j; k < 6; k++) A[j][k] = A[j][k] + c[j] * c[k];
      }
      const double damp = options.damping * options.damping;
#pragma unroll
      for (int j = 0; j < 6; j++) A[j][j] = A[j][j] + damp;
      double L[6][6], D[6], y[6];
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
          double l = A[j][i];
#pragma unroll
          for (int k = 0; k < j; k++) l = l - (L[i][k] * L[j][k]) * D[k];
          L[i][j] = l / d;
        }
      }
      {
        double forward[6];
#pragma unroll
        for (int i = 0; i < 6; i++)
        {
          double v = w[i] * e[i];
#pragma unroll
          for (int k = 0; k < i; k++) v = v - L[i][k] * forward[k];
          forward[i] = v;
        }
#pragma unroll
        for (int i = 5; i >= 0; i--)
        {
          double v = forward[i] / D[i];
#pragma unroll
          for (int k = i + 1; k < 6; k++) v = v - L[k][i] * y[k];
          y[i] = v;
        }
      }
#pragma unroll
      for (int i = 0; i < 6; i++)
        if (!IkFinite(y[i])) degenerate = true;
      if (degenerate)
      {
        status = VGT_HIP_IK_DEGENERATE;
        break;
      }
      // dq per moving link, kept in the first word of its slot; the largest of them
      double largest = 0.0;
      slot = tree.moving_links;
      for (int at = tree.chain_links - 1; at >= 0; at--)
      {
        const KinematicLink& link = tree.links[tree.chain[at]];
        if (link.joint_type == kJointFixed) continue;
        slot--;
        double* kept = tile + (slot * 6) * kIkThreads + lane;
        double c[6];
        IkColumn(kept, link.joint_type, p, w, c);
        const double dq = ((((c[0] * y[0] + c[1] * y[1]) + c[2] * y[2]) + c[3] * y[3]) + c[4] * y[4]) + c[5] * y[5];
        kept[0] = dq;
        if (fabs(dq) > largest) largest = fabs(dq);
      }
      const bool shorten = largest > options.max_step;
      const double scale = options.max_step / largest;
      slot = tree.moving_links;
      for (int at = tree.chain_links - 1; at >= 0; at--)
      {
        const KinematicLink& link = tree.links[tree.chain[at]];
        if (link.joint_type == kJointFixed) continue;
        slot--;
        double dq = tile[(slot * 6) * kIkThreads + lane];
        if (shorten) dq = dq * scale;
        const int j = link.joint_index;
        double value = q[j] + dq;
        if (limits)
        {
          const double lower = limits[2 * j], upper = limits[2 * j + 1];
          value = value < lower ? lower : value;
          value = value > upper ? upper : value;
        }
        q[j] = value;
      }
      steps++;
    }

    if (limits) bits |= LimitBits(limits, J, joint);
    out.status[b] = status;
    if (out.iterations) out.iterations[b] = steps;
    if (out.fk_status) out.fk_status[b] = bits;
    if (out.error)
    {
#pragma unroll
      for (int k = 0; k < 6; k++) out.error[b * 6 + k] = e[k];
    }
    if (out.tip_pose)
    {
      double* line = out.tip_pose + b * 16;
#pragma unroll
      for (int col = 0; col < 4; col++)
      {
#pragma unroll
        for (int r = 0; r < 3; r++) line[4 * col + r] = tip.m[3 * col + r];
        line[4 * col + 3] = col == 3 ? 1.0 : 0.0;
      }
    }
  }
}
}  // namespace

hipError_t LaunchSolveIk(const KinematicLink* links_dev, int64_t num_joints, const int32_t* chain_dev, int chain_links,
                         int moving_links, const double* targets_dev, int64_t seeds_per_target, const double* seeds_dev,
                         int64_t num_problems, const double* world_from_base_host, const double* limits_dev,
                         const IkOptions& options, const IkOutputs& out, int max_workgroups, hipStream_t stream)
{
  if (num_problems <= 0) return hipSuccess;
  if (chain_links <= 0 || moving_links < 0 || moving_links > kIkMaxChainJoints || moving_links > chain_links ||
      seeds_per_target <= 0 || (!out.joints && num_joints > 0) || !out.status)
    return hipErrorInvalidValue;
  const KinematicsBase base = MakeKinematicsBase(world_from_base_host);
  const IkChain tree{links_dev, chain_dev, chain_links, moving_links, static_cast<int>(num_joints)};
  const int64_t groups = (num_problems + kIkThreads - 1) / kIkThreads;
  const int64_t most = max_workgroups > 0 ? max_workgroups : kIkMaxWorkgroups;
  const int64_t workgroups = groups < most ? groups : most;
  const size_t lds_bytes = static_cast<size_t>(moving_links) * 6 * kIkThreads * sizeof(double);
  hipLaunchKernelGGL(SolveIkKernel, dim3(static_cast<unsigned>(workgroups)), dim3(kIkThreads), lds_bytes, stream, tree,
                     targets_dev, seeds_per_target, seeds_dev, num_problems, base, limits_dev, options, out);
  return hipGetLastError();
}
}  // namespace vgt
