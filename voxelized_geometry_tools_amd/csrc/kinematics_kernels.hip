// Forward kinematics and the clearance gradient in joint space for gfx950.  Semantics and every output:
// include/vgt_hip.h, vgt_hip_forward_kinematics / vgt_hip_clearance_joint_gradient.  Everything is plain double
// arithmetic in the header's order (the build's -ffp-contract=off keeps every operator on its own); sin / cos are the
// header's own, not OCML's, so the numpy restatement gives the same bits.
//
// Forward kinematics.  One lane per configuration, walking the links in order; a workgroup is one wave, so nothing here
// needs a barrier and the lanes may diverge.  The link table (KinematicLink, 144 B per link) is the same for every lane:
// the index is wave-uniform, the loads are scalar.  Every lane writes its 128-byte pose as one aligned line of the output
// (eight 16-byte stores when the output is 16-byte aligned, sixteen 8-byte ones otherwise).
//
// Where a link's parent pose comes from -- the values are the same on every path, each pose being one fixed sequence of
// operations --:
//   registers   the parent is the link just before (every link of a serial arm, most links of a tree): the pose the lane
//               has just computed;
//   LDS         otherwise, when the parent has a slot: tile[slot][element][lane], doubles, so consecutive lanes touch
//               consecutive 8-byte words (no bank conflicts); 96 B per lane and slot;
//   the output  otherwise: the lane reads back the line it wrote itself (same lane, same address, program order).
// Slots go to the links that are the parent of a link other than the next one -- the branch points --, in link order,
// to the first kKinematicsLdsLinks = 10 of them (AssignKinematicsLdsSlots, when the tree is made).  Their number sizes
// the launch's dynamic LDS: 6 KiB per slot, 60 KiB at the budget.  A chain takes none and leaves the occupancy to the
// registers; a body with three branch points takes 18 KiB.
//
// Waves are persistent: workgroup w takes the groups of 64 configurations w, w + workgroups, ...; at most
// kKinematicsMaxWorkgroups per launch.
//
// Gradient.  One lane per (configuration, joint): the lane walks the chain of the sphere(s) from the link to the base and
// adds the terms of the links that read its joint, in the header's order -- which is then trivially the order of the
// definition.  Persistent too.
//
// In bounds by construction: a lane with b >= B forms no address; parent, joint_type and joint_index were validated on
// the host when the tree was made (parent in [-1, i), joint_index in [0, J) on links that are not fixed); a sphere index
// or a sphere's link from device memory is compared against [0, S) resp. [0, L) before any address is formed from it.
#include "kinematics_math.hpp"
#include "vgt_internal.hpp"

#include <cmath>

namespace vgt
{
namespace
{
constexpr int kKinematicsThreads = 64;  // forward kinematics: one wave per workgroup
constexpr int kGradientThreads = 256;
// Workgroups of a launch: 32 waves per CU on 256 CUs for the forward kinematics, eight workgroups of four for the gradient.
constexpr int kKinematicsMaxWorkgroups = 8192;
constexpr int kGradientMaxWorkgroups = 2048;

__global__ __launch_bounds__(kKinematicsThreads) void ForwardKinematicsKernel(
    const KinematicLink* __restrict__ links, int num_links, int num_joints,
    const double* __restrict__ joint_values, int64_t num_configurations, const KinematicsBase base,
    const double* __restrict__ limits, double* poses, uint8_t* __restrict__ status, int wide_stores)
{
  extern __shared__ __attribute__((aligned(16))) double tile[];  // [slots][12][64]
  const int lane = static_cast<int>(threadIdx.x);
  const int64_t groups = (num_configurations + kKinematicsThreads - 1) / kKinematicsThreads;
  for (int64_t group = blockIdx.x; group < groups; group += gridDim.x)
  {
    const int64_t b = group * kKinematicsThreads + lane;
    if (b >= num_configurations) continue;  // (no barrier anywhere below)
    const double* q = joint_values + b * num_joints;
    const auto joint = [&](int j) { return q[j]; };
    uint8_t bits = limits ? LimitBits(limits, num_joints, joint) : 0;
    LinkPose previous;  // the pose of link i - 1
#pragma unroll
    for (int e = 0; e < 12; e++) previous.m[e] = 0.0;
    double* line = poses + b * num_links * 16;
    for (int i = 0; i < num_links; i++, line += 16)
    {
      const KinematicLink& link = links[i];
      const LinkPose frame = LinkFrame(link, i, base, previous, [&](int parent) {
        LinkPose from;
        if (link.parent_slot >= 0)
        {
          const double* kept = tile + (link.parent_slot * 12) * kKinematicsThreads + lane;
#pragma unroll
          for (int e = 0; e < 12; e++) from.m[e] = kept[e * kKinematicsThreads];
        }
        else
        {
          const double* written = poses + (b * num_links + parent) * 16;  // this lane's own earlier line
#pragma unroll
          for (int e = 0; e < 12; e++) from.m[e] = written[4 * (e / 3) + e % 3];
        }
        return from;
      });
      const LinkPose of_link = LinkPoseFromFrame(link, frame, joint, bits);
      const double* pose = of_link.m;

      if (wide_stores)
      {
        double2* wide = reinterpret_cast<double2*>(line);
        wide[0] = make_double2(pose[0], pose[1]);
        wide[1] = make_double2(pose[2], 0.0);
        wide[2] = make_double2(pose[3], pose[4]);
        wide[3] = make_double2(pose[5], 0.0);
        wide[4] = make_double2(pose[6], pose[7]);
        wide[5] = make_double2(pose[8], 0.0);
        wide[6] = make_double2(pose[9], pose[10]);
        wide[7] = make_double2(pose[11], 1.0);
      }
      else
      {
#pragma unroll
        for (int col = 0; col < 4; col++)
        {
#pragma unroll
          for (int r = 0; r < 3; r++) line[4 * col + r] = pose[3 * col + r];
          line[4 * col + 3] = col == 3 ? 1.0 : 0.0;
        }
      }
      if (link.keep_slot >= 0)
      {
        double* kept = tile + (link.keep_slot * 12) * kKinematicsThreads + lane;
#pragma unroll
        for (int e = 0; e < 12; e++) kept[e * kKinematicsThreads] = pose[e];
      }
      previous = of_link;
    }
    if (status) status[b] = bits;
  }
}

struct GradientModel
{
  const KinematicLink* links;
  const double* poses;  // [B][L][16]
  const double* xyzr;   // [S][4]
  const int32_t* link;  // [S]
  int num_links, num_joints, num_spheres;
  int64_t num_configurations;
};

// The terms of one sphere (index s, on link k in [0, L)) for joint j, added to acc in walk order.
template <bool kWeighted>
__device__ __forceinline__ double WalkSphere(const GradientModel& model, int64_t b, int s, int k, int j, double g0,
                                             double g1, double g2, double weight, double acc)
{
  const double* first = model.poses + b * model.num_links * 16;
  const double* m = first + static_cast<int64_t>(k) * 16;
  const double* centre = model.xyzr + 4 * static_cast<int64_t>(s);
  const double cx = centre[0], cy = centre[1], cz = centre[2];
  double p[3];
#pragma unroll
  for (int r = 0; r < 3; r++) p[r] = ((m[r] * cx + m[4 + r] * cy) + m[8 + r] * cz) + m[12 + r];
  for (int i = k; i >= 0; i = model.links[i].parent)
  {
    const KinematicLink& link = model.links[i];
    if (link.joint_type == kJointFixed || link.joint_index != j) continue;
    m = first + static_cast<int64_t>(i) * 16;
    const double x = link.axis[0], y = link.axis[1], z = link.axis[2];
    double a[3];
#pragma unroll
    for (int r = 0; r < 3; r++) a[r] = (m[r] * x + m[4 + r] * y) + m[8 + r] * z;
    double term;
    if (link.joint_type == kJointRevolute)
    {
      const double d0 = p[0] - m[12], d1 = p[1] - m[13], d2 = p[2] - m[14];
      const double u0 = a[1] * d2 - a[2] * d1, u1 = a[2] * d0 - a[0] * d2, u2 = a[0] * d1 - a[1] * d0;
      term = (g0 * u0 + g1 * u1) + g2 * u2;
    }
    else
      term = (g0 * a[0] + g1 * a[1]) + g2 * a[2];
    acc = acc + (kWeighted ? weight * term : term);
  }
  return acc;
}

template <bool kWeighted>
__global__ __launch_bounds__(kGradientThreads) void ClearanceJointGradientKernel(
    const GradientModel model, const int32_t* __restrict__ min_sphere, const double* __restrict__ min_gradient,
    const double* __restrict__ sphere_weight, const double* __restrict__ sphere_gradient,
    double* __restrict__ joint_gradient)
{
  const double nan = __longlong_as_double(0x7ff8000000000000ll);
  const int L = model.num_links, J = model.num_joints, S = model.num_spheres;
  const int64_t total = model.num_configurations * J;
  const int64_t stride = static_cast<int64_t>(gridDim.x) * kGradientThreads;
  for (int64_t item = static_cast<int64_t>(blockIdx.x) * kGradientThreads + threadIdx.x; item < total; item += stride)
  {
    const int64_t b = item / J;
    const int j = static_cast<int>(item - b * J);
    double acc = 0.0;
    if (!kWeighted)
    {
      const int s = min_sphere[b];
      int k = -1;
      if (s >= 0 && s < S) k = model.link[s];
      if (k >= 0 && k < L)
      {
        const double* g = min_gradient + 3 * b;
        acc = WalkSphere<false>(model, b, s, k, j, g[0], g[1], g[2], 1.0, acc);
      }
      else
        acc = nan;
    }
    else
    {
      const double* weights = sphere_weight + b * S;
      const double* gradients = sphere_gradient + 3 * (b * S);
      for (int s = 0; s < S; s++)
      {
        const double weight = weights[s];
        const int k = model.link[s];
        if (weight == 0.0 || k < 0 || k >= L) continue;
        const double* g = gradients + 3 * static_cast<int64_t>(s);
        acc = WalkSphere<true>(model, b, s, k, j, g[0], g[1], g[2], weight, acc);
      }
    }
    joint_gradient[item] = acc;
  }
}
}  // namespace

int AssignKinematicsLdsSlots(KinematicLink* links_host, int64_t num_links)
{
  for (int64_t i = 0; i < num_links; i++) links_host[i].keep_slot = links_host[i].parent_slot = -1;
  // -2: a branch point that has no slot yet
  for (int64_t i = 0; i < num_links; i++)
  {
    const int64_t parent = links_host[i].parent;
    if (parent >= 0 && parent != i - 1) links_host[parent].keep_slot = -2;
  }
  int slots = 0;
  for (int64_t i = 0; i < num_links; i++)
    if (links_host[i].keep_slot == -2) links_host[i].keep_slot = slots < kKinematicsLdsLinks ? slots++ : -1;
  for (int64_t i = 0; i < num_links; i++)
  {
    const int64_t parent = links_host[i].parent;
    if (parent >= 0 && parent != i - 1) links_host[i].parent_slot = links_host[parent].keep_slot;
  }
  return slots;
}

hipError_t LaunchForwardKinematics(const KinematicLink* links_dev, int64_t num_links, int64_t num_joints, int lds_links,
                                   const double* joint_values_dev, int64_t num_configurations,
                                   const double* world_from_base_host, const double* limits_dev, double* link_poses_dev,
                                   uint8_t* status_dev, int max_workgroups, hipStream_t stream)
{
  if (num_configurations <= 0) return hipSuccess;
  if (lds_links < 0 || lds_links > kKinematicsLdsLinks) return hipErrorInvalidValue;
  const KinematicsBase base = MakeKinematicsBase(world_from_base_host);
  const int64_t groups = (num_configurations + kKinematicsThreads - 1) / kKinematicsThreads;
  const int64_t most = max_workgroups > 0 ? max_workgroups : kKinematicsMaxWorkgroups;
  const int64_t workgroups = groups < most ? groups : most;
  const size_t lds_bytes = static_cast<size_t>(lds_links) * 12 * kKinematicsThreads * sizeof(double);
  const int wide_stores = (reinterpret_cast<uintptr_t>(link_poses_dev) & 15) == 0 ? 1 : 0;
  hipLaunchKernelGGL(ForwardKinematicsKernel, dim3(static_cast<unsigned>(workgroups)), dim3(kKinematicsThreads), lds_bytes,
                     stream, links_dev, static_cast<int>(num_links), static_cast<int>(num_joints),
                     joint_values_dev, num_configurations, base, limits_dev, link_poses_dev, status_dev, wide_stores);
  return hipGetLastError();
}

hipError_t LaunchClearanceJointGradient(const KinematicLink* links_dev, int64_t num_links, int64_t num_joints,
                                        const double* link_poses_dev, int64_t num_configurations,
                                        const double* sphere_xyzr_dev, const int32_t* sphere_link_dev,
                                        int64_t num_spheres, const int32_t* min_sphere_dev,
                                        const double* min_gradient_dev, const double* sphere_weight_dev,
                                        const double* sphere_gradient_dev, double* joint_gradient_dev,
                                        int max_workgroups, hipStream_t stream)
{
  const int64_t total = num_configurations * num_joints;
  if (total <= 0) return hipSuccess;
  const GradientModel model{links_dev,
                            link_poses_dev,
                            sphere_xyzr_dev,
                            sphere_link_dev,
                            static_cast<int>(num_links),
                            static_cast<int>(num_joints),
                            static_cast<int>(num_spheres),
                            num_configurations};
  int64_t workgroups = (total + kGradientThreads - 1) / kGradientThreads;
  const int64_t most = max_workgroups > 0 ? max_workgroups : kGradientMaxWorkgroups;
  if (workgroups > most) workgroups = most;
  if (min_sphere_dev)
    hipLaunchKernelGGL(ClearanceJointGradientKernel<false>, dim3(static_cast<unsigned>(workgroups)),
                       dim3(kGradientThreads), 0, stream, model, min_sphere_dev, min_gradient_dev, sphere_weight_dev,
                       sphere_gradient_dev, joint_gradient_dev);
  else
    hipLaunchKernelGGL(ClearanceJointGradientKernel<true>, dim3(static_cast<unsigned>(workgroups)),
                       dim3(kGradientThreads), 0, stream, model, min_sphere_dev, min_gradient_dev, sphere_weight_dev,
                       sphere_gradient_dev, joint_gradient_dev);
  return hipGetLastError();
}
}  // namespace vgt
