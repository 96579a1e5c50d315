// Device code shared by the kernels that walk a kinematic tree (kinematics_kernels.hip: forward kinematics;
// motion_kernels.hip: motions checked against an SDF): sin / cos, the product of two transforms, the limit test, the frame
// of a link from its parent's pose and the step from the frame to the link's pose, each in the one operation order of include/vgt_hip.h, vgt_hip_forward_kinematics.  One
// definition, so that both kernels give the same bits.  Every translation unit that includes this is built without
// contraction.
#pragma once

#include "vgt_internal.hpp"

#include <cmath>

namespace vgt
{
namespace
{
struct KinematicsBase
{
  double m[12];  // m[3 c + r]
  int given;
};

inline KinematicsBase MakeKinematicsBase(const double* world_from_base_host)
{
  KinematicsBase base{};
  if (world_from_base_host)
  {
    base.given = 1;
    for (int c = 0; c < 4; c++)
      for (int r = 0; r < 3; r++) base.m[3 * c + r] = world_from_base_host[4 * c + r];
  }
  return base;
}

// sin / cos of include/vgt_hip.h for a finite q with |q| <= 2^20
__device__ __forceinline__ void SinCos(double q, double& s, double& c)
{
  const double k = __builtin_rint(q * 0x1.45f306dc9c883p-1);
  const double r = ((q - k * 0x1.921fb54400000p+0) - k * 0x1.0b4611a600000p-34) - k * 0x1.3198a2e037073p-69;
  const double z = r * r;
  double ps = 0x1.952c77030ad4ap-49;    // 1 / 17!
  ps = ps * z + -0x1.ae7f3e733b81fp-41;  // -1 / 15!
  ps = ps * z + 0x1.6124613a86d09p-33;   // 1 / 13!
  ps = ps * z + -0x1.ae64567f544e4p-26;  // -1 / 11!
  ps = ps * z + 0x1.71de3a556c734p-19;   // 1 / 9!
  ps = ps * z + -0x1.a01a01a01a01ap-13;  // -1 / 7!
  ps = ps * z + 0x1.1111111111111p-7;    // 1 / 5!
  ps = ps * z + -0x1.5555555555555p-3;   // -1 / 3!
  const double sin_r = r + (r * z) * ps;
  double pc = 0x1.ae7f3e733b81fp-45;     // 1 / 16!
  pc = pc * z + -0x1.93974a8c07c9dp-37;  // -1 / 14!
  pc = pc * z + 0x1.1eed8eff8d898p-29;   // 1 / 12!
  pc = pc * z + -0x1.27e4fb7789f5cp-22;  // -1 / 10!
  pc = pc * z + 0x1.a01a01a01a01ap-16;   // 1 / 8!
  pc = pc * z + -0x1.6c16c16c16c17p-10;  // -1 / 6!
  pc = pc * z + 0x1.5555555555555p-5;    // 1 / 4!
  pc = pc * z + -0x1.0000000000000p-1;   // -1 / 2!
  const double cos_r = 1.0 + z * pc;
  const int quadrant = static_cast<int>(static_cast<long long>(k) & 3);
  s = quadrant == 0 ? sin_r : quadrant == 1 ? cos_r : quadrant == 2 ? -sin_r : -cos_r;
  c = quadrant == 0 ? cos_r : quadrant == 1 ? -sin_r : quadrant == 2 ? -cos_r : sin_r;
}

// out = a . b, transforms as twelve doubles m[3 c + r]
__device__ __forceinline__ void Compose(const double* a, const double* b, double* out)
{
#pragma unroll
  for (int r = 0; r < 3; r++)
  {
#pragma unroll
    for (int c = 0; c < 3; c++) out[3 * c + r] = (a[r] * b[3 * c] + a[3 + r] * b[3 * c + 1]) + a[6 + r] * b[3 * c + 2];
    out[9 + r] = ((a[r] * b[9] + a[3 + r] * b[10]) + a[6 + r] * b[11]) + a[9 + r];
  }
}

struct LinkPose
{
  double m[12];  // m[3 c + r]
};

// The pose of a link that is not FIXED from its frame F and the value of its joint.  *usable false: the value cannot be
// used (VGT_HIP_FK_NOT_COMPUTABLE), and the pose is NaN.  (By value: each side keeps its arrays in registers.)
__device__ __forceinline__ LinkPose ApplyJoint(const KinematicLink& link, const LinkPose frame_of_link, double value,
                                               bool* is_usable)
{
  const double* const frame = frame_of_link.m;
  LinkPose result = frame_of_link;
  double* const pose = result.m;
  const double nan = __longlong_as_double(0x7ff8000000000000ll);
  const double x = link.axis[0], y = link.axis[1], z = link.axis[2];
  const bool finite = fabs(value) <= 0x1.fffffffffffffp+1023;  // (false for NaN)
  const bool usable = link.joint_type == kJointRevolute ? finite && fabs(value) <= 0x1p+20 : finite;
  if (!usable)
  {
#pragma unroll
    for (int e = 0; e < 12; e++) pose[e] = nan;
  }
  else if (link.joint_type == kJointRevolute)
  {
    double s, c;
    SinCos(value, s, c);
    const double v = 1.0 - c;
    double rotation[9];  // rotation[3 c + r]
    rotation[0] = c + (x * x) * v;
    rotation[3] = (x * y) * v - z * s;
    rotation[6] = (x * z) * v + y * s;
    rotation[1] = (x * y) * v + z * s;
    rotation[4] = c + (y * y) * v;
    rotation[7] = (y * z) * v - x * s;
    rotation[2] = (x * z) * v - y * s;
    rotation[5] = (y * z) * v + x * s;
    rotation[8] = c + (z * z) * v;
#pragma unroll
    for (int r = 0; r < 3; r++)
#pragma unroll
      for (int col = 0; col < 3; col++)
        pose[3 * col + r] = (frame[r] * rotation[3 * col] + frame[3 + r] * rotation[3 * col + 1]) +
                            frame[6 + r] * rotation[3 * col + 2];
  }
  else
  {
    const double t0 = x * value, t1 = y * value, t2 = z * value;
#pragma unroll
    for (int r = 0; r < 3; r++) pose[9 + r] = ((frame[r] * t0 + frame[3 + r] * t1) + frame[6 + r] * t2) + frame[9 + r];
  }
  *is_usable = usable;
  return result;
}

// VGT_HIP_FK_OUTSIDE_LIMITS (2) when a joint value lies outside its limits [J][2], else 0; value(j) gives joint j.
template <class JointValue>
__device__ __forceinline__ uint8_t LimitBits(const double* __restrict__ limits, int num_joints, JointValue value)
{
  uint8_t bits = 0;
  for (int j = 0; j < num_joints; j++)
  {
    const double v = value(j);
    if (v < limits[2 * j] || v > limits[2 * j + 1]) bits |= 2;
  }
  return bits;
}

// The frame of link i, F = P . origin_i: P is the base for parent -1 (without a base F is the origin as it is), the pose
// of link i - 1 when that is the parent (`previous`, which the caller has in registers), and parent_pose(parent) -- the
// caller's store of earlier poses -- otherwise.
template <class ParentPose>
__device__ __forceinline__ LinkPose LinkFrame(const KinematicLink& link, int i, const KinematicsBase& base,
                                              const LinkPose previous, ParentPose parent_pose)
{
  const int parent = link.parent;
  LinkPose origin, frame;
#pragma unroll
  for (int e = 0; e < 12; e++) origin.m[e] = link.origin[e];
  if (parent < 0 && !base.given) return origin;
  LinkPose from;
  if (parent < 0)
  {
#pragma unroll
    for (int e = 0; e < 12; e++) from.m[e] = base.m[e];
  }
  else if (parent == i - 1)
    from = previous;
  else
    from = parent_pose(parent);
  Compose(from.m, origin.m, frame.m);
  return frame;
}

// The pose of a link from its frame: the frame itself for a FIXED link, ApplyJoint on value(joint_index) otherwise,
// which adds VGT_HIP_FK_NOT_COMPUTABLE (1) to `bits` where the value cannot be used.
template <class JointValue>
__device__ __forceinline__ LinkPose LinkPoseFromFrame(const KinematicLink& link, const LinkPose frame, JointValue value,
                                                      uint8_t& bits)
{
  if (link.joint_type == kJointFixed) return frame;
  bool usable;
  const LinkPose pose = ApplyJoint(link, frame, value(link.joint_index), &usable);
  if (!usable) bits |= 1;
  return pose;
}
}  // namespace
}  // namespace vgt
