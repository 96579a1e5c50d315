// Forward kinematics of the C++ host layer: joint values to the link poses the body queries take, the clearance gradient
// of a sphere-model check mapped back to joint space, and the check straight from joint values, chained on the device
// (vgt_hip_forward_kinematics, vgt_hip_clearance_joint_gradient and vgt_hip_check_spheres_from_joints of vgt_hip.h,
// which states every output).
#pragma once

#include <array>
#include <cstdint>
#include <memory>
#include <vector>

#include "body_queries.hpp"
#include "host_types.hpp"

struct vgt_hip_kinematics;

namespace vgt_hip
{
// One link of a kinematic tree: VGT_HIP_JOINT_FIXED / _REVOLUTE / _PRISMATIC, the column of the joint values it reads
// (ignored for a fixed link), its axis in the joint frame (used as it is) and parent_from_joint (the URDF <origin>).
struct KinematicLink
{
  int32_t parent = -1;  // -1: on the base; otherwise an earlier link
  int32_t joint_type = 0;
  int32_t joint_index = 0;
  std::array<double, 3> axis{{0.0, 0.0, 1.0}};
  Isometry3 origin;
};

// A validated tree.  Construction needs no device: std::invalid_argument names the first offending link as the C ABI does
// ("link 5: parent 7 is not below 5").  The device copy is made by the first call that needs one, on the process's shared
// context of `hip_device`, and lives as long as the last copy of this object.
class KinematicTree
{
public:
  KinematicTree(std::vector<KinematicLink> links, int64_t num_joints, int hip_device = 0);
  int64_t NumLinks() const;
  int64_t NumJoints() const;
  int HipDevice() const;
  const std::vector<KinematicLink>& Links() const;
  // The C ABI's handle, made on first use: std::runtime_error when the device cannot be opened.
  const vgt_hip_kinematics* DeviceTree() const;

private:
  struct State;
  std::shared_ptr<State> state_;
};

// link_poses: B * NumLinks() * 16 doubles, world_from_link column-major, what CheckSphereModel, RasterizeSphereModel and
// the point cover take; status: VGT_HIP_FK_NOT_COMPUTABLE | VGT_HIP_FK_OUTSIDE_LIMITS per configuration.
struct LinkPoses
{
  std::vector<double> link_poses;
  std::vector<uint8_t> status;
};
// joint_values: num_configurations * NumJoints() doubles.  world_from_base may be null; joint_limits is empty or
// NumJoints() * 2 doubles (lower, upper).  Throws std::invalid_argument where the C ABI reports an invalid argument (and
// for vectors of the wrong length), std::runtime_error for its other errors.  No configurations: no device is needed.
LinkPoses ComputeLinkPoses(const KinematicTree& tree, const std::vector<double>& joint_values, int64_t num_configurations,
                           const Isometry3* world_from_base = nullptr, const std::vector<double>& joint_limits = {});

// d min_clearance / d q, B * NumJoints() doubles: what `checks` (of these link poses and this model) says about the worst
// sphere of every configuration, through the kinematic Jacobian.  NaN rows where a configuration has no worst sphere.
std::vector<double> ClearanceJointGradient(const KinematicTree& tree, const std::vector<double>& link_poses,
                                           const SphereModel& model, const SphereModelChecks& checks);
// The summed form: sphere_weight B * S and sphere_gradient B * S * 3 doubles (e.g. the per-sphere gradients of the check
// under a penalty's weights); a sphere of weight 0 is skipped.
std::vector<double> ClearanceJointGradient(const KinematicTree& tree, const std::vector<double>& link_poses,
                                           const SphereModel& model, const std::vector<double>& sphere_weight,
                                           const std::vector<double>& sphere_gradient);

struct JointSphereModelOptions : SphereModelOptions
{
  bool joint_gradient = false;            // also return the worst-sphere joint gradient
  bool has_world_from_base = false;
  Isometry3 world_from_base;
  std::vector<double> joint_limits;       // empty, or NumJoints() * 2
};
struct JointSphereModelChecks
{
  SphereModelChecks checks;
  std::vector<uint8_t> fk_status;         // the forward kinematics' status
  std::vector<double> joint_gradient;     // B * NumJoints(), empty unless asked for
};
// CheckSphereModel from joint values: forward kinematics, the check and (optionally) the joint gradient in one call on
// the device; the poses never visit the host.  Runs on the tree's device (options.hip_device is not used).
JointSphereModelChecks CheckSphereModel(const SignedDistanceField& sdf, const SphereModel& model,
                                        const KinematicTree& tree, const std::vector<double>& joint_values,
                                        const JointSphereModelOptions& options = {});
}  // namespace vgt_hip
