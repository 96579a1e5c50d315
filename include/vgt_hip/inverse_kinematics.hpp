// Inverse kinematics of the C++ host layer: poses of a tool frame to joint values, batched over targets and seeds, by
// damped least-squares steps on the device (vgt_hip_solve_ik of vgt_hip.h, which states every output).  The rows it
// returns are what ComputeLinkPoses, CheckSphereModel from joint values, CheckSelfCollision and the motion checks take.
#pragma once

#include <array>
#include <cstdint>
#include <limits>
#include <vector>

#include "host_types.hpp"
#include "kinematics.hpp"

namespace vgt_hip
{
struct IkOptions
{
  int64_t seeds_per_target = 1;            // R: problem b aims at target b / R
  int32_t max_iterations = 50;             // K in [0, 10000]; 0 evaluates the seeds only
  double damping = 0.01;                   // lambda >= 0
  double max_step = 0.5;                   // > 0, the largest change of a joint per step; infinity is allowed
  double position_tolerance = 1e-6;
  double rotation_tolerance = 1e-6;
  // (x, y, z, rx, ry, rz): each finite and >= 0; 0 takes the component out of the step and of the convergence test
  std::array<double, 6> task_weights{{1.0, 1.0, 1.0, 1.0, 1.0, 1.0}};
  bool has_world_from_base = false;
  Isometry3 world_from_base;
  std::vector<double> joint_limits;        // empty, or NumJoints() * 2
};

// One entry per problem: joints B * NumJoints(), status VGT_HIP_IK_*, iterations (the steps taken), error B * 6 (the
// unweighted task error at the returned row), tip_pose B * 16 (world_from_tip, column-major), fk_status
// VGT_HIP_FK_NOT_COMPUTABLE (from the chain) | VGT_HIP_FK_OUTSIDE_LIMITS (over all columns of the returned row).
struct IkSolutions
{
  std::vector<double> joints;
  std::vector<uint8_t> status;
  std::vector<int32_t> iterations;
  std::vector<double> error;
  std::vector<double> tip_pose;
  std::vector<uint8_t> fk_status;
};

// The links on the way from the base to tip_link, base first: the chain whose joints SolveInverseKinematics moves.  Needs
// no device.  std::invalid_argument for a tip outside [0, NumLinks()).
std::vector<int32_t> KinematicChain(const KinematicTree& tree, int32_t tip_link);

// targets: T poses of the tip; seeds: T * options.seeds_per_target * NumJoints() doubles.  Throws std::invalid_argument
// where the C ABI reports an invalid argument, in its words and before a device is asked for (and for vectors of the
// wrong length): options outside their ranges, a tip outside the tree, two moving links of the chain that read one column
// (a mimic joint on the chain; the message names both links), a chain with more moving links than
// vgt_hip_ik_max_chain_joints(); std::runtime_error for the C ABI's other errors.  No targets: no device is needed.
IkSolutions SolveInverseKinematics(const KinematicTree& tree, int32_t tip_link, const std::vector<Isometry3>& targets,
                                   const std::vector<double>& seeds, const IkOptions& options = {});
}  // namespace vgt_hip
