// Motion checks of the C++ host layer: straight joint-space motions of a kinematic tree carrying a sphere model, sampled
// and checked against a signed distance field on the device, one verdict per motion (vgt_hip_check_motions of vgt_hip.h,
// which states the samples, every output and the statuses).  The link poses of the samples never leave the device.
#pragma once

#include <array>
#include <cstdint>
#include <vector>

#include "body_queries.hpp"
#include "host_types.hpp"
#include "kinematics.hpp"

namespace vgt_hip
{
struct MotionOptions
{
  double minimum_clearance = 0.0;
  bool outside_is_collision = false;      // VGT_HIP_SPHERES_OUTSIDE_IS_COLLISION
  bool stop_at_collision = false;         // VGT_HIP_MOTION_STOP_AT_COLLISION: the samples after the first collision do not exist
  bool has_world_from_base = false;
  Isometry3 world_from_base;
  std::vector<double> joint_limits;       // empty, or NumJoints() * 2 (lower, upper)
};

// The verdict on one motion.
struct MotionCheck
{
  uint8_t status = 0;                     // VGT_HIP_MOTION_CLEAR / _COLLISION / _NO_VALUE
  int32_t first_collision = -1;           // the least colliding sample, -1: none
  double min_clearance = 0.0;             // the least clearance of a sample, NaN: none
  int32_t min_sample = -1;                // the sample that has it (the lowest on ties)
  int32_t min_sphere = -1;                // that sample's worst sphere
  std::array<double, 3> min_gradient{{0.0, 0.0, 0.0}};  // and its gradient
  uint8_t fk_status = 0;                  // VGT_HIP_FK_* bits of the samples, ORed
};

// joint_from and joint_to: E * NumJoints() doubles each; num_steps: one count per motion (a motion of n steps has n + 1
// samples), or a single count for all of them.  The number of motions is that of the rows of joint_from; for a tree
// without joints, that of num_steps.  Runs on the tree's device.  Throws std::invalid_argument where the C ABI reports an
// invalid argument (in its words: "motion 12: num_steps -3") and for vectors of the wrong length, std::runtime_error for
// its other errors.  No motions: no device is needed.
std::vector<MotionCheck> CheckMotions(const SignedDistanceField& sdf, const SphereModel& model, const KinematicTree& tree,
                                      const std::vector<double>& joint_from, const std::vector<double>& joint_to,
                                      const std::vector<int32_t>& num_steps, const MotionOptions& options = {});
}  // namespace vgt_hip
