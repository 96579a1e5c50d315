// Motion checks with the self part, of the C++ host layer: straight joint-space motions of a kinematic tree carrying a
// sphere model, sampled and checked on the device against a signed distance field and against the model itself over a
// list of sphere pairs, one verdict per motion (vgt_hip_check_motions_with_self of vgt_hip.h, which states the samples,
// the two parts, every output and the statuses).  Link poses and sphere centres are made once per sample and never leave
// the device.
#pragma once

#include <array>
#include <cstdint>
#include <vector>

#include "body_queries.hpp"
#include "host_types.hpp"
#include "kinematics.hpp"
#include "motion_queries.hpp"
#include "self_collision.hpp"

namespace vgt_hip
{
struct MotionSelfOptions
{
  double minimum_clearance = 0.0;           // the environment part: a sphere with clearance <= this collides
  double self_minimum_clearance = 0.0;      // the self part: a pair with clearance <= this collides
  bool outside_is_collision = false;        // VGT_HIP_SPHERES_OUTSIDE_IS_COLLISION
  bool stop_at_collision = false;           // VGT_HIP_MOTION_STOP_AT_COLLISION, on the combined verdict
  bool self_no_value_is_collision = false;  // VGT_HIP_MOTION_SELF_NO_VALUE_IS_COLLISION
  bool has_world_from_base = false;
  Isometry3 world_from_base;
  std::vector<double> joint_limits;         // empty, or NumJoints() * 2 (lower, upper)
};

// The verdict on one motion.
struct MotionSelfCheck
{
  uint8_t status = 0;                       // VGT_HIP_MOTION_CLEAR / _COLLISION / _NO_VALUE
  int32_t first_collision = -1;             // the least colliding sample, -1: none
  uint8_t collision_cause = 0;              // VGT_HIP_MOTION_CAUSE_ENVIRONMENT | VGT_HIP_MOTION_CAUSE_SELF of that sample
  double min_clearance = 0.0;               // the environment part: the least clearance of a sample, NaN: none
  int32_t min_sample = -1;                  // the sample that has it (the lowest on ties)
  int32_t min_sphere = -1;                  // that sample's worst sphere
  std::array<double, 3> min_gradient{{0.0, 0.0, 0.0}};  // and its gradient
  double self_min_clearance = 0.0;          // the self part: the least pair clearance of a sample, NaN: none
  int32_t self_min_sample = -1;             // the sample that has it (the lowest on ties)
  int32_t self_min_pair = -1;               // that sample's worst pair, an index into `pairs`
  uint8_t fk_status = 0;                    // VGT_HIP_FK_* bits of the samples, ORed
};

// sdf_or_null: nullptr for no environment part; pairs: empty for no self part (one of the two must be there).
// joint_from, joint_to and num_steps as CheckMotions takes them.  Runs on the tree's device.  Throws
// std::invalid_argument where the C ABI reports an invalid argument (in its words: "pair 12: (5, 5) is not ascending") and
// for vectors of the wrong length, std::runtime_error for its other errors.  No motions: no device is needed.
std::vector<MotionSelfCheck> CheckMotionsWithSelf(const SignedDistanceField* sdf_or_null, const SphereModel& model,
                                                  const KinematicTree& tree, const std::vector<SpherePair>& pairs,
                                                  const std::vector<double>& joint_from,
                                                  const std::vector<double>& joint_to,
                                                  const std::vector<int32_t>& num_steps,
                                                  const MotionSelfOptions& options = {});
}  // namespace vgt_hip
