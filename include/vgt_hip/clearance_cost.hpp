// The obstacle cost of the C++ host layer: configurations of a kinematic tree carrying a sphere model, given as joint
// values, scored against a signed distance field on the device -- the hinge of a safety margin on the clearance of every
// sphere, summed per configuration, and that cost's gradient with respect to the joints (vgt_hip_clearance_cost of
// vgt_hip.h, which states the hinge, the order of the sums and every output).  Link poses and per-sphere values never
// leave the device.
#pragma once

#include <cstdint>
#include <vector>

#include "body_queries.hpp"
#include "host_types.hpp"
#include "kinematics.hpp"

namespace vgt_hip
{
struct ClearanceCostOptions
{
  bool with_gradient = true;              // false (roll-out scoring): joint_gradient and num_without_gradient stay empty,
                                          // and no gradient is loaded on the device
  bool has_world_from_base = false;
  Isometry3 world_from_base;
  std::vector<double> joint_limits;       // empty, or NumJoints() * 2 (lower, upper)
};

// One entry per configuration (a struct of vectors: a million configurations are four allocations, not a million).
struct ClearanceCosts
{
  std::vector<double> cost;                   // the sum of the spheres' hinge costs, in sphere order
  std::vector<double> joint_gradient;         // B * NumJoints(): d cost / d joint values
  std::vector<int32_t> num_active;            // spheres with a value and a weight
  std::vector<int32_t> num_outside;           // spheres without a value
  std::vector<int32_t> num_without_gradient;  // active spheres the gradient had to skip (a NaN field gradient)
  std::vector<uint8_t> fk_status;             // VGT_HIP_FK_* bits
};

// joint_values: B * NumJoints() doubles; for a tree without joints num_configurations gives B (otherwise it may be left
// at -1, or must agree).  margin: positive and finite.  Runs on the tree's device.  Throws std::invalid_argument where
// the C ABI reports an invalid argument (in its words: "sphere 17: ...") and for vectors of the wrong length,
// std::runtime_error for its other errors.  No configurations: no device is needed.
ClearanceCosts ClearanceCost(const SignedDistanceField& sdf, const SphereModel& model, const KinematicTree& tree,
                             const std::vector<double>& joint_values, double margin,
                             const ClearanceCostOptions& options = {}, int64_t num_configurations = -1);
}  // namespace vgt_hip
