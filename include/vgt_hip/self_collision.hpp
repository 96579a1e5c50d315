// Self-collision of the C++ host layer: configurations of a kinematic tree carrying a sphere model, given as joint
// values, checked on the device for spheres of the model that touch each other (vgt_hip_check_self_collision of
// vgt_hip.h, which states the pair arithmetic, the order and every output), and the pair list such a check takes
// (vgt_hip_self_collision_pairs).  Link poses and sphere centres never leave the device.  The environment is another
// call's business (CheckSphereModel, CheckMotions, ClearanceCost): a caller combines the two verdicts.
#pragma once

#include <array>
#include <cstdint>
#include <vector>

#include "body_queries.hpp"
#include "host_types.hpp"
#include "kinematics.hpp"

namespace vgt_hip
{
using SpherePair = std::array<int32_t, 2>;  // (a, b), a < b: indices into the model
using LinkPair = std::array<int32_t, 2>;    // unordered

struct SelfCollisionPairOptions
{
  bool skip_adjacent = false;  // leave out the pairs of a link and its direct parent
};

// In lexicographic order every (a, b), a < b, of spheres on different links that are not one of `ignored_link_pairs`
// and (skip_adjacent) not parent and child in `tree`.  Host only: no device is needed.  Throws std::invalid_argument
// where the C ABI reports an invalid argument, in its words ("sphere 3: link 9 is not in [0, num_links)").
std::vector<SpherePair> SelfCollisionPairs(const SphereModel& model, const KinematicTree& tree,
                                           const std::vector<LinkPair>& ignored_link_pairs = {},
                                           const SelfCollisionPairOptions& options = {});

struct SelfCollisionOptions
{
  double minimum_clearance = 0.0;      // a pair with clearance <= this collides
  bool no_value_is_collision = false;  // a pair without a value collides too
  bool with_gradient = true;           // false: joint_gradient stays empty
  bool per_pair = false;               // also return every pair's clearance
  bool has_world_from_base = false;
  Isometry3 world_from_base;
  std::vector<double> joint_limits;    // empty, or NumJoints() * 2 (lower, upper)
};

// One entry per configuration (a struct of vectors: a million configurations are a few allocations, not a million).
struct SelfCollisionChecks
{
  std::vector<uint8_t> status;             // VGT_HIP_SELF_CLEAR / _COLLISION / _NO_VALUE
  std::vector<int32_t> num_below;          // pairs with clearance <= minimum_clearance
  std::vector<int32_t> num_without_value;  // pairs whose clearance is NaN
  std::vector<double> min_clearance;       // NaN: no pair has a value
  std::vector<int32_t> min_pair;           // an index into `pairs`, -1: none
  std::vector<double> min_direction;       // 3 per configuration: from sphere b to sphere a of min_pair
  std::vector<double> joint_gradient;      // B * NumJoints(): d min_clearance / d joint values
  std::vector<uint8_t> fk_status;          // VGT_HIP_FK_* bits
  std::vector<double> pair_clearance;      // B * pairs.size(), empty unless per_pair
};

// joint_values: B * NumJoints() doubles; for a tree without joints num_configurations gives B (otherwise it may be left
// at -1, or must agree).  Runs on the tree's device.  Throws std::invalid_argument where the C ABI reports an invalid
// argument (in its words: "pair 12: (5, 5) is not ascending") and for vectors of the wrong length, std::runtime_error
// for its other errors.  No configurations: no device is needed.
SelfCollisionChecks CheckSelfCollision(const SphereModel& model, const KinematicTree& tree,
                                       const std::vector<SpherePair>& pairs, const std::vector<double>& joint_values,
                                       const SelfCollisionOptions& options = {}, int64_t num_configurations = -1);
}  // namespace vgt_hip
