// KinematicChain and SolveInverseKinematics (include/vgt_hip/inverse_kinematics.hpp) on the C ABI (vgt_hip_solve_ik).
#include "../../../include/vgt_hip/inverse_kinematics.hpp"
#include "host_internal.hpp"

#include <algorithm>
#include <cmath>

namespace vgt_hip
{
std::vector<int32_t> KinematicChain(const KinematicTree& tree, int32_t tip_link)
{
  if (tip_link < 0 || tip_link >= tree.NumLinks())
    throw std::invalid_argument("tip link " + std::to_string(tip_link) + " is not in [0, " +
                                std::to_string(tree.NumLinks()) + ")");
  std::vector<int32_t> chain;
  for (int32_t i = tip_link; i >= 0; i = tree.Links()[static_cast<size_t>(i)].parent) chain.push_back(i);
  std::reverse(chain.begin(), chain.end());
  return chain;
}

IkSolutions SolveInverseKinematics(const KinematicTree& tree, int32_t tip_link, const std::vector<Isometry3>& targets,
                                   const std::vector<double>& seeds, const IkOptions& options)
{
  // (what the C ABI would refuse, refused before a device is asked for, in its words)
  if (options.seeds_per_target <= 0)
    throw std::invalid_argument("inverse kinematics needs at least one target and one seed per target");
  const int64_t num_targets = static_cast<int64_t>(targets.size());
  if (num_targets > 0x7fffffffLL || options.seeds_per_target > 0x7fffffffLL ||
      num_targets * options.seeds_per_target > 0x7fffffffLL)
    throw std::invalid_argument("inverse kinematics supports fewer than 2^31 problems");
  const int64_t problems = num_targets * options.seeds_per_target;
  if (seeds.size() != static_cast<size_t>(problems) * static_cast<size_t>(tree.NumJoints()))
    throw std::invalid_argument("seeds must hold one value per problem and joint");
  if (!options.joint_limits.empty() && options.joint_limits.size() != static_cast<size_t>(tree.NumJoints()) * 2)
    throw std::invalid_argument("joint_limits must hold a lower and an upper value per joint");
  if (options.max_iterations < 0 || options.max_iterations > 10000)
    throw std::invalid_argument("max_iterations must lie in [0, 10000]");
  if (!(options.damping >= 0.0) || !std::isfinite(options.damping))
    throw std::invalid_argument("the damping must be finite and not negative");
  if (!(options.max_step > 0.0)) throw std::invalid_argument("max_step must be positive (+infinity is allowed)");
  if (!(options.position_tolerance >= 0.0) || !(options.rotation_tolerance >= 0.0))
    throw std::invalid_argument("a tolerance must not be negative");
  for (const double weight : options.task_weights)
    if (!(weight >= 0.0) || !std::isfinite(weight))
      throw std::invalid_argument("a task weight must be finite and not negative");
  const std::vector<int32_t> chain = KinematicChain(tree, tip_link);
  std::vector<int32_t> reader(static_cast<size_t>(tree.NumJoints()), -1);  // per column the moving chain link that reads it
  int64_t moving = 0;
  for (const int32_t i : chain)
  {
    const KinematicLink& link = tree.Links()[static_cast<size_t>(i)];
    if (link.joint_type == VGT_HIP_JOINT_FIXED) continue;
    int32_t& first = reader[static_cast<size_t>(link.joint_index)];
    if (first >= 0)
      throw std::invalid_argument("links " + std::to_string(first) + " and " + std::to_string(i) + " on the chain to link " +
                                  std::to_string(tip_link) + " both read column " + std::to_string(link.joint_index) +
                                  ": inverse kinematics does not take a mimic joint on the chain");
    first = i;
    moving++;
  }
  if (moving > vgt_hip_ik_max_chain_joints())
    throw std::invalid_argument("the chain to link " + std::to_string(tip_link) + " has " + std::to_string(moving) +
                                " moving links; inverse kinematics takes at most " +
                                std::to_string(vgt_hip_ik_max_chain_joints()));

  IkSolutions out;
  if (problems == 0) return out;  // (no device is needed)
  const size_t b = static_cast<size_t>(problems);
  out.joints.resize(b * static_cast<size_t>(tree.NumJoints()));
  out.status.resize(b);
  out.iterations.resize(b);
  out.error.resize(b * 6);
  out.tip_pose.resize(b * 16);
  out.fk_status.resize(b);
  static_assert(sizeof(Isometry3) == 16 * sizeof(double), "the targets are passed as packed doubles");
  const int rc = vgt_hip_solve_ik(
      detail::SharedSdfContext(tree.HipDevice()), tree.DeviceTree(), tip_link, targets[0].m.data(), num_targets,
      options.seeds_per_target, seeds.data(), options.has_world_from_base ? options.world_from_base.m.data() : nullptr,
      options.joint_limits.empty() ? nullptr : options.joint_limits.data(), options.task_weights.data(),
      options.max_iterations, options.damping, options.max_step, options.position_tolerance, options.rotation_tolerance,
      out.joints.data(), out.status.data(), out.iterations.data(), out.error.data(), out.tip_pose.data(),
      out.fk_status.data());
  if (rc != VGT_HIP_OK) detail::ThrowForCode(rc, vgt_hip_last_error());
  return out;
}
}  // namespace vgt_hip
