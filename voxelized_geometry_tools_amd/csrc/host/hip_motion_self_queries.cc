// CheckMotionsWithSelf (include/vgt_hip/motion_self_queries.hpp) on the C ABI (vgt_hip_check_motions_with_self).
#include "../../../include/vgt_hip/motion_self_queries.hpp"
#include "host_internal.hpp"

#include <cmath>

namespace vgt_hip
{
std::vector<MotionSelfCheck> CheckMotionsWithSelf(const SignedDistanceField* sdf_or_null, const SphereModel& model,
                                                  const KinematicTree& tree, const std::vector<SpherePair>& pairs,
                                                  const std::vector<double>& joint_from,
                                                  const std::vector<double>& joint_to,
                                                  const std::vector<int32_t>& num_steps, const MotionSelfOptions& options)
{
  const DenseGrid* const g = sdf_or_null ? &sdf_or_null->grid : nullptr;
  if (g && !g->IsInitialized()) throw std::invalid_argument("Grid must be initialized");
  if (!g && pairs.empty())
    throw std::invalid_argument("neither a field nor a pair: there is nothing to check the motions against");
  if (model.link.size() != model.xyzr.size())
    throw std::invalid_argument("a sphere model holds one link and one (x, y, z, r) per sphere");
  static_assert(sizeof(std::array<double, 4>) == 4 * sizeof(double), "the spheres are passed as packed doubles");
  static_assert(sizeof(SpherePair) == 2 * sizeof(int32_t), "the pairs are passed as packed int32");
  if (g && std::isnan(options.minimum_clearance)) throw std::invalid_argument("minimum_clearance must not be NaN");
  if (!pairs.empty() && std::isnan(options.self_minimum_clearance))
    throw std::invalid_argument("self_minimum_clearance must not be NaN");
  if (!options.joint_limits.empty() && options.joint_limits.size() != static_cast<size_t>(tree.NumJoints()) * 2)
    throw std::invalid_argument("joint_limits must hold a lower and an upper value per joint");
  const int64_t s = static_cast<int64_t>(model.link.size());
  const int64_t p = static_cast<int64_t>(pairs.size());
  const size_t joints = static_cast<size_t>(tree.NumJoints());
  if (joint_from.size() != joint_to.size() || (joints == 0 ? !joint_from.empty() : joint_from.size() % joints != 0))
    throw std::invalid_argument("joint_from and joint_to must hold one value per motion and joint");
  const size_t motions = joints == 0 ? num_steps.size() : joint_from.size() / joints;
  if (num_steps.size() != motions && num_steps.size() != 1)
    throw std::invalid_argument("num_steps must hold one count per motion, or one for all");
  // (what needs no device, refused before one is asked for, in the C ABI's words; the arrays' contents are its business)
  for (size_t e = 0; e < num_steps.size(); e++)
    if (num_steps[e] < 0)
      throw std::invalid_argument("motion " + std::to_string(e) + ": num_steps " + std::to_string(num_steps[e]));
  if (motions > 0x7fffffffu || motions * joints > 0x7fffffffu || static_cast<uint64_t>(p) > 0x7fffffffu)
    throw std::invalid_argument("motion checks support fewer than 2^31 motions, pairs and (motion, joint) pairs");

  std::vector<MotionSelfCheck> out(motions);
  if (motions == 0) return out;  // (no device is needed)
  const bool uniform = num_steps.size() != motions;  // (one count for several motions)
  std::vector<uint8_t> status(motions), cause(motions), fk_status(motions);
  std::vector<int32_t> first_collision(motions), min_sample(motions), min_sphere(motions), self_min_sample(motions),
      self_min_pair(motions);
  std::vector<double> min_clearance(motions), min_gradient(motions * 3), self_min_clearance(motions);
  std::array<double, 9> rotation{};
  if (g)
    for (int row = 0; row < 3; row++)
      for (int col = 0; col < 3; col++) rotation[static_cast<size_t>(row * 3 + col)] = g->OriginTransform()(row, col);
  const uint32_t flags = (options.outside_is_collision ? VGT_HIP_SPHERES_OUTSIDE_IS_COLLISION : 0u) |
                         (options.stop_at_collision ? VGT_HIP_MOTION_STOP_AT_COLLISION : 0u) |
                         (options.self_no_value_is_collision ? VGT_HIP_MOTION_SELF_NO_VALUE_IS_COLLISION : 0u);
  const int rc = vgt_hip_check_motions_with_self(
      detail::SharedSdfContext(tree.HipDevice()), g ? g->GetImmutableRawData().data() : nullptr,
      g ? g->NumXVoxels() : 0, g ? g->NumYVoxels() : 0, g ? g->NumZVoxels() : 0, g ? g->Resolution() : 0.0,
      g ? g->InverseOriginTransform().m.data() : nullptr, g ? rotation.data() : nullptr,
      s ? model.xyzr[0].data() : nullptr, s ? model.link.data() : nullptr, s, p ? pairs[0].data() : nullptr, p,
      tree.DeviceTree(), joints ? joint_from.data() : nullptr, joints ? joint_to.data() : nullptr,
      uniform ? nullptr : num_steps.data(), uniform ? num_steps[0] : 0, static_cast<int64_t>(motions),
      options.has_world_from_base ? options.world_from_base.m.data() : nullptr,
      options.joint_limits.empty() ? nullptr : options.joint_limits.data(), options.minimum_clearance,
      options.self_minimum_clearance, flags, status.data(), first_collision.data(), cause.data(), min_clearance.data(),
      min_sample.data(), min_sphere.data(), min_gradient.data(), self_min_clearance.data(), self_min_sample.data(),
      self_min_pair.data(), fk_status.data());
  if (rc != VGT_HIP_OK) detail::ThrowForCode(rc, vgt_hip_last_error());
  for (size_t e = 0; e < motions; e++)
  {
    MotionSelfCheck& check = out[e];
    check.status = status[e];
    check.first_collision = first_collision[e];
    check.collision_cause = cause[e];
    check.min_clearance = min_clearance[e];
    check.min_sample = min_sample[e];
    check.min_sphere = min_sphere[e];
    check.min_gradient = {{min_gradient[3 * e], min_gradient[3 * e + 1], min_gradient[3 * e + 2]}};
    check.self_min_clearance = self_min_clearance[e];
    check.self_min_sample = self_min_sample[e];
    check.self_min_pair = self_min_pair[e];
    check.fk_status = fk_status[e];
  }
  return out;
}
}  // namespace vgt_hip
