// CheckMotions (include/vgt_hip/motion_queries.hpp) on the C ABI (vgt_hip_check_motions).
#include "../../../include/vgt_hip/motion_queries.hpp"
#include "host_internal.hpp"

#include <cmath>

namespace vgt_hip
{
std::vector<MotionCheck> CheckMotions(const SignedDistanceField& sdf, const SphereModel& model, const KinematicTree& tree,
                                      const std::vector<double>& joint_from, const std::vector<double>& joint_to,
                                      const std::vector<int32_t>& num_steps, const MotionOptions& options)
{
  const DenseGrid& g = sdf.grid;
  if (!g.IsInitialized()) throw std::invalid_argument("Grid must be initialized");
  if (model.link.size() != model.xyzr.size())
    throw std::invalid_argument("a sphere model holds one link and one (x, y, z, r) per sphere");
  static_assert(sizeof(std::array<double, 4>) == 4 * sizeof(double), "the spheres are passed as packed doubles");
  if (std::isnan(options.minimum_clearance)) throw std::invalid_argument("minimum_clearance must not be NaN");
  if (!options.joint_limits.empty() && options.joint_limits.size() != static_cast<size_t>(tree.NumJoints()) * 2)
    throw std::invalid_argument("joint_limits must hold a lower and an upper value per joint");
  // (what the C ABI would refuse, refused before a device is asked for, in its words)
  const int64_t s = static_cast<int64_t>(model.link.size());
  for (int64_t i = 0; i < s; i++)
  {
    const size_t k = static_cast<size_t>(i);
    if (model.link[k] < 0 || model.link[k] >= tree.NumLinks())
      throw std::invalid_argument("sphere " + std::to_string(i) + ": link " + std::to_string(model.link[k]) +
                                  " is not in [0, num_links)");
    if (!(model.xyzr[k][3] >= 0.0))
      throw std::invalid_argument("sphere " + std::to_string(i) + ": the radius must not be negative or NaN");
  }
  const size_t joints = static_cast<size_t>(tree.NumJoints());
  if (joint_from.size() != joint_to.size() || (joints == 0 ? !joint_from.empty() : joint_from.size() % joints != 0))
    throw std::invalid_argument("joint_from and joint_to must hold one value per motion and joint");
  const size_t motions = joints == 0 ? num_steps.size() : joint_from.size() / joints;
  if (num_steps.size() != motions && num_steps.size() != 1)
    throw std::invalid_argument("num_steps must hold one count per motion, or one for all");
  for (size_t e = 0; e < num_steps.size(); e++)
    if (num_steps[e] < 0)
      throw std::invalid_argument("motion " + std::to_string(e) + ": num_steps " + std::to_string(num_steps[e]));
  if (motions > 0x7fffffffu || motions * joints > 0x7fffffffu)
    throw std::invalid_argument("motion checks support fewer than 2^31 motions and (motion, joint) pairs");
  if (vgt_hip_motion_tile_samples(tree.NumLinks()) == 0)
  {
    // (the library says which trees it takes; the most links for the message: the tile sizes do not grow with the links)
    int64_t most = 1;
    for (int64_t step = int64_t{1} << 30; step > 0; step >>= 1)
      if (vgt_hip_motion_tile_samples(most + step) != 0) most += step;
    throw std::invalid_argument("motion checks take trees of at most " + std::to_string(most) + " links, this one has " +
                                std::to_string(tree.NumLinks()));
  }

  std::vector<MotionCheck> out(motions);
  if (motions == 0) return out;  // (no device is needed)
  const bool uniform = num_steps.size() != motions;  // (one count for several motions)
  std::vector<uint8_t> status(motions), fk_status(motions);
  std::vector<int32_t> first_collision(motions), min_sample(motions), min_sphere(motions);
  std::vector<double> min_clearance(motions), min_gradient(motions * 3);
  std::array<double, 9> rotation{};
  for (int row = 0; row < 3; row++)
    for (int col = 0; col < 3; col++) rotation[static_cast<size_t>(row * 3 + col)] = g.OriginTransform()(row, col);
  const uint32_t flags = (options.outside_is_collision ? VGT_HIP_SPHERES_OUTSIDE_IS_COLLISION : 0u) |
                         (options.stop_at_collision ? VGT_HIP_MOTION_STOP_AT_COLLISION : 0u);
  const int rc = vgt_hip_check_motions(
      detail::SharedSdfContext(tree.HipDevice()), g.GetImmutableRawData().data(), g.NumXVoxels(), g.NumYVoxels(),
      g.NumZVoxels(), g.Resolution(), g.InverseOriginTransform().m.data(), rotation.data(),
      s ? model.xyzr[0].data() : nullptr, s ? model.link.data() : nullptr, s, tree.DeviceTree(),
      joints ? joint_from.data() : nullptr, joints ? joint_to.data() : nullptr, uniform ? nullptr : num_steps.data(),
      uniform ? num_steps[0] : 0, static_cast<int64_t>(motions),
      options.has_world_from_base ? options.world_from_base.m.data() : nullptr,
      options.joint_limits.empty() ? nullptr : options.joint_limits.data(), options.minimum_clearance, flags,
      status.data(), first_collision.data(), min_clearance.data(), min_sample.data(), min_sphere.data(),
      min_gradient.data(), fk_status.data());
  if (rc != VGT_HIP_OK) detail::ThrowForCode(rc, vgt_hip_last_error());
  for (size_t e = 0; e < motions; e++)
  {
    MotionCheck& check = out[e];
    check.status = status[e];
    check.first_collision = first_collision[e];
    check.min_clearance = min_clearance[e];
    check.min_sample = min_sample[e];
    check.min_sphere = min_sphere[e];
    check.min_gradient = {{min_gradient[3 * e], min_gradient[3 * e + 1], min_gradient[3 * e + 2]}};
    check.fk_status = fk_status[e];
  }
  return out;
}
}  // namespace vgt_hip
