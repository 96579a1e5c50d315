// SelfCollisionPairs and CheckSelfCollision (include/vgt_hip/self_collision.hpp) on the C ABI
// (vgt_hip_self_collision_pairs, vgt_hip_check_self_collision).
#include "../../../include/vgt_hip/self_collision.hpp"
#include "host_internal.hpp"

#include <cmath>

namespace vgt_hip
{
namespace
{
void CheckModelLengths(const SphereModel& model)
{
  if (model.link.size() != model.xyzr.size())
    throw std::invalid_argument("a sphere model holds one link and one (x, y, z, r) per sphere");
}
}  // namespace

std::vector<SpherePair> SelfCollisionPairs(const SphereModel& model, const KinematicTree& tree,
                                           const std::vector<LinkPair>& ignored_link_pairs,
                                           const SelfCollisionPairOptions& options)
{
  CheckModelLengths(model);
  static_assert(sizeof(SpherePair) == 2 * sizeof(int32_t), "the pairs are passed as packed int32");
  std::vector<int32_t> parent;
  for (const KinematicLink& link : tree.Links()) parent.push_back(link.parent);
  const int64_t spheres = static_cast<int64_t>(model.link.size());
  const int64_t ignored = static_cast<int64_t>(ignored_link_pairs.size());
  const uint32_t flags = options.skip_adjacent ? VGT_HIP_SELF_PAIRS_SKIP_ADJACENT : 0u;
  std::vector<SpherePair> out;
  int64_t count = 0;
  // (once to count, once to fill)
  for (int pass = 0; pass < 2; pass++)
  {
    const int rc = vgt_hip_self_collision_pairs(spheres ? model.link.data() : nullptr, spheres, parent.data(),
                                                tree.NumLinks(), ignored ? ignored_link_pairs[0].data() : nullptr,
                                                ignored, flags, out.empty() ? nullptr : out[0].data(),
                                                static_cast<int64_t>(out.size()), &count);
    if (rc != VGT_HIP_OK) detail::ThrowForCode(rc, vgt_hip_last_error());
    if (pass == 0 && count > 0) out.resize(static_cast<size_t>(count));
    if (count == 0) break;
  }
  return out;
}

SelfCollisionChecks CheckSelfCollision(const SphereModel& model, const KinematicTree& tree,
                                       const std::vector<SpherePair>& pairs, const std::vector<double>& joint_values,
                                       const SelfCollisionOptions& options, int64_t num_configurations)
{
  CheckModelLengths(model);
  static_assert(sizeof(std::array<double, 4>) == 4 * sizeof(double), "the spheres are passed as packed doubles");
  if (std::isnan(options.minimum_clearance)) throw std::invalid_argument("minimum_clearance must not be NaN");
  if (!options.joint_limits.empty() && options.joint_limits.size() != static_cast<size_t>(tree.NumJoints()) * 2)
    throw std::invalid_argument("joint_limits must hold a lower and an upper value per joint");
  // (what the C ABI would refuse, refused before a device is asked for, in its words)
  const int64_t s = static_cast<int64_t>(model.link.size());
  const int64_t p = static_cast<int64_t>(pairs.size());
  for (int64_t i = 0; i < s; i++)
  {
    const size_t k = static_cast<size_t>(i);
    if (!(model.xyzr[k][3] >= 0.0))
      throw std::invalid_argument("sphere " + std::to_string(i) + ": the radius must not be negative or NaN");
  }
  for (int64_t i = 0; s > 0 && i < p; i++)
  {
    const SpherePair& pair = pairs[static_cast<size_t>(i)];
    for (const int32_t sphere : pair)
      if (sphere < 0 || sphere >= s)
        throw std::invalid_argument("pair " + std::to_string(i) + ": sphere " + std::to_string(sphere) +
                                    " is outside [0, " + std::to_string(s) + ")");
    if (pair[0] >= pair[1])
      throw std::invalid_argument("pair " + std::to_string(i) + ": (" + std::to_string(pair[0]) + ", " +
                                  std::to_string(pair[1]) + ") is not ascending");
  }
  for (int64_t i = 0; i < s; i++)
  {
    const size_t k = static_cast<size_t>(i);
    if (model.link[k] < 0 || model.link[k] >= tree.NumLinks())
      throw std::invalid_argument("sphere " + std::to_string(i) + ": link " + std::to_string(model.link[k]) +
                                  " is not in [0, num_links)");
  }
  const size_t joints = static_cast<size_t>(tree.NumJoints());
  if (joints == 0 ? (!joint_values.empty() || num_configurations < 0)
                  : (joint_values.size() % joints != 0 ||
                     (num_configurations >= 0 && joint_values.size() / joints != static_cast<size_t>(num_configurations))))
    throw std::invalid_argument("joint_values must hold one value per configuration and joint");
  const size_t configurations = joints == 0 ? static_cast<size_t>(num_configurations) : joint_values.size() / joints;
  const uint64_t most = 0x7fffffffu;
  if (configurations > most || static_cast<uint64_t>(p) > most || configurations * joints > most ||
      configurations * static_cast<uint64_t>(tree.NumLinks()) > most ||
      (options.per_pair && configurations * static_cast<uint64_t>(p) > most))
    throw std::invalid_argument(
        "self-collision checks support fewer than 2^31 configurations, pairs and (configuration, joint / link / pair) "
        "pairs");
  if (vgt_hip_self_collision_tile_samples(tree.NumLinks(), s) == 0)
    throw std::invalid_argument("self-collision checks take 96 bytes per link + 32 per sphere + 256 within 65536, this "
                                "model has " + std::to_string(tree.NumLinks()) + " links and " + std::to_string(s) +
                                " spheres");

  SelfCollisionChecks out;
  if (configurations == 0) return out;  // (no device is needed)
  out.status.resize(configurations);
  out.num_below.resize(configurations);
  out.num_without_value.resize(configurations);
  out.min_clearance.resize(configurations);
  out.min_pair.resize(configurations);
  out.min_direction.resize(configurations * 3);
  out.fk_status.resize(configurations);
  if (options.with_gradient) out.joint_gradient.resize(configurations * joints);
  // (NaN: a model without spheres leaves the per-pair output as it is)
  if (options.per_pair) out.pair_clearance.assign(configurations * static_cast<size_t>(p), std::nan(""));
  // (a tree without joints, a list without pairs: the output has no elements, and one double stands in for its address)
  double none = 0.0;
  const int rc = vgt_hip_check_self_collision(
      detail::SharedSdfContext(tree.HipDevice()), s ? model.xyzr[0].data() : nullptr, s ? model.link.data() : nullptr, s,
      p ? pairs[0].data() : nullptr, p, tree.DeviceTree(), joints ? joint_values.data() : nullptr,
      static_cast<int64_t>(configurations), options.has_world_from_base ? options.world_from_base.m.data() : nullptr,
      options.joint_limits.empty() ? nullptr : options.joint_limits.data(), options.minimum_clearance,
      options.no_value_is_collision ? VGT_HIP_SELF_NO_VALUE_IS_COLLISION : 0u, out.status.data(), out.num_below.data(),
      out.num_without_value.data(), out.min_clearance.data(), out.min_pair.data(), out.min_direction.data(),
      options.with_gradient ? (joints ? out.joint_gradient.data() : &none) : nullptr, out.fk_status.data(),
      options.per_pair ? (out.pair_clearance.empty() ? &none : out.pair_clearance.data()) : nullptr);
  if (rc != VGT_HIP_OK) detail::ThrowForCode(rc, vgt_hip_last_error());
  return out;
}
}  // namespace vgt_hip
