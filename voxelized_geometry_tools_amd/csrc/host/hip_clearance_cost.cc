// ClearanceCost (include/vgt_hip/clearance_cost.hpp) on the C ABI (vgt_hip_clearance_cost).
#include "../../../include/vgt_hip/clearance_cost.hpp"
#include "host_internal.hpp"

#include <cmath>

namespace vgt_hip
{
ClearanceCosts ClearanceCost(const SignedDistanceField& sdf, const SphereModel& model, const KinematicTree& tree,
                             const std::vector<double>& joint_values, double margin, const ClearanceCostOptions& options,
                             int64_t num_configurations)
{
  const DenseGrid& g = sdf.grid;
  if (!g.IsInitialized()) throw std::invalid_argument("Grid must be initialized");
  if (model.link.size() != model.xyzr.size())
    throw std::invalid_argument("a sphere model holds one link and one (x, y, z, r) per sphere");
  static_assert(sizeof(std::array<double, 4>) == 4 * sizeof(double), "the spheres are passed as packed doubles");
  if (!(margin > 0.0) || !std::isfinite(margin)) throw std::invalid_argument("margin must be positive and finite");
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
  if (joints == 0 ? (!joint_values.empty() || num_configurations < 0)
                  : (joint_values.size() % joints != 0 ||
                     (num_configurations >= 0 && joint_values.size() / joints != static_cast<size_t>(num_configurations))))
    throw std::invalid_argument("joint_values must hold one value per configuration and joint");
  const size_t configurations = joints == 0 ? static_cast<size_t>(num_configurations) : joint_values.size() / joints;
  const uint64_t most = 0x7fffffffu;
  if (configurations > most || configurations * joints > most || configurations * static_cast<uint64_t>(s) > most ||
      configurations * static_cast<uint64_t>(tree.NumLinks()) > most)
    throw std::invalid_argument(
        "clearance costs support fewer than 2^31 configurations and (configuration, joint / sphere / link) pairs");
  if (vgt_hip_cost_tile_samples(tree.NumLinks()) == 0)
  {
    // (the library says which trees it takes; the most links for the message: the tile sizes do not grow with the links)
    int64_t links = 1;
    for (int64_t step = int64_t{1} << 30; step > 0; step >>= 1)
      if (vgt_hip_cost_tile_samples(links + step) != 0) links += step;
    throw std::invalid_argument("clearance costs take trees of at most " + std::to_string(links) +
                                " links, this one has " + std::to_string(tree.NumLinks()));
  }

  ClearanceCosts out;
  if (configurations == 0) return out;  // (no device is needed)
  out.cost.resize(configurations);
  out.num_active.resize(configurations);
  out.num_outside.resize(configurations);
  out.fk_status.resize(configurations);
  if (options.with_gradient)
  {
    out.joint_gradient.resize(configurations * joints);
    out.num_without_gradient.resize(configurations);
  }
  // (a tree without joints: the gradient has no elements, and one double stands in for its address)
  double none = 0.0;
  std::array<double, 9> rotation{};
  for (int row = 0; row < 3; row++)
    for (int col = 0; col < 3; col++) rotation[static_cast<size_t>(row * 3 + col)] = g.OriginTransform()(row, col);
  const int rc = vgt_hip_clearance_cost(
      detail::SharedSdfContext(tree.HipDevice()), g.GetImmutableRawData().data(), g.NumXVoxels(), g.NumYVoxels(),
      g.NumZVoxels(), g.Resolution(), g.InverseOriginTransform().m.data(), rotation.data(),
      s ? model.xyzr[0].data() : nullptr, s ? model.link.data() : nullptr, s, tree.DeviceTree(),
      joints ? joint_values.data() : nullptr, static_cast<int64_t>(configurations),
      options.has_world_from_base ? options.world_from_base.m.data() : nullptr,
      options.joint_limits.empty() ? nullptr : options.joint_limits.data(), margin, 0u, out.cost.data(),
      options.with_gradient ? (joints ? out.joint_gradient.data() : &none) : nullptr, out.num_active.data(),
      out.num_outside.data(), options.with_gradient ? out.num_without_gradient.data() : nullptr, out.fk_status.data());
  if (rc != VGT_HIP_OK) detail::ThrowForCode(rc, vgt_hip_last_error());
  return out;
}
}  // namespace vgt_hip
