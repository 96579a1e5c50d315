// CheckSphereModel of include/vgt_hip/body_queries.hpp on the C ABI (vgt_hip_check_spheres).
#include "../../../include/vgt_hip/body_queries.hpp"
#include "host_internal.hpp"

#include <cmath>
#include <limits>

namespace vgt_hip
{
SphereModelChecks CheckSphereModel(const SignedDistanceField& sdf, const SphereModel& model,
                                   const std::vector<double>& link_poses, int64_t num_links,
                                   const SphereModelOptions& options)
{
  const DenseGrid& g = sdf.grid;
  if (!g.IsInitialized()) throw std::invalid_argument("Grid must be initialized");
  if (model.link.size() != model.xyzr.size())
    throw std::invalid_argument("a sphere model holds one link and one (x, y, z, r) per sphere");
  // (what the C ABI would refuse, refused before a device is asked for)
  if (num_links < 0) throw std::invalid_argument("num_links must not be negative");
  if (std::isnan(options.minimum_clearance)) throw std::invalid_argument("minimum_clearance must not be NaN");
  const int64_t s = static_cast<int64_t>(model.link.size());
  if (num_links == 0 && s > 0) throw std::invalid_argument("a model with spheres needs at least one link (num_links == 0)");
  for (int64_t i = 0; i < s; i++)
  {
    const size_t k = static_cast<size_t>(i);
    if (model.link[k] < 0 || model.link[k] >= num_links)
      throw std::invalid_argument("sphere " + std::to_string(i) + ": link " + std::to_string(model.link[k]) +
                                  " is not in [0, num_links)");
    if (!(model.xyzr[k][3] >= 0.0))
      throw std::invalid_argument("sphere " + std::to_string(i) + ": the radius must not be negative or NaN");
  }
  const size_t per_configuration = static_cast<size_t>(num_links) * 16;
  if (per_configuration == 0 ? !link_poses.empty() : link_poses.size() % per_configuration != 0)
    throw std::invalid_argument("link_poses must hold num_links * 16 doubles per configuration");
  const int64_t b = per_configuration == 0 ? 0 : static_cast<int64_t>(link_poses.size() / per_configuration);
  if (b * s > 0x7fffffffLL)
    throw std::invalid_argument("sphere-model checks support fewer than 2^31 (configuration, sphere) pairs");

  SphereModelChecks out;
  const size_t nb = static_cast<size_t>(b), ns = static_cast<size_t>(s);
  const double nan = std::numeric_limits<double>::quiet_NaN();
  out.status.assign(nb, VGT_HIP_SPHERES_NO_VALUE);
  out.min_clearance.assign(nb, nan);
  out.min_sphere.assign(nb, -1);
  out.num_below.assign(nb, 0);
  out.num_outside.assign(nb, 0);
  out.min_gradient.assign(nb * 3, nan);
  if (options.per_sphere)
  {
    out.sphere_clearance.assign(nb * ns, nan);
    out.sphere_gradient.assign(nb * ns * 3, nan);
  }
  if (b == 0 || s == 0) return out;  // (nothing is comparable: no device is needed)

  std::array<double, 9> rotation{};
  for (int row = 0; row < 3; row++)
    for (int col = 0; col < 3; col++) rotation[static_cast<size_t>(row * 3 + col)] = g.OriginTransform()(row, col);
  static_assert(sizeof(std::array<double, 4>) == 4 * sizeof(double), "the spheres are passed as packed doubles");
  const int rc = vgt_hip_check_spheres(
      detail::SharedSdfContext(options.hip_device), g.GetImmutableRawData().data(), g.NumXVoxels(), g.NumYVoxels(),
      g.NumZVoxels(), g.Resolution(), g.InverseOriginTransform().m.data(), rotation.data(), model.xyzr[0].data(),
      model.link.data(), s, link_poses.data(), num_links, b, options.minimum_clearance,
      options.outside_is_collision ? VGT_HIP_SPHERES_OUTSIDE_IS_COLLISION : 0u, out.status.data(),
      out.min_clearance.data(), out.min_sphere.data(), out.num_below.data(), out.num_outside.data(),
      out.min_gradient.data(), options.per_sphere ? out.sphere_clearance.data() : nullptr,
      options.per_sphere ? out.sphere_gradient.data() : nullptr);
  if (rc != VGT_HIP_OK) detail::ThrowForCode(rc, vgt_hip_last_error());
  return out;
}
}  // namespace vgt_hip
