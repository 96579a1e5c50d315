// RasterizeSphereModel, RasterizeSphereModelIntoOccupancyMap and FindPointsOnSphereModel of
// include/vgt_hip/body_volumes.hpp on the C ABI (vgt_hip_rasterize_spheres, vgt_hip_spheres_cover_points).
#include "../../../include/vgt_hip/body_volumes.hpp"
#include "host_internal.hpp"

#include <cmath>
#include <limits>

namespace vgt_hip
{
namespace
{
// What the C ABI would refuse about the model and the poses, refused before a device is asked for; returns B.
int64_t CheckModelAndPoses(const SphereModel& model, const std::vector<double>& link_poses, int64_t num_links,
                           double padding)
{
  if (model.link.size() != model.xyzr.size())
    throw std::invalid_argument("a sphere model holds one link and one (x, y, z, r) per sphere");
  if (num_links < 0) throw std::invalid_argument("num_links must not be negative");
  if (!std::isfinite(padding)) throw std::invalid_argument("padding must be finite");
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
    throw std::invalid_argument("sphere volumes support fewer than 2^31 (configuration, sphere) pairs");
  return b;
}

static_assert(sizeof(std::array<double, 4>) == 4 * sizeof(double), "the spheres are passed as packed doubles");
const double* Spheres(const SphereModel& model) { return model.xyzr.empty() ? nullptr : model.xyzr[0].data(); }
}  // namespace

std::vector<int32_t> RasterizeSphereModel(int64_t num_x, int64_t num_y, int64_t num_z, double resolution,
                                          const Isometry3& origin_transform, const SphereModel& model,
                                          const std::vector<double>& link_poses, int64_t num_links,
                                          const SphereVolumeOptions& options, const std::vector<int32_t>* keep)
{
  if (num_x < 0 || num_y < 0 || num_z < 0) throw std::invalid_argument("grid extents must not be negative");
  if (!(resolution > 0.0) || !std::isfinite(resolution))
    throw std::invalid_argument("Grid must have uniform, positive resolution");
  const int64_t most = 0x7fffffffLL;
  if (num_x > most || num_y > most || num_z > most ||
      (num_x > 0 && num_y > 0 && num_z > 0 && (num_x * num_y > most || num_x * num_y * num_z > most)))
    throw std::invalid_argument("sphere volumes support grids below 2^31 cells");
  const int64_t b = CheckModelAndPoses(model, link_poses, num_links, options.padding);
  if (options.first_configuration_base < 0 || options.first_configuration_base > most - b)
    throw std::invalid_argument(
        "first_configuration_base must not be negative, and base + configurations at most 2^31 - 1");
  const size_t cells = static_cast<size_t>(num_x * num_y * num_z);
  if (keep != nullptr && keep->size() != cells)
    throw std::invalid_argument("the array to keep must hold one entry per cell of the grid");
  std::vector<int32_t> first = keep != nullptr ? *keep : std::vector<int32_t>(cells, -1);
  const int64_t s = static_cast<int64_t>(model.link.size());
  if (cells == 0 || b == 0 || s == 0) return first;  // (nothing covers anything: no device is needed)
  const Isometry3 grid_from_world = origin_transform.Inverse();
  const int rc = vgt_hip_rasterize_spheres(detail::SharedSdfContext(options.hip_device), num_x, num_y, num_z, resolution,
                                           grid_from_world.m.data(), Spheres(model), model.link.data(), s,
                                           link_poses.data(), num_links, b, options.padding,
                                           options.first_configuration_base, keep != nullptr ? VGT_HIP_SPHERES_KEEP : 0u,
                                           first.data());
  if (rc != VGT_HIP_OK) detail::ThrowForCode(rc, vgt_hip_last_error());
  return first;
}

int64_t RasterizeSphereModelIntoOccupancyMap(OccupancyMap& map, const SphereModel& model,
                                             const std::vector<double>& link_poses, int64_t num_links,
                                             const SphereOccupancyOptions& options)
{
  if (!map.IsInitialized()) throw std::invalid_argument("Grid must be initialized");
  SphereVolumeOptions volume;
  volume.padding = options.padding;
  volume.first_configuration_base = options.first_configuration_base;
  volume.hip_device = options.hip_device;
  const size_t cells = static_cast<size_t>(map.NumTotalVoxels());
  if (options.keep && (options.first_configuration == nullptr || options.first_configuration->size() != cells))
    throw std::invalid_argument("the array to keep must hold one entry per cell of the grid");
  const std::vector<int32_t>* keep = options.keep ? options.first_configuration : nullptr;
  // (the map's stored inverse is the one its other consumers pass on; RasterizeSphereModel inverts the same transform)
  std::vector<int32_t> first =
      RasterizeSphereModel(map.NumXVoxels(), map.NumYVoxels(), map.NumZVoxels(), map.Resolution(), map.OriginTransform(),
                           model, link_poses, num_links, volume, keep);
  auto& data = map.GetMutableRawData();
  int64_t covered = 0;
  for (size_t i = 0; i < cells; i++)
    if (first[i] >= 0)
    {
      data[i] = options.filled_value;
      covered++;
    }
  if (options.first_configuration != nullptr) *options.first_configuration = std::move(first);
  return covered;
}

PointsOnSphereModel FindPointsOnSphereModel(const std::vector<float>& points, const Isometry3& world_from_points,
                                            const SphereModel& model, const std::vector<double>& link_poses,
                                            int64_t num_links, const PointsOnSphereModelOptions& options)
{
  if (points.size() % 3 != 0) throw std::invalid_argument("points must hold three floats per point");
  const int64_t n = static_cast<int64_t>(points.size() / 3);
  if (n > 0x7fffffffLL) throw std::invalid_argument("sphere volumes support fewer than 2^31 points");
  const int64_t b = CheckModelAndPoses(model, link_poses, num_links, options.padding);
  PointsOnSphereModel out;
  out.first_configuration.assign(static_cast<size_t>(n), -1);
  out.first_sphere.assign(static_cast<size_t>(n), -1);
  if (options.filtered) out.filtered = points;
  const int64_t s = static_cast<int64_t>(model.link.size());
  if (n == 0 || b == 0 || s == 0) return out;  // (nothing covers anything: no device is needed)
  const int rc = vgt_hip_spheres_cover_points(
      detail::SharedSdfContext(options.hip_device), points.data(), n, world_from_points.m.data(), Spheres(model),
      model.link.data(), s, link_poses.data(), num_links, b, options.padding, 0u, out.first_configuration.data(),
      out.first_sphere.data(), options.filtered ? out.filtered.data() : nullptr);
  if (rc != VGT_HIP_OK) detail::ThrowForCode(rc, vgt_hip_last_error());
  return out;
}

PointsOnSphereModel FindPointsOnSphereModel(const PointCloudWrapper& cloud, const SphereModel& model,
                                            const std::vector<double>& link_poses, int64_t num_links,
                                            const PointsOnSphereModelOptions& options)
{
  const int64_t n = cloud.Size();
  if (n < 0) throw std::invalid_argument("the cloud's size must not be negative");
  std::vector<float> points(static_cast<size_t>(n) * 3);
  for (int64_t i = 0; i < n; i++) cloud.CopyPointLocationIntoFloatPtr(i, points.data() + 3 * i);
  return FindPointsOnSphereModel(points, cloud.PointCloudOriginTransform(), model, link_poses, num_links, options);
}
}  // namespace vgt_hip
