// Body volumes of the C++ host layer: a robot modelled as spheres attached to links, rasterised into a voxel grid over a
// batch of configurations (the swept volume of a motion) or laid over a point cloud (the self-filter in front of the
// voxelizer), on the device (vgt_hip_rasterize_spheres / vgt_hip_spheres_cover_points of vgt_hip.h, which state every
// rule and output).  Forward kinematics stays with the caller.
#pragma once

#include <cstdint>
#include <vector>

#include "body_queries.hpp"
#include "host_types.hpp"

namespace vgt_hip
{
struct SphereVolumeOptions
{
  double padding = 0.0;                  // added to every radius; finite, may be negative
  int64_t first_configuration_base = 0;  // an answer is base + the configuration's index
  int hip_device = 0;
};
// The cells of a num_x x num_y x num_z grid at `resolution` under `origin_transform` (world_from_grid) that the model
// covers in some configuration: per cell, X-major / Z-fastest, base + the least such configuration, -1 where none does.
// `link_poses`: B * num_links * 16 doubles, world_from_link column-major, in the frame the origin transform maps to.
// `keep` (optional): the result of an earlier call over the same grid; the answer is then the unsigned minimum of the
// two, so a motion can be rasterised piece by piece with rising bases, in any order.
// Uses the process's shared context of `hip_device`.  Throws std::invalid_argument where the C ABI reports an invalid
// argument (and for a model whose two vectors differ in length, poses that are not a whole number of configurations,
// or a `keep` of another size), std::runtime_error for its other errors.
std::vector<int32_t> RasterizeSphereModel(int64_t num_x, int64_t num_y, int64_t num_z, double resolution,
                                          const Isometry3& origin_transform, const SphereModel& model,
                                          const std::vector<double>& link_poses, int64_t num_links,
                                          const SphereVolumeOptions& options = {},
                                          const std::vector<int32_t>* keep = nullptr);

struct SphereOccupancyOptions
{
  double padding = 0.0;
  int64_t first_configuration_base = 0;
  float filled_value = 1.0f;  // what a covered cell is set to
  int hip_device = 0;
  // When not null: receives the per-cell answer of RasterizeSphereModel.  With `keep` it is input as well (it must then
  // hold one entry per cell: the result of an earlier call), the answer is the unsigned minimum of the two as above, and
  // the cells set to filled are all those covered in it afterwards.
  std::vector<int32_t>* first_configuration = nullptr;
  bool keep = false;
};
// Sets the cells of `map` that the model covers to options.filled_value and leaves every other cell as it is.
// Returns the number of covered cells.
int64_t RasterizeSphereModelIntoOccupancyMap(OccupancyMap& map, const SphereModel& model,
                                             const std::vector<double>& link_poses, int64_t num_links,
                                             const SphereOccupancyOptions& options = {});

// One entry per point; `filtered` (3 floats per point: the point bit for bit where nothing covers it, NaN x3 where
// something does -- a cloud the voxelizer takes as it stands, since it skips non-finite points) only when asked for.
struct PointsOnSphereModel
{
  std::vector<int32_t> first_configuration, first_sphere;
  std::vector<float> filtered;
};
struct PointsOnSphereModelOptions
{
  double padding = 0.0;
  bool filtered = true;
  int hip_device = 0;
};
// `points`: 3 floats per point in the frame `world_from_points` maps to the world of the link poses.
PointsOnSphereModel FindPointsOnSphereModel(const std::vector<float>& points, const Isometry3& world_from_points,
                                            const SphereModel& model, const std::vector<double>& link_poses,
                                            int64_t num_links, const PointsOnSphereModelOptions& options = {});
// The cloud's points under its PointCloudOriginTransform().
PointsOnSphereModel FindPointsOnSphereModel(const PointCloudWrapper& cloud, const SphereModel& model,
                                            const std::vector<double>& link_poses, int64_t num_links,
                                            const PointsOnSphereModelOptions& options = {});
}  // namespace vgt_hip
