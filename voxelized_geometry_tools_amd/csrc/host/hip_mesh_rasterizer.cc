// include/vgt_hip/mesh_rasterizer.hpp on the C ABI (vgt_hip_rasterize_mesh, vgt_hip_mesh_grid_for).
#include "../../../include/vgt_hip/mesh_rasterizer.hpp"

#include "../../../include/vgt_hip/hip_pointcloud_voxelizer.hpp"
#include "host_internal.hpp"

namespace vgt_hip
{
namespace mesh_rasterizer
{
namespace
{
static_assert(sizeof(Vector3d) == 3 * sizeof(double) && sizeof(Vector3i) == 3 * sizeof(int32_t),
              "vertices and triangles are passed to the C ABI as packed arrays");

using detail::ThrowForCode;

template <typename Map>
void Rasterize(const std::vector<Vector3d>& vertices, const Vector3i* triangles, size_t num_triangles, Map& map,
               const Isometry3& inverse_origin, bool enforce, int hip_device, ClosestPointRule rule)
{
  if (!map.IsInitialized()) throw std::invalid_argument("occupancy_map must be initialized");
  auto& cells = map.GetMutableRawData();
  static_assert(sizeof(cells[0]) == 4 || sizeof(cells[0]) == 8, "OccupancyCell or OccupancyComponentCell");
  if (num_triangles == 0) return;
  // (the process's context of that device: it keeps the rasterizer's scratch between calls)
  vgt_hip_ctx* const ctx = detail::SharedSdfContext(hip_device);
  const double no_vertex[3] = {0.0, 0.0, 0.0};  // (an empty vector has no data(): every index is out of range then)
  const int rc = vgt_hip_rasterize_mesh(
      ctx, vertices.empty() ? no_vertex : vertices.data()->data(), static_cast<int64_t>(vertices.size()),
      triangles->data(), static_cast<int64_t>(num_triangles), cells.data(), static_cast<int>(sizeof(cells[0])),
      map.NumXVoxels(), map.NumYVoxels(), map.NumZVoxels(), map.Resolution(), map.OriginTransform().m.data(),
      inverse_origin.m.data(), enforce ? 1 : 0, static_cast<int>(rule));
  if (rc != VGT_HIP_OK) ThrowForCode(rc, vgt_hip_last_error());
}

void RasterizeInto(const std::vector<Vector3d>& vertices, const Vector3i* triangles, size_t num_triangles,
                   OccupancyMap& map, bool enforce, int hip_device, ClosestPointRule rule)
{
  Rasterize(vertices, triangles, num_triangles, map, map.InverseOriginTransform(), enforce, hip_device, rule);
}
void RasterizeInto(const std::vector<Vector3d>& vertices, const Vector3i* triangles, size_t num_triangles,
                   OccupancyComponentMap& map, bool enforce, int hip_device, ClosestPointRule rule)
{
  Rasterize(vertices, triangles, num_triangles, map, map.OriginTransform().Inverse(), enforce, hip_device, rule);
}

struct GridFor
{
  int64_t nx = 0, ny = 0, nz = 0;
  Isometry3 origin;
};
GridFor MeshGridFor(const std::vector<Vector3d>& vertices, double resolution)
{
  if (!(resolution > 0.0)) throw std::invalid_argument("resolution must be greater than zero");  // (:238-241)
  GridFor grid;
  double origin[3];
  const int rc = vgt_hip_mesh_grid_for(vertices.empty() ? nullptr : vertices.data()->data(),
                                       static_cast<int64_t>(vertices.size()), resolution, &grid.nx, &grid.ny, &grid.nz,
                                       origin);
  if (rc != VGT_HIP_OK) ThrowForCode(rc, vgt_hip_last_error());
  grid.origin = Isometry3::Translation(origin[0], origin[1], origin[2]);
  return grid;
}
}  // namespace

void RasterizeTriangle(const std::vector<Vector3d>& vertices, const std::vector<Vector3i>& triangles,
                       size_t triangle_index, OccupancyMap& occupancy_map, bool enforce_occupancy_map_contains_triangle,
                       int hip_device, ClosestPointRule rule)
{
  RasterizeInto(vertices, &triangles.at(triangle_index), 1, occupancy_map, enforce_occupancy_map_contains_triangle,
                hip_device, rule);
}

void RasterizeTriangle(const std::vector<Vector3d>& vertices, const std::vector<Vector3i>& triangles,
                       size_t triangle_index, OccupancyComponentMap& occupancy_map,
                       bool enforce_occupancy_map_contains_triangle, int hip_device, ClosestPointRule rule)
{
  RasterizeInto(vertices, &triangles.at(triangle_index), 1, occupancy_map, enforce_occupancy_map_contains_triangle,
                hip_device, rule);
}

void RasterizeMesh(const std::vector<Vector3d>& vertices, const std::vector<Vector3i>& triangles,
                   OccupancyMap& occupancy_map, bool enforce_occupancy_map_contains_mesh, int hip_device,
                   ClosestPointRule rule)
{
  RasterizeInto(vertices, triangles.data(), triangles.size(), occupancy_map, enforce_occupancy_map_contains_mesh,
                hip_device, rule);
}

void RasterizeMesh(const std::vector<Vector3d>& vertices, const std::vector<Vector3i>& triangles,
                   OccupancyComponentMap& occupancy_map, bool enforce_occupancy_map_contains_mesh, int hip_device,
                   ClosestPointRule rule)
{
  RasterizeInto(vertices, triangles.data(), triangles.size(), occupancy_map, enforce_occupancy_map_contains_mesh,
                hip_device, rule);
}

OccupancyMap RasterizeMeshIntoOccupancyMap(const std::vector<Vector3d>& vertices, const std::vector<Vector3i>& triangles,
                                           double resolution, int hip_device, ClosestPointRule rule)
{
  const GridFor grid = MeshGridFor(vertices, resolution);
  OccupancyMap occupancy_map(grid.origin, "mesh", resolution, grid.nx, grid.ny, grid.nz, 0.0f);  // (:271-273)
  RasterizeMesh(vertices, triangles, occupancy_map, true, hip_device, rule);                       // (:275)
  return occupancy_map;
}

OccupancyComponentMap RasterizeMeshIntoOccupancyComponentMap(const std::vector<Vector3d>& vertices,
                                                             const std::vector<Vector3i>& triangles, double resolution,
                                                             int hip_device, ClosestPointRule rule)
{
  const GridFor grid = MeshGridFor(vertices, resolution);
  OccupancyComponentMap occupancy_map(grid.origin, "mesh", resolution, grid.nx, grid.ny, grid.nz,
                                      OccupancyComponentCell{0.0f, 0u});
  RasterizeMesh(vertices, triangles, occupancy_map, true, hip_device, rule);
  return occupancy_map;
}

SignedDistanceField MeshToSignedDistanceField(const std::vector<Vector3d>& vertices,
                                              const std::vector<Vector3i>& triangles, double resolution,
                                              const SignedDistanceFieldGenerationParameters& parameters,
                                              ClosestPointRule rule)
{
  const OccupancyMap occupancy_map = RasterizeMeshIntoOccupancyMap(vertices, triangles, resolution, parameters.hip_device, rule);
  return ExtractSignedDistanceField(occupancy_map, parameters);
}

OccupancyMap RasterizeSolidMeshIntoOccupancyMap(const std::vector<Vector3d>& vertices,
                                                const std::vector<Vector3i>& triangles, double resolution,
                                                int hip_device, ClosestPointRule rule)
{
  OccupancyMap occupancy_map = RasterizeMeshIntoOccupancyMap(vertices, triangles, resolution, hip_device, rule);
  FillEnclosedSpace(occupancy_map, true, hip_device);
  return occupancy_map;
}

OccupancyComponentMap RasterizeSolidMeshIntoOccupancyComponentMap(const std::vector<Vector3d>& vertices,
                                                                  const std::vector<Vector3i>& triangles,
                                                                  double resolution, int hip_device,
                                                                  ClosestPointRule rule)
{
  OccupancyComponentMap occupancy_map =
      RasterizeMeshIntoOccupancyComponentMap(vertices, triangles, resolution, hip_device, rule);
  FillEnclosedSpace(occupancy_map, true, hip_device);
  return occupancy_map;
}

SignedDistanceField SolidMeshToSignedDistanceField(const std::vector<Vector3d>& vertices,
                                                   const std::vector<Vector3i>& triangles, double resolution,
                                                   const SignedDistanceFieldGenerationParameters& parameters,
                                                   ClosestPointRule rule)
{
  const OccupancyMap occupancy_map =
      RasterizeSolidMeshIntoOccupancyMap(vertices, triangles, resolution, parameters.hip_device, rule);
  return ExtractSignedDistanceField(occupancy_map, parameters);
}
}  // namespace mesh_rasterizer
}  // namespace vgt_hip
