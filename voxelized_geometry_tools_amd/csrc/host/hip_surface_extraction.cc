// include/vgt_hip/surface_extraction.hpp on the C ABI (vgt_hip_extract_surface, vgt_hip_cells_extract_surface): one call
// counts, the mesh's vectors are sized, a second call fills them.  The host never loops over the voxels.
#include "../../../include/vgt_hip/surface_extraction.hpp"

#include <cmath>

#include "host_internal.hpp"

namespace vgt_hip
{
namespace
{
static_assert(sizeof(mesh_rasterizer::Vector3d) == 3 * sizeof(double) &&
                  sizeof(mesh_rasterizer::Vector3i) == 3 * sizeof(int32_t),
              "the C ABI fills vertices and triangles as packed arrays");

using detail::SharedSdfContext;
using detail::ThrowForCode;

// call(vertices, vertex_cells, vertex_capacity, triangles, triangle_capacity, &num_vertices, &num_triangles) -> code
template <typename Call>
SurfaceMesh CountThenFetch(const Call& call)
{
  SurfaceMesh mesh;
  int64_t num_vertices = 0, num_triangles = 0;
  int rc = call(nullptr, nullptr, 0, nullptr, 0, &num_vertices, &num_triangles);
  if (rc != VGT_HIP_OK) ThrowForCode(rc, vgt_hip_last_error());
  if (num_vertices == 0) return mesh;
  mesh.vertices.resize(static_cast<size_t>(num_vertices));
  mesh.vertex_cells.resize(static_cast<size_t>(num_vertices));
  mesh.triangles.resize(static_cast<size_t>(num_triangles));
  rc = call(mesh.vertices.data()->data(), mesh.vertex_cells.data(), num_vertices,
            num_triangles ? mesh.triangles.data()->data() : nullptr, num_triangles, &num_vertices, &num_triangles);
  if (rc != VGT_HIP_OK) ThrowForCode(rc, vgt_hip_last_error());
  return mesh;
}

// A float grid (OccupancyMap, the grid of a SignedDistanceField): the values go up with the call.
SurfaceMesh Extract(const DenseGrid& grid, float iso, int inside_above, int hip_device)
{
  if (!grid.IsInitialized()) throw std::invalid_argument("Grid must be initialized");
  if (!std::isfinite(iso)) throw std::invalid_argument("the iso level must be finite");
  vgt_hip_ctx* const ctx = SharedSdfContext(hip_device);
  return CountThenFetch([&](double* vertices, int32_t* vertex_cells, int64_t vertex_capacity, int32_t* triangles,
                            int64_t triangle_capacity, int64_t* num_vertices, int64_t* num_triangles) {
    return vgt_hip_extract_surface(ctx, grid.GetImmutableRawData().data(), grid.NumXVoxels(), grid.NumYVoxels(),
                                   grid.NumZVoxels(), iso, inside_above, grid.Resolution(),
                                   grid.OriginTransform().m.data(), vertices, vertex_cells, vertex_capacity, triangles,
                                   triangle_capacity, num_vertices, num_triangles);
  });
}

// A grid of cell records: uploaded once, both calls read the device copy.
template <typename Cell>
SurfaceMesh Extract(const CellGrid<Cell>& map, int hip_device)
{
  if (!map.IsInitialized()) throw std::invalid_argument("Grid must be initialized");
  vgt_hip_ctx* const ctx = SharedSdfContext(hip_device);
  vgt_hip_cells* cells = nullptr;
  // (the object ids play no part: every layout is uploaded as records with the occupancy first)
  const int created = vgt_hip_cells_create(ctx, map.GetImmutableRawData().data(), map.NumXVoxels(), map.NumYVoxels(),
                                           map.NumZVoxels(), static_cast<int32_t>(sizeof(Cell)), -1, &cells);
  if (created != VGT_HIP_OK) ThrowForCode(created, vgt_hip_last_error());
  struct Destroy
  {
    vgt_hip_cells* cells;
    ~Destroy() { vgt_hip_cells_destroy(cells); }
  } destroy{cells};
  return CountThenFetch([&](double* vertices, int32_t* vertex_cells, int64_t vertex_capacity, int32_t* triangles,
                            int64_t triangle_capacity, int64_t* num_vertices, int64_t* num_triangles) {
    return vgt_hip_cells_extract_surface(ctx, cells, map.Resolution(), map.OriginTransform().m.data(), vertices,
                                         vertex_cells, vertex_capacity, triangles, triangle_capacity, num_vertices,
                                         num_triangles);
  });
}
}  // namespace

SurfaceMesh ExtractSurfaceMesh(const SignedDistanceField& sdf, float iso, int hip_device)
{
  return Extract(sdf.grid, iso, 0, hip_device);
}
SurfaceMesh ExtractSurfaceMesh(const OccupancyMap& map, int hip_device) { return Extract(map, 0.5f, 1, hip_device); }
SurfaceMesh ExtractSurfaceMesh(const OccupancyComponentMap& map, int hip_device) { return Extract(map, hip_device); }
SurfaceMesh ExtractSurfaceMesh(const TaggedObjectOccupancyMap& map, int hip_device) { return Extract(map, hip_device); }
SurfaceMesh ExtractSurfaceMesh(const TaggedObjectOccupancyComponentMap& map, int hip_device)
{
  return Extract(map, hip_device);
}
}  // namespace vgt_hip
