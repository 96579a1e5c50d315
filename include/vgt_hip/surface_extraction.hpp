// The iso-surface of a signed distance field or of a map's occupancy as an indexed triangle mesh, on the HIP backend
// (an extension: the reference exports cubes only).  Surface nets on the lattice of cell centres; include/vgt_hip.h,
// vgt_hip_extract_surface, states every rule: which cubes carry a vertex and where it lies, which lattice edges carry a
// quad, the orientation (normals point from inside to outside, a closed mesh has positive signed volume) and the two
// orders (vertices by their cube's linear index, quads by their edge's lower sample, then axis x, y, z).
// Implemented in csrc/host/hip_surface_extraction.cc on vgt_hip_extract_surface / vgt_hip_cells_extract_surface.
//
// The grid's Resolution() is the cell size and its OriginTransform() maps the vertices to the grid's frame, as the
// display exports of hip_pointcloud_voxelizer.hpp place their cubes.  The mesh has the types of mesh_rasterizer.hpp:
// mesh_rasterizer::RasterizeMesh takes `vertices` and `triangles` as they are.
//
// Exceptions: std::invalid_argument for a grid that is not initialised, a non-finite iso and a surface of 2^31 / 3
// triangles or more; std::runtime_error for a device that cannot be used.
#pragma once

#include <cstdint>
#include <vector>

#include "host_types.hpp"
#include "mesh_rasterizer.hpp"

namespace vgt_hip
{
struct SurfaceMesh
{
  std::vector<mesh_rasterizer::Vector3d> vertices;   // x, y, z in the grid's frame
  std::vector<mesh_rasterizer::Vector3i> triangles;  // indices into `vertices`; two consecutive triangles are one quad
  std::vector<int32_t> vertex_cells;  // per vertex: (x * NumYVoxels + y) * NumZVoxels + z of its cube's lowest corner
};

// Inside is distance < iso.
SurfaceMesh ExtractSurfaceMesh(const SignedDistanceField& sdf, float iso = 0.0f, int hip_device = 0);
// Inside is occupancy > 0.5: the surface between the filled cells and everything else.
SurfaceMesh ExtractSurfaceMesh(const OccupancyMap& map, int hip_device = 0);
SurfaceMesh ExtractSurfaceMesh(const OccupancyComponentMap& map, int hip_device = 0);
SurfaceMesh ExtractSurfaceMesh(const TaggedObjectOccupancyMap& map, int hip_device = 0);
SurfaceMesh ExtractSurfaceMesh(const TaggedObjectOccupancyComponentMap& map, int hip_device = 0);
}  // namespace vgt_hip
