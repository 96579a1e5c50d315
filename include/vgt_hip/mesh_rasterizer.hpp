// mesh_rasterizer (I/mesh_rasterizer.hpp, S/mesh_rasterizer.cpp) on the HIP backend, over the stand-alone types of
// host_types.hpp: the reference's six signatures in namespace vgt_hip::mesh_rasterizer, the DegreeOfParallelism argument
// replaced by the device to run on.  Implemented in csrc/host/hip_mesh_rasterizer.cc on vgt_hip_rasterize_mesh.
//
// Exceptions as in the reference: std::invalid_argument for a map that is not initialised and a resolution that is not
// greater than zero; std::runtime_error("Triangle is not contained by occupancy map ...") when an intersecting cell lies
// outside the map and containment is enforced.  Divergence: a vertex index out of range, a non-finite vertex and a
// triangle whose normal has zero length are std::invalid_argument (vgt_hip.h).
#pragma once

#include <array>
#include <cstddef>
#include <cstdint>
#include <vector>

#include "host_types.hpp"

namespace vgt_hip
{
namespace mesh_rasterizer
{
using Vector3d = std::array<double, 3>;
using Vector3i = std::array<int32_t, 3>;
// The closest-point rule (vgt_hip.h, VGT_HIP_MESH_RULE_*): the reference's literal one, or the watertight extension.
enum class ClosestPointRule : int { REFERENCE = 0, NEAREST = 1 };

void RasterizeTriangle(const std::vector<Vector3d>& vertices, const std::vector<Vector3i>& triangles,
                       size_t triangle_index, OccupancyMap& occupancy_map,
                       bool enforce_occupancy_map_contains_triangle = true, int hip_device = 0,
                       ClosestPointRule rule = ClosestPointRule::REFERENCE);
void RasterizeTriangle(const std::vector<Vector3d>& vertices, const std::vector<Vector3i>& triangles,
                       size_t triangle_index, OccupancyComponentMap& occupancy_map,
                       bool enforce_occupancy_map_contains_triangle = true, int hip_device = 0,
                       ClosestPointRule rule = ClosestPointRule::REFERENCE);

void RasterizeMesh(const std::vector<Vector3d>& vertices, const std::vector<Vector3i>& triangles,
                   OccupancyMap& occupancy_map, bool enforce_occupancy_map_contains_mesh = true, int hip_device = 0,
                   ClosestPointRule rule = ClosestPointRule::REFERENCE);
void RasterizeMesh(const std::vector<Vector3d>& vertices, const std::vector<Vector3i>& triangles,
                   OccupancyComponentMap& occupancy_map, bool enforce_occupancy_map_contains_mesh = true,
                   int hip_device = 0, ClosestPointRule rule = ClosestPointRule::REFERENCE);

OccupancyMap RasterizeMeshIntoOccupancyMap(const std::vector<Vector3d>& vertices, const std::vector<Vector3i>& triangles,
                                           double resolution, int hip_device = 0,
                                           ClosestPointRule rule = ClosestPointRule::REFERENCE);
OccupancyComponentMap RasterizeMeshIntoOccupancyComponentMap(const std::vector<Vector3d>& vertices,
                                                             const std::vector<Vector3i>& triangles, double resolution,
                                                             int hip_device = 0,
                                                             ClosestPointRule rule = ClosestPointRule::REFERENCE);

// Mesh -> SDF: RasterizeMeshIntoOccupancyMap, then OccupancyMap::ExtractSignedDistanceField<float> on parameters.hip_device.
SignedDistanceField MeshToSignedDistanceField(const std::vector<Vector3d>& vertices,
                                              const std::vector<Vector3i>& triangles, double resolution,
                                              const SignedDistanceFieldGenerationParameters& parameters,
                                              ClosestPointRule rule = ClosestPointRule::REFERENCE);

// Solid bodies (an extension): the three functions above followed by FillEnclosedSpace (hip_pointcloud_voxelizer.hpp,
// unknown_is_filled = true), so that what a closed mesh encloses is filled and its field is negative inside the body.
// `rule` defaults to NEAREST here: only that rule guarantees a sealed shell for a closed mesh (every cell the surface
// passes through is marked, and a face-connected path from inside to outside crosses the surface inside one of them).
// REFERENCE can miss cells along slanted edges; the interior is then filled only where the shell happens to be sealed
// (the test torus encloses 7070 cells under NEAREST and 1 under REFERENCE).  A mesh that is not closed encloses nothing.
OccupancyMap RasterizeSolidMeshIntoOccupancyMap(const std::vector<Vector3d>& vertices,
                                                const std::vector<Vector3i>& triangles, double resolution,
                                                int hip_device = 0, ClosestPointRule rule = ClosestPointRule::NEAREST);
OccupancyComponentMap RasterizeSolidMeshIntoOccupancyComponentMap(const std::vector<Vector3d>& vertices,
                                                                  const std::vector<Vector3i>& triangles,
                                                                  double resolution, int hip_device = 0,
                                                                  ClosestPointRule rule = ClosestPointRule::NEAREST);
SignedDistanceField SolidMeshToSignedDistanceField(const std::vector<Vector3d>& vertices,
                                                   const std::vector<Vector3i>& triangles, double resolution,
                                                   const SignedDistanceFieldGenerationParameters& parameters,
                                                   ClosestPointRule rule = ClosestPointRule::NEAREST);
}  // namespace mesh_rasterizer
}  // namespace vgt_hip
