// Launchers of the mesh rasterizer (mesh_kernels.hip) for the C ABI source.  Internal, like vgt_internal.hpp.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

namespace vgt
{
// Bits of the status word the kernels OR their findings into (never a trap or an abort); MeshStatus::first[b] holds the
// smallest triangle index that set bit b (0xffffffff: none).
constexpr uint32_t kMeshBadIndex = 1u;     // a vertex index outside [0, num_vertices)
constexpr uint32_t kMeshNonFinite = 2u;    // a vertex with a NaN or infinite coordinate
constexpr uint32_t kMeshDegenerate = 4u;   // a normal whose squared norm is not > 0
constexpr uint32_t kMeshNotContained = 8u; // enforce: an intersecting cell outside the grid
struct MeshStatus
{
  uint32_t bits;
  uint32_t first[4];
  uint32_t pad[3];
};
// What the set-up leaves for the host: bricks (work items) and candidate cells of the whole mesh, each saturating at
// kMeshCountCap.
struct MeshTotals
{
  unsigned long long bricks, cells;
};
constexpr unsigned long long kMeshCountCap = 1ull << 40;
// The most candidate cells one call evaluates (vgt_hip_rasterize_mesh*: refused beyond).
constexpr unsigned long long kMeshMaxCandidateCells = 1ull << 36;

struct MeshGrid
{
  int64_t nx, ny, nz;
  double resolution;
  double max_check_radius_squared;  // pow(resolution * 0.5 * sqrt(3.0), 2.0), evaluated by the host
  double world_from_grid[16];       // OriginTransform, column-major
  double grid_from_world[16];       // its inverse
  int has_transform;                // 0: locations are in the grid frame, no transform is applied
  int enforce;                      // 0: ranges are clamped to the grid; else evaluated literally, outside hits are errors
  int rule;                         // VGT_HIP_MESH_RULE_*
  int cell_bytes;                   // 4 or 8, the float occupancy at offset 0
};

size_t MeshScratchBytes(int64_t num_triangles);
// All asynchronous on `stream`; scratch_dev: MeshScratchBytes(num_triangles) bytes.
// Set-up + prefix sums: afterwards *MeshTotalsPtr / *MeshStatusPtr hold the totals and what validation found.
hipError_t LaunchMeshSetup(const double* vertices_dev, int64_t num_vertices, const int32_t* triangles_dev,
                           int64_t num_triangles, const MeshGrid& grid, void* scratch_dev, hipStream_t stream);
const MeshTotals* MeshTotalsPtr(const void* scratch_dev, int64_t num_triangles);
const MeshStatus* MeshStatusPtr(const void* scratch_dev, int64_t num_triangles);
// The bricks: stores 1.0f into every intersecting cell of cells_dev; total_bricks as read from MeshTotalsPtr.
hipError_t LaunchMeshBricks(const MeshGrid& grid, int64_t num_triangles, unsigned long long total_bricks,
                            void* scratch_dev, void* cells_dev, hipStream_t stream);
}  // namespace vgt
