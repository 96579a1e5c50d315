// Cost-to-go fields of the C++ host layer: how far every cell of a map is from a set of sources THROUGH passable cells,
// which neighbour to step to, and batched path tracing (vgt_hip_travel_cost / vgt_hip_trace_paths of vgt_hip.h, which
// states the passable cells, the moves and their weights, the corner rule, the limit and every output).  The navigation
// function of a grid planner, the admissible heuristic of a sampling one, "reachable within this budget".
#pragma once

#include <array>
#include <cstdint>
#include <vector>

#include "host_types.hpp"

namespace vgt_hip
{
struct GridIndex
{
  int64_t x = 0, y = 0, z = 0;
};

struct TravelCostOptions
{
  // the cost of a move with 1, 2, 3 non-zero components; 0 disables the class ({1,0,0}: 6-connected step counts)
  std::array<uint32_t, 3> weights{{10u, 14u, 17u}};
  bool no_corner_cutting = false;       // VGT_HIP_TRAVEL_NO_CORNER_CUTTING
  bool unknown_is_filled = true;        // maps only: occupancy == 0.5 blocks
  uint32_t cost_limit = 0xfffffffeu;    // that value: no limit
  std::vector<uint32_t> source_costs;   // empty: every source starts at 0; else one per source
  std::vector<uint32_t> objects_to_use; // tagged maps only: the objects that block (empty: every filled cell)
  bool with_toward = true;
  int hip_device = 0;
};

// cost[c] / toward[c] for the linear index c = (x * ny + y) * nz + z; toward is empty without with_toward.
struct TravelCostField
{
  int64_t nx = 0, ny = 0, nz = 0;
  std::vector<uint32_t> cost;   // VGT_HIP_TRAVEL_UNREACHED where there is no path within the limit
  std::vector<int32_t> toward;  // -1 unreached, c itself at a root
  int64_t num_reached = 0;
  int64_t LinearIndex(const GridIndex& i) const
  {
    const bool inside = i.x >= 0 && i.x < nx && i.y >= 0 && i.y < ny && i.z >= 0 && i.z < nz;
    return inside ? (i.x * ny + i.y) * nz + i.z : -1;
  }
  GridIndex Index(int64_t c) const { return GridIndex{c / (ny * nz), c / nz % ny, c % nz}; }
};

// Path i: cells[i * max_cells + k], k < lengths[i], start first and root last (linear indices; TravelCostField::Index
// turns them back); the slots behind a path's length hold -1.
struct TracedPaths
{
  int32_t max_cells = 0;
  std::vector<int32_t> cells, lengths;
  std::vector<uint8_t> status;  // VGT_HIP_TRACE_OK / _UNREACHED / _TRUNCATED / _INVALID
};

// A source outside the grid, on a blocked cell or above the limit contributes nothing.  All use the process's shared
// context of options.hip_device.  Throw std::invalid_argument where the C ABI reports an invalid argument (and for a map
// without cells, or source_costs that do not match the sources), std::runtime_error for its other errors.
// Blocked: occupancy > 0.5, or == 0.5 with unknown_is_filled (tagged maps: AND the object is listed, if any is).
TravelCostField ComputeTravelCost(const OccupancyMap& map, const std::vector<GridIndex>& sources,
                                  const TravelCostOptions& options = TravelCostOptions());
TravelCostField ComputeTravelCost(const OccupancyComponentMap& map, const std::vector<GridIndex>& sources,
                                  const TravelCostOptions& options = TravelCostOptions());
TravelCostField ComputeTravelCost(const TaggedObjectOccupancyMap& map, const std::vector<GridIndex>& sources,
                                  const TravelCostOptions& options = TravelCostOptions());
TravelCostField ComputeTravelCost(const TaggedObjectOccupancyComponentMap& map, const std::vector<GridIndex>& sources,
                                  const TravelCostOptions& options = TravelCostOptions());
// Blocked: distance <= minimum_distance (the map inflated by the robot's radius).
TravelCostField ComputeTravelCost(const SignedDistanceField& sdf, double minimum_distance,
                                  const std::vector<GridIndex>& sources,
                                  const TravelCostOptions& options = TravelCostOptions());
// Follows field.toward from every start (a start outside the grid is VGT_HIP_TRACE_INVALID).
TracedPaths TracePaths(const TravelCostField& field, const std::vector<GridIndex>& starts, int32_t max_cells,
                       int hip_device = 0);
}  // namespace vgt_hip
