// Nearest cell of the other class per voxel, of the C++ host layer: for every cell of a map the linear index of a cell
// of the OTHER class (filled / not filled) at minimal Euclidean distance, and the exact squared distance in cells
// (vgt_hip_nearest_dev of vgt_hip.h states the one contract: the filled predicate, ties, -1 where the map holds no cell
// of the other class, no virtual border, the limits).  The vector to the obstacle surface, a contact cell for a
// penetrating point, the partition of free space by nearest object -- without a gradient stencil and in one extraction.
#pragma once

#include <cstdint>
#include <vector>

#include "host_types.hpp"

namespace vgt_hip
{
// One entry per cell, in the map's raw order x * ny * nz + y * nz + z.
struct NearestCells
{
  std::vector<int32_t> index;             // -1: the map holds no cell of the other class
  std::vector<int32_t> squared_distance;  // in cells; 0x7fffffff goes with -1
  std::vector<uint32_t> object_id;        // tagged maps only (empty otherwise): the cell's own object id where it is
                                          // filled, else the id stored at `index`, 0 where index is -1
};
// All three use the process's shared context of `hip_device`.  Throw std::invalid_argument where the C ABI reports an
// invalid argument (and for a map without cells), std::runtime_error for its other errors.
// A cell is filled when its occupancy is > 0.5, or == 0.5 with unknown_is_filled.
NearestCells ExtractNearestCells(const OccupancyMap& map, bool unknown_is_filled = true, int hip_device = 0);
// ... AND (objects_to_use is empty or lists the cell's object id): the predicate of the maps' ExtractSignedDistanceField.
NearestCells ExtractNearestCells(const TaggedObjectOccupancyMap& map, const std::vector<uint32_t>& objects_to_use,
                                 bool unknown_is_filled = true, int hip_device = 0);
NearestCells ExtractNearestCells(const TaggedObjectOccupancyComponentMap& map, const std::vector<uint32_t>& objects_to_use,
                                 bool unknown_is_filled = true, int hip_device = 0);
}  // namespace vgt_hip
