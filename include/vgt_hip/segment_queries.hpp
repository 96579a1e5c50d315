// Segment queries of the C++ host layer: a batch of segments cast through an occupancy map or a signed distance field
// on the device (vgt_hip_cast_segments of vgt_hip.h, which states the cells a segment examines, in which order, and
// every output).  The question a sampling planner asks for each edge, a sensor model for each line of sight.
#pragma once

#include <cstdint>
#include <vector>

#include "host_types.hpp"

namespace vgt_hip
{
// One entry per segment; min_value / min_index are filled by the SDF overload only (empty otherwise).
struct SegmentCasts
{
  std::vector<uint8_t> status;  // VGT_HIP_SEGMENT_CLEAR / _HIT / _MISSED_GRID / _INVALID
  std::vector<int32_t> hit_index, cells_examined;
  std::vector<double> hit_fraction;
  std::vector<float> min_value;
  std::vector<int32_t> min_index;
};
// `segments_xyz`: 6 doubles per segment (a, b), in the frame the map's origin transform maps to; the map's inverse
// origin transform is the call's grid_from_world.  Both use the process's shared context of `hip_device`.  Throw
// std::invalid_argument where the C ABI reports an invalid argument (and for a map without cells or a vector that does
// not hold 6 doubles per segment), std::runtime_error for its other errors.
// A cell is a hit when its occupancy is > 0.5, or == 0.5 with unknown_is_filled; a cast stops at its first hit.
SegmentCasts CastSegments(const OccupancyMap& map, const std::vector<double>& segments_xyz, bool unknown_is_filled = true,
                          int hip_device = 0);
// A cell is a hit when its distance is <= minimum_distance; min_value / min_index give the least distance among the
// examined cells -- with walk_through, which examines every cell of the segment, the segment's clearance at cell centres.
SegmentCasts CastSegments(const SignedDistanceField& sdf, const std::vector<double>& segments_xyz, double minimum_distance,
                          bool walk_through = false, int hip_device = 0);
}  // namespace vgt_hip
