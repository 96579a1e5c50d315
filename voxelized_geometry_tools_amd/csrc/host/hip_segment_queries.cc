// CastSegments of include/vgt_hip/segment_queries.hpp on the C ABI (vgt_hip_cast_segments).
#include "../../../include/vgt_hip/segment_queries.hpp"
#include "host_internal.hpp"

#include <cmath>

namespace vgt_hip
{
namespace
{
SegmentCasts Cast(const DenseGrid& grid, const std::vector<double>& segments_xyz, int32_t mode, bool unknown_is_filled,
                  double threshold, uint32_t flags, int hip_device)
{
  if (!grid.IsInitialized()) throw std::invalid_argument("Grid must be initialized");
  if (segments_xyz.size() % 6 != 0) throw std::invalid_argument("segments_xyz must hold 6 doubles per segment");
  // (what the C ABI would refuse, refused before a device is asked for)
  if (std::isnan(threshold)) throw std::invalid_argument("minimum_distance must not be NaN");
  const int64_t n = static_cast<int64_t>(segments_xyz.size() / 6);
  const bool with_min = mode == VGT_HIP_SEGMENT_SDF_BELOW;
  SegmentCasts out;
  out.status.resize(static_cast<size_t>(n));
  out.hit_index.resize(static_cast<size_t>(n));
  out.cells_examined.resize(static_cast<size_t>(n));
  out.hit_fraction.resize(static_cast<size_t>(n));
  if (with_min)
  {
    out.min_value.resize(static_cast<size_t>(n));
    out.min_index.resize(static_cast<size_t>(n));
  }
  if (n == 0) return out;  // (nothing to do: no device is needed)
  const int rc = vgt_hip_cast_segments(
      detail::SharedSdfContext(hip_device), grid.GetImmutableRawData().data(), grid.NumXVoxels(), grid.NumYVoxels(),
      grid.NumZVoxels(), grid.Resolution(), mode, unknown_is_filled ? 1 : 0, threshold, flags,
      grid.InverseOriginTransform().m.data(), segments_xyz.data(), n, out.status.data(),
      out.hit_index.data(), out.hit_fraction.data(), out.cells_examined.data(), with_min ? out.min_value.data() : nullptr,
      with_min ? out.min_index.data() : nullptr);
  if (rc != VGT_HIP_OK) detail::ThrowForCode(rc, vgt_hip_last_error());
  return out;
}
}  // namespace

SegmentCasts CastSegments(const OccupancyMap& map, const std::vector<double>& segments_xyz, bool unknown_is_filled,
                          int hip_device)
{
  return Cast(map, segments_xyz, VGT_HIP_SEGMENT_OCCUPANCY, unknown_is_filled, 0.0, 0u, hip_device);
}

SegmentCasts CastSegments(const SignedDistanceField& sdf, const std::vector<double>& segments_xyz, double minimum_distance,
                          bool walk_through, int hip_device)
{
  return Cast(sdf.grid, segments_xyz, VGT_HIP_SEGMENT_SDF_BELOW, true, minimum_distance,
              walk_through ? VGT_HIP_SEGMENT_WALK_THROUGH : 0u, hip_device);
}
}  // namespace vgt_hip
