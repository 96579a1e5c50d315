// ExtractNearestCells of include/vgt_hip/nearest_cells.hpp on the C ABI (vgt_hip_nearest_from_occupancy_f32,
// vgt_hip_cells_nearest).
#include "../../../include/vgt_hip/nearest_cells.hpp"
#include "host_internal.hpp"

namespace vgt_hip
{
namespace
{
template <typename Cell>
NearestCells ExtractTagged(const CellGrid<Cell>& map, const std::vector<uint32_t>& objects_to_use, bool unknown_is_filled,
                           int hip_device)
{
  if (!map.IsInitialized()) throw std::invalid_argument("Grid must be initialized");
  vgt_hip_ctx* const ctx = detail::SharedSdfContext(hip_device);
  vgt_hip_cells* cells = nullptr;
  int rc = vgt_hip_cells_create(ctx, map.GetImmutableRawData().data(), map.NumXVoxels(), map.NumYVoxels(),
                                map.NumZVoxels(), static_cast<int32_t>(sizeof(Cell)), 4, &cells);
  if (rc != VGT_HIP_OK) detail::ThrowForCode(rc, vgt_hip_last_error());
  const size_t n = map.GetImmutableRawData().size();
  NearestCells out;
  out.index.resize(n);
  out.squared_distance.resize(n);
  out.object_id.resize(n);
  rc = vgt_hip_cells_nearest(ctx, cells, objects_to_use.empty() ? nullptr : objects_to_use.data(),
                             static_cast<int64_t>(objects_to_use.size()), unknown_is_filled ? 1 : 0, out.index.data(),
                             out.squared_distance.data(), out.object_id.data());
  const std::string msg = (rc == VGT_HIP_OK) ? std::string() : std::string(vgt_hip_last_error());
  vgt_hip_cells_destroy(cells);
  if (rc != VGT_HIP_OK) detail::ThrowForCode(rc, msg);
  return out;
}
}  // namespace

NearestCells ExtractNearestCells(const OccupancyMap& map, bool unknown_is_filled, int hip_device)
{
  if (!map.IsInitialized()) throw std::invalid_argument("Grid must be initialized");
  const size_t n = map.GetImmutableRawData().size();
  NearestCells out;
  out.index.resize(n);
  out.squared_distance.resize(n);
  const int rc = vgt_hip_nearest_from_occupancy_f32(
      detail::SharedSdfContext(hip_device), map.GetImmutableRawData().data(), map.NumXVoxels(), map.NumYVoxels(),
      map.NumZVoxels(), unknown_is_filled ? 1 : 0, out.index.data(), out.squared_distance.data());
  if (rc != VGT_HIP_OK) detail::ThrowForCode(rc, vgt_hip_last_error());
  return out;
}

NearestCells ExtractNearestCells(const TaggedObjectOccupancyMap& map, const std::vector<uint32_t>& objects_to_use,
                                 bool unknown_is_filled, int hip_device)
{
  return ExtractTagged(map, objects_to_use, unknown_is_filled, hip_device);
}

NearestCells ExtractNearestCells(const TaggedObjectOccupancyComponentMap& map, const std::vector<uint32_t>& objects_to_use,
                                 bool unknown_is_filled, int hip_device)
{
  return ExtractTagged(map, objects_to_use, unknown_is_filled, hip_device);
}
}  // namespace vgt_hip
