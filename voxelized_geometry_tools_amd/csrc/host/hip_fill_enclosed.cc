// FillEnclosedSpace of include/vgt_hip/hip_pointcloud_voxelizer.hpp on the C ABI (vgt_hip_fill_enclosed).
#include "../../../include/vgt_hip/hip_pointcloud_voxelizer.hpp"
#include "host_internal.hpp"

namespace vgt_hip
{
namespace
{
template <typename Map>
int64_t Fill(Map& map, bool unknown_is_filled, int hip_device)
{
  if (!map.IsInitialized()) throw std::invalid_argument("Grid must be initialized");
  auto& cells = map.GetMutableRawData();
  static_assert(sizeof(cells[0]) == 4 || sizeof(cells[0]) == 8, "OccupancyCell or OccupancyComponentCell");
  // (the process's context of that device: it keeps the labelling scratch between calls)
  vgt_hip_ctx* const ctx = detail::SharedSdfContext(hip_device);
  int64_t count = 0;
  const int rc = vgt_hip_fill_enclosed(ctx, cells.data(), static_cast<int>(sizeof(cells[0])), map.NumXVoxels(),
                                       map.NumYVoxels(), map.NumZVoxels(), unknown_is_filled ? 1 : 0, &count);
  if (rc != VGT_HIP_OK) detail::ThrowForCode(rc, vgt_hip_last_error());
  return count;
}
}  // namespace

int64_t FillEnclosedSpace(OccupancyMap& map, bool unknown_is_filled, int hip_device)
{
  return Fill(map, unknown_is_filled, hip_device);
}

int64_t FillEnclosedSpace(OccupancyComponentMap& map, bool unknown_is_filled, int hip_device)
{
  return Fill(map, unknown_is_filled, hip_device);
}
}  // namespace vgt_hip
