// Internal declarations of the nearest-other-class transform (nearest_kernels.hip), shared with the C ABI source.
// The contract is stated once, in include/vgt_hip.h (vgt_hip_nearest_dev).
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

namespace vgt
{
// Records between the passes.
//  Z pass -> uint16 per cell: bit 15 = the cell is filled, bits 0-14 = z of the nearest cell of the other class on the
//            cell's own Z line (the lower z on a tie), kNearestNoneZ when the line holds none.
//  Y pass -> uint32 per cell: the low half as above, with z* now the z of the nearest cell of the other class in the
//            cell's YZ plane; bits 16-29 = its y.  kNearestNoneZ in the low half: the plane holds none.
//  X pass -> the linear index (int32) and, when asked, the squared distance.
constexpr uint32_t kNearestFilledBit = 0x8000u;
constexpr uint32_t kNearestNoneZ = 0x7fffu;
constexpr int32_t kNearestNoIndex = -1;
constexpr int32_t kNearestNoDistance = 0x7fffffff;

struct NearestGrid
{
  int32_t nx, ny, nz;  // 1 .. 16384 each, nx * ny * nz < 2^31
  int unknown_is_filled;
};

// The caller's workspace: the two record fields and the hull stacks of the line passes, laid out [slot][lane] for a
// bounded number of lanes in flight -- so the stacks grow with the axis lengths, not with the volume.
struct NearestWorkspace
{
  size_t z_records, y_records, stacks;  // byte offsets
  int64_t y_lanes, x_lanes;             // lanes in flight of the Y and the X pass (multiples of the block size);
                                        // a lane's stack has one slot per row of its line
  size_t bytes;
};
NearestWorkspace CarveNearestWorkspace(int64_t nx, int64_t ny, int64_t nz);

// The three passes on `stream`.  InT: float (occupancy) or uint8_t (mask, filled = non-zero).  d2_dev may be nullptr.
template <typename InT>
hipError_t LaunchNearest(const InT* input_dev, const NearestGrid& grid, int32_t* nearest_dev, int32_t* d2_dev,
                         void* workspace_dev, hipStream_t stream);

// object[c] = the cell's own object id where mask[c] != 0, else the id stored at nearest[c], 0 where nearest[c] is -1.
hipError_t LaunchNearestObjectId(const void* cells_dev, int64_t num_cells, int cell_bytes, int object_id_offset,
                                 const uint8_t* mask_dev, const int32_t* nearest_dev, uint32_t* object_dev,
                                 hipStream_t stream);
}  // namespace vgt
