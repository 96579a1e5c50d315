// Exact signed Euclidean distance transform for gfx950 (MI355X): what the pipeline needs besides its three passes.
//
// What is computed (reference: OccupancyMap::ExtractSignedDistanceField<float>,
// include/voxelized_geometry_tools/occupancy_map.hpp:174-210 ->
// signed_distance_field_generation.hpp:39-113 -> signed_distance_field_generation.cpp:258-391):
// for every voxel the exact squared Euclidean distance (integer, voxel units) to the nearest
// voxel of the OTHER class (filled vs free), turned into
//     sdf = float( sqrt(double(d2)) * resolution ), negated on filled voxels,
// +-inf when the other class is absent.  The reference runs two separate double-precision
// Felzenszwalb-Huttenlocher transforms (one per class) in X,Y,Z order; the result is
// order-independent and integral, so here both classes travel through three passes as ONE
// signed integer field (a voxel only ever needs the distance to the other class, and a voxel of
// the other class is a zero-valued site):
//     pass 1  Z (contiguous axis): the binarised input as class records (edt_record_kernels.hip)
//     pass 2  Y: lower envelope of parabolas over the squared distances along Z that the records give
//     pass 3  X: same, fused with sqrt / resolution / sign / virtual border / min-max
// (passes 2 and 3: lane-per-line sweeps, edt_sweep_kernels.hip; lines of few rows: edt_short_kernels.hip).
//
// This file holds the rest: the slab carries of the multi-GPU path, the extrema's initialisation and decoding, and the
// X pass's choice between the short-line kernels and the sweeps.
#include "edt_device.hpp"

namespace vgt
{
namespace
{
// Multi-GPU: per-line carries of slab `rank` from the gathered summaries of all slabs
// (summaries[slab][line], 4 bytes each, see vgt_internal.hpp): nearest filled / free voxel below = the last such
// voxel of the nearest lower slab that has one, above = the first such voxel of the nearest upper slab (-1 when
// absent).  A slab's first (last) voxel of one class is its first (last) voxel; where that is follows from SlabRange.
__global__ __launch_bounds__(256) void SlabCarriesKernel(const SlabLineSummary* __restrict__ summaries,
                                                        int world, int rank, int64_t lines, int nz_global,
                                                        SlabLineCarry* __restrict__ carries)
{
  const int share = nz_global / world, extra = nz_global % world;
  for (int64_t line = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x; line < lines;
       line += static_cast<int64_t>(gridDim.x) * blockDim.x)
  {
    int prev_filled = -1, prev_free = -1, next_filled = -1, next_free = -1;
    for (int r = 0; r < rank; r++)
    {
      const uint16_t rec = summaries[static_cast<int64_t>(r) * lines + line].last;
      const int end = (r + 1) * share + min(r + 1, extra) - 1;  // the slab's last voxel
      const int other = (rec & kSlabNone) == kSlabNone ? -1 : static_cast<int>(rec & kSlabNone);
      const bool filled = (rec & kSlabFilledBit) != 0;
      prev_filled = max(prev_filled, filled ? end : other);
      prev_free = max(prev_free, filled ? other : end);
    }
    for (int r = world - 1; r > rank; r--)
    {
      const uint16_t rec = summaries[static_cast<int64_t>(r) * lines + line].first;
      const int begin = r * share + min(r, extra);  // the slab's first voxel
      const int other = (rec & kSlabNone) == kSlabNone ? -1 : static_cast<int>(rec & kSlabNone);
      const bool filled = (rec & kSlabFilledBit) != 0;
      const int first_filled = filled ? begin : other, first_free = filled ? other : begin;
      if (first_filled >= 0) next_filled = first_filled;
      if (first_free >= 0) next_free = first_free;
    }
    SlabLineCarry c;
    c.prev_filled = static_cast<int16_t>(prev_filled);
    c.next_filled = static_cast<int16_t>(next_filled);
    c.prev_free = static_cast<int16_t>(prev_free);
    c.next_free = static_cast<int16_t>(next_free);
    carries[line] = c;
  }
}

__global__ void InitMinMaxKernel(uint32_t* minmax_enc, int count)
{
  for (int i = static_cast<int>(threadIdx.x); i < count; i += static_cast<int>(blockDim.x))
  {
    minmax_enc[2 * i] = 0xffffffffu;
    minmax_enc[2 * i + 1] = 0u;
  }
  // (one grid: pass 1's counts of one-class lines and of lines seen, which the X pass chooses its kernel by, start at zero
  // in the same dispatch)
  if (count == 1 && threadIdx.x == 0) minmax_enc[kOneClassWord] = minmax_enc[kOneClassWord + 1] = 0u;
}
__global__ void DecodeMinMaxKernel(const uint32_t* minmax_enc, float* out, int count)
{
  for (int i = static_cast<int>(threadIdx.x); i < 2 * count; i += static_cast<int>(blockDim.x))
    out[i] = DecodeOrdered(minmax_enc[i]);
}

int GridFor(int64_t work_items, int block)
{
  // Memory-bound grid-stride launches: enough blocks to fill 256 CUs several times over.
  const int64_t blocks = (work_items + block - 1) / block;
  const int64_t cap = 256 * 32;
  return static_cast<int>(blocks < 1 ? 1 : (blocks > cap ? cap : blocks));
}
}  // namespace

hipError_t LaunchSlabCarries(const SlabLineSummary* summaries, int world, int rank, int64_t lines, int64_t nz_global,
                             SlabLineCarry* carries, hipStream_t stream)
{
  hipLaunchKernelGGL(SlabCarriesKernel, dim3(GridFor(lines, 256)), dim3(256), 0, stream, summaries, world, rank,
                     lines, static_cast<int>(nz_global), carries);
  return hipGetLastError();
}

hipError_t LaunchPassXFinalize(const int32_t* in32, float* sdf, uint32_t* minmax_enc, SweepScratch scratch,
                               const SdfParams& p, hipStream_t stream)
{
  return LaunchPassXFinalizeRange(in32, sdf, minmax_enc, scratch, p, 0, -1, stream);
}

hipError_t LaunchPassXFinalizeRange(const int32_t* in32, float* sdf, uint32_t* minmax_enc, SweepScratch scratch,
                                    const SdfParams& p, int64_t outer_begin, int64_t outer_count, hipStream_t stream)
{
  // (The X pass keeps the sweeps beyond 64 rows even when a launch has few items: measured equal at 80 - 128 rows,
  // profiles/r5/short_vs_sweep.txt -- its rows pay for the final conversion either way.  The Y pass gains a third there.)
  if (p.nx <= ShortLineRows())
    return LaunchPassXShortFinalizeRange(in32, sdf, minmax_enc, p, outer_begin, outer_count, stream);
  return LaunchPassXSweepFinalizeRange(in32, sdf, minmax_enc, scratch, p, outer_begin, outer_count, stream);
}

hipError_t LaunchInitMinMax(uint32_t* minmax_enc, hipStream_t stream, int64_t count)
{
  hipLaunchKernelGGL(InitMinMaxKernel, dim3(1), dim3(count > 1 ? 64 : 1), 0, stream, minmax_enc, static_cast<int>(count));
  return hipGetLastError();
}

hipError_t LaunchDecodeMinMax(const uint32_t* minmax_enc, float* minmax_out, hipStream_t stream, int64_t count)
{
  hipLaunchKernelGGL(DecodeMinMaxKernel, dim3(1), dim3(count > 1 ? 64 : 1), 0, stream, minmax_enc, minmax_out,
                     static_cast<int>(count));
  return hipGetLastError();
}
}  // namespace vgt
