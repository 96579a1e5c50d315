// Stable, ordered selection of cells: a per-cell predicate, then the selected cells in ascending linear index (X-major,
// Z fastest: the order of every loop of the reference that collects cells) with up to two 4-byte payloads each.  What the
// reference computes with a host loop over every voxel --
//   IsSurfaceIndex               S/occupancy_map.cpp:201-246, occupancy_component_map.cpp:234-280,
//                                tagged_object_occupancy_map.cpp:215-260 (the 26-neighbour rule, one text in every map type)
//   ExportVoxelGridToRViz        I/ros_interface.hpp:92-148 (keep the cells whose colour has alpha > 0)
//   ExtractComponentSurfaces     S/occupancy_component_map.cpp:511-571 (SurfaceMaskKernel's rule, component_kernels.hip)
// -- becomes count -> scan -> emit:
//   A. Mark    one lane per cell, a wave holds 64 consecutive cells of the linear order.  One ballot per wave is one
//              word of the bit grid (1 bit per voxel); a block of kBlockCells cells adds up its popcounts.
//              The 26-neighbour rule reduces every cell to three flags (>= 0.5, <= 0.5, != 0.5).  Their OR over the
//              3 x 3 x 3 box is separable, and the cell's own flags never fire its own rule, so a lane ORs the flags of the
//              at most 9 lines round it at its own z and takes the z - 1 and z + 1 contributions from the cells beside it
//              in the block's strip, through LDS.  Only the strip's first and last cell fetch theirs from memory, and
//              only inside a line: where the strip crosses a line end the neighbour along z does not exist.
//   B. Scan    the block counts -> offsets and the total, by the labelling's single-workgroup scan (LaunchScanBlocks).
//   C. Emit    reads the bit words only: a lane whose bit is set ranks itself by popcount(word & lanes below) and writes
//              its index and the payloads, which are read at the selected cells alone.
// No workgroup waits for another one: the three steps are three launches.
#include "vgt_internal.hpp"

namespace vgt
{
namespace
{
constexpr int kBlock = 256;
constexpr int kRowsPerBlock = 4;
constexpr int kBlockCells = kBlock * kRowsPerBlock;  // cells per block count of the scan
constexpr int kWordsPerBlock = kBlockCells / 64;
constexpr int kWordsPerWave = kWordsPerBlock / (kBlock / 64);

__device__ __forceinline__ float LoadValue(const SelectGrid& g, int64_t i)
{
  return *reinterpret_cast<const float*>(static_cast<const uint8_t*>(g.cells_dev) + i * g.cell_bytes);
}

__device__ __forceinline__ uint32_t LoadLabelOf(const SelectGrid& g, int64_t i)
{
  return *reinterpret_cast<const uint32_t*>(static_cast<const uint8_t*>(g.labels_dev) + i * g.label_stride);
}

__device__ __forceinline__ int ClassBit(float v, float t)
{
  return v > t ? kSelectClassAbove : (v < t ? kSelectClassBelow : (v == t ? kSelectClassEqual : kSelectClassUnordered));
}

// bit 0: some cell is >= 0.5, bit 1: <= 0.5, bit 2: != 0.5 (a NaN sets this one only), over the in-grid lines
// (x - 1 .. x + 1, y - 1 .. y + 1) at the z of cell i = (x, y, z)
__device__ __forceinline__ uint32_t LineFlags(const SelectGrid& g, int64_t i, int x, int y)
{
  const int64_t sy = g.nz, sx = static_cast<int64_t>(g.ny) * g.nz;
  uint32_t flags = 0u;
  for (int dx = -1; dx <= 1; dx++)
  {
    if (static_cast<unsigned>(x + dx) >= static_cast<unsigned>(g.nx)) continue;
    for (int dy = -1; dy <= 1; dy++)
    {
      if (static_cast<unsigned>(y + dy) >= static_cast<unsigned>(g.ny)) continue;
      const float v = LoadValue(g, i + dx * sx + dy * sy);
      flags |= (v >= 0.5f ? 1u : 0u) | (v <= 0.5f ? 2u : 0u) | (v != 0.5f ? 4u : 0u);
    }
  }
  return flags;
}

template <int kRule>
__global__ __launch_bounds__(kBlock) void SelectMarkKernel(SelectGrid g, int64_t total,
                                                           unsigned long long* __restrict__ words,
                                                           int32_t* __restrict__ block_counts)
{
  __shared__ int wave_count[kBlock / 64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int count = 0;
  for (int r = 0; r < kRowsPerBlock; r++)
  {
    // (whole waves run: the shuffles and the ballot need every lane; lanes past the end select nothing)
    const int64_t i = static_cast<int64_t>(blockIdx.x) * kBlockCells + r * kBlock + threadIdx.x;
    const int64_t wave_first = i - lane;
    if (wave_first >= total) break;  // the same for every lane of the wave
    const bool inside = i < total;
    float v = 0.0f;
    int x = 0, y = 0, z = 0;
    if (inside)
    {
      v = LoadValue(g, i);
      // (the grid has fewer than 2^31 cells: 32-bit divisions)
      const uint32_t line = static_cast<uint32_t>(i) / static_cast<uint32_t>(g.nz);
      z = static_cast<int>(static_cast<uint32_t>(i) - line * static_cast<uint32_t>(g.nz));
      x = static_cast<int>(line / static_cast<uint32_t>(g.ny));
      y = static_cast<int>(line - static_cast<uint32_t>(x) * static_cast<uint32_t>(g.ny));
    }
    const bool in_class = inside && (g.class_mask & ClassBit(v, g.threshold)) != 0;
    bool selected = false;
    if (kRule == kSelectAll)
      selected = in_class;
    else if (kRule == kSelectComponentSurface)
    {
      if (in_class)
      {
        selected = x == 0 || y == 0 || z == 0 || x == g.nx - 1 || y == g.ny - 1 || z == g.nz - 1;
        if (!selected)
        {
          const uint32_t own = LoadLabelOf(g, i);
          const int64_t sy = g.nz, sx = static_cast<int64_t>(g.ny) * g.nz;
          selected = LoadLabelOf(g, i - 1) != own || LoadLabelOf(g, i + 1) != own || LoadLabelOf(g, i - sy) != own ||
                     LoadLabelOf(g, i + sy) != own || LoadLabelOf(g, i - sx) != own || LoadLabelOf(g, i + sx) != own;
        }
      }
    }
    const unsigned long long word = __ballot(selected);
    if (lane == 0) words[wave_first >> 6] = word;
    count += __popcll(word);
  }
  if (lane == 0) wave_count[wave] = count;
  __syncthreads();
  if (threadIdx.x == 0)
  {
    int sum = 0;
    for (int w = 0; w < kBlock / 64; w++) sum += wave_count[w];
    block_counts[blockIdx.x] = sum;
  }
}

// The 26-neighbour rule.  Every cell of the block's strip of kBlockCells consecutive cells puts the flags of its (up to) 9
// lines into LDS; after the barrier a cell ORs its own entry with those of cells i - 1 and i + 1 where z has that step
// (they are the same lines one step along z then).  Only the strip's first and last cell fetch a neighbour's flags from
// memory: 9 loads per cell and two more sets per block.
__global__ __launch_bounds__(kBlock) void SelectMarkSurface26Kernel(SelectGrid g, int64_t total,
                                                                    unsigned long long* __restrict__ words,
                                                                    int32_t* __restrict__ block_counts)
{
  __shared__ uint32_t flags[kBlockCells + 2];  // [1 + local] of the strip's cells, [0] and [kBlockCells + 1] beside it
  __shared__ int wave_count[kBlock / 64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t block_first = static_cast<int64_t>(blockIdx.x) * kBlockCells;
  float v[kRowsPerBlock];
  uint32_t steps[kRowsPerBlock];  // bit 0: the cell has a neighbour at z - 1, bit 1: at z + 1
#pragma unroll
  for (int r = 0; r < kRowsPerBlock; r++)
  {
    const int local = r * kBlock + static_cast<int>(threadIdx.x);
    const int64_t i = block_first + local;
    uint32_t own = 0u;
    v[r] = 0.0f;
    steps[r] = 0u;
    if (i < total)
    {
      v[r] = LoadValue(g, i);
      // (the grid has fewer than 2^31 cells: 32-bit divisions)
      const uint32_t line = static_cast<uint32_t>(i) / static_cast<uint32_t>(g.nz);
      const int z = static_cast<int>(static_cast<uint32_t>(i) - line * static_cast<uint32_t>(g.nz));
      const int x = static_cast<int>(line / static_cast<uint32_t>(g.ny));
      const int y = static_cast<int>(line - static_cast<uint32_t>(x) * static_cast<uint32_t>(g.ny));
      own = LineFlags(g, i, x, y);
      steps[r] = (z > 0 ? 1u : 0u) | (z < g.nz - 1 ? 2u : 0u);  // (bit 1: i + 1 < total)
      if (local == 0 && (steps[r] & 1u)) flags[0] = LineFlags(g, i - 1, x, y);
      if (local == kBlockCells - 1 && (steps[r] & 2u)) flags[kBlockCells + 1] = LineFlags(g, i + 1, x, y);
    }
    flags[1 + local] = own;
  }
  __syncthreads();
  int count = 0;
#pragma unroll
  for (int r = 0; r < kRowsPerBlock; r++)
  {
    // (whole waves run: the ballot needs every lane; lanes past the end select nothing)
    const int local = r * kBlock + static_cast<int>(threadIdx.x);
    const int64_t i = block_first + local;
    const int64_t wave_first = i - lane;
    if (wave_first >= total) break;  // the same for every lane of the wave
    // (an entry beside the strip is read only by the cell that made its owner write it)
    const uint32_t box = flags[1 + local] | ((steps[r] & 1u) ? flags[local] : 0u) | ((steps[r] & 2u) ? flags[2 + local] : 0u);
    // IsSurfaceIndex: our < 0.5 and some other >= 0.5; our > 0.5 and some other <= 0.5; our == 0.5 and some other != 0.5
    const float our = v[r];
    const uint32_t wanted = our < 0.5f ? 1u : (our > 0.5f ? 2u : (our == 0.5f ? 4u : 0u));
    const bool selected = i < total && (g.class_mask & ClassBit(our, g.threshold)) != 0 && (box & wanted) != 0u;
    const unsigned long long word = __ballot(selected);
    if (lane == 0) words[wave_first >> 6] = word;
    count += __popcll(word);
  }
  if (lane == 0) wave_count[wave] = count;
  __syncthreads();
  if (threadIdx.x == 0)
  {
    int sum = 0;
    for (int w = 0; w < kBlock / 64; w++) sum += wave_count[w];
    block_counts[blockIdx.x] = sum;
  }
}

__global__ __launch_bounds__(kBlock) void SelectEmitKernel(SelectGrid g, int64_t total,
                                                           const unsigned long long* __restrict__ words,
                                                           const int32_t* __restrict__ block_offsets, SelectOutput out)
{
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t num_words = (total + 63) / 64;
  const int64_t first_word = static_cast<int64_t>(blockIdx.x) * kWordsPerBlock;
  int64_t rank = block_offsets[blockIdx.x];
  for (int w = 0; w < wave * kWordsPerWave; w++)
    if (first_word + w < num_words) rank += __popcll(words[first_word + w]);
  for (int k = 0; k < kWordsPerWave; k++)
  {
    const int64_t word_index = first_word + wave * kWordsPerWave + k;
    if (word_index >= num_words) break;
    const unsigned long long word = words[word_index];
    if ((word >> lane) & 1ull)
    {
      const int64_t at = rank + __popcll(word & ((1ull << lane) - 1ull));
      const int64_t i = word_index * 64 + lane;
      // (at < capacity always: the host compares the scan's total with the capacity before this launch)
      if (at < out.capacity)
      {
        out.indices_dev[at] = static_cast<int32_t>(i);
        if (out.values_dev) out.values_dev[at] = LoadValue(g, i);
        if (out.payload_dev)
          out.payload_dev[at] =
              *reinterpret_cast<const uint32_t*>(static_cast<const uint8_t*>(out.payload_source_dev) + i * out.payload_stride);
      }
    }
    rank += __popcll(word);
  }
}

unsigned Blocks(int64_t items, int per_block) { return static_cast<unsigned>((items + per_block - 1) / per_block); }

struct ScratchLayout
{
  size_t words, block_counts, count, bytes;
};
ScratchLayout CarveScratch(int64_t num_cells)
{
  const auto align = [](size_t v) { return (v + 255) / 256 * 256; };
  ScratchLayout s;
  s.words = 0;
  s.block_counts = align(static_cast<size_t>((num_cells + 63) / 64) * sizeof(unsigned long long));
  s.count = s.block_counts + align(static_cast<size_t>(Blocks(num_cells, kBlockCells)) * sizeof(int32_t));
  s.bytes = s.count + 256;
  return s;
}
}  // namespace

size_t SelectScratchBytes(int64_t num_cells) { return num_cells > 0 ? CarveScratch(num_cells).bytes : 0; }

const uint32_t* SelectCountPtr(const void* scratch_dev, int64_t num_cells)
{
  return reinterpret_cast<const uint32_t*>(static_cast<const char*>(scratch_dev) + CarveScratch(num_cells).count);
}

hipError_t LaunchSelectMark(const SelectGrid& g, void* scratch_dev, hipStream_t stream)
{
  const int64_t total = static_cast<int64_t>(g.nx) * g.ny * g.nz;
  const ScratchLayout s = CarveScratch(total);
  char* const base = static_cast<char*>(scratch_dev);
  unsigned long long* const words = reinterpret_cast<unsigned long long*>(base + s.words);
  int32_t* const block_counts = reinterpret_cast<int32_t*>(base + s.block_counts);
  const unsigned blocks = Blocks(total, kBlockCells);
  switch (g.rule)
  {
    case kSelectAll:
      SelectMarkKernel<kSelectAll><<<blocks, kBlock, 0, stream>>>(g, total, words, block_counts);
      break;
    case kSelectSurface26:
      SelectMarkSurface26Kernel<<<blocks, kBlock, 0, stream>>>(g, total, words, block_counts);
      break;
    case kSelectComponentSurface:
      SelectMarkKernel<kSelectComponentSurface><<<blocks, kBlock, 0, stream>>>(g, total, words, block_counts);
      break;
    default:
      return hipErrorInvalidValue;
  }
  const hipError_t err = hipGetLastError();
  if (err != hipSuccess) return err;
  return LaunchScanBlocks(block_counts, static_cast<int64_t>(blocks), reinterpret_cast<uint32_t*>(base + s.count), stream);
}

hipError_t LaunchSelectEmit(const SelectGrid& g, const SelectOutput& out, const void* scratch_dev, hipStream_t stream)
{
  const int64_t total = static_cast<int64_t>(g.nx) * g.ny * g.nz;
  const ScratchLayout s = CarveScratch(total);
  const char* const base = static_cast<const char*>(scratch_dev);
  SelectEmitKernel<<<Blocks(total, kBlockCells), kBlock, 0, stream>>>(
      g, total, reinterpret_cast<const unsigned long long*>(base + s.words),
      reinterpret_cast<const int32_t*>(base + s.block_counts), out);
  return hipGetLastError();
}
}  // namespace vgt
