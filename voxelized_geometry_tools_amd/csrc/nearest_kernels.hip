// Nearest cell of the other class per voxel (the feature transform of the signed EDT): contract in include/vgt_hip.h
// (vgt_hip_nearest_dev), records between the passes in nearest_internal.hpp, the per-line routine in nearest_line.hpp.
//
// Separable in the EDT's order Z, Y, X; every pass carries the site and no distance field is stored:
//   Z pass  one wave per Z line.  A wave's load covers 64 consecutive z, a ballot turns them into one class word; the
//           nearest cell of the other class inside a word comes from bit scans, across words from carries along the line
//           (from below while the wave walks up, from above out of a table the wave built before).  2 B per voxel out.
//   Y pass  one lane per line (x, z), 64 neighbouring z per wave, so every row access is one contiguous segment.
//           Two lower envelopes per line, one per query class (nearest_line.hpp).  4 B per voxel out: (y*, z*) + class.
//   X pass  the same along x over lines (y, z), heights (y - y*)^2 + (z - z*)^2 recomputed from the Y records; writes
//           the linear index and, when asked, the squared distance.
// The hull stacks live in the caller's workspace, laid out [slot][lane] for a bounded number of persistent lanes.
// Nothing here is atomic and no result depends on the launch order: the output is a pure function of the input.
// Untuned: the line passes run each envelope as two sweeps over the line's records and keep only the hull's top entry
// in registers.
#include "nearest_internal.hpp"
#include "nearest_line.hpp"

namespace vgt
{
namespace
{
constexpr int kBlock = 256;
constexpr int kWavesPerBlock = kBlock / 64;
constexpr int kMaxWords = 16384 / 64;               // 64-voxel words of the longest Z line
constexpr int64_t kStackLanesMax = 131072;          // lanes in flight of a line pass: 2 waves per SIMD on 256 CUs
constexpr size_t kStackBudgetBytes = size_t{1} << 30;  // ... fewer where the lines are long
constexpr unsigned kMaxBlocks = 256 * 8;

__device__ __forceinline__ bool IsFilledInput(float occupancy, int unknown_is_filled)
{
  return (occupancy > 0.5f) || (unknown_is_filled && (occupancy == 0.5f));
}
__device__ __forceinline__ bool IsFilledInput(uint8_t mask, int) { return mask != 0; }

// Z pass.  Every wave of a block takes one line per round; rounds, word counts and barriers are uniform over the block
// (a wave without a line walks along with nothing to load or store).
template <typename InT>
__global__ __launch_bounds__(kBlock) void NearestZKernel(const InT* __restrict__ in, int64_t lines, int nz,
                                                        int unknown_is_filled, uint16_t* __restrict__ out)
{
  __shared__ unsigned long long words[kWavesPerBlock][kMaxWords];
  // z of the first filled / free cell in the words above word w, -1: none
  __shared__ int16_t first_filled_above[kWavesPerBlock][kMaxWords];
  __shared__ int16_t first_free_above[kWavesPerBlock][kMaxWords];
  const int wave = static_cast<int>(threadIdx.x) >> 6;
  const int lane = static_cast<int>(threadIdx.x) & 63;
  const int num_words = (nz + 63) >> 6;
  const unsigned long long last_valid = (nz & 63) ? ((1ull << (nz & 63)) - 1ull) : ~0ull;
  for (int64_t base = static_cast<int64_t>(blockIdx.x) * kWavesPerBlock; base < lines;
       base += static_cast<int64_t>(gridDim.x) * kWavesPerBlock)
  {
    const int64_t line = base + wave;
    const bool active = line < lines;
    const InT* const src = in + (active ? line : 0) * nz;
    for (int w = 0; w < num_words; w++)
    {
      const int z = (w << 6) + lane;
      const bool filled = active && z < nz && IsFilledInput(src[z], unknown_is_filled);
      const unsigned long long m = __builtin_amdgcn_ballot_w64(filled);
      if (lane == 0) words[wave][w] = m;
    }
    __syncthreads();
    if (lane == 0)
    {
      int filled_above = -1, free_above = -1;
      for (int w = num_words - 1; w >= 0; w--)
      {
        first_filled_above[wave][w] = static_cast<int16_t>(filled_above);
        first_free_above[wave][w] = static_cast<int16_t>(free_above);
        const unsigned long long m = words[wave][w];
        const unsigned long long e = ~m & (w == num_words - 1 ? last_valid : ~0ull);
        if (m) filled_above = (w << 6) + __ffsll(static_cast<long long>(m)) - 1;
        if (e) free_above = (w << 6) + __ffsll(static_cast<long long>(e)) - 1;
      }
    }
    __syncthreads();
    int filled_below = -1, free_below = -1;  // z of the last filled / free cell in the words below
    for (int w = 0; w < num_words; w++)
    {
      const unsigned long long m = words[wave][w];
      const unsigned long long e = ~m & (w == num_words - 1 ? last_valid : ~0ull);
      const int z = (w << 6) + lane;
      if (active && z < nz)
      {
        const bool mine = (m >> lane) & 1ull;
        const unsigned long long other = mine ? e : m;
        const unsigned long long below = other & ((1ull << lane) - 1ull);
        const unsigned long long above = other & ~((2ull << lane) - 1ull);
        const int lo = below ? (w << 6) + 63 - __clzll(static_cast<long long>(below)) : (mine ? free_below : filled_below);
        const int hi = above ? (w << 6) + __ffsll(static_cast<long long>(above)) - 1
                             : (mine ? first_free_above[wave][w] : first_filled_above[wave][w]);
        uint32_t zs = kNearestNoneZ;
        if (lo >= 0 && (hi < 0 || z - lo <= hi - z))
          zs = static_cast<uint32_t>(lo);  // (the lower z on a tie)
        else if (hi >= 0)
          zs = static_cast<uint32_t>(hi);
        out[line * nz + z] = static_cast<uint16_t>((mine ? kNearestFilledBit : 0u) | zs);
      }
      if (m) filled_below = (w << 6) + 63 - __clzll(static_cast<long long>(m));
      if (e) free_below = (w << 6) + 63 - __clzll(static_cast<long long>(e));
    }
    __syncthreads();  // (the next round overwrites the tables)
  }
}

// A lane's hull stack in the workspace: slot j of lane l at [j * lanes + l].
struct StridedStack
{
  uint2* base;
  int64_t lanes;
  __device__ __forceinline__ void Put(int slot, uint32_t a, uint32_t b) const { base[slot * lanes] = make_uint2(a, b); }
  __device__ __forceinline__ void Get(int slot, uint32_t* a, uint32_t* b) const
  {
    const uint2 v = base[slot * lanes];
    *a = v.x;
    *b = v.y;
  }
};

// Persistent waves: wave w of the launch takes the 64-line groups w, w + waves, ...; its lanes own the stack columns
// of their global thread index (the launch has at most `stack_lanes` threads).
__global__ __launch_bounds__(kBlock) void NearestYKernel(const uint16_t* __restrict__ z_records,
                                                        uint32_t* __restrict__ y_records, int nx, int ny, int nz,
                                                        uint2* __restrict__ stacks, int64_t stack_lanes)
{
  const int64_t tid = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x;
  const int lane = static_cast<int>(threadIdx.x) & 63;
  const int64_t waves = static_cast<int64_t>(gridDim.x) * kWavesPerBlock;
  const int64_t z_groups = (nz + 63) >> 6;
  const int64_t groups = nx * z_groups;
  const StridedStack stack{stacks + tid, stack_lanes};
  for (int64_t g = tid >> 6; g < groups; g += waves)
  {
    const int64_t x = g / z_groups;
    const int z = static_cast<int>(g % z_groups) * 64 + lane;
    if (z >= nz) continue;
    const int64_t first = x * ny * nz + z;
    const YLine line{z_records + first, y_records + first, nz, z};
    NearestLine(ny, line, stack);
  }
}

__global__ __launch_bounds__(kBlock) void NearestXKernel(const uint32_t* __restrict__ y_records,
                                                        int32_t* __restrict__ nearest, int32_t* __restrict__ d2,
                                                        int nx, int ny, int nz, uint2* __restrict__ stacks,
                                                        int64_t stack_lanes)
{
  const int64_t tid = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x;
  const int lane = static_cast<int>(threadIdx.x) & 63;
  const int64_t waves = static_cast<int64_t>(gridDim.x) * kWavesPerBlock;
  const int64_t lines = static_cast<int64_t>(ny) * nz;
  const int64_t groups = (lines + 63) >> 6;
  const StridedStack stack{stacks + tid, stack_lanes};
  for (int64_t g = tid >> 6; g < groups; g += waves)
  {
    const int64_t p = g * 64 + lane;
    if (p >= lines) continue;
    const XLine line{y_records + p, nearest + p, d2 ? d2 + p : nullptr, lines, nz, static_cast<int32_t>(p / nz),
                     static_cast<int32_t>(p % nz)};
    NearestLine(nx, line, stack);
  }
}

// Tagged maps: the nearest object of every cell from the nearest cell (mask: the call's filled predicate).
__global__ __launch_bounds__(kBlock) void NearestObjectIdKernel(const uint8_t* __restrict__ cells, int64_t num_cells,
                                                               int cell_bytes, int object_id_offset,
                                                               const uint8_t* __restrict__ mask,
                                                               const int32_t* __restrict__ nearest,
                                                               uint32_t* __restrict__ object)
{
  for (int64_t i = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x; i < num_cells;
       i += static_cast<int64_t>(gridDim.x) * blockDim.x)
  {
    const int64_t from = mask[i] ? i : static_cast<int64_t>(nearest[i]);
    object[i] = (from >= 0 && from < num_cells)
                    ? *reinterpret_cast<const uint32_t*>(cells + from * cell_bytes + object_id_offset)
                    : 0u;
  }
}

size_t Align256(size_t v) { return (v + 255) / 256 * 256; }
int64_t RoundUpToBlock(int64_t v) { return (v + kBlock - 1) / kBlock * kBlock; }
unsigned BlocksFor(int64_t waves_wanted, int64_t lanes_allowed)
{
  const int64_t wanted = (waves_wanted + kWavesPerBlock - 1) / kWavesPerBlock;
  const int64_t allowed = lanes_allowed / kBlock;
  return static_cast<unsigned>(wanted < allowed ? wanted : allowed);
}

// Lanes in flight of a line pass over `lanes_wanted` lanes with stacks of `rows` slots, within the two limits.
int64_t StackLanes(int64_t lanes_wanted, int64_t rows)
{
  int64_t lanes = RoundUpToBlock(lanes_wanted);
  if (lanes > kStackLanesMax) lanes = kStackLanesMax;
  int64_t within_budget = static_cast<int64_t>(kStackBudgetBytes / (static_cast<size_t>(rows) * sizeof(uint2)));
  within_budget = within_budget / kBlock * kBlock;
  if (within_budget < kBlock) within_budget = kBlock;
  return lanes < within_budget ? lanes : within_budget;
}
}  // namespace

NearestWorkspace CarveNearestWorkspace(int64_t nx, int64_t ny, int64_t nz)
{
  const size_t cells = static_cast<size_t>(nx * ny * nz);
  NearestWorkspace ws;
  ws.z_records = 0;
  ws.y_records = Align256(cells * sizeof(uint16_t));
  ws.stacks = ws.y_records + Align256(cells * sizeof(uint32_t));
  // the Y pass runs lines of ny rows, 64 z per wave of each x; the X pass lines of nx rows over the flat (y, z)
  ws.y_lanes = StackLanes(nx * ((nz + 63) / 64) * 64, ny);
  ws.x_lanes = StackLanes(ny * nz, nx);
  const size_t y_bytes = static_cast<size_t>(ws.y_lanes) * static_cast<size_t>(ny) * sizeof(uint2);
  const size_t x_bytes = static_cast<size_t>(ws.x_lanes) * static_cast<size_t>(nx) * sizeof(uint2);
  ws.bytes = ws.stacks + (y_bytes > x_bytes ? y_bytes : x_bytes);  // (the passes use the area one after the other)
  return ws;
}

template <typename InT>
hipError_t LaunchNearest(const InT* input_dev, const NearestGrid& grid, int32_t* nearest_dev, int32_t* d2_dev,
                         void* workspace_dev, hipStream_t stream)
{
  const NearestWorkspace ws = CarveNearestWorkspace(grid.nx, grid.ny, grid.nz);
  char* const base = static_cast<char*>(workspace_dev);
  uint16_t* const z_records = reinterpret_cast<uint16_t*>(base + ws.z_records);
  uint32_t* const y_records = reinterpret_cast<uint32_t*>(base + ws.y_records);
  uint2* const stacks = reinterpret_cast<uint2*>(base + ws.stacks);
  const int64_t z_lines = static_cast<int64_t>(grid.nx) * grid.ny;
  const int64_t z_blocks = (z_lines + kWavesPerBlock - 1) / kWavesPerBlock;
  hipLaunchKernelGGL((NearestZKernel<InT>), dim3(static_cast<unsigned>(z_blocks < kMaxBlocks ? z_blocks : kMaxBlocks)),
                     dim3(kBlock), 0, stream, input_dev, z_lines, grid.nz, grid.unknown_is_filled, z_records);
  hipError_t err = hipGetLastError();
  if (err != hipSuccess) return err;
  const int64_t y_groups = static_cast<int64_t>(grid.nx) * ((grid.nz + 63) / 64);
  hipLaunchKernelGGL(NearestYKernel, dim3(BlocksFor(y_groups, ws.y_lanes)), dim3(kBlock), 0, stream, z_records,
                     y_records, grid.nx, grid.ny, grid.nz, stacks, ws.y_lanes);
  err = hipGetLastError();
  if (err != hipSuccess) return err;
  const int64_t x_groups = (static_cast<int64_t>(grid.ny) * grid.nz + 63) / 64;
  hipLaunchKernelGGL(NearestXKernel, dim3(BlocksFor(x_groups, ws.x_lanes)), dim3(kBlock), 0, stream, y_records,
                     nearest_dev, d2_dev, grid.nx, grid.ny, grid.nz, stacks, ws.x_lanes);
  return hipGetLastError();
}
template hipError_t LaunchNearest<float>(const float*, const NearestGrid&, int32_t*, int32_t*, void*, hipStream_t);
template hipError_t LaunchNearest<uint8_t>(const uint8_t*, const NearestGrid&, int32_t*, int32_t*, void*, hipStream_t);

hipError_t LaunchNearestObjectId(const void* cells_dev, int64_t num_cells, int cell_bytes, int object_id_offset,
                                 const uint8_t* mask_dev, const int32_t* nearest_dev, uint32_t* object_dev,
                                 hipStream_t stream)
{
  const int64_t blocks = (num_cells + kBlock - 1) / kBlock;
  hipLaunchKernelGGL(NearestObjectIdKernel, dim3(static_cast<unsigned>(blocks < kMaxBlocks ? blocks : kMaxBlocks)),
                     dim3(kBlock), 0, stream, static_cast<const uint8_t*>(cells_dev), num_cells, cell_bytes,
                     object_id_offset, mask_dev, nearest_dev, object_dev);
  return hipGetLastError();
}
}  // namespace vgt
