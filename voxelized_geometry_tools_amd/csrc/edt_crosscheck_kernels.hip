// The cross-check EDT: kernels and launchers (interface and encodings: edt_crosscheck.hpp).  Compiled once, with
// -DVGT_HIP_TESTING, and linked into libvgt_hip_testing.so only.
//
// An implementation of the transform that is independent of the product's class records and sweeps, for the parity
// tests to compare the product against:
//     pass 1  Z (contiguous axis): nearest-site scan on the binarised input, wave ballots -> int16 distances
//     pass 2  Y: per voxel, a pruned outward search over the squared pass-1 distances of its line
//     pass 3  X: same, fused with sqrt / resolution / sign / virtual border / min-max.
// Also here: the finalize check, a diagnostic that compares the product's fast final conversion with the exact one.
#include "edt_crosscheck.hpp"

#include "edt_device.hpp"

namespace vgt
{
namespace
{
constexpr int kWave = kWaveSize;
constexpr int kScanBlock = 256;
constexpr int kScanWaves = kScanBlock / kWave;
constexpr int kMaxChunks = static_cast<int>(kMaxExtent / kWave);

// is_filled predicate of OccupancyMap (occupancy_map.hpp:181-205).
__device__ __forceinline__ bool IsFilled(float occupancy, int unknown_is_filled)
{
  return (occupancy > 0.5f) || (unknown_is_filled && (occupancy == 0.5f));
}
__device__ __forceinline__ bool IsFilled(uint8_t mask, int) { return mask != 0; }

// Slab summary halves (vgt_internal.hpp): `boundary` = slab-local z of the slab's first (last) voxel, at_filled /
// at_free = slab-local z of the first (last) voxel of each class, -1 when absent.
__device__ __forceinline__ uint16_t SummaryHalf(int at_filled, int at_free, int boundary, int z_offset)
{
  const bool filled = at_filled == boundary;
  const int other = filled ? at_free : at_filled;
  return static_cast<uint16_t>((filled ? kSlabFilledBit : 0u) |
                               (other < 0 ? kSlabNone : static_cast<uint16_t>(other + z_offset)));
}

// ---------------------------------------------------------------------------------------------
// Pass 1: one wave per Z line.  Each 64-voxel chunk becomes one ballot mask; a voxel's distance
// to the nearest voxel of the other class is a clz/ffs on that mask, falling back to the nearest
// such voxel in the chunks before / after (carried as scalars).  Input is read exactly once.
// ---------------------------------------------------------------------------------------------
template <typename InT>
__global__ __launch_bounds__(kScanBlock) void ScanZKernel(const InT* __restrict__ in,
                                                         int16_t* __restrict__ out,
                                                         int64_t num_lines, int nz,
                                                         int unknown_is_filled,
                                                         SlabLineSummary* __restrict__ summary,
                                                         int z_offset)
{
  // [wave][chunk]: ballot of "filled", then first position >= chunk end holding a filled /
  // free voxel (or -1).  Written and read by the same wave only.
  __shared__ uint64_t s_filled[kScanWaves][kMaxChunks];
  __shared__ int32_t s_next_filled[kScanWaves][kMaxChunks];
  __shared__ int32_t s_next_free[kScanWaves][kMaxChunks];

  const int lane = threadIdx.x & (kWave - 1);
  const int wave = threadIdx.x / kWave;
  const int nchunks = (nz + kWave - 1) / kWave;
  volatile uint64_t* filled = s_filled[wave];
  volatile int32_t* next_filled = s_next_filled[wave];
  volatile int32_t* next_free = s_next_free[wave];

  for (int64_t line = static_cast<int64_t>(blockIdx.x) * kScanWaves + wave; line < num_lines;
       line += static_cast<int64_t>(gridDim.x) * kScanWaves)
  {
    const InT* src = in + line * nz;
    int16_t* dst = out + line * nz;

    for (int c = 0; c < nchunks; c++)
    {
      const int z = c * kWave + lane;
      const bool f = (z < nz) && IsFilled(src[z], unknown_is_filled);
      const uint64_t m = __ballot(f);
      if (lane == 0) filled[c] = m;
    }
    __builtin_amdgcn_wave_barrier();

    // Backward sweep (uniform per wave): nearest filled / free voxel after each chunk.
    if (lane == 0)
    {
      int32_t nf = -1, ne = -1;
      for (int c = nchunks - 1; c >= 0; c--)
      {
        next_filled[c] = nf;
        next_free[c] = ne;
        const int rem = nz - c * kWave;
        const uint64_t valid = (rem >= kWave) ? ~0ull : ((1ull << rem) - 1ull);
        const uint64_t F = filled[c];
        const uint64_t E = ~F & valid;
        if (F) nf = c * kWave + (__ffsll(static_cast<long long>(F)) - 1);
        if (E) ne = c * kWave + (__ffsll(static_cast<long long>(E)) - 1);
      }
      if (summary) summary[line].first = SummaryHalf(nf, ne, 0, z_offset);
    }
    __builtin_amdgcn_wave_barrier();

    // Forward sweep: per-lane distances.
    int32_t prev_filled = -1, prev_free = -1;  // last filled / free position before this chunk
    for (int c = 0; c < nchunks; c++)
    {
      const int rem = nz - c * kWave;
      const uint64_t valid = (rem >= kWave) ? ~0ull : ((1ull << rem) - 1ull);
      const uint64_t F = filled[c];
      const uint64_t E = ~F & valid;
      const int z = c * kWave + lane;
      if (z < nz)
      {
        const bool is_filled = (F >> lane) & 1ull;
        const uint64_t other = is_filled ? E : F;
        const int32_t prev_other = is_filled ? prev_free : prev_filled;
        const int32_t next_other = is_filled ? next_free[c] : next_filled[c];
        const uint64_t below = other & ((1ull << lane) - 1ull);
        const uint64_t above = (lane == kWave - 1) ? 0ull : (other >> (lane + 1));
        int32_t d_below = kInf16, d_above = kInf16;
        if (below)
          d_below = lane - (63 - __clzll(static_cast<long long>(below)));
        else if (prev_other >= 0)
          d_below = z - prev_other;
        if (above)
          d_above = __ffsll(static_cast<long long>(above));
        else if (next_other >= 0)
          d_above = next_other - z;
        const int32_t d = min(d_below, d_above);
        dst[z] = static_cast<int16_t>(is_filled ? -d : d);
      }
      if (F) prev_filled = c * kWave + (63 - __clzll(static_cast<long long>(F)));
      if (E) prev_free = c * kWave + (63 - __clzll(static_cast<long long>(E)));
    }
    if (summary && lane == 0) summary[line].last = SummaryHalf(prev_filled, prev_free, nz - 1, z_offset);
    __builtin_amdgcn_wave_barrier();
  }
}

// Multi-GPU: a voxel's distance along Z to the other class is the minimum of the slab-local
// distance and the distances to the nearest such voxel in the slabs below / above.
__global__ __launch_bounds__(256) void SlabFixupKernel(int16_t* __restrict__ io,
                                                      const SlabLineCarry* __restrict__ carries,
                                                      int64_t total, int nz, int z_offset)
{
  for (int64_t i = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x; i < total;
       i += static_cast<int64_t>(gridDim.x) * blockDim.x)
  {
    const int64_t line = i / nz;
    const int z = static_cast<int>(i - line * nz) + z_offset;
    const SlabLineCarry c = carries[line];
    const int16_t v = io[i];
    const bool filled = v < 0;
    int32_t d = filled ? -static_cast<int32_t>(v) : static_cast<int32_t>(v);
    const int prev_other = filled ? c.prev_free : c.prev_filled;
    const int next_other = filled ? c.next_free : c.next_filled;
    if (prev_other >= 0) d = min(d, z - prev_other);
    if (next_other >= 0) d = min(d, next_other - z);
    io[i] = static_cast<int16_t>(filled ? -d : d);
  }
}

// Exact 1-D lower-envelope value at position q by outward search with pruning: a site at
// offset k can only improve the answer while k*k < best, and the first voxel of the other
// class (a zero-valued site) ends the search on both sides.  O(sqrt(answer)) per voxel.
template <typename InT>
__device__ __forceinline__ int32_t LineSearch(const InT* __restrict__ centre, int64_t stride,
                                              int q, int n, bool negative, int32_t own)
{
  int32_t best = own;
  for (int k = 1; k < n; k++)
  {
    const int32_t kk = k * k;
    if (kk >= best) break;
    const bool has_lo = (q - k) >= 0;
    const bool has_hi = (q + k) < n;
    if (!has_lo && !has_hi) break;
    if (has_lo)
    {
      bool neg;
      int32_t f;
      Decode(centre[-static_cast<int64_t>(k) * stride], neg, f);
      const int32_t cand = (neg != negative) ? kk : ((f == kInf32) ? kInf32 : kk + f);
      best = min(best, cand);
    }
    if (has_hi)
    {
      bool neg;
      int32_t f;
      Decode(centre[static_cast<int64_t>(k) * stride], neg, f);
      const int32_t cand = (neg != negative) ? kk : ((f == kInf32) ? kInf32 : kk + f);
      best = min(best, cand);
    }
  }
  return best;
}

__global__ __launch_bounds__(256) void PassYBruteKernel(const int16_t* __restrict__ in,
                                                       int32_t* __restrict__ out, int64_t total,
                                                       int ny, int nz)
{
  for (int64_t i = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x; i < total;
       i += static_cast<int64_t>(gridDim.x) * blockDim.x)
  {
    const int y = static_cast<int>((i / nz) % ny);
    bool negative;
    int32_t own;
    Decode(in[i], negative, own);
    const int32_t best = LineSearch(in + i, static_cast<int64_t>(nz), y, ny, negative, own);
    out[i] = negative ? -best : best;
  }
}

__global__ __launch_bounds__(256) void PassXBruteFinalizeKernel(
    const int32_t* __restrict__ in, float* __restrict__ sdf, uint32_t* __restrict__ minmax_enc,
    int64_t total, int nx, int ny, int nz, double resolution, int add_virtual_border, int z_offset,
    int nz_global)
{
  uint32_t lo = 0xffffffffu, hi = 0u;
  const int64_t plane = static_cast<int64_t>(ny) * nz;
  for (int64_t i = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x; i < total;
       i += static_cast<int64_t>(gridDim.x) * blockDim.x)
  {
    const int x = static_cast<int>(i / plane);
    const int64_t r = i - static_cast<int64_t>(x) * plane;
    const int y = static_cast<int>(r / nz);
    const int z = static_cast<int>(r - static_cast<int64_t>(y) * nz);
    bool negative;
    int32_t own;
    Decode(in[i], negative, own);
    const int32_t best = LineSearch(in + i, plane, x, nx, negative, own);
    const float v = FinalizeSdf(best, negative, x, y, z + z_offset, nx, ny, nz_global, resolution,
                                add_virtual_border);
    sdf[i] = v;
    const uint32_t e = EncodeOrdered(v);
    lo = min(lo, e);
    hi = max(hi, e);
  }
  BlockMinMax(lo, hi, minmax_enc);
}

// Diagnostic: compares the fast final conversion with the exact one over a range of squared
// distances; result[0] = number of differing values, result[1] = first differing d2 (or ~0).
__global__ __launch_bounds__(256) void FinalizeCheckKernel(int64_t first, int64_t count, double resolution,
                                                          unsigned long long* __restrict__ result)
{
  unsigned long long bad = 0, first_bad = ~0ull;
  for (int64_t i = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x; i < count;
       i += static_cast<int64_t>(gridDim.x) * blockDim.x)
  {
    const int32_t d2 = static_cast<int32_t>(first + i);
    const float fast = SqrtTimesResolution(d2, resolution);
    const float exact = SqrtTimesResolutionExact(d2, resolution);
    if (__float_as_uint(fast) != __float_as_uint(exact))
    {
      bad++;
      first_bad = min(first_bad, static_cast<unsigned long long>(d2));
    }
  }
  if (bad)
  {
    atomicAdd(&result[0], bad);
    atomicMin(&result[1], first_bad);
  }
}

int GridFor(int64_t work_items, int block)
{
  // Memory-bound grid-stride launches: enough blocks to fill 256 CUs several times over.
  const int64_t blocks = (work_items + block - 1) / block;
  const int64_t cap = 256 * 32;
  return static_cast<int>(blocks < 1 ? 1 : (blocks > cap ? cap : blocks));
}

template <typename InT>
hipError_t LaunchScanZ(const InT* in, int16_t* out16, const SdfParams& p, int unknown_is_filled,
                       SlabLineSummary* summary, hipStream_t stream)
{
  const int z_offset = static_cast<int>(p.z_offset);
  const int64_t lines = p.nx * p.ny;
  const int nz = static_cast<int>(p.nz);
  const int grid = GridFor(lines, kScanWaves);
  hipLaunchKernelGGL(ScanZKernel<InT>, dim3(grid), dim3(kScanBlock), 0, stream, in, out16, lines, nz, unknown_is_filled,
                     summary, z_offset);
  return hipGetLastError();
}
}  // namespace

hipError_t LaunchCrossCheckScanZFromOccupancy(const float* occupancy, int16_t* out16, const SdfParams& p,
                                              SlabLineSummary* summary, hipStream_t stream)
{
  return LaunchScanZ<float>(occupancy, out16, p, p.unknown_is_filled, summary, stream);
}

hipError_t LaunchCrossCheckScanZFromMask(const uint8_t* mask, int16_t* out16, const SdfParams& p,
                                         SlabLineSummary* summary, hipStream_t stream)
{
  return LaunchScanZ<uint8_t>(mask, out16, p, 0, summary, stream);
}

hipError_t LaunchCrossCheckSlabFixup(int16_t* io16, const SlabLineCarry* carries, const SdfParams& p,
                                     hipStream_t stream)
{
  const int64_t total = p.nx * p.ny * p.nz;
  hipLaunchKernelGGL(SlabFixupKernel, dim3(GridFor(total, 256)), dim3(256), 0, stream, io16,
                     carries, total, static_cast<int>(p.nz), static_cast<int>(p.z_offset));
  return hipGetLastError();
}

hipError_t LaunchCrossCheckPassY(const int16_t* in16, int32_t* out32, const SdfParams& p, hipStream_t stream)
{
  const int64_t total = p.nx * p.ny * p.nz;
  hipLaunchKernelGGL(PassYBruteKernel, dim3(GridFor(total, 256)), dim3(256), 0, stream, in16,
                     out32, total, static_cast<int>(p.ny), static_cast<int>(p.nz));
  return hipGetLastError();
}

hipError_t LaunchCrossCheckPassXFinalize(const int32_t* in32, float* sdf, uint32_t* minmax_enc, const SdfParams& p,
                                         hipStream_t stream)
{
  const int64_t total = p.nx * p.ny * p.nz;
  hipLaunchKernelGGL(PassXBruteFinalizeKernel, dim3(GridFor(total, 256)), dim3(256), 0, stream,
                     in32, sdf, minmax_enc, total, static_cast<int>(p.nx), static_cast<int>(p.ny),
                     static_cast<int>(p.nz), p.resolution, p.add_virtual_border,
                     static_cast<int>(p.z_offset),
                     static_cast<int>(p.nz_global > 0 ? p.nz_global : p.nz));
  return hipGetLastError();
}

hipError_t LaunchFinalizeCheck(int64_t first, int64_t count, double resolution,
                               unsigned long long* result_dev, hipStream_t stream)
{
  hipLaunchKernelGGL(FinalizeCheckKernel, dim3(4096), dim3(256), 0, stream, first, count, resolution,
                     result_dev);
  return hipGetLastError();
}
}  // namespace vgt
