// Cost-to-go fields through free space for gfx950: the least cost of a path of grid moves from a set of sources to every
// passable cell, the neighbour to step to (`toward`), and batched path tracing.  The contract -- passable cells, moves,
// weights, the corner rule, the limit, every output -- is stated once: include/vgt_hip.h, vgt_hip_travel_cost.
//
// The cost field is the unique fixed point of  cost[c] = min(init(c), min over allowed moves c -> b of cost[b] + weight),
// and the kernels only ever lower a cell to the cost of a real path, so ANY order of relaxations that keeps going while
// something can still fall ends at that fixed point.  The steps:
//   A. Classify  one lane per cell, one ballot per wave = one 64-bit word of the passable bit plane (the ballot words of
//                select_kernels.hip).  Every later step reads 1 bit per cell instead of the field.
//   B. Seed      cost is filled with UNREACHED (a memset); one lane per source does atomicMin on its cell (sources may be
//                duplicated) and sets the activity flag of the cell's tile and of every neighbouring tile that has the
//                cell in its halo (no run of a tile lowers its seed).  The only atomics `cost` ever sees.
//   C. Rounds    one launch per round, one workgroup per tile of kTileX x kTileY x kTileZ cells (Z fastest).  A tile whose
//                flag is clear exits at once.  An active tile clears its flag, loads its cells and a one-cell halo (costs
//                and passable bits) into LDS, relaxes there until a workgroup-wide vote finds no lane that lowered a cell,
//                and writes back ITS OWN changed cells only: one writer per cell.  Where a cell on a face, an edge or a
//                corner of the tile changed, the flags of the neighbouring tiles that see that cell in their halo are set
//                for the NEXT round (the flags are double-buffered) together with the round's "any tile active" word, the
//                one word the host reads per round.
//   D. Toward    one lane per cell on the converged field, fixed offset order; counts the reached cells.  Then the roots.
//   E. Trace     one lane per start follows `toward`.
//
// What correctness rests on.  A halo may be read while the neighbouring tile, possibly on another XCD, rewrites it in the
// same launch.  Whatever is read is a 32-bit value that some launch stored: an older cost of that cell, i.e. the cost of
// a real path, a valid upper bound.  The neighbour that lowered a face cell flags this tile for the next round, and a
// kernel boundary makes everything visible.  So a tile stops being run only when its halo did not change after its last
// run, which is the fixed-point condition.  Nothing polls a flag inside a launch, nothing spins, no workgroup waits for
// another one.  Costs are integers that only fall, so the rounds end; the host bounds them all the same (vgt_hip.h).
//
// In bounds: a halo cell outside the grid is "not passable" and never loaded; the bit plane has one word per started 64
// cells; a tile index comes from an in-grid cell or is tested against the tile counts before its flag is touched.
#include "vgt_internal.hpp"

namespace vgt
{
namespace
{
constexpr int kTileX = kTravelTileX, kTileY = kTravelTileY, kTileZ = kTravelTileZ;
constexpr int kTileCells = kTileX * kTileY * kTileZ;
constexpr int kThreads = 256;
constexpr int kCellsPerThread = kTileCells / kThreads;
static_assert(kTileCells % kThreads == 0, "whole cells per thread");
constexpr int kHaloX = kTileX + 2, kHaloY = kTileY + 2, kHaloZ = kTileZ + 2;
constexpr int kHaloCells = kHaloX * kHaloY * kHaloZ;
constexpr uint32_t kUnreached = 0xffffffffu;

// Bit (dx + 1) * 9 + (dy + 1) * 3 + (dz + 1): ascending in the lexicographic order of (dx, dy, dz), the order of `toward`.
constexpr int OffsetBit(int dx, int dy, int dz) { return (dx + 1) * 9 + (dy + 1) * 3 + (dz + 1); }
constexpr int kCentreBit = OffsetBit(0, 0, 0);

// The cells whose passable bits the move (dx, dy, dz) needs: both ends, and with the corner rule every a + s, s_i in
// {0, d_i}.
constexpr uint32_t NeedMask(int dx, int dy, int dz, bool no_corner_cutting)
{
  uint32_t need = (1u << kCentreBit) | (1u << OffsetBit(dx, dy, dz));
  if (no_corner_cutting)
    for (int sx = 0; sx <= 1; sx++)
      for (int sy = 0; sy <= 1; sy++)
        for (int sz = 0; sz <= 1; sz++) need |= 1u << OffsetBit(sx * dx, sy * dy, sz * dz);
  return need;
}

struct Moves
{
  uint32_t weights[3];
  uint32_t flags;
  uint32_t cost_limit;
};

// Allowed moves of a cell, one bit per offset (OffsetBit), from the passable bits of its 3 x 3 x 3 box (same numbering;
// cells outside the grid are not passable).
__device__ __forceinline__ uint32_t MoveMask(uint32_t box, const Moves& m)
{
  uint32_t mask = 0u;
  const bool strict = (m.flags & 1u) != 0u;
#pragma unroll
  for (int dx = -1; dx <= 1; dx++)
#pragma unroll
    for (int dy = -1; dy <= 1; dy++)
#pragma unroll
      for (int dz = -1; dz <= 1; dz++)
      {
        const int k = (dx != 0) + (dy != 0) + (dz != 0);
        if (k == 0) continue;
        const uint32_t need = strict ? NeedMask(dx, dy, dz, true) : NeedMask(dx, dy, dz, false);
        if (m.weights[k - 1] != 0u && (box & need) == need) mask |= 1u << OffsetBit(dx, dy, dz);
      }
  return mask;
}

__device__ __forceinline__ bool PassableBit(const unsigned long long* __restrict__ words, uint32_t c)
{
  return ((words[c >> 6] >> (c & 63u)) & 1ull) != 0ull;
}

// kSource 0: float occupancy, 1: float SDF (blocked when (double)v <= threshold), 2: uint8 filled mask.
template <int kSource>
__global__ __launch_bounds__(kThreads) void TravelClassifyKernel(const void* __restrict__ field, int64_t total,
                                                                 int unknown_is_filled, double threshold,
                                                                 unsigned long long* __restrict__ words)
{
  // (whole waves run: the ballot needs every lane; lanes past the end are not passable)
  const int64_t i = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x;
  const int lane = threadIdx.x & 63;
  const int64_t wave_first = i - lane;
  if (wave_first >= total) return;  // the same for every lane of the wave
  bool passable = false;
  if (i < total)
  {
    if constexpr (kSource == 0)
    {
      const float v = static_cast<const float*>(field)[i];
      passable = !(v > 0.5f || (unknown_is_filled && v == 0.5f));
    }
    else if constexpr (kSource == 1)
    {
      const float v = static_cast<const float*>(field)[i];
      passable = !(static_cast<double>(v) <= threshold);
    }
    else
      passable = static_cast<const uint8_t*>(field)[i] == 0;
  }
  const unsigned long long word = __ballot(passable);
  if (lane == 0) words[wave_first >> 6] = word;
}

struct Tiles
{
  int nx, ny, nz;     // cells
  int tx, ty, tz;     // tiles per axis
};

__device__ __forceinline__ bool TileInRange(const Tiles& t, int x, int y, int z)
{
  return static_cast<unsigned>(x) < static_cast<unsigned>(t.tx) && static_cast<unsigned>(y) < static_cast<unsigned>(t.ty) &&
         static_cast<unsigned>(z) < static_cast<unsigned>(t.tz);
}

__device__ __forceinline__ void CellCoords(const Tiles& t, uint32_t c, int* x, int* y, int* z)
{
  const uint32_t line = c / static_cast<uint32_t>(t.nz);
  *z = static_cast<int>(c - line * static_cast<uint32_t>(t.nz));
  *x = static_cast<int>(line / static_cast<uint32_t>(t.ny));
  *y = static_cast<int>(line - static_cast<uint32_t>(*x) * static_cast<uint32_t>(t.ny));
}

// A source that contributes: inside the grid, passable, initial cost within the limit.
__device__ __forceinline__ bool SourceContributes(const int32_t* __restrict__ sources,
                                                  const uint32_t* __restrict__ source_costs, int64_t i, uint32_t cells,
                                                  uint32_t cost_limit, const unsigned long long* __restrict__ words,
                                                  uint32_t* cell, uint32_t* init)
{
  const int32_t s = sources[i];
  if (s < 0 || static_cast<uint32_t>(s) >= cells) return false;
  *cell = static_cast<uint32_t>(s);
  *init = source_costs ? source_costs[i] : 0u;
  return *init <= cost_limit && PassableBit(words, *cell);
}

__global__ __launch_bounds__(kThreads) void TravelSeedKernel(const int32_t* __restrict__ sources,
                                                             const uint32_t* __restrict__ source_costs,
                                                             int64_t num_sources, Tiles t, uint32_t cost_limit,
                                                             const unsigned long long* __restrict__ words,
                                                             uint32_t* __restrict__ cost, uint32_t* __restrict__ flags,
                                                             TravelStatus* __restrict__ status)
{
  const int64_t i = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x;
  if (i >= num_sources) return;
  const uint32_t cells = static_cast<uint32_t>(t.nx) * static_cast<uint32_t>(t.ny) * static_cast<uint32_t>(t.nz);
  uint32_t c, init;
  if (!SourceContributes(sources, source_costs, i, cells, cost_limit, words, &c, &init)) return;
  atomicMin(&cost[c], init);
  int x, y, z;
  CellCoords(t, c, &x, &y, &z);
  // the cell's tile, and every neighbouring tile that sees the cell in its halo: a seed on a face is a changed face cell
  const int txi = x / kTileX, tyi = y / kTileY, tzi = z / kTileZ;
  const int lx = x - txi * kTileX, ly = y - tyi * kTileY, lz = z - tzi * kTileZ;
  for (int sx = -1; sx <= 1; sx++)
    for (int sy = -1; sy <= 1; sy++)
      for (int sz = -1; sz <= 1; sz++)
      {
        const bool on_x = sx == 0 || (sx < 0 ? lx == 0 : lx == kTileX - 1);
        const bool on_y = sy == 0 || (sy < 0 ? ly == 0 : ly == kTileY - 1);
        const bool on_z = sz == 0 || (sz < 0 ? lz == 0 : lz == kTileZ - 1);
        const int nxt = txi + sx, nyt = tyi + sy, nzt = tzi + sz;
        if (on_x && on_y && on_z && TileInRange(t, nxt, nyt, nzt))
          atomicOr(&flags[(static_cast<uint32_t>(nxt) * t.ty + nyt) * t.tz + nzt], 1u);
      }
  atomicOr(&status->active[0], 1u);
}

// One round.  flags_now: this round's activity flags (a tile clears its own), flags_next / status->active[next]: what
// the next round runs.  Block 0 also clears status->active[now], which the host read before this launch.
__global__ __launch_bounds__(kThreads) void TravelRoundKernel(Tiles t, Moves m,
                                                              const unsigned long long* __restrict__ words,
                                                              uint32_t* __restrict__ cost, uint32_t* __restrict__ flags_now,
                                                              uint32_t* __restrict__ flags_next,
                                                              TravelStatus* __restrict__ status, int now)
{
  __shared__ uint32_t cost_s[kHaloCells];
  __shared__ uint8_t pass_s[kHaloCells];
  __shared__ uint32_t dirty_s;  // one bit per neighbouring tile (OffsetBit) that must run next round

  const uint32_t tile = blockIdx.x;
  if (tile == 0u && threadIdx.x == 0) status->active[now] = 0u;
  if (flags_now[tile] == 0u) return;  // the same for every lane of the workgroup
  __syncthreads();                    // (every lane has read the flag)
  if (threadIdx.x == 0)
  {
    flags_now[tile] = 0u;
    dirty_s = 0u;
    atomicAdd(&status->tiles_run, 1ull);
  }
  const int tzi = static_cast<int>(tile % static_cast<uint32_t>(t.tz));
  const int tyi = static_cast<int>((tile / static_cast<uint32_t>(t.tz)) % static_cast<uint32_t>(t.ty));
  const int txi = static_cast<int>(tile / (static_cast<uint32_t>(t.tz) * static_cast<uint32_t>(t.ty)));
  const int ox = txi * kTileX - 1, oy = tyi * kTileY - 1, oz = tzi * kTileZ - 1;  // the halo's lowest corner

  for (int h = threadIdx.x; h < kHaloCells; h += kThreads)
  {
    const int hz = h % kHaloZ, hy = (h / kHaloZ) % kHaloY, hx = h / (kHaloZ * kHaloY);
    const int gx = ox + hx, gy = oy + hy, gz = oz + hz;
    bool passable = false;
    uint32_t value = kUnreached;
    if (static_cast<unsigned>(gx) < static_cast<unsigned>(t.nx) && static_cast<unsigned>(gy) < static_cast<unsigned>(t.ny) &&
        static_cast<unsigned>(gz) < static_cast<unsigned>(t.nz))
    {
      const uint32_t c = (static_cast<uint32_t>(gx) * t.ny + gy) * t.nz + gz;
      passable = PassableBit(words, c);
      // (a halo value may be rewritten by its owner during this launch: any value read is an older valid cost)
      if (passable) value = __hip_atomic_load(&cost[c], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    pass_s[h] = passable ? 1 : 0;
    cost_s[h] = value;
  }
  __syncthreads();

  // this lane's cells: local index j = threadIdx.x + k * kThreads, z fastest
  int at[kCellsPerThread];          // index into the halo arrays
  uint32_t moves[kCellsPerThread];  // allowed moves; 0 for a blocked cell or one outside the grid
  uint32_t own[kCellsPerThread];
#pragma unroll
  for (int k = 0; k < kCellsPerThread; k++)
  {
    const int j = threadIdx.x + k * kThreads;
    const int lz = j % kTileZ, ly = (j / kTileZ) % kTileY, lx = j / (kTileZ * kTileY);
    at[k] = ((lx + 1) * kHaloY + (ly + 1)) * kHaloZ + (lz + 1);
    uint32_t box = 0u;
    if (pass_s[at[k]])
    {
#pragma unroll
      for (int dx = -1; dx <= 1; dx++)
#pragma unroll
        for (int dy = -1; dy <= 1; dy++)
#pragma unroll
          for (int dz = -1; dz <= 1; dz++)
            box |= static_cast<uint32_t>(pass_s[at[k] + (dx * kHaloY + dy) * kHaloZ + dz]) << OffsetBit(dx, dy, dz);
    }
    moves[k] = (box >> kCentreBit) & 1u ? MoveMask(box, m) : 0u;
    own[k] = cost_s[at[k]];
  }

  uint32_t changed_cells = 0u;  // bit k: cell k of this lane was lowered in this run
  const unsigned long long limit = m.cost_limit;
  for (;;)
  {
    int changed = 0;
#pragma unroll
    for (int k = 0; k < kCellsPerThread; k++)
    {
      if (moves[k] == 0u) continue;
      uint32_t best = own[k];
#pragma unroll
      for (int dx = -1; dx <= 1; dx++)
#pragma unroll
        for (int dy = -1; dy <= 1; dy++)
#pragma unroll
          for (int dz = -1; dz <= 1; dz++)
          {
            const int cls = (dx != 0) + (dy != 0) + (dz != 0);
            if (cls == 0) continue;
            if ((moves[k] >> OffsetBit(dx, dy, dz)) & 1u)
            {
              // (64 bits: UNREACHED + weight is above every limit, nothing wraps)
              const unsigned long long candidate =
                  static_cast<unsigned long long>(cost_s[at[k] + (dx * kHaloY + dy) * kHaloZ + dz]) + m.weights[cls - 1];
              if (candidate <= limit && candidate < best) best = static_cast<uint32_t>(candidate);
            }
          }
      if (best < own[k])
      {
        own[k] = best;
        cost_s[at[k]] = best;  // (only this lane writes this entry)
        changed = 1;
        changed_cells |= 1u << k;
      }
    }
    if (!__syncthreads_or(changed)) break;
  }

  // write back this tile's changed cells; collect the neighbouring tiles that see one of them in their halo
  uint32_t dirty = 0u;
#pragma unroll
  for (int k = 0; k < kCellsPerThread; k++)
  {
    if (!((changed_cells >> k) & 1u)) continue;
    const int j = threadIdx.x + k * kThreads;
    const int lz = j % kTileZ, ly = (j / kTileZ) % kTileY, lx = j / (kTileZ * kTileY);
    const uint32_t c = (static_cast<uint32_t>(ox + 1 + lx) * t.ny + (oy + 1 + ly)) * t.nz + (oz + 1 + lz);
    __hip_atomic_store(&cost[c], own[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#pragma unroll
    for (int sx = -1; sx <= 1; sx++)
#pragma unroll
      for (int sy = -1; sy <= 1; sy++)
#pragma unroll
        for (int sz = -1; sz <= 1; sz++)
        {
          if (sx == 0 && sy == 0 && sz == 0) continue;
          const bool on_x = sx == 0 || (sx < 0 ? lx == 0 : lx == kTileX - 1);
          const bool on_y = sy == 0 || (sy < 0 ? ly == 0 : ly == kTileY - 1);
          const bool on_z = sz == 0 || (sz < 0 ? lz == 0 : lz == kTileZ - 1);
          if (on_x && on_y && on_z) dirty |= 1u << OffsetBit(sx, sy, sz);
        }
  }
  if (dirty) atomicOr(&dirty_s, dirty);
  __syncthreads();
  if (threadIdx.x < 27 && threadIdx.x != kCentreBit && ((dirty_s >> threadIdx.x) & 1u))
  {
    const int b = threadIdx.x;
    const int nxt = txi + b / 9 - 1, nyt = tyi + (b / 3) % 3 - 1, nzt = tzi + b % 3 - 1;
    if (TileInRange(t, nxt, nyt, nzt))
    {
      atomicOr(&flags_next[(static_cast<uint32_t>(nxt) * t.ty + nyt) * t.tz + nzt], 1u);
      atomicOr(&status->active[now ^ 1], 1u);
    }
  }
}

// toward from the converged cost (the root rule comes after, TravelRootsKernel) and the number of reached cells.
constexpr int kTowardRows = 4;
template <bool kToward>
__global__ __launch_bounds__(kThreads) void TravelTowardKernel(Tiles t, Moves m,
                                                               const unsigned long long* __restrict__ words,
                                                               const uint32_t* __restrict__ cost,
                                                               int32_t* __restrict__ toward,
                                                               TravelStatus* __restrict__ status)
{
  __shared__ unsigned int reached_s;
  if (threadIdx.x == 0) reached_s = 0u;
  __syncthreads();
  const uint32_t cells = static_cast<uint32_t>(t.nx) * static_cast<uint32_t>(t.ny) * static_cast<uint32_t>(t.nz);
  unsigned int reached = 0u;
  for (int r = 0; r < kTowardRows; r++)
  {
    const int64_t i = (static_cast<int64_t>(blockIdx.x) * kTowardRows + r) * kThreads + threadIdx.x;
    if (i >= cells) break;
    const uint32_t c = static_cast<uint32_t>(i);
    const uint32_t own = cost[c];
    if (own != kUnreached) reached++;
    if constexpr (kToward)
    {
      int32_t next = -1;
      if (own != kUnreached)
      {
        int x, y, z;
        CellCoords(t, c, &x, &y, &z);
        uint32_t box = 0u;
#pragma unroll
        for (int dx = -1; dx <= 1; dx++)
#pragma unroll
          for (int dy = -1; dy <= 1; dy++)
#pragma unroll
            for (int dz = -1; dz <= 1; dz++)
            {
              const bool in_grid = static_cast<unsigned>(x + dx) < static_cast<unsigned>(t.nx) &&
                                   static_cast<unsigned>(y + dy) < static_cast<unsigned>(t.ny) &&
                                   static_cast<unsigned>(z + dz) < static_cast<unsigned>(t.nz);
              if (in_grid && PassableBit(words, c + static_cast<uint32_t>((dx * t.ny + dy) * t.nz + dz)))
                box |= 1u << OffsetBit(dx, dy, dz);
            }
        const uint32_t moves = MoveMask(box, m);
        // descending, the last match kept: the FIRST in ascending (dx, dy, dz) without a data-dependent exit
#pragma unroll
        for (int dx = 1; dx >= -1; dx--)
#pragma unroll
          for (int dy = 1; dy >= -1; dy--)
#pragma unroll
            for (int dz = 1; dz >= -1; dz--)
            {
              const int cls = (dx != 0) + (dy != 0) + (dz != 0);
              if (cls == 0) continue;
              if ((moves >> OffsetBit(dx, dy, dz)) & 1u)
              {
                const uint32_t b = c + static_cast<uint32_t>((dx * t.ny + dy) * t.nz + dz);
                if (static_cast<unsigned long long>(cost[b]) + m.weights[cls - 1] == own) next = static_cast<int32_t>(b);
              }
            }
      }
      toward[c] = next;
    }
  }
  if (reached) atomicAdd(&reached_s, reached);
  __syncthreads();
  if (threadIdx.x == 0 && reached_s) atomicAdd(&status->reached, static_cast<unsigned long long>(reached_s));
}

// The root rule, applied last: a contributing source whose initial cost is its cell's cost points to itself.
__global__ __launch_bounds__(kThreads) void TravelRootsKernel(const int32_t* __restrict__ sources,
                                                              const uint32_t* __restrict__ source_costs,
                                                              int64_t num_sources, uint32_t cells, uint32_t cost_limit,
                                                              const unsigned long long* __restrict__ words,
                                                              const uint32_t* __restrict__ cost,
                                                              int32_t* __restrict__ toward)
{
  const int64_t i = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x;
  if (i >= num_sources) return;
  uint32_t c, init;
  if (!SourceContributes(sources, source_costs, i, cells, cost_limit, words, &c, &init)) return;
  if (cost[c] == init) toward[c] = static_cast<int32_t>(c);  // (duplicates store the same value)
}

__global__ __launch_bounds__(kThreads) void TracePathsKernel(const int32_t* __restrict__ toward, int64_t cells,
                                                             const int32_t* __restrict__ starts, int64_t num_starts,
                                                             int32_t max_cells, int32_t* __restrict__ paths,
                                                             int32_t* __restrict__ lengths, uint8_t* __restrict__ status)
{
  const int64_t i = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x;
  if (i >= num_starts) return;
  int32_t* const path = paths + i * max_cells;
  int64_t cur = starts[i];
  int32_t length = 0;
  uint8_t result = kTraceInvalid;
  // at most max_cells trips: every trip that goes on has written one cell
  while (cur >= 0 && cur < cells)
  {
    const int32_t next = toward[cur];
    if (next < -1 || next >= cells) break;
    if (next == -1)
    {
      if (length == 0) result = kTraceUnreached;
      break;
    }
    path[length++] = static_cast<int32_t>(cur);
    if (next == cur)
    {
      result = kTraceOk;
      break;
    }
    if (length == max_cells)
    {
      result = kTraceTruncated;
      break;
    }
    cur = next;
  }
  lengths[i] = length;
  status[i] = result;
}

Tiles MakeTiles(const TravelGrid& g)
{
  return Tiles{g.nx,
               g.ny,
               g.nz,
               (g.nx + kTileX - 1) / kTileX,
               (g.ny + kTileY - 1) / kTileY,
               (g.nz + kTileZ - 1) / kTileZ};
}
Moves MakeMoves(const TravelGrid& g) { return Moves{{g.weights[0], g.weights[1], g.weights[2]}, g.flags, g.cost_limit}; }
unsigned Blocks(int64_t items, int per_block) { return static_cast<unsigned>((items + per_block - 1) / per_block); }
}  // namespace

TravelWorkspace CarveTravelWorkspace(int64_t nx, int64_t ny, int64_t nz)
{
  const auto up = [](size_t v) { return (v + 255) / 256 * 256; };
  TravelWorkspace w{};
  w.tiles = ((nx + kTileX - 1) / kTileX) * ((ny + kTileY - 1) / kTileY) * ((nz + kTileZ - 1) / kTileZ);
  const size_t words = static_cast<size_t>((nx * ny * nz + 63) / 64);
  w.status_offset = 0;
  w.flags_offset[0] = up(sizeof(TravelStatus));
  w.flags_offset[1] = w.flags_offset[0] + up(static_cast<size_t>(w.tiles) * sizeof(uint32_t));
  w.words_offset = w.flags_offset[1] + up(static_cast<size_t>(w.tiles) * sizeof(uint32_t));
  w.bytes = w.words_offset + up(words * sizeof(unsigned long long));
  return w;
}

hipError_t LaunchTravelSeed(const void* field_dev, int source, int unknown_is_filled, double threshold,
                            const TravelGrid& g, const int32_t* sources_dev, const uint32_t* source_costs_dev,
                            int64_t num_sources, uint32_t* cost_dev, void* workspace_dev, hipStream_t stream)
{
  const int64_t cells = static_cast<int64_t>(g.nx) * g.ny * g.nz;
  const TravelWorkspace w = CarveTravelWorkspace(g.nx, g.ny, g.nz);
  char* const base = static_cast<char*>(workspace_dev);
  auto* const words = reinterpret_cast<unsigned long long*>(base + w.words_offset);
  // status and both flag arrays are one zeroed range
  hipError_t err = hipMemsetAsync(base, 0, w.words_offset, stream);
  if (err != hipSuccess) return err;
  err = hipMemsetAsync(cost_dev, 0xff, static_cast<size_t>(cells) * sizeof(uint32_t), stream);
  if (err != hipSuccess) return err;
  const dim3 blocks(Blocks(cells, kThreads)), threads(kThreads);
  if (source == kTravelFromOccupancy)
    hipLaunchKernelGGL(TravelClassifyKernel<0>, blocks, threads, 0, stream, field_dev, cells, unknown_is_filled, threshold,
                       words);
  else if (source == kTravelFromSdf)
    hipLaunchKernelGGL(TravelClassifyKernel<1>, blocks, threads, 0, stream, field_dev, cells, unknown_is_filled, threshold,
                       words);
  else
    hipLaunchKernelGGL(TravelClassifyKernel<2>, blocks, threads, 0, stream, field_dev, cells, unknown_is_filled, threshold,
                       words);
  if (num_sources > 0)
    hipLaunchKernelGGL(TravelSeedKernel, dim3(Blocks(num_sources, kThreads)), threads, 0, stream, sources_dev,
                       source_costs_dev, num_sources, MakeTiles(g), g.cost_limit, words, cost_dev,
                       reinterpret_cast<uint32_t*>(base + w.flags_offset[0]),
                       reinterpret_cast<TravelStatus*>(base + w.status_offset));
  return hipGetLastError();
}

hipError_t LaunchTravelRound(const TravelGrid& g, uint32_t* cost_dev, void* workspace_dev, int64_t round,
                             hipStream_t stream)
{
  const TravelWorkspace w = CarveTravelWorkspace(g.nx, g.ny, g.nz);
  char* const base = static_cast<char*>(workspace_dev);
  const int now = static_cast<int>(round & 1);
  hipLaunchKernelGGL(TravelRoundKernel, dim3(static_cast<unsigned>(w.tiles)), dim3(kThreads), 0, stream, MakeTiles(g),
                     MakeMoves(g), reinterpret_cast<const unsigned long long*>(base + w.words_offset), cost_dev,
                     reinterpret_cast<uint32_t*>(base + w.flags_offset[now]),
                     reinterpret_cast<uint32_t*>(base + w.flags_offset[now ^ 1]),
                     reinterpret_cast<TravelStatus*>(base + w.status_offset), now);
  return hipGetLastError();
}

hipError_t LaunchTravelToward(const TravelGrid& g, const int32_t* sources_dev, const uint32_t* source_costs_dev,
                              int64_t num_sources, const uint32_t* cost_dev, int32_t* toward_dev, void* workspace_dev,
                              hipStream_t stream)
{
  const int64_t cells = static_cast<int64_t>(g.nx) * g.ny * g.nz;
  const TravelWorkspace w = CarveTravelWorkspace(g.nx, g.ny, g.nz);
  char* const base = static_cast<char*>(workspace_dev);
  const auto* const words = reinterpret_cast<const unsigned long long*>(base + w.words_offset);
  auto* const status = reinterpret_cast<TravelStatus*>(base + w.status_offset);
  const dim3 blocks(Blocks(cells, kThreads * kTowardRows)), threads(kThreads);
  if (toward_dev)
    hipLaunchKernelGGL(TravelTowardKernel<true>, blocks, threads, 0, stream, MakeTiles(g), MakeMoves(g), words, cost_dev,
                       toward_dev, status);
  else
    hipLaunchKernelGGL(TravelTowardKernel<false>, blocks, threads, 0, stream, MakeTiles(g), MakeMoves(g), words, cost_dev,
                       toward_dev, status);
  if (toward_dev && num_sources > 0)
    hipLaunchKernelGGL(TravelRootsKernel, dim3(Blocks(num_sources, kThreads)), threads, 0, stream, sources_dev,
                       source_costs_dev, num_sources, static_cast<uint32_t>(cells), g.cost_limit, words, cost_dev,
                       toward_dev);
  return hipGetLastError();
}

hipError_t LaunchTracePaths(const int32_t* toward_dev, int64_t cells, const int32_t* starts_dev, int64_t num_starts,
                            int32_t max_cells, int32_t* paths_dev, int32_t* lengths_dev, uint8_t* status_dev,
                            hipStream_t stream)
{
  if (num_starts <= 0) return hipSuccess;
  hipLaunchKernelGGL(TracePathsKernel, dim3(Blocks(num_starts, kThreads)), dim3(kThreads), 0, stream, toward_dev, cells,
                     starts_dev, num_starts, max_cells, paths_dev, lengths_dev, status_dev);
  return hipGetLastError();
}
}  // namespace vgt
