// Triangle meshes -> occupancy: mesh_rasterizer::RasterizeMesh (S/mesh_rasterizer.cpp:105-229) on the device.
//
// Per triangle (RasterizeTriangleImpl, :105-201): the bounding box of the three vertices becomes an index range through
// LocationToGridIndex, every cell of that range is a candidate -- nothing is padded, nothing outside it is touched --
// and a cell is set to occupancy 1.0f when the squared distance from its centre to the "closest point" of the triangle is
// <= max_check_radius_squared = pow(resolution * 0.5 * sqrt(3.0), 2.0) (evaluated by the host in double, :117-119).
//
// Two closest-point rules (MeshGrid::rule):
//   0 REFERENCE  the literal port of CalcClosestPointOnTriangle (:59-102).  When the query point does not project inside
//                the triangle, the reference ranks the three edge candidates by their OWN squared norm (:82-84), i.e. by
//                their distance to the origin of the frame the vertices are in -- not by their distance to the query
//                point -- with the `<=` tie order of :85-98 (edge 12, then 23, then 31).  The chosen candidate is
//                therefore often not the nearest one: the result changes when a mesh is translated, and cells along
//                slanted edges can be missed.  That is the reference's behaviour and rule 0 reproduces it as it is.
//   1 NEAREST    the same structure, the candidates ranked by their squared distance to the query point (same tie
//                order): the watertight variant, an extension.
//
// Operation order (double, compiled with -ffp-contract=off: no FMA contraction; every sum left to right; the parts of
// the reference that live in common_robotics_utilities, whose source is not available here, are fixed as stated):
//   dot(a, b)    = a.x*b.x + a.y*b.y + a.z*b.z            sq(a) = dot(a, a)
//   cross(a, b)  = (a.y*b.z - a.z*b.y, a.z*b.x - a.x*b.z, a.x*b.y - a.y*b.x)
//   M * (x,y,z,1): row r = M[r]*x + M[4+r]*y + M[8+r]*z + M[12+r] (column-major, row by row, left to right); no
//                transform at all when the caller passed none (the grid frame)
//   set-up, per triangle (v1, v2, v3 = its vertices):
//     normal   = cross(v2 - v1, v3 - v1); nn = sq(normal)                                        (:126-131)
//     lower    = per-axis min of the vertices, upper = per-axis max                             (:133-139)
//     lo index = floor((grid_from_world * lower) * (1 / resolution)) per axis, hi index from upper alike  (:141-144);
//                the candidates are lo.x..hi.x, lo.y..hi.y, lo.z..hi.z (none when lo > hi on an axis: the reference's
//                loops do not run); without `enforce` the range is clamped to the grid first (the reference skips outside
//                cells anyway, :187-191)
//     e_k      = B - A for the edges (A, B) = (v1, v2), (v2, v3), (v3, v1); ee_k = sq(e_k)
//     c1_k     = cross(e_k, P - A), P the vertex opposite the edge                               (:34-35)
//   per candidate cell:
//     centre   = (index + 0.5) * resolution per axis; q = world_from_grid * centre               (:157-159)
//     inside   = for k = 0, 1, 2: dot(c1_k, cross(e_k, q - A_k)) >= 0.0                           (:30-42)
//     inside:    v = q - v1; closest = v1 + (v - (dot(normal, v) / nn) * normal)                 (:68-72; VectorRejection
//                fixed as v - ((n.v) / (n.n)) * n -- unpinned against the reference)
//     otherwise: per edge  ratio = dot(e_k, q - A_k) / ee_k; clamped = min(max(ratio, 0), 1) (ClampValue);
//                candidate_k = A_k + e_k * clamped                                               (:45-57)
//                rank_k = sq(candidate_k) (rule 0) or sq(candidate_k - q) (rule 1); edge 12 when rank_12 <= both others,
//                else edge 23 when rank_23 <= both others, else edge 31                         (:82-98)
//     hit      = sq(closest - q) <= max_check_radius_squared                                     (:164, :182-183)
// tests/mesh_ref.py restates exactly this in numpy; the device result equals it on every voxel.
//
// Divergence from the reference: a triangle whose normal has squared norm 0 (or not > 0), a vertex that is not finite
// and a vertex index out of range are reported as errors (bits of MeshStatus) and nothing is rasterized; what the
// reference does there depends on code that is not available (NaN ratios, ClampValue's assertions, vector::at).
//
// Shape of the work: MeshSetupKernel, one thread per triangle, validates, computes the constants above and counts the
// triangle's BRICKS -- runs of up to 64 consecutive Z cells at one (x, y) of its range; an exclusive prefix sum over the
// counts makes the flat work list of (triangle, brick) pairs; MeshBrickKernel gives every wave one brick at a time, lanes
// along Z (the fastest axis), so a huge triangle and a tiny one cost in proportion to their cells, the triangle's
// constants are wave-uniform and a wave's stores fall into one contiguous segment.  Writers only ever store the constant
// 1.0f: plain vector stores, no atomics and no read-modify-write on the map; cells that do not intersect are not written,
// nor are the other 4 bytes of an 8-byte cell.  64-bit cell indexing throughout.
#include "mesh_kernels.hpp"

namespace vgt
{
namespace
{
constexpr int kSetupThreads = 256;
constexpr int kBrickThreads = 256;
constexpr int kBrickCells = 64;  // one wave
constexpr double kIndexLimit = 2305843009213693952.0;  // 2^61: indices are clamped to it before they become int64

struct MeshTriangle
{
  double v[3][3];   // v1, v2, v3
  double e[3][3];   // v2 - v1, v3 - v2, v1 - v3
  double c1[3][3];  // cross(e_k, opposite vertex - A_k)
  double ee[3];
  double normal[3];
  double nn;
  int64_t lo[3];
  int64_t extent[3];  // candidates per axis, 0 when the range is empty
};

size_t AlignUp256(size_t v) { return (v + 255) / 256 * 256; }
int64_t SetupBlocks(int64_t num_triangles) { return (num_triangles + kSetupThreads - 1) / kSetupThreads; }

struct ScratchLayout
{
  size_t triangles, offsets, block_bricks, block_cells, totals, status, bytes;
};
ScratchLayout Layout(int64_t num_triangles)
{
  const size_t t = static_cast<size_t>(num_triangles), b = static_cast<size_t>(SetupBlocks(num_triangles));
  ScratchLayout l;
  l.triangles = 0;
  l.offsets = AlignUp256(t * sizeof(MeshTriangle));
  l.block_bricks = l.offsets + AlignUp256((t + 1) * sizeof(unsigned long long));
  l.block_cells = l.block_bricks + AlignUp256(b * sizeof(unsigned long long));
  l.totals = l.block_cells + AlignUp256(b * sizeof(unsigned long long));
  l.status = l.totals + 256;
  l.bytes = l.status + 256;
  return l;
}

__device__ __forceinline__ double Dot(const double* a, const double* b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }
__device__ __forceinline__ void Cross(const double* a, const double* b, double* out)
{
  out[0] = a[1] * b[2] - a[2] * b[1];
  out[1] = a[2] * b[0] - a[0] * b[2];
  out[2] = a[0] * b[1] - a[1] * b[0];
}
__device__ __forceinline__ void Transform(const double* M, const double* p, double* out)
{
  out[0] = M[0] * p[0] + M[4] * p[1] + M[8] * p[2] + M[12];
  out[1] = M[1] * p[0] + M[5] * p[1] + M[9] * p[2] + M[13];
  out[2] = M[2] * p[0] + M[6] * p[1] + M[10] * p[2] + M[14];
}
__device__ __forceinline__ bool IsFinite(double v)
{
  return (static_cast<unsigned long long>(__double_as_longlong(v)) & 0x7ff0000000000000ull) != 0x7ff0000000000000ull;
}
__device__ __forceinline__ int64_t FloorIndex(double g, double inverse_resolution)
{
  double f = floor(g * inverse_resolution);
  f = f < -kIndexLimit ? -kIndexLimit : f;
  f = f > kIndexLimit ? kIndexLimit : f;
  return static_cast<int64_t>(f);  // (g is finite: the vertices are, and so is the transform's product or the range is empty)
}
__device__ __forceinline__ void Report(MeshStatus* status, int bit_index, uint32_t triangle)
{
  atomicOr(&status->bits, 1u << bit_index);
  atomicMin(&status->first[bit_index], triangle);
}

__global__ void MeshInitKernel(MeshStatus* status, MeshTotals* totals)
{
  if (threadIdx.x == 0)
  {
    status->bits = 0u;
    for (int b = 0; b < 4; b++) status->first[b] = 0xffffffffu;
    totals->bricks = 0ull;
    totals->cells = 0ull;
  }
}

// One thread per triangle; offsets[t] receives the exclusive sum of the brick counts INSIDE the workgroup, block_bricks /
// block_cells the workgroup's sums (saturating at kMeshCountCap).
__global__ __launch_bounds__(kSetupThreads) void MeshSetupKernel(
    const double* __restrict__ vertices, int64_t num_vertices, const int32_t* __restrict__ triangles,
    int64_t num_triangles, const MeshGrid grid, MeshTriangle* __restrict__ records,
    unsigned long long* __restrict__ offsets, unsigned long long* __restrict__ block_bricks,
    unsigned long long* __restrict__ block_cells, MeshStatus* __restrict__ status)
{
  __shared__ unsigned long long scan[kSetupThreads];
  __shared__ unsigned long long cells_sum[kSetupThreads];
  const int64_t t = static_cast<int64_t>(blockIdx.x) * kSetupThreads + threadIdx.x;
  unsigned long long bricks = 0ull, cells = 0ull;
  if (t < num_triangles)
  {
    MeshTriangle rec;
    for (int a = 0; a < 3; a++) rec.lo[a] = rec.extent[a] = 0;
    const int64_t i0 = triangles[3 * t], i1 = triangles[3 * t + 1], i2 = triangles[3 * t + 2];
    const int64_t idx[3] = {i0, i1, i2};
    bool ok = true;
    if (i0 < 0 || i0 >= num_vertices || i1 < 0 || i1 >= num_vertices || i2 < 0 || i2 >= num_vertices)
    {
      Report(status, 0, static_cast<uint32_t>(t));
      ok = false;
    }
    if (ok)
    {
      for (int k = 0; k < 3; k++)
        for (int a = 0; a < 3; a++)
        {
          rec.v[k][a] = vertices[3 * idx[k] + a];
          ok = ok && IsFinite(rec.v[k][a]);
        }
      if (!ok) Report(status, 1, static_cast<uint32_t>(t));
    }
    if (ok)
    {
      double v1v2[3], v1v3[3];
      for (int a = 0; a < 3; a++)
      {
        v1v2[a] = rec.v[1][a] - rec.v[0][a];
        v1v3[a] = rec.v[2][a] - rec.v[0][a];
      }
      Cross(v1v2, v1v3, rec.normal);
      rec.nn = Dot(rec.normal, rec.normal);
      if (!(rec.nn > 0.0))
      {
        Report(status, 2, static_cast<uint32_t>(t));
        ok = false;
      }
    }
    if (ok)
    {
      for (int k = 0; k < 3; k++)
      {
        const double* A = rec.v[k];
        const double* B = rec.v[(k + 1) % 3];
        const double* P = rec.v[(k + 2) % 3];
        double ap[3];
        for (int a = 0; a < 3; a++)
        {
          rec.e[k][a] = B[a] - A[a];
          ap[a] = P[a] - A[a];
        }
        Cross(rec.e[k], ap, rec.c1[k]);
        rec.ee[k] = Dot(rec.e[k], rec.e[k]);
      }
      double lower[3], upper[3];
      for (int a = 0; a < 3; a++)
      {
        lower[a] = fmin(fmin(rec.v[0][a], rec.v[1][a]), rec.v[2][a]);
        upper[a] = fmax(fmax(rec.v[0][a], rec.v[1][a]), rec.v[2][a]);
      }
      double lower_g[3], upper_g[3];
      if (grid.has_transform)
      {
        Transform(grid.grid_from_world, lower, lower_g);
        Transform(grid.grid_from_world, upper, upper_g);
      }
      else
        for (int a = 0; a < 3; a++)
        {
          lower_g[a] = lower[a];
          upper_g[a] = upper[a];
        }
      const double inverse_resolution = 1.0 / grid.resolution;
      const int64_t extents[3] = {grid.nx, grid.ny, grid.nz};
      bool empty = false;
      double cells_d = 1.0;
      for (int a = 0; a < 3; a++)
      {
        // (a transform with non-finite entries can make these NaN: no candidates then)
        if (!IsFinite(lower_g[a]) || !IsFinite(upper_g[a]))
        {
          empty = true;
          continue;
        }
        int64_t lo = FloorIndex(lower_g[a], inverse_resolution), hi = FloorIndex(upper_g[a], inverse_resolution);
        if (!grid.enforce)
        {
          lo = lo < 0 ? 0 : lo;
          hi = hi > extents[a] - 1 ? extents[a] - 1 : hi;
        }
        rec.lo[a] = lo;
        rec.extent[a] = hi >= lo ? hi - lo + 1 : 0;
        if (rec.extent[a] == 0) empty = true;
        cells_d *= static_cast<double>(rec.extent[a]);
      }
      if (empty)
        for (int a = 0; a < 3; a++) rec.extent[a] = 0;
      else if (cells_d >= static_cast<double>(kMeshCountCap))
        bricks = cells = kMeshCountCap;  // (refused by the host: far beyond kMeshMaxCandidateCells)
      else
      {
        const unsigned long long ex = static_cast<unsigned long long>(rec.extent[0]),
                                 ey = static_cast<unsigned long long>(rec.extent[1]),
                                 ez = static_cast<unsigned long long>(rec.extent[2]);
        cells = ex * ey * ez;
        bricks = ex * ey * ((ez + kBrickCells - 1) / kBrickCells);
      }
    }
    records[t] = rec;
  }
  // exclusive scan of the brick counts and sum of the cell counts inside the workgroup (each <= 2^40: no overflow)
  scan[threadIdx.x] = bricks;
  cells_sum[threadIdx.x] = cells;
  __syncthreads();
  for (int step = 1; step < kSetupThreads; step <<= 1)
  {
    const unsigned long long add = threadIdx.x >= static_cast<unsigned>(step) ? scan[threadIdx.x - step] : 0ull;
    __syncthreads();
    scan[threadIdx.x] += add;
    __syncthreads();
  }
  for (int step = kSetupThreads / 2; step > 0; step >>= 1)
  {
    if (threadIdx.x < static_cast<unsigned>(step)) cells_sum[threadIdx.x] += cells_sum[threadIdx.x + step];
    __syncthreads();
  }
  if (t < num_triangles) offsets[t] = scan[threadIdx.x] - bricks;
  if (threadIdx.x == kSetupThreads - 1)
    block_bricks[blockIdx.x] = scan[threadIdx.x] > kMeshCountCap ? kMeshCountCap : scan[threadIdx.x];
  if (threadIdx.x == 0) block_cells[blockIdx.x] = cells_sum[0] > kMeshCountCap ? kMeshCountCap : cells_sum[0];
}

// One workgroup: exclusive scan of the workgroups' brick sums in place, and the totals.  At most 2^23 entries of at most
// 2^40 each: the sums stay below 2^63.
__global__ __launch_bounds__(kSetupThreads) void MeshScanBlocksKernel(unsigned long long* __restrict__ block_bricks,
                                                                      const unsigned long long* __restrict__ block_cells,
                                                                      int64_t num_blocks, MeshTotals* __restrict__ totals)
{
  __shared__ unsigned long long scan[kSetupThreads];
  __shared__ unsigned long long cells_sum[kSetupThreads];
  unsigned long long carry = 0ull, cells = 0ull;
  for (int64_t base = 0; base < num_blocks; base += kSetupThreads)
  {
    const int64_t i = base + threadIdx.x;
    const unsigned long long mine = i < num_blocks ? block_bricks[i] : 0ull;
    cells += i < num_blocks ? block_cells[i] : 0ull;
    scan[threadIdx.x] = mine;
    __syncthreads();
    for (int step = 1; step < kSetupThreads; step <<= 1)
    {
      const unsigned long long add = threadIdx.x >= static_cast<unsigned>(step) ? scan[threadIdx.x - step] : 0ull;
      __syncthreads();
      scan[threadIdx.x] += add;
      __syncthreads();
    }
    if (i < num_blocks) block_bricks[i] = carry + scan[threadIdx.x] - mine;
    carry += scan[kSetupThreads - 1];
    __syncthreads();
  }
  cells_sum[threadIdx.x] = cells;
  __syncthreads();
  if (threadIdx.x == 0)
  {
    unsigned long long all = 0ull;
    for (int i = 0; i < kSetupThreads; i++) all += cells_sum[i];
    totals->bricks = carry > kMeshCountCap ? kMeshCountCap : carry;
    totals->cells = all > kMeshCountCap ? kMeshCountCap : all;
  }
}

__global__ __launch_bounds__(kSetupThreads) void MeshOffsetsKernel(unsigned long long* __restrict__ offsets,
                                                                   const unsigned long long* __restrict__ block_bricks,
                                                                   int64_t num_triangles,
                                                                   const MeshTotals* __restrict__ totals)
{
  const int64_t t = static_cast<int64_t>(blockIdx.x) * kSetupThreads + threadIdx.x;
  if (t < num_triangles) offsets[t] += block_bricks[blockIdx.x];
  if (t == num_triangles - 1) offsets[num_triangles] = totals->bricks;
}

// One wave per work item at a time (grid-stride over the list); lane = cell along Z inside the brick.
__global__ __launch_bounds__(kBrickThreads) void MeshBrickKernel(const MeshGrid grid, int64_t num_triangles,
                                                                unsigned long long total_bricks,
                                                                const MeshTriangle* __restrict__ records,
                                                                const unsigned long long* __restrict__ offsets,
                                                                char* __restrict__ cells, MeshStatus* __restrict__ status)
{
  const unsigned lane = threadIdx.x % kBrickCells;
  const unsigned long long waves_per_block = kBrickThreads / kBrickCells;
  const unsigned long long first_item = static_cast<unsigned long long>(blockIdx.x) * waves_per_block +
                                        static_cast<unsigned long long>(__builtin_amdgcn_readfirstlane(threadIdx.x / kBrickCells));
  const unsigned long long stride = static_cast<unsigned long long>(gridDim.x) * waves_per_block;
  for (unsigned long long item = first_item; item < total_bricks; item += stride)
  {
    // the triangle of this item: the last t with offsets[t] <= item (offsets[num_triangles] = total_bricks > item)
    int64_t low = 0, high = num_triangles - 1;
    while (low < high)
    {
      const int64_t mid = low + (high - low + 1) / 2;
      if (offsets[mid] <= item)
        low = mid;
      else
        high = mid - 1;
    }
    const int64_t t = low;
    const MeshTriangle& tri = records[t];
    const unsigned long long brick = item - offsets[t];
    const unsigned long long ey = static_cast<unsigned long long>(tri.extent[1]),
                             ez = static_cast<unsigned long long>(tri.extent[2]);
    const unsigned long long bricks_z = (ez + kBrickCells - 1) / kBrickCells;
    const unsigned long long column = brick / bricks_z, z_brick = brick % bricks_z;
    const unsigned long long z_in_range = z_brick * kBrickCells + lane;
    if (z_in_range >= ez) continue;
    const int64_t ix = tri.lo[0] + static_cast<int64_t>(column / ey);
    const int64_t iy = tri.lo[1] + static_cast<int64_t>(column % ey);
    const int64_t iz = tri.lo[2] + static_cast<int64_t>(z_in_range);

    const double centre[3] = {(static_cast<double>(ix) + 0.5) * grid.resolution,
                              (static_cast<double>(iy) + 0.5) * grid.resolution,
                              (static_cast<double>(iz) + 0.5) * grid.resolution};
    double q[3];
    if (grid.has_transform)
      Transform(grid.world_from_grid, centre, q);
    else
      for (int a = 0; a < 3; a++) q[a] = centre[a];

    double aq[3][3];
    bool inside = true;
    for (int k = 0; k < 3; k++)
    {
      for (int a = 0; a < 3; a++) aq[k][a] = q[a] - tri.v[k][a];
      double cross2[3];
      Cross(tri.e[k], aq[k], cross2);
      inside = inside && (Dot(tri.c1[k], cross2) >= 0.0);
    }
    double closest[3];
    if (inside)
    {
      const double scale = Dot(tri.normal, aq[0]) / tri.nn;
      for (int a = 0; a < 3; a++) closest[a] = tri.v[0][a] + (aq[0][a] - scale * tri.normal[a]);
    }
    else
    {
      double candidate[3][3], rank[3];
      for (int k = 0; k < 3; k++)
      {
        const double ratio = Dot(tri.e[k], aq[k]) / tri.ee[k];
        double clamped = ratio < 0.0 ? 0.0 : ratio;
        clamped = clamped > 1.0 ? 1.0 : clamped;
        for (int a = 0; a < 3; a++) candidate[k][a] = tri.v[k][a] + tri.e[k][a] * clamped;
        if (grid.rule == 0)
          rank[k] = Dot(candidate[k], candidate[k]);
        else
        {
          double d[3];
          for (int a = 0; a < 3; a++) d[a] = candidate[k][a] - q[a];
          rank[k] = Dot(d, d);
        }
      }
      const int chosen = (rank[0] <= rank[1] && rank[0] <= rank[2]) ? 0 : ((rank[1] <= rank[0] && rank[1] <= rank[2]) ? 1 : 2);
      for (int a = 0; a < 3; a++) closest[a] = chosen == 0 ? candidate[0][a] : (chosen == 1 ? candidate[1][a] : candidate[2][a]);
    }
    double diff[3];
    for (int a = 0; a < 3; a++) diff[a] = closest[a] - q[a];
    if (Dot(diff, diff) <= grid.max_check_radius_squared)
    {
      if (ix >= 0 && ix < grid.nx && iy >= 0 && iy < grid.ny && iz >= 0 && iz < grid.nz)
      {
        const int64_t index = (ix * grid.ny + iy) * grid.nz + iz;
        *reinterpret_cast<float*>(cells + index * grid.cell_bytes) = 1.0f;
      }
      else if (grid.enforce)
        Report(status, 3, static_cast<uint32_t>(t));
    }
  }
}
}  // namespace

size_t MeshScratchBytes(int64_t num_triangles) { return Layout(num_triangles).bytes; }

const MeshTotals* MeshTotalsPtr(const void* scratch_dev, int64_t num_triangles)
{
  return reinterpret_cast<const MeshTotals*>(static_cast<const char*>(scratch_dev) + Layout(num_triangles).totals);
}
const MeshStatus* MeshStatusPtr(const void* scratch_dev, int64_t num_triangles)
{
  return reinterpret_cast<const MeshStatus*>(static_cast<const char*>(scratch_dev) + Layout(num_triangles).status);
}

hipError_t LaunchMeshSetup(const double* vertices_dev, int64_t num_vertices, const int32_t* triangles_dev,
                           int64_t num_triangles, const MeshGrid& grid, void* scratch_dev, hipStream_t stream)
{
  const ScratchLayout l = Layout(num_triangles);
  char* const base = static_cast<char*>(scratch_dev);
  MeshTriangle* const records = reinterpret_cast<MeshTriangle*>(base + l.triangles);
  unsigned long long* const offsets = reinterpret_cast<unsigned long long*>(base + l.offsets);
  unsigned long long* const block_bricks = reinterpret_cast<unsigned long long*>(base + l.block_bricks);
  unsigned long long* const block_cells = reinterpret_cast<unsigned long long*>(base + l.block_cells);
  MeshTotals* const totals = reinterpret_cast<MeshTotals*>(base + l.totals);
  MeshStatus* const status = reinterpret_cast<MeshStatus*>(base + l.status);
  const int64_t blocks = SetupBlocks(num_triangles);
  MeshInitKernel<<<1, 64, 0, stream>>>(status, totals);
  MeshSetupKernel<<<dim3(static_cast<unsigned>(blocks)), kSetupThreads, 0, stream>>>(
      vertices_dev, num_vertices, triangles_dev, num_triangles, grid, records, offsets, block_bricks, block_cells, status);
  MeshScanBlocksKernel<<<1, kSetupThreads, 0, stream>>>(block_bricks, block_cells, blocks, totals);
  MeshOffsetsKernel<<<dim3(static_cast<unsigned>(blocks)), kSetupThreads, 0, stream>>>(offsets, block_bricks,
                                                                                       num_triangles, totals);
  return hipGetLastError();
}

hipError_t LaunchMeshBricks(const MeshGrid& grid, int64_t num_triangles, unsigned long long total_bricks,
                            void* scratch_dev, void* cells_dev, hipStream_t stream)
{
  if (total_bricks == 0ull) return hipSuccess;
  const ScratchLayout l = Layout(num_triangles);
  char* const base = static_cast<char*>(scratch_dev);
  const unsigned long long waves_per_block = kBrickThreads / kBrickCells;
  unsigned long long blocks = (total_bricks + waves_per_block - 1) / waves_per_block;
  // (enough workgroups to fill the device several times over; beyond that a wave strides through the list)
  constexpr unsigned long long kMaxBlocks = 1ull << 16;
  if (blocks > kMaxBlocks) blocks = kMaxBlocks;
  MeshBrickKernel<<<dim3(static_cast<unsigned>(blocks)), kBrickThreads, 0, stream>>>(
      grid, num_triangles, total_bricks, reinterpret_cast<const MeshTriangle*>(base + l.triangles),
      reinterpret_cast<const unsigned long long*>(base + l.offsets), static_cast<char*>(cells_dev),
      reinterpret_cast<MeshStatus*>(base + l.status));
  return hipGetLastError();
}
}  // namespace vgt
