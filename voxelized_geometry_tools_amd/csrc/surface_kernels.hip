// The iso-surface of a float field as an indexed triangle mesh: surface nets on the lattice of cell centres
// (include/vgt_hip.h, vgt_hip_extract_surface, states every rule).  One vertex per active cube, one quad per crossing
// lattice edge whose four cubes are active; vertices in ascending index of their cube, quads in ascending index of the
// edge's lower sample, then axis x, y, z.  Every step is a predicate followed by an ordered compaction, the pattern of
// select_kernels.hip: lanes along Z, a wave holds 64 consecutive samples of the linear order, one ballot per wave is one
// word of a bit plane, a block of kBlockCells samples adds up its popcounts, LaunchScanBlocks turns them into offsets.
//   A. Mark       a lane loads the four columns (x .. x + 1, y .. y + 1) at its z and takes the four values at z + 1 from
//                 the next lane (the wave's last lane loads its own); from the 8 values: cube active, the three edges
//                 p -> p + e_a cross, p inside.  Five bit planes, and the active cubes per block.
//   B. Face mark  bit planes only: a crossing bit survives when the four cubes round the edge are active.  The face bits
//                 replace the crossing bits in place (a wave reads and writes its own word of them and nobody else's);
//                 the quads per block, and their exact number in 64 bits (a grid below 2^31 cells can hold more quads
//                 than the int32 scan can add up; the host refuses such a result from this number).
//   C. Scan       twice: vertex offsets and quad offsets, and the two totals.
//   D. Vertices   only active cubes re-read their 8 corners.  rank = block offset + popcounts; also the rank of every
//                 word's first lane (4 bytes per 64 samples), so that E finds any cube's vertex index as
//                 base[word] + popcount(active word & lanes below) without a dense index map.
//   E. Faces      bit planes and bases only; 6 int32 per quad.
// No workgroup waits for another one, no atomics on the outputs, plain vector stores: the result is a function of the
// input alone.  Scratch: 5 bits per voxel (the planes) + 4 bytes per 64 voxels (the bases) + 8 bytes per 1024 voxels
// (the two block counts) = 0.70 bytes per voxel.
// Double arithmetic without FMA contraction (-ffp-contract=off, as mesh_kernels.hip): tests/surface_ref.py restates it
// operation for operation.
#include "vgt_internal.hpp"

namespace vgt
{
namespace
{
constexpr int kBlock = 256;
constexpr int kRowsPerBlock = 4;
constexpr int kBlockCells = kBlock * kRowsPerBlock;  // samples per block count of the scans
constexpr int kWordsPerBlock = kBlockCells / 64;
constexpr int kWordsPerWave = kWordsPerBlock / (kBlock / 64);
enum Plane
{
  kActive = 0,
  kCrossX = 1,  // after step B: the face bits
  kCrossY = 2,
  kCrossZ = 3,
  kInside = 4,
  kPlanes = 5
};
using Word = unsigned long long;

__device__ __forceinline__ float LoadValue(const SurfaceGrid& g, int64_t i)
{
  return *reinterpret_cast<const float*>(static_cast<const uint8_t*>(g.values_dev) + i * g.value_stride);
}

__device__ __forceinline__ bool Inside(const SurfaceGrid& g, float v) { return g.inside_above ? v > g.iso : v < g.iso; }

__device__ __forceinline__ bool Finite(float v) { return fabsf(v) <= 3.402823466e+38f; }  // (false for a NaN)

// (the grid has fewer than 2^31 cells: 32-bit divisions)
__device__ __forceinline__ void Decode(const SurfaceGrid& g, int64_t i, int* x, int* y, int* z)
{
  const uint32_t line = static_cast<uint32_t>(i) / static_cast<uint32_t>(g.nz);
  *z = static_cast<int>(static_cast<uint32_t>(i) - line * static_cast<uint32_t>(g.nz));
  *x = static_cast<int>(line / static_cast<uint32_t>(g.ny));
  *y = static_cast<int>(line - static_cast<uint32_t>(*x) * static_cast<uint32_t>(g.ny));
}

__device__ __forceinline__ Word LanesBelow(int lane) { return (1ull << lane) - 1ull; }

__device__ __forceinline__ bool BitAt(const Word* plane, int64_t i) { return (plane[i >> 6] >> (i & 63)) & 1ull; }

// The block's sum of per-wave counts into counts[blockIdx.x]; returns it to thread 0.
__device__ __forceinline__ int BlockSum(int count, int* wave_count, int32_t* counts)
{
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) wave_count[wave] = count;
  __syncthreads();
  int sum = 0;
  if (threadIdx.x == 0)
  {
    for (int w = 0; w < kBlock / 64; w++) sum += wave_count[w];
    counts[blockIdx.x] = sum;
  }
  return sum;
}

__global__ __launch_bounds__(kBlock) void SurfaceMarkKernel(SurfaceGrid g, int64_t total, int64_t num_words,
                                                            Word* __restrict__ planes,
                                                            int32_t* __restrict__ vertex_counts)
{
  __shared__ int wave_count[kBlock / 64];
  const int lane = threadIdx.x & 63;
  const int64_t sy = g.nz, sx = static_cast<int64_t>(g.ny) * g.nz;
  int count = 0;
  for (int r = 0; r < kRowsPerBlock; r++)
  {
    // (whole waves run: the shuffles and the ballots need every lane; lanes past the end mark nothing)
    const int64_t i = static_cast<int64_t>(blockIdx.x) * kBlockCells + r * kBlock + threadIdx.x;
    const int64_t wave_first = i - lane;
    if (wave_first >= total) break;  // the same for every lane of the wave
    const bool in = i < total;
    int x = 0, y = 0, z = 0;
    if (in) Decode(g, i, &x, &y, &z);
    const bool hx = in && x + 1 < g.nx, hy = in && y + 1 < g.ny, hz = in && z + 1 < g.nz;
    // v[a][b]: the sample (x + a, y + b, z); w[a][b]: (x + a, y + b, z + 1).  A value that does not exist is never used.
    const float v00 = in ? LoadValue(g, i) : 0.0f;
    const float v10 = hx ? LoadValue(g, i + sx) : 0.0f;
    const float v01 = hy ? LoadValue(g, i + sy) : 0.0f;
    const float v11 = hx && hy ? LoadValue(g, i + sx + sy) : 0.0f;
    // (with hz the next lane holds sample i + 1 of the same line: the same x and y, hence the same four columns)
    float w00 = __shfl_down(v00, 1), w10 = __shfl_down(v10, 1), w01 = __shfl_down(v01, 1), w11 = __shfl_down(v11, 1);
    if (hz && lane == 63)
    {
      w00 = LoadValue(g, i + 1);
      w10 = hx ? LoadValue(g, i + 1 + sx) : 0.0f;
      w01 = hy ? LoadValue(g, i + 1 + sy) : 0.0f;
      w11 = hx && hy ? LoadValue(g, i + 1 + sx + sy) : 0.0f;
    }
    const bool in00 = Inside(g, v00);
    bool active = false;
    if (hx && hy && hz)
    {
      const bool finite = Finite(v00) && Finite(v10) && Finite(v01) && Finite(v11) && Finite(w00) && Finite(w10) &&
                          Finite(w01) && Finite(w11);
      const int inside = in00 + Inside(g, v10) + Inside(g, v01) + Inside(g, v11) + Inside(g, w00) + Inside(g, w10) +
                         Inside(g, w01) + Inside(g, w11);
      active = finite && inside > 0 && inside < 8;
    }
    const Word active_word = __ballot(active);
    const Word cross_x = __ballot(hx && in00 != Inside(g, v10));
    const Word cross_y = __ballot(hy && in00 != Inside(g, v01));
    const Word cross_z = __ballot(hz && in00 != Inside(g, w00));
    const Word inside_word = __ballot(in && in00);
    if (lane == 0)
    {
      const int64_t word = wave_first >> 6;
      planes[kActive * num_words + word] = active_word;
      planes[kCrossX * num_words + word] = cross_x;
      planes[kCrossY * num_words + word] = cross_y;
      planes[kCrossZ * num_words + word] = cross_z;
      planes[kInside * num_words + word] = inside_word;
    }
    count += __popcll(active_word);
  }
  BlockSum(count, wave_count, vertex_counts);
}

// (planes is read and written: the crossing words become the face words; no __restrict__)
__global__ __launch_bounds__(kBlock) void SurfaceFaceMarkKernel(SurfaceGrid g, int64_t total, int64_t num_words,
                                                                Word* planes, int32_t* __restrict__ face_counts,
                                                                Word* __restrict__ num_quads)
{
  __shared__ int wave_count[kBlock / 64];
  const int lane = threadIdx.x & 63;
  const int64_t sy = g.nz, sx = static_cast<int64_t>(g.ny) * g.nz;
  const Word* const active = planes + kActive * num_words;
  int count = 0;
  for (int r = 0; r < kRowsPerBlock; r++)
  {
    const int64_t i = static_cast<int64_t>(blockIdx.x) * kBlockCells + r * kBlock + threadIdx.x;
    const int64_t wave_first = i - lane;
    if (wave_first >= total) break;  // the same for every lane of the wave
    const int64_t word = wave_first >> 6;
    const Word cross_x = planes[kCrossX * num_words + word], cross_y = planes[kCrossY * num_words + word],
               cross_z = planes[kCrossZ * num_words + word];
    bool face_x = false, face_y = false, face_z = false;
    // (a set bit of any plane belongs to a sample inside the grid; an active cube exists)
    if ((((cross_x | cross_y | cross_z) & active[word]) >> lane) & 1ull)
    {
      int x, y, z;
      Decode(g, i, &x, &y, &z);
      // the four cubes round the edge p -> p + e_a, (b, c) the next two axes cyclically: p - e_b - e_c, p - e_c, p, p - e_b
      face_x = ((cross_x >> lane) & 1ull) && y >= 1 && z >= 1 && BitAt(active, i - sy - 1) && BitAt(active, i - 1) &&
               BitAt(active, i - sy);
      face_y = ((cross_y >> lane) & 1ull) && z >= 1 && x >= 1 && BitAt(active, i - 1 - sx) && BitAt(active, i - sx) &&
               BitAt(active, i - 1);
      face_z = ((cross_z >> lane) & 1ull) && x >= 1 && y >= 1 && BitAt(active, i - sx - sy) && BitAt(active, i - sy) &&
               BitAt(active, i - sx);
    }
    const Word face_word_x = __ballot(face_x), face_word_y = __ballot(face_y), face_word_z = __ballot(face_z);
    if (lane == 0)
    {
      planes[kCrossX * num_words + word] = face_word_x;
      planes[kCrossY * num_words + word] = face_word_y;
      planes[kCrossZ * num_words + word] = face_word_z;
    }
    count += __popcll(face_word_x) + __popcll(face_word_y) + __popcll(face_word_z);
  }
  const int sum = BlockSum(count, wave_count, face_counts);
  // (scratch, not an output; an integer sum does not depend on the order of its terms)
  if (threadIdx.x == 0 && sum > 0) atomicAdd(num_quads, static_cast<Word>(sum));
}

// The vertex of active cube (x, y, z): the mean of the crossing points of its 12 edges, in the order and with the
// operations of include/vgt_hip.h.
__device__ __forceinline__ void CubeVertex(const SurfaceGrid& g, int64_t i, int x, int y, int z, double* out)
{
  const int64_t sy = g.nz, sx = static_cast<int64_t>(g.ny) * g.nz;
  float corner[8];  // [4 dx + 2 dy + dz]
#pragma unroll
  for (int c = 0; c < 8; c++) corner[c] = LoadValue(g, i + (c >> 2) * sx + ((c >> 1) & 1) * sy + (c & 1));
  double offset[3] = {0.0, 0.0, 0.0};
  int crossings = 0;
  const double iso = static_cast<double>(g.iso);
#pragma unroll
  for (int a = 0; a < 3; a++)
  {
    const int b = (a + 1) % 3, c = (a + 2) % 3;
#pragma unroll
    for (int e = 0; e < 4; e++)
    {
      const int db = e >> 1, dc = e & 1;
      int d[3];
      d[a] = 0;
      d[b] = db;
      d[c] = dc;
      const float v0 = corner[4 * d[0] + 2 * d[1] + d[2]];
      d[a] = 1;
      const float v1 = corner[4 * d[0] + 2 * d[1] + d[2]];
      if (Inside(g, v0) != Inside(g, v1))
      {
        const double t = (iso - static_cast<double>(v0)) / (static_cast<double>(v1) - static_cast<double>(v0));
        offset[a] += t;
        offset[b] += static_cast<double>(db);
        offset[c] += static_cast<double>(dc);
        crossings++;
      }
    }
  }
  const double n = static_cast<double>(crossings);
  const double px = ((static_cast<double>(x) + 0.5) + offset[0] / n) * g.resolution;
  const double py = ((static_cast<double>(y) + 0.5) + offset[1] / n) * g.resolution;
  const double pz = ((static_cast<double>(z) + 0.5) + offset[2] / n) * g.resolution;
  if (g.has_transform)
  {
    const double* const m = g.world_from_grid;
#pragma unroll
    for (int r = 0; r < 3; r++) out[r] = m[r] * px + m[4 + r] * py + m[8 + r] * pz + m[12 + r];
  }
  else
  {
    out[0] = px;
    out[1] = py;
    out[2] = pz;
  }
}

__global__ __launch_bounds__(kBlock) void SurfaceEmitVerticesKernel(SurfaceGrid g, int64_t num_words,
                                                                    const Word* __restrict__ active,
                                                                    const int32_t* __restrict__ vertex_offsets,
                                                                    uint32_t* __restrict__ vertex_base,
                                                                    double* __restrict__ vertices,
                                                                    int32_t* __restrict__ vertex_cells)
{
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t first_word = static_cast<int64_t>(blockIdx.x) * kWordsPerBlock;
  int64_t rank = vertex_offsets[blockIdx.x];
  for (int w = 0; w < wave * kWordsPerWave; w++)
    if (first_word + w < num_words) rank += __popcll(active[first_word + w]);
  for (int k = 0; k < kWordsPerWave; k++)
  {
    const int64_t word_index = first_word + wave * kWordsPerWave + k;
    if (word_index >= num_words) break;
    const Word word = active[word_index];
    if (lane == 0) vertex_base[word_index] = static_cast<uint32_t>(rank);
    if ((word >> lane) & 1ull)
    {
      // (at < the vertex capacity: the host compares the scan's total with it before this launch)
      const int64_t at = rank + __popcll(word & LanesBelow(lane));
      const int64_t i = word_index * 64 + lane;
      int x, y, z;
      Decode(g, i, &x, &y, &z);
      double p[3];
      CubeVertex(g, i, x, y, z, p);
      vertices[3 * at] = p[0];
      vertices[3 * at + 1] = p[1];
      vertices[3 * at + 2] = p[2];
      if (vertex_cells) vertex_cells[at] = static_cast<int32_t>(i);
    }
    rank += __popcll(word);
  }
}

__device__ __forceinline__ int32_t VertexOf(const Word* active, const uint32_t* vertex_base, int64_t cube)
{
  return static_cast<int32_t>(vertex_base[cube >> 6] + __popcll(active[cube >> 6] & LanesBelow(static_cast<int>(cube & 63))));
}

__device__ __forceinline__ void StoreQuad(int32_t* triangles, int64_t quad, bool outward_plus, int32_t c00, int32_t c10,
                                          int32_t c11, int32_t c01)
{
  // counter-clockwise seen from + a: c00, c10, c11, c01; the normal points from inside to outside
  const int32_t q1 = outward_plus ? c10 : c01, q3 = outward_plus ? c01 : c10;
  int32_t* const t = triangles + 6 * quad;
  t[0] = c00;
  t[1] = q1;
  t[2] = c11;
  t[3] = c00;
  t[4] = c11;
  t[5] = q3;
}

__global__ __launch_bounds__(kBlock) void SurfaceEmitFacesKernel(SurfaceGrid g, int64_t num_words,
                                                                 const Word* __restrict__ planes,
                                                                 const int32_t* __restrict__ face_offsets,
                                                                 const uint32_t* __restrict__ vertex_base,
                                                                 int32_t* __restrict__ triangles)
{
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t sy = g.nz, sx = static_cast<int64_t>(g.ny) * g.nz;
  const Word* const active = planes + kActive * num_words;
  const Word* const faces_x = planes + kCrossX * num_words;
  const Word* const faces_y = planes + kCrossY * num_words;
  const Word* const faces_z = planes + kCrossZ * num_words;
  const Word* const inside = planes + kInside * num_words;
  const int64_t first_word = static_cast<int64_t>(blockIdx.x) * kWordsPerBlock;
  int64_t rank = face_offsets[blockIdx.x];
  for (int w = 0; w < wave * kWordsPerWave; w++)
    if (first_word + w < num_words)
      rank += __popcll(faces_x[first_word + w]) + __popcll(faces_y[first_word + w]) + __popcll(faces_z[first_word + w]);
  for (int k = 0; k < kWordsPerWave; k++)
  {
    const int64_t word_index = first_word + wave * kWordsPerWave + k;
    if (word_index >= num_words) break;
    const Word fx = faces_x[word_index], fy = faces_y[word_index], fz = faces_z[word_index];
    if (((fx | fy | fz) >> lane) & 1ull)
    {
      // ascending sample, then axis: the quads of the lanes below, then this lane's own lower axes
      const Word below = LanesBelow(lane);
      int64_t at = rank + __popcll(fx & below) + __popcll(fy & below) + __popcll(fz & below);
      const int64_t i = word_index * 64 + lane;
      const bool outward_plus = (inside[word_index] >> lane) & 1ull;
      const int32_t here = VertexOf(active, vertex_base, i);
      // (at < the quad capacity: the host compares the exact total with it before this launch)
      if ((fx >> lane) & 1ull)
        StoreQuad(triangles, at++, outward_plus, VertexOf(active, vertex_base, i - sy - 1),
                  VertexOf(active, vertex_base, i - 1), here, VertexOf(active, vertex_base, i - sy));
      if ((fy >> lane) & 1ull)
        StoreQuad(triangles, at++, outward_plus, VertexOf(active, vertex_base, i - 1 - sx),
                  VertexOf(active, vertex_base, i - sx), here, VertexOf(active, vertex_base, i - 1));
      if ((fz >> lane) & 1ull)
        StoreQuad(triangles, at++, outward_plus, VertexOf(active, vertex_base, i - sx - sy),
                  VertexOf(active, vertex_base, i - sy), here, VertexOf(active, vertex_base, i - sx));
    }
    rank += __popcll(fx) + __popcll(fy) + __popcll(fz);
  }
}

unsigned Blocks(int64_t items, int per_block) { return static_cast<unsigned>((items + per_block - 1) / per_block); }

struct ScratchLayout
{
  size_t planes, vertex_base, vertex_counts, face_counts, counts, bytes;
  int64_t num_words;
};
ScratchLayout CarveScratch(int64_t num_cells)
{
  const auto align = [](size_t v) { return (v + 255) / 256 * 256; };
  ScratchLayout s;
  s.num_words = (num_cells + 63) / 64;
  const size_t blocks = Blocks(num_cells, kBlockCells);
  s.planes = 0;
  s.vertex_base = align(static_cast<size_t>(s.num_words) * kPlanes * sizeof(Word));
  s.vertex_counts = s.vertex_base + align(static_cast<size_t>(s.num_words) * sizeof(uint32_t));
  s.face_counts = s.vertex_counts + align(blocks * sizeof(int32_t));
  s.counts = s.face_counts + align(blocks * sizeof(int32_t));
  s.bytes = s.counts + 256;
  return s;
}
}  // namespace

size_t SurfaceScratchBytes(int64_t num_cells) { return num_cells > 0 ? CarveScratch(num_cells).bytes : 0; }

const SurfaceCounts* SurfaceCountsPtr(const void* scratch_dev, int64_t num_cells)
{
  return reinterpret_cast<const SurfaceCounts*>(static_cast<const char*>(scratch_dev) + CarveScratch(num_cells).counts);
}

hipError_t LaunchSurfaceMark(const SurfaceGrid& g, void* scratch_dev, hipStream_t stream)
{
  const int64_t total = static_cast<int64_t>(g.nx) * g.ny * g.nz;
  const ScratchLayout s = CarveScratch(total);
  char* const base = static_cast<char*>(scratch_dev);
  Word* const planes = reinterpret_cast<Word*>(base + s.planes);
  int32_t* const vertex_counts = reinterpret_cast<int32_t*>(base + s.vertex_counts);
  int32_t* const face_counts = reinterpret_cast<int32_t*>(base + s.face_counts);
  SurfaceCounts* const counts = reinterpret_cast<SurfaceCounts*>(base + s.counts);
  hipError_t err = hipMemsetAsync(counts, 0, sizeof(*counts), stream);
  if (err != hipSuccess) return err;
  const unsigned blocks = Blocks(total, kBlockCells);
  SurfaceMarkKernel<<<blocks, kBlock, 0, stream>>>(g, total, s.num_words, planes, vertex_counts);
  SurfaceFaceMarkKernel<<<blocks, kBlock, 0, stream>>>(g, total, s.num_words, planes, face_counts, &counts->quads);
  err = hipGetLastError();
  if (err != hipSuccess) return err;
  err = LaunchScanBlocks(vertex_counts, static_cast<int64_t>(blocks), &counts->vertices, stream);
  if (err != hipSuccess) return err;
  return LaunchScanBlocks(face_counts, static_cast<int64_t>(blocks), &counts->quads_scanned, stream);
}

hipError_t LaunchSurfaceEmit(const SurfaceGrid& g, const SurfaceOutput& out, void* scratch_dev, hipStream_t stream)
{
  const int64_t total = static_cast<int64_t>(g.nx) * g.ny * g.nz;
  const ScratchLayout s = CarveScratch(total);
  char* const base = static_cast<char*>(scratch_dev);
  const Word* const planes = reinterpret_cast<const Word*>(base + s.planes);
  uint32_t* const vertex_base = reinterpret_cast<uint32_t*>(base + s.vertex_base);
  const unsigned blocks = Blocks(total, kBlockCells);
  SurfaceEmitVerticesKernel<<<blocks, kBlock, 0, stream>>>(g, s.num_words, planes + kActive * s.num_words,
                                                           reinterpret_cast<const int32_t*>(base + s.vertex_counts),
                                                           vertex_base, out.vertices_dev, out.vertex_cells_dev);
  if (out.triangles_dev)
    SurfaceEmitFacesKernel<<<blocks, kBlock, 0, stream>>>(g, s.num_words, planes,
                                                          reinterpret_cast<const int32_t*>(base + s.face_counts),
                                                          vertex_base, out.triangles_dev);
  return hipGetLastError();
}
}  // namespace vgt
