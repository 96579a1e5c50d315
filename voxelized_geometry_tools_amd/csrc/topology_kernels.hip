// Per-component holes and voids (the reference's topology_computation::ComputeComponentTopology,
// I/topology_computation.hpp:331-670, called from S/occupancy_component_map.cpp:594-653 and
// S/tagged_object_occupancy_component_map.cpp:566-625) as a stencil over the vertex lattice plus a union-find.
//
// The reference walks hash sets per component; the result is this closed form (include/vgt_hip.h states it in full).
// Lattice vertex (i, j, k), 0 <= i <= nx etc., touches the 8 cells (i-1..i, j-1..j, k-1..k); a cell outside the grid
// belongs to no component.  For a component c of a selected class:
//   V_c      = vertices where some of the 8 cells are of c and some are not;
//   an edge  of the lattice at such a vertex is EXPOSED when its 4 cells are mixed in the same sense (6-bit mask in
//              the reference's order z-, z+, y-, y+, x-, x+); M3 / M5 / M6 = vertices of V_c with 3 / 5 / 6 of them;
//   surfaces = connected components of (V_c, exposed edges); voids = surfaces - 1;
//   holes    = 1 + (M5 + 2 M6 - M3) / 8 + voids   (int32 division, toward zero).
// (The reference reads the Z + 1 neighbour at Z - 1 when it collects V_c, :388-391; this is the evident intent.)
//
// A NODE is a pair (vertex, component): a vertex is in V_c for up to 8 components at once.  Nodes are a surface, not
// a volume, so they are stored compactly:
//   1. CountNodes   one lane per vertex (Z fastest: a wave reads 64-cell runs of 4 label lines, and takes the k - 1
//                   cell from the lane below), nodes counted per block.
//   2. ScanBlocks   exclusive scan of the block counts by one workgroup, the total in 64 bits -> the host sizes the
//                   node arrays.
//   3. EmitNodes    the same stencil again: first_node[vertex], the records (vertex, component, edge mask) and the
//                   per-component counters.  A scene is typically a few huge components, so the lanes of a wave that
//                   share a component are counted with ballots and ONE lane adds for them.
//   4. MergeNodes   one lane per node: union with the node of the same component at the far end of each exposed +
//                   edge (the far vertex's 8 cells contain the edge's 4, so that node exists).
//   5. CountRoots   every node -> its root; one add per root into the component's surface count.
//   6. Finalize     one lane per component.
// All counters are int32 sums: the result does not depend on the order the atomics land in.
#include "union_find_device.hpp"
#include "vgt_internal.hpp"

namespace vgt
{
namespace
{
constexpr int kBlock = 256;
constexpr int kScanThreads = 1024;
constexpr uint32_t kOutside = 0xffffffffu;  // "label" of a cell outside the grid (never analysed: see Analysed)
constexpr int kLeaderRounds = 2;            // components per wave and cell slot that are counted with ballots

struct Lattice
{
  const uint8_t* cells;  // records of cell_bytes bytes, float occupancy first
  int cell_bytes;
  const uint32_t* labels;
  int nx, ny, nz;
  int64_t vertices;  // (nx + 1)(ny + 1)(nz + 1) < 2^31
  int types;
  uint32_t num_components;
};

struct TopologyNode
{
  int32_t vertex;
  uint32_t label;
  uint32_t edges;
};

__device__ __forceinline__ bool Analysed(const Lattice& g, uint32_t label)
{
  return label >= 1u && label <= g.num_components;
}

// bit q = dx * 4 + dy * 2 + dz of `same`: cell (i - 1 + dx, j - 1 + dy, k - 1 + dz) is of the component
__device__ __forceinline__ uint32_t ExposedEdges(uint32_t same)
{
  const auto mixed = [same](uint32_t four) -> uint32_t {
    const uint32_t s = same & four;
    return (s != 0u && s != four) ? 1u : 0u;
  };
  return mixed(0x55u) | (mixed(0xaau) << 1) | (mixed(0x33u) << 2) | (mixed(0xccu) << 3) | (mixed(0x0fu) << 4) |
         (mixed(0xf0u) << 5);
}

// The stencil of one vertex.  Every lane of the wave calls it (shuffles); a lane past the last vertex gets no node.
// Returns the bits q whose cell is the first of the 8 with its label, the label being an analysed component of a
// selected class that does not fill all 8 cells; label[q] and same[q] (which cells carry label[q]) are valid for them.
__device__ __forceinline__ uint32_t VertexNodes(const Lattice& g, int64_t v, int lane, int* vertex_k, uint32_t label[8],
                                                uint32_t same[8])
{
  const bool active = v < g.vertices;
  const int nzv = g.nz + 1;
  const int64_t line = active ? v / nzv : 0;
  const int k = static_cast<int>(active ? v - line * nzv : 0);
  const int j = static_cast<int>(line % (g.ny + 1));
  const int i = static_cast<int>(line / (g.ny + 1));
  *vertex_k = k;
  // lane - 1 holds vertex v - 1: for k > 0 the same (i, j) with k - 1, whose upper cell is this vertex's lower one
  const bool from_below = lane > 0 && k > 0;
#pragma unroll
  for (int dxy = 0; dxy < 4; dxy++)
  {
    const int x = i - 1 + (dxy >> 1), y = j - 1 + (dxy & 1);
    const bool in_line = active && x >= 0 && x < g.nx && y >= 0 && y < g.ny;
    const int64_t base = (static_cast<int64_t>(x) * g.ny + y) * g.nz;
    const uint32_t upper = (in_line && k < g.nz) ? g.labels[base + k] : kOutside;
    const uint32_t below = static_cast<uint32_t>(__shfl_up(static_cast<int>(upper), 1));
    uint32_t lower = kOutside;
    if (from_below)
      lower = below;
    else if (in_line && k > 0)
      lower = g.labels[base + k - 1];
    label[dxy * 2] = lower;
    label[dxy * 2 + 1] = upper;
  }
  bool all_equal = true;
#pragma unroll
  for (int q = 1; q < 8; q++) all_equal = all_equal && label[q] == label[0];
  if (!active || all_equal) return 0u;
  uint32_t nodes = 0u;
#pragma unroll
  for (int q = 0; q < 8; q++)
  {
    uint32_t s = 0u;
#pragma unroll
    for (int r = 0; r < 8; r++) s |= (label[r] == label[q] ? 1u : 0u) << r;
    same[q] = s;
    // the first of the 8 cells with this label (no lower bit of s), not all 8, a component that is analysed
    if ((s & ((1u << q) - 1u)) != 0u || s == 0xffu || !Analysed(g, label[q])) continue;
    const int x = i - 1 + (q >> 2), y = j - 1 + ((q >> 1) & 1), z = k - 1 + (q & 1);
    const int64_t cell = (static_cast<int64_t>(x) * g.ny + y) * g.nz + z;
    const float o = *reinterpret_cast<const float*>(g.cells + cell * g.cell_bytes);
    const int bit = o > 0.5f ? 1 : (o < 0.5f ? 2 : 4);  // (the rule of SurfaceMaskKernel)
    if (g.types & bit) nodes |= 1u << q;
  }
  return nodes;
}

// Sum of `value` over the block, valid in thread 0; *before = sum over the threads below this one.
__device__ __forceinline__ int BlockExclusiveScan(int value, int* wave_sum, int* before)
{
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int scanned = WaveInclusiveScan(value, lane);
  if (lane == 63) wave_sum[wave] = scanned;
  __syncthreads();
  int offset = scanned - value, total = 0;
  for (int w = 0; w < kBlock / 64; w++)
  {
    if (w < wave) offset += wave_sum[w];
    total += wave_sum[w];
  }
  *before = offset;
  return total;
}

__global__ __launch_bounds__(kBlock) void CountNodesKernel(Lattice g, int32_t* __restrict__ block_nodes)
{
  __shared__ int wave_sum[kBlock / 64];
  const int64_t v = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x;
  uint32_t label[8], same[8];
  int k;
  const uint32_t nodes = VertexNodes(g, v, threadIdx.x & 63, &k, label, same);
  int before;
  const int total = BlockExclusiveScan(__popc(nodes), wave_sum, &before);
  if (threadIdx.x == 0) block_nodes[blockIdx.x] = total;
}

// block_nodes[b] -> exclusive prefix sum in place (int32: only used when the total is below 2^31), *total in 64 bits.
__global__ __launch_bounds__(kScanThreads) void ScanNodeBlocksKernel(int32_t* __restrict__ block_nodes, int64_t blocks,
                                                                     unsigned long long* __restrict__ total)
{
  __shared__ long long wave_sum[kScanThreads / 64];
  const int64_t chunk = (blocks + kScanThreads - 1) / kScanThreads;
  const int64_t begin = threadIdx.x * chunk;
  const int64_t end = begin + chunk < blocks ? begin + chunk : blocks;
  long long sum = 0;
  for (int64_t b = begin; b < end; b++) sum += block_nodes[b];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  long long scanned = sum;
  for (int d = 1; d < 64; d <<= 1)
  {
    const long long other = __shfl_up(scanned, d);
    if (lane >= d) scanned += other;
  }
  if (lane == 63) wave_sum[wave] = scanned;
  __syncthreads();
  long long offset = scanned - sum;
  for (int w = 0; w < wave; w++) offset += wave_sum[w];
  for (int64_t b = begin; b < end; b++)
  {
    const int here = block_nodes[b];
    block_nodes[b] = static_cast<int32_t>(offset);
    offset += here;
  }
  if (threadIdx.x == kScanThreads - 1) *total = static_cast<unsigned long long>(offset);
}

__global__ __launch_bounds__(kBlock) void EmitNodesKernel(Lattice g, const int32_t* __restrict__ block_offset,
                                                          int32_t* __restrict__ first_node,
                                                          TopologyNode* __restrict__ node, int32_t* __restrict__ parent,
                                                          ComponentTopologyEntry* table)
{
  __shared__ int wave_sum[kBlock / 64];
  const int64_t v = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x;
  const int lane = threadIdx.x & 63;
  uint32_t label[8], same[8];
  int k;
  const uint32_t nodes = VertexNodes(g, v, lane, &k, label, same);
  int before;
  BlockExclusiveScan(__popc(nodes), wave_sum, &before);
  int32_t next = block_offset[blockIdx.x] + before;
  if (v < g.vertices)
  {
    first_node[v] = next;
    if (v == g.vertices - 1) first_node[g.vertices] = next + __popc(nodes);  // (the end of the last vertex's nodes)
  }
  if (__ballot(nodes != 0u) == 0ull) return;  // (wave-uniform)
#pragma unroll
  for (int q = 0; q < 8; q++)
  {
    bool has = ((nodes >> q) & 1u) != 0u;
    const uint32_t edges = has ? ExposedEdges(same[q]) : 0u;
    const int exposed = __popc(edges);
    if (has)
    {
      node[next] = TopologyNode{static_cast<int32_t>(v), label[q], edges};
      parent[next] = next;
      next++;
    }
    // counters: the first components of the wave by ballot, one lane adding for all its lanes ...
    unsigned long long todo = __ballot(has);
    for (int round = 0; round < kLeaderRounds && todo != 0ull; round++)
    {
      const int leader = __ffsll(static_cast<long long>(todo)) - 1;
      const uint32_t lead = static_cast<uint32_t>(__shfl(static_cast<int>(label[q]), leader));
      const bool mine = has && label[q] == lead;
      const unsigned long long all = __ballot(mine), m3 = __ballot(mine && exposed == 3),
                               m5 = __ballot(mine && exposed == 5), m6 = __ballot(mine && exposed == 6);
      if (lane == leader)
      {
        ComponentTopologyEntry* const t = table + lead;
        atomicAdd(&t->num_surface_vertices, __popcll(all));
        if (m3) atomicAdd(&t->m3, __popcll(m3));
        if (m5) atomicAdd(&t->m5, __popcll(m5));
        if (m6) atomicAdd(&t->m6, __popcll(m6));
      }
      todo &= ~all;
      if (mine) has = false;
    }
    // ... every further one (many tiny components) on its own
    if (has)
    {
      ComponentTopologyEntry* const t = table + label[q];
      atomicAdd(&t->num_surface_vertices, 1);
      if (exposed == 3) atomicAdd(&t->m3, 1);
      if (exposed == 5) atomicAdd(&t->m5, 1);
      if (exposed == 6) atomicAdd(&t->m6, 1);
    }
  }
}

__global__ __launch_bounds__(kBlock) void MergeNodesKernel(int64_t num_nodes, int64_t vertices, int ny, int nz,
                                                           const TopologyNode* __restrict__ node,
                                                           const int32_t* __restrict__ first_node, int32_t* parent)
{
  const int64_t n = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x;
  if (n >= num_nodes) return;
  const TopologyNode here = node[n];
  const int64_t stride[3] = {1, nz + 1, static_cast<int64_t>(ny + 1) * (nz + 1)};
#pragma unroll
  for (int axis = 0; axis < 3; axis++)
  {
    if (!((here.edges >> (2 * axis + 1)) & 1u)) continue;  // z+, y+, x+
    const int64_t far = here.vertex + stride[axis];
    if (far >= vertices) continue;  // (cannot happen: an edge that leaves the lattice has no cell of the grid)
    const int32_t end = first_node[far + 1];
    for (int32_t m = first_node[far]; m < end; m++)
      if (node[m].label == here.label)
      {
        Union(parent, static_cast<int32_t>(n), m);
        break;
      }
  }
}

__global__ __launch_bounds__(kBlock) void CountRootsKernel(int64_t num_nodes, const TopologyNode* __restrict__ node,
                                                           int32_t* parent, ComponentTopologyEntry* table)
{
  const int64_t n = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x;
  if (n >= num_nodes) return;
  const int32_t up = LoadLabel(parent, static_cast<int32_t>(n));
  if (up == n)
    atomicAdd(&table[node[n].label].num_surfaces, 1);
  else
    parent[n] = FindRoot(parent, up);  // (roots do not move in this kernel; a shortcut keeps every concurrent walk valid)
}

__global__ __launch_bounds__(kBlock) void FinalizeTopologyKernel(uint32_t num_components, ComponentTopologyEntry* table)
{
  const int64_t c = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x + 1;
  if (c > num_components) return;
  ComponentTopologyEntry t = table[c];
  // every component has a cell and the grid is finite: a selected component has surface vertices
  t.present = t.num_surface_vertices > 0 ? 1 : 0;
  if (t.present)
  {
    t.num_voids = t.num_surfaces - 1;
    t.num_holes = 1 + (t.m5 + 2 * t.m6 - t.m3) / 8 + t.num_voids;
  }
  table[c] = t;
}

unsigned Blocks(int64_t items, int per_block) { return static_cast<unsigned>((items + per_block - 1) / per_block); }

Lattice MakeLattice(const TopologyGrid& grid)
{
  Lattice g;
  g.cells = static_cast<const uint8_t*>(grid.cells_dev);
  g.cell_bytes = grid.cell_bytes;
  g.labels = grid.labels_dev;
  g.nx = static_cast<int>(grid.nx);
  g.ny = static_cast<int>(grid.ny);
  g.nz = static_cast<int>(grid.nz);
  g.vertices = TopologyVertices(grid.nx, grid.ny, grid.nz);
  g.types = grid.component_types;
  g.num_components = grid.num_components;
  return g;
}

struct VertexScratch
{
  size_t first_node, block_nodes, total, bytes;
};
VertexScratch CarveVertexScratch(int64_t vertices)
{
  const auto align = [](size_t v) { return (v + 255) / 256 * 256; };
  VertexScratch s;
  s.first_node = 0;
  s.block_nodes = align(static_cast<size_t>(vertices + 1) * sizeof(int32_t));
  s.total = s.block_nodes + align(static_cast<size_t>(Blocks(vertices, kBlock)) * sizeof(int32_t));
  s.bytes = s.total + 256;
  return s;
}
}  // namespace

size_t TopologyVertexScratchBytes(int64_t nx, int64_t ny, int64_t nz)
{
  return CarveVertexScratch(TopologyVertices(nx, ny, nz)).bytes;
}

const unsigned long long* TopologyNodeCountPtr(const void* vertex_scratch_dev, int64_t nx, int64_t ny, int64_t nz)
{
  return reinterpret_cast<const unsigned long long*>(static_cast<const char*>(vertex_scratch_dev) +
                                                     CarveVertexScratch(TopologyVertices(nx, ny, nz)).total);
}

size_t TopologyNodeScratchBytes(int64_t num_nodes)
{
  return static_cast<size_t>(num_nodes) * (sizeof(TopologyNode) + sizeof(int32_t));
}

hipError_t LaunchTopologyCountNodes(const TopologyGrid& grid, void* vertex_scratch_dev, hipStream_t stream)
{
  const Lattice g = MakeLattice(grid);
  const VertexScratch s = CarveVertexScratch(g.vertices);
  char* const base = static_cast<char*>(vertex_scratch_dev);
  int32_t* const block_nodes = reinterpret_cast<int32_t*>(base + s.block_nodes);
  const unsigned blocks = Blocks(g.vertices, kBlock);
  CountNodesKernel<<<blocks, kBlock, 0, stream>>>(g, block_nodes);
  ScanNodeBlocksKernel<<<1, kScanThreads, 0, stream>>>(block_nodes, static_cast<int64_t>(blocks),
                                                      reinterpret_cast<unsigned long long*>(base + s.total));
  return hipGetLastError();
}

hipError_t LaunchTopologyFromNodes(const TopologyGrid& grid, void* vertex_scratch_dev, int64_t num_nodes,
                                   void* node_scratch_dev, ComponentTopologyEntry* table_dev, hipStream_t stream)
{
  const Lattice g = MakeLattice(grid);
  const VertexScratch s = CarveVertexScratch(g.vertices);
  char* const base = static_cast<char*>(vertex_scratch_dev);
  int32_t* const first_node = reinterpret_cast<int32_t*>(base + s.first_node);
  const int32_t* const block_offset = reinterpret_cast<const int32_t*>(base + s.block_nodes);
  TopologyNode* const node = static_cast<TopologyNode*>(node_scratch_dev);
  int32_t* const parent = reinterpret_cast<int32_t*>(node + num_nodes);
  hipError_t err = hipMemsetAsync(table_dev, 0, (static_cast<size_t>(grid.num_components) + 1) * sizeof(*table_dev),
                                  stream);
  if (err != hipSuccess) return err;
  EmitNodesKernel<<<Blocks(g.vertices, kBlock), kBlock, 0, stream>>>(g, block_offset, first_node, node, parent,
                                                                     table_dev);
  if (num_nodes > 0)
  {
    const unsigned node_blocks = Blocks(num_nodes, kBlock);
    MergeNodesKernel<<<node_blocks, kBlock, 0, stream>>>(num_nodes, g.vertices, g.ny, g.nz, node, first_node, parent);
    CountRootsKernel<<<node_blocks, kBlock, 0, stream>>>(num_nodes, node, parent, table_dev);
  }
  if (grid.num_components > 0)
    FinalizeTopologyKernel<<<Blocks(grid.num_components, kBlock), kBlock, 0, stream>>>(grid.num_components, table_dev);
  return hipGetLastError();
}
}  // namespace vgt
