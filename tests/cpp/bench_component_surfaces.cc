// ExtractComponentSurfaces of the C++ host layer beside the route it took before the cell selection existed: the dense
// mask of vgt_hip_component_surface_mask brought to the host and sorted into per-component lists by a loop over every
// voxel.  Both start from the same labelled OccupancyComponentMap and must give the same lists.
//   make -C tests/cpp BINARIES=bench_component_surfaces bench_component_surfaces     (the Makefile's rule for its binaries)
//   bench_component_surfaces [n = 256] [repeats = 5]     prints one JSON line (profiles/select/)
#include <vgt_hip.h>
#include <vgt_hip/hip_pointcloud_voxelizer.hpp>

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <vector>

using namespace vgt_hip;

static double Seconds()
{
  return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

static ComponentSurfaces DenseMaskRoute(vgt_hip_ctx* ctx, const OccupancyComponentMap& map, uint8_t component_types)
{
  const std::vector<OccupancyComponentCell>& data = map.GetImmutableRawData();
  std::vector<float> occupancy(data.size());
  std::vector<uint32_t> labels(data.size());
  for (size_t i = 0; i < data.size(); i++)
  {
    occupancy[i] = data[i].occupancy;
    labels[i] = data[i].component;
  }
  std::vector<uint8_t> mask(data.size());
  if (vgt_hip_component_surface_mask(ctx, occupancy.data(), labels.data(), map.NumXVoxels(), map.NumYVoxels(),
                                     map.NumZVoxels(), component_types, mask.data()) != VGT_HIP_OK)
  {
    std::printf("component surface mask failed: %s\n", vgt_hip_last_error());
    std::exit(1);
  }
  ComponentSurfaces surfaces;
  const int64_t ny = map.NumYVoxels(), nz = map.NumZVoxels();
  for (size_t i = 0; i < mask.size(); i++)
    if (mask[i])
    {
      const int64_t index = static_cast<int64_t>(i);
      surfaces[labels[i]].push_back({index / (ny * nz), (index / nz) % ny, index % nz});
    }
  return surfaces;
}

int main(int argc, char** argv)
{
  const int64_t n = argc > 1 ? std::atoll(argv[1]) : 256;
  const int repeats = argc > 2 ? std::atoi(argv[2]) : 5;
  // filled balls on a lattice of pitch 32, radius 10: many components with curved surfaces
  OccupancyComponentMap map(Isometry3::Identity(), "world", 0.01, n, n, n, OccupancyComponentCell());
  std::vector<OccupancyComponentCell>& data = map.GetMutableRawData();
  for (int64_t x = 0; x < n; x++)
    for (int64_t y = 0; y < n; y++)
      for (int64_t z = 0; z < n; z++)
      {
        const int64_t dx = x % 32 - 16, dy = y % 32 - 16, dz = z % 32 - 16;
        data[static_cast<size_t>((x * n + y) * n + z)].occupancy = dx * dx + dy * dy + dz * dz <= 100 ? 1.0f : 0.0f;
      }
  const uint32_t components = UpdateConnectedComponents(map);
  vgt_hip_ctx* ctx = nullptr;
  if (vgt_hip_create(0, -1, &ctx) != VGT_HIP_OK)
  {
    std::printf("no device: %s\n", vgt_hip_last_error());
    return 1;
  }
  const uint8_t types = FILLED_COMPONENTS;
  // (first calls: contexts, scratch and page-locking are set up)
  const ComponentSurfaces want = DenseMaskRoute(ctx, map, types);
  const ComponentSurfaces got = ExtractComponentSurfaces(map, types);
  size_t cells = 0;
  for (const auto& kv : got) cells += kv.second.size();
  std::vector<double> dense_s, compact_s;
  for (int r = 0; r < repeats; r++)
  {
    double t = Seconds();
    const ComponentSurfaces a = DenseMaskRoute(ctx, map, types);
    dense_s.push_back(Seconds() - t);
    t = Seconds();
    const ComponentSurfaces b = ExtractComponentSurfaces(map, types);
    compact_s.push_back(Seconds() - t);
    if (a.size() != b.size()) return 1;
  }
  vgt_hip_destroy(ctx);
  std::sort(dense_s.begin(), dense_s.end());
  std::sort(compact_s.begin(), compact_s.end());
  const double dense = dense_s[dense_s.size() / 2], compact = compact_s[compact_s.size() / 2];
  std::printf("{\"bench\": \"extract_component_surfaces\", \"grid\": %lld, \"components\": %u, \"surface_cells\": %zu, "
              "\"identical\": %s, \"repeats\": %d, \"dense_mask_route_median_s\": %.6f, \"compact_route_median_s\": %.6f, "
              "\"speedup\": %.3f}\n",
              static_cast<long long>(n), components, cells, got == want ? "true" : "false", repeats, dense, compact,
              dense / compact);
  return got == want ? 0 : 1;
}
