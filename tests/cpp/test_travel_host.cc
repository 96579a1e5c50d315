// ComputeTravelCost / TracePaths of the C++ host layer (include/vgt_hip/travel_cost.hpp) against a restatement of the
// definition of include/vgt_hip.h (vgt_hip_travel_cost) in this program, compared value for value.
//   test_travel_host              needs a HIP device
//   test_travel_host --no-device  the restatement against answers derived by hand, and the argument errors that are
//                                 raised before a device is touched (also what runs under the sanitizers)
#include <vgt_hip.h>
#include <vgt_hip/travel_cost.hpp>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <functional>
#include <limits>
#include <queue>
#include <stdexcept>
#include <vector>

using namespace vgt_hip;

static int g_failures = 0;
#define CHECK(cond)                                                    \
  do                                                                   \
  {                                                                    \
    if (!(cond))                                                       \
    {                                                                  \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);    \
      g_failures++;                                                    \
    }                                                                  \
  } while (0)

template <typename Fn>
static bool ThrowsInvalidArgument(const Fn& fn)
{
  try
  {
    fn();
  }
  catch (const std::invalid_argument&)
  {
    return true;
  }
  catch (...)
  {
  }
  return false;
}

constexpr uint32_t U = VGT_HIP_TRAVEL_UNREACHED;

struct Restated
{
  std::vector<uint32_t> cost;
  std::vector<int32_t> toward;
  int64_t reached = 0;
};

// The definition, one rule at a time: a heap Dijkstra in 64 bits, then the toward rule.
static Restated Restate(const std::vector<uint8_t>& passable, int64_t nx, int64_t ny, int64_t nz,
                        const std::array<uint32_t, 3>& weights, bool no_corner_cutting, const std::vector<int64_t>& sources,
                        const std::vector<uint32_t>& source_costs, uint32_t cost_limit)
{
  const int64_t n = nx * ny * nz;
  const auto free_at = [&](int64_t x, int64_t y, int64_t z) {
    return x >= 0 && x < nx && y >= 0 && y < ny && z >= 0 && z < nz && passable[static_cast<size_t>((x * ny + y) * nz + z)] != 0;
  };
  // the move (x, y, z) -> + (dx, dy, dz) is allowed; -> its weight, 0 when it is not
  const auto move = [&](int64_t x, int64_t y, int64_t z, int dx, int dy, int dz) -> uint32_t {
    const int k = (dx != 0) + (dy != 0) + (dz != 0);
    if (k == 0 || weights[static_cast<size_t>(k - 1)] == 0u) return 0u;
    if (!free_at(x, y, z) || !free_at(x + dx, y + dy, z + dz)) return 0u;
    if (no_corner_cutting)
      for (int sx = 0; sx <= 1; sx++)
        for (int sy = 0; sy <= 1; sy++)
          for (int sz = 0; sz <= 1; sz++)
            if (!free_at(x + sx * dx, y + sy * dy, z + sz * dz)) return 0u;
    return weights[static_cast<size_t>(k - 1)];
  };
  std::vector<uint64_t> best(static_cast<size_t>(n), std::numeric_limits<uint64_t>::max());
  std::vector<uint64_t> init(static_cast<size_t>(n), std::numeric_limits<uint64_t>::max());
  using Entry = std::pair<uint64_t, int64_t>;
  std::priority_queue<Entry, std::vector<Entry>, std::greater<Entry>> heap;
  for (size_t i = 0; i < sources.size(); i++)
  {
    const int64_t s = sources[i];
    const uint64_t c0 = source_costs.empty() ? 0u : source_costs[i];
    if (s < 0 || s >= n || !passable[static_cast<size_t>(s)] || c0 > cost_limit) continue;
    init[static_cast<size_t>(s)] = std::min(init[static_cast<size_t>(s)], c0);
    heap.push({c0, s});
  }
  std::vector<uint8_t> done(static_cast<size_t>(n), 0);
  while (!heap.empty())
  {
    const Entry e = heap.top();
    heap.pop();
    const size_t a = static_cast<size_t>(e.second);
    if (done[a]) continue;
    done[a] = 1;
    best[a] = e.first;
    const int64_t x = e.second / (ny * nz), y = e.second / nz % ny, z = e.second % nz;
    for (int dx = -1; dx <= 1; dx++)
      for (int dy = -1; dy <= 1; dy++)
        for (int dz = -1; dz <= 1; dz++)
        {
          const uint32_t w = move(x, y, z, dx, dy, dz);
          if (w == 0u || e.first + w > cost_limit) continue;
          const int64_t b = ((x + dx) * ny + (y + dy)) * nz + (z + dz);
          if (!done[static_cast<size_t>(b)]) heap.push({e.first + w, b});
        }
  }
  Restated out;
  out.cost.assign(static_cast<size_t>(n), U);
  out.toward.assign(static_cast<size_t>(n), -1);
  for (int64_t c = 0; c < n; c++)
  {
    const size_t at = static_cast<size_t>(c);
    if (!done[at]) continue;
    out.cost[at] = static_cast<uint32_t>(best[at]);
    out.reached++;
    const int64_t x = c / (ny * nz), y = c / nz % ny, z = c % nz;
    bool found = false;
    for (int dx = -1; dx <= 1 && !found; dx++)
      for (int dy = -1; dy <= 1 && !found; dy++)
        for (int dz = -1; dz <= 1 && !found; dz++)
        {
          const uint32_t w = move(x, y, z, dx, dy, dz);
          if (w == 0u) continue;
          const int64_t b = ((x + dx) * ny + (y + dy)) * nz + (z + dz);
          if (done[static_cast<size_t>(b)] && best[static_cast<size_t>(b)] + w == best[at])
          {
            out.toward[at] = static_cast<int32_t>(b);
            found = true;
          }
        }
    if (init[at] == best[at]) out.toward[at] = static_cast<int32_t>(c);  // a root: applied last
  }
  return out;
}

static std::vector<uint8_t> AllFree(int64_t n) { return std::vector<uint8_t>(static_cast<size_t>(n), 1); }

static int RunNoDevice()
{
  // a 1 x 1 x 5 corridor
  {
    const Restated r = Restate(AllFree(5), 1, 1, 5, {{1u, 0u, 0u}}, false, {0}, {}, 0xfffffffeu);
    CHECK((r.cost == std::vector<uint32_t>{0, 1, 2, 3, 4}));
    CHECK((r.toward == std::vector<int32_t>{0, 0, 1, 2, 3}));
    CHECK(r.reached == 5);
  }
  // a 3 x 3 x 1 plate with a blocked centre, from the corner, under each weight set
  {
    std::vector<uint8_t> plate = AllFree(9);
    plate[4] = 0;
    const auto cost = [&](std::array<uint32_t, 3> w, bool strict) {
      return Restate(plate, 3, 3, 1, w, strict, {0}, {}, 0xfffffffeu).cost;
    };
    CHECK((cost({{1u, 0u, 0u}}, false) == std::vector<uint32_t>{0, 1, 2, 1, U, 3, 2, 3, 4}));
    CHECK((cost({{2u, 3u, 0u}}, false) == std::vector<uint32_t>{0, 2, 4, 2, U, 5, 4, 5, 7}));
    CHECK((cost({{10u, 14u, 17u}}, false) == std::vector<uint32_t>{0, 10, 20, 10, U, 24, 20, 24, 34}));
    CHECK((cost({{1u, 1u, 1u}}, false) == std::vector<uint32_t>{0, 1, 2, 1, U, 2, 2, 2, 3}));
    CHECK((cost({{5u, 0u, 7u}}, false) == std::vector<uint32_t>{0, 5, 10, 5, U, 15, 10, 15, 20}));
    // every 2 x 2 block of the plate holds the centre: the corner rule leaves the axis moves
    CHECK((cost({{2u, 3u, 0u}}, true) == std::vector<uint32_t>{0, 2, 4, 2, U, 6, 4, 6, 8}));
  }
  // the diagonal gap
  {
    const std::vector<uint8_t> gap{1, 0, 0, 1};
    CHECK((Restate(gap, 2, 2, 1, {{10u, 14u, 17u}}, false, {0}, {}, 0xfffffffeu).cost == std::vector<uint32_t>{0, U, U, 14}));
    CHECK((Restate(gap, 2, 2, 1, {{10u, 14u, 17u}}, true, {0}, {}, 0xfffffffeu).cost == std::vector<uint32_t>{0, U, U, U}));
  }
  // ties take the first offset in (dx, dy, dz) order; a dominated source is no root
  {
    const Restated r = Restate(AllFree(9), 3, 3, 1, {{1u, 1u, 1u}}, false, {0}, {}, 0xfffffffeu);
    CHECK((r.toward == std::vector<int32_t>{0, 0, 1, 0, 0, 1, 3, 3, 4}));
    const Restated d = Restate(AllFree(8), 1, 1, 8, {{2u, 0u, 0u}}, false, {3, 5, 5}, {0, 9, 11}, 0xfffffffeu);
    CHECK(d.cost[5] == 4 && d.toward[5] == 4 && d.toward[3] == 3);
  }

  // the argument errors of the C ABI, before a device is touched (the context pointer is never dereferenced)
  float field[64];
  std::fill(field, field + 64, 0.25f);
  vgt_hip_ctx* const stand_in = reinterpret_cast<vgt_hip_ctx*>(field);
  const uint32_t weights[3] = {10u, 14u, 17u};
  const int32_t sources[2] = {0, 5};
  std::vector<uint32_t> cost(64, 9u);
  std::vector<int32_t> toward(64, 9);
  int64_t reached = -7;
  const auto host = [&](vgt_hip_ctx* ctx, const float* f, int64_t nx, int32_t mode, double threshold, const uint32_t* w,
                        uint32_t flags, const int32_t* s, int64_t ns, uint32_t limit, uint32_t* c) {
    return vgt_hip_travel_cost(ctx, f, nx, 4, 4, mode, 1, threshold, w, flags, s, nullptr, ns, limit, c, toward.data(),
                               &reached);
  };
  const uint32_t no_limit = 0xfffffffeu;
  CHECK(host(nullptr, field, 4, 0, 0.0, weights, 0u, sources, 2, no_limit, cost.data()) == VGT_HIP_ERR_INVALID_ARGUMENT);
  CHECK(std::strstr(vgt_hip_last_error(), "null") != nullptr);
  CHECK(host(stand_in, nullptr, 4, 0, 0.0, weights, 0u, sources, 2, no_limit, cost.data()) == VGT_HIP_ERR_INVALID_ARGUMENT);
  CHECK(host(stand_in, field, 4, 0, 0.0, nullptr, 0u, sources, 2, no_limit, cost.data()) == VGT_HIP_ERR_INVALID_ARGUMENT);
  CHECK(host(stand_in, field, 4, 0, 0.0, weights, 0u, nullptr, 2, no_limit, cost.data()) == VGT_HIP_ERR_INVALID_ARGUMENT);
  CHECK(host(stand_in, field, 4, 0, 0.0, weights, 0u, sources, 2, no_limit, nullptr) == VGT_HIP_ERR_INVALID_ARGUMENT);
  CHECK(host(stand_in, field, -4, 0, 0.0, weights, 0u, sources, 2, no_limit, cost.data()) == VGT_HIP_ERR_INVALID_ARGUMENT);
  CHECK(std::strstr(vgt_hip_last_error(), "negative") != nullptr);
  CHECK(host(stand_in, field, int64_t{1} << 31, 0, 0.0, weights, 0u, sources, 2, no_limit, cost.data()) ==
        VGT_HIP_ERR_INVALID_ARGUMENT);
  CHECK(std::strstr(vgt_hip_last_error(), "2^31") != nullptr);
  CHECK(host(stand_in, field, 4, 2, 0.0, weights, 0u, sources, 2, no_limit, cost.data()) == VGT_HIP_ERR_INVALID_ARGUMENT);
  CHECK(std::strstr(vgt_hip_last_error(), "mode") != nullptr);
  CHECK(host(stand_in, field, 4, 0, 0.0, weights, 2u, sources, 2, no_limit, cost.data()) == VGT_HIP_ERR_INVALID_ARGUMENT);
  CHECK(std::strstr(vgt_hip_last_error(), "flag") != nullptr);
  CHECK(host(stand_in, field, 4, 1, std::nan(""), weights, 0u, sources, 2, no_limit, cost.data()) ==
        VGT_HIP_ERR_INVALID_ARGUMENT);
  CHECK(std::strstr(vgt_hip_last_error(), "threshold") != nullptr);
  const uint32_t zero_first[3] = {0u, 14u, 17u}, too_large[3] = {10u, 65536u, 17u};
  CHECK(host(stand_in, field, 4, 0, 0.0, zero_first, 0u, sources, 2, no_limit, cost.data()) == VGT_HIP_ERR_INVALID_ARGUMENT);
  CHECK(host(stand_in, field, 4, 0, 0.0, too_large, 0u, sources, 2, no_limit, cost.data()) == VGT_HIP_ERR_INVALID_ARGUMENT);
  CHECK(std::strstr(vgt_hip_last_error(), "65535") != nullptr);
  CHECK(host(stand_in, field, 4, 0, 0.0, weights, 0u, sources, 2, U, cost.data()) == VGT_HIP_ERR_INVALID_ARGUMENT);
  CHECK(host(stand_in, field, 4, 0, 0.0, weights, 0u, sources, -1, no_limit, cost.data()) == VGT_HIP_ERR_INVALID_ARGUMENT);
  CHECK(vgt_hip_travel_cost_dev(stand_in, field, 4, 4, 4, 0, 1, 0.0, weights, 0u, sources, nullptr, 2, no_limit, cost.data(),
                                nullptr, nullptr, field, vgt_hip_travel_cost_workspace_bytes(4, 4, 4) - 1) ==
        VGT_HIP_ERR_INVALID_ARGUMENT);
  CHECK(std::strstr(vgt_hip_last_error(), "workspace") != nullptr);
  CHECK(vgt_hip_travel_cost_workspace_bytes(0, 4, 4) == 0 && vgt_hip_travel_cost_workspace_bytes(int64_t{1} << 31, 1, 1) == 0);
  CHECK(vgt_hip_cells_travel_cost(stand_in, nullptr, nullptr, 0, 1, weights, 0u, sources, nullptr, 2, no_limit, cost.data(),
                                  nullptr, nullptr) == VGT_HIP_ERR_INVALID_ARGUMENT);
  int32_t lengths[2] = {9, 9};
  uint8_t status[2] = {9, 9};
  CHECK(vgt_hip_trace_paths(stand_in, toward.data(), 64, sources, 2, 0, toward.data(), lengths, status) ==
        VGT_HIP_ERR_INVALID_ARGUMENT);
  CHECK(std::strstr(vgt_hip_last_error(), "max_cells") != nullptr);
  CHECK(vgt_hip_trace_paths_dev(stand_in, nullptr, 64, sources, 2, 4, toward.data(), lengths, status) ==
        VGT_HIP_ERR_INVALID_ARGUMENT);
  CHECK(reached == -7 && lengths[0] == 9 && status[1] == 9);
  CHECK(std::all_of(cost.begin(), cost.end(), [](uint32_t v) { return v == 9u; }));
  CHECK(std::all_of(toward.begin(), toward.end(), [](int32_t v) { return v == 9; }));
  // an empty grid succeeds and writes the count only
  CHECK(host(stand_in, field, 0, 0, 0.0, weights, 0u, sources, 2, no_limit, cost.data()) == VGT_HIP_OK && reached == 0);

  // the layer's own checks, all before a device is asked for
  const OccupancyMap map(Isometry3::Identity(), "f", 1.0, 3, 3, 3, 0.0f);
  const std::vector<GridIndex> one{GridIndex{0, 0, 0}};
  CHECK(ThrowsInvalidArgument([&] { ComputeTravelCost(OccupancyMap(), one); }));
  TravelCostOptions o;
  o.weights = {{0u, 1u, 1u}};
  CHECK(ThrowsInvalidArgument([&] { ComputeTravelCost(map, one, o); }));
  o = TravelCostOptions();
  o.weights = {{1u, 70000u, 1u}};
  CHECK(ThrowsInvalidArgument([&] { ComputeTravelCost(map, one, o); }));
  o = TravelCostOptions();
  o.cost_limit = U;
  CHECK(ThrowsInvalidArgument([&] { ComputeTravelCost(map, one, o); }));
  o = TravelCostOptions();
  o.source_costs = {1u, 2u};
  CHECK(ThrowsInvalidArgument([&] { ComputeTravelCost(map, one, o); }));
  o = TravelCostOptions();
  o.objects_to_use = {1u};
  CHECK(ThrowsInvalidArgument([&] { ComputeTravelCost(map, one, o); }));
  CHECK(ThrowsInvalidArgument([&] {
    ComputeTravelCost(OccupancyComponentMap(Isometry3::Identity(), "f", 1.0, 3, 3, 3, OccupancyComponentCell()), one, o);
  }));
  SignedDistanceField sdf;
  sdf.grid = map;
  CHECK(ThrowsInvalidArgument([&] { ComputeTravelCost(sdf, std::nan(""), one); }));
  TravelCostField empty_field;
  CHECK(ThrowsInvalidArgument([&] { TracePaths(empty_field, one, 4); }));
  TravelCostField small;
  small.nx = small.ny = small.nz = 1;
  small.toward = {0};
  CHECK(ThrowsInvalidArgument([&] { TracePaths(small, one, 0); }));
  CHECK(TracePaths(small, {}, 4).status.empty());
  CHECK(small.LinearIndex(GridIndex{0, 0, 1}) == -1 && small.LinearIndex(GridIndex{0, 0, 0}) == 0);
  return g_failures;
}

// A deterministic value in [0, 1) per cell.
static float Noise(int64_t i, uint32_t salt)
{
  uint32_t h = static_cast<uint32_t>(i) * 2654435761u + salt * 40503u;
  h ^= h >> 15;
  h *= 2246822519u;
  h ^= h >> 13;
  return static_cast<float>(h >> 8) / 16777216.0f;
}

static bool Same(const TravelCostField& got, const Restated& want)
{
  return got.cost == want.cost && got.toward == want.toward && got.num_reached == want.reached;
}

static int RunDevice()
{
  const Isometry3 origin = Isometry3::FromQuaternion(0.9238795325112867, 0.0, 0.3826834323650898, 0.0, 1.0, -2.0, 0.5);
  const int64_t shapes[2][3] = {{9, 7, 70}, {20, 33, 17}};
  for (const auto& shape : shapes)
  {
    const int64_t nx = shape[0], ny = shape[1], nz = shape[2], n = nx * ny * nz;
    OccupancyMap map(origin, "test_frame", 0.25, nx, ny, nz, 0.0f);
    OccupancyComponentMap component(origin, "test_frame", 0.25, nx, ny, nz, OccupancyComponentCell());
    TaggedObjectOccupancyMap tagged(origin, "test_frame", 0.25, nx, ny, nz, TaggedObjectOccupancyCell());
    TaggedObjectOccupancyComponentMap wide(origin, "test_frame", 0.25, nx, ny, nz, TaggedObjectOccupancyComponentCell());
    SignedDistanceField sdf;
    sdf.grid = DenseGrid(origin, "test_frame", 0.25, nx, ny, nz, 0.0f);
    std::vector<uint8_t> free_known(static_cast<size_t>(n)), free_unknown(static_cast<size_t>(n)),
        free_objects(static_cast<size_t>(n)), free_sdf(static_cast<size_t>(n));
    const double minimum_distance = 0.3;
    for (int64_t i = 0; i < n; i++)
    {
      const float r = Noise(i, 2);
      float occ = r < 0.6f ? 0.0f : (r < 0.7f ? 0.5f : 1.0f);
      if (i == 0 || i == n - 1) occ = 0.0f;
      const uint32_t id = static_cast<uint32_t>(i % 5);
      const size_t at = static_cast<size_t>(i);
      map.GetMutableRawData()[at] = occ;
      component.GetMutableRawData()[at] = OccupancyComponentCell{occ, id + 7u};
      tagged.GetMutableRawData()[at] = TaggedObjectOccupancyCell{occ, id};
      wide.GetMutableRawData()[at] = TaggedObjectOccupancyComponentCell{occ, id, id + 7u, 0xDEADBEEFu};
      float d = 2.0f * Noise(i, 3) - 0.4f;
      if (i % 397 == 11) d = std::numeric_limits<float>::quiet_NaN();
      if (i % 1013 == 5) d = -std::numeric_limits<float>::infinity();
      if (i % 1013 == 6) d = 0.3f;
      if (i == 0) d = 1.0f;
      sdf.grid.GetMutableRawData()[at] = d;
      free_unknown[at] = occ > 0.5f ? 0 : 1;
      free_known[at] = occ >= 0.5f ? 0 : 1;
      free_objects[at] = (occ >= 0.5f && (id == 1u || id == 3u)) ? 0 : 1;
      free_sdf[at] = static_cast<double>(d) <= minimum_distance ? 0 : 1;
    }
    const std::vector<GridIndex> sources{GridIndex{0, 0, 0}, GridIndex{nx - 1, ny - 1, nz - 1}, GridIndex{nx, 0, 0},
                                         GridIndex{0, 0, 0}};
    const std::vector<int64_t> linear{0, n - 1, -1, 0};
    TravelCostOptions o;
    o.source_costs = {5u, 0u, 0u, 3u};
    o.no_corner_cutting = true;
    const Restated want = Restate(free_known, nx, ny, nz, o.weights, true, linear, o.source_costs, o.cost_limit);
    CHECK(want.reached > n / 4);
    CHECK(Same(ComputeTravelCost(map, sources, o), want));
    CHECK(Same(ComputeTravelCost(component, sources, o), want));
    CHECK(Same(ComputeTravelCost(tagged, sources, o), want));
    CHECK(Same(ComputeTravelCost(wide, sources, o), want));
    o.unknown_is_filled = false;
    o.no_corner_cutting = false;
    o.weights = {{2u, 3u, 0u}};
    o.cost_limit = 40u;
    const Restated limited = Restate(free_unknown, nx, ny, nz, o.weights, false, linear, o.source_costs, 40u);
    CHECK(limited.reached > 0 && limited.reached < want.reached);
    CHECK(Same(ComputeTravelCost(map, sources, o), limited));
    CHECK(Same(ComputeTravelCost(wide, sources, o), limited));
    // tagged maps: only the listed objects block
    TravelCostOptions objects;
    objects.objects_to_use = {3u, 1u, 3u};
    const Restated by_object = Restate(free_objects, nx, ny, nz, objects.weights, false, {0}, {}, objects.cost_limit);
    CHECK(Same(ComputeTravelCost(tagged, {GridIndex{0, 0, 0}}, objects), by_object));
    CHECK(Same(ComputeTravelCost(wide, {GridIndex{0, 0, 0}}, objects), by_object));
    // the SDF overload: blocked at or below the distance, NaN passable
    const TravelCostOptions defaults;
    const Restated inflated = Restate(free_sdf, nx, ny, nz, defaults.weights, false, {0}, {}, defaults.cost_limit);
    CHECK(inflated.reached > n / 4);
    const TravelCostField got = ComputeTravelCost(sdf, minimum_distance, {GridIndex{0, 0, 0}});
    CHECK(Same(got, inflated));
    // cost alone
    TravelCostOptions cost_only;
    cost_only.with_toward = false;
    const TravelCostField bare = ComputeTravelCost(sdf, minimum_distance, {GridIndex{0, 0, 0}}, cost_only);
    CHECK(bare.cost == inflated.cost && bare.toward.empty() && bare.num_reached == inflated.reached);

    // paths: from the farthest reached cell, an unreached one, one outside the grid
    int64_t far = 0, blocked = -1;
    for (int64_t c = 0; c < n; c++)
    {
      if (got.cost[static_cast<size_t>(c)] != U && got.cost[static_cast<size_t>(c)] > got.cost[static_cast<size_t>(far)]) far = c;
      if (got.cost[static_cast<size_t>(c)] == U) blocked = c;
    }
    const std::vector<GridIndex> starts{got.Index(far), got.Index(blocked), GridIndex{0, -1, 0}, GridIndex{0, 0, 0}};
    const TracedPaths paths = TracePaths(got, starts, 512);
    CHECK(paths.status == (std::vector<uint8_t>{VGT_HIP_TRACE_OK, VGT_HIP_TRACE_UNREACHED, VGT_HIP_TRACE_INVALID,
                                                VGT_HIP_TRACE_OK}));
    CHECK(paths.lengths[0] > 2 && paths.lengths[1] == 0 && paths.lengths[2] == 0 && paths.lengths[3] == 1);
    CHECK(paths.cells[0] == far && paths.cells[static_cast<size_t>(paths.lengths[0] - 1)] == 0);
    for (int32_t k = 0; k + 1 < paths.lengths[0]; k++)
    {
      const size_t a = static_cast<size_t>(paths.cells[static_cast<size_t>(k)]);
      const size_t b = static_cast<size_t>(paths.cells[static_cast<size_t>(k + 1)]);
      CHECK(got.toward[a] == static_cast<int32_t>(b) && got.cost[b] < got.cost[a]);
    }
    CHECK(paths.cells[static_cast<size_t>(paths.lengths[0])] == -1);
    const TracedPaths cut = TracePaths(got, starts, 2);
    CHECK(cut.status[0] == VGT_HIP_TRACE_TRUNCATED && cut.lengths[0] == 2 && cut.status[3] == VGT_HIP_TRACE_OK);
  }
  // no sources: nothing is reached
  const TravelCostField none = ComputeTravelCost(OccupancyMap(Isometry3::Identity(), "f", 1.0, 3, 2, 5, 0.0f), {});
  CHECK(none.num_reached == 0 && std::all_of(none.cost.begin(), none.cost.end(), [](uint32_t v) { return v == U; }));
  CHECK(std::all_of(none.toward.begin(), none.toward.end(), [](int32_t v) { return v == -1; }));
  return g_failures;
}

int main(int argc, char** argv)
{
  const bool no_device = argc > 1 && std::strcmp(argv[1], "--no-device") == 0;
  const int failures = no_device ? RunNoDevice() : (RunNoDevice(), RunDevice());
  if (failures == 0) std::printf("PASSED\n");
  return failures == 0 ? 0 : 1;
}
