// ExtractNearestCells of the C++ host layer (include/vgt_hip/nearest_cells.hpp): the contract of vgt_hip_nearest_dev
// checked for every cell against a plain separable minimum search in this program.
//   test_nearest_host              needs a HIP device
//   test_nearest_host --no-device  only the argument errors that are raised before a device is touched
#include <vgt_hip.h>
#include <vgt_hip/nearest_cells.hpp>

#include <algorithm>
#include <cstdio>
#include <cstring>
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

static int RunNoDevice()
{
  CHECK(ThrowsInvalidArgument([] { ExtractNearestCells(OccupancyMap()); }));
  CHECK(ThrowsInvalidArgument([] { ExtractNearestCells(TaggedObjectOccupancyMap(), {}); }));
  CHECK(ThrowsInvalidArgument([] { ExtractNearestCells(TaggedObjectOccupancyComponentMap(), {1u}); }));
  // the C ABI rejects these before any HIP call and leaves its outputs alone (the grid stands in for a context: a
  // non-null context pointer is not dereferenced before the other checks)
  OccupancyMap map(Isometry3::Identity(), "f", 1.0, 4, 4, 4, 0.0f);
  const float* occupancy = map.GetImmutableRawData().data();
  vgt_hip_ctx* stand_in = reinterpret_cast<vgt_hip_ctx*>(const_cast<float*>(occupancy));
  std::vector<int32_t> nearest(64, 9), d2(64, 9);
  std::vector<uint8_t> workspace(1 << 16, 0);
  CHECK(vgt_hip_nearest_workspace_bytes(4, 4, 4) >= 6 * 64 && vgt_hip_nearest_workspace_bytes(4, 4, 4) <= workspace.size());
  CHECK(vgt_hip_nearest_workspace_bytes(0, 4, 4) == 0 && vgt_hip_nearest_workspace_bytes(16385, 1, 1) == 0);
  CHECK(vgt_hip_nearest_workspace_bytes(2048, 1024, 1024) == 0);
  const auto host = [&](vgt_hip_ctx* ctx, const float* occ, int64_t nx, int64_t ny, int64_t nz, int32_t* out) {
    return vgt_hip_nearest_from_occupancy_f32(ctx, occ, nx, ny, nz, 1, out, d2.data());
  };
  CHECK(host(nullptr, occupancy, 4, 4, 4, nearest.data()) == VGT_HIP_ERR_INVALID_ARGUMENT);
  CHECK(std::strstr(vgt_hip_last_error(), "null") != nullptr);
  CHECK(host(stand_in, nullptr, 4, 4, 4, nearest.data()) == VGT_HIP_ERR_INVALID_ARGUMENT);
  CHECK(host(stand_in, occupancy, 4, 4, 4, nullptr) == VGT_HIP_ERR_INVALID_ARGUMENT);
  CHECK(host(stand_in, occupancy, 4, 0, 4, nearest.data()) == VGT_HIP_ERR_INVALID_ARGUMENT);
  CHECK(std::strstr(vgt_hip_last_error(), "positive") != nullptr);
  CHECK(host(stand_in, occupancy, 16385, 1, 1, nearest.data()) == VGT_HIP_ERR_INVALID_ARGUMENT);
  CHECK(std::strstr(vgt_hip_last_error(), "16384") != nullptr);
  CHECK(host(stand_in, occupancy, 2048, 1024, 1024, nearest.data()) == VGT_HIP_ERR_INVALID_ARGUMENT);
  CHECK(std::strstr(vgt_hip_last_error(), "2^31") != nullptr);
  CHECK(vgt_hip_nearest_dev(stand_in, occupancy, 4, 4, 4, 1, nearest.data(), d2.data(), workspace.data(), 6 * 64) ==
        VGT_HIP_ERR_INVALID_ARGUMENT);
  CHECK(std::strstr(vgt_hip_last_error(), "workspace too small") != nullptr);
  CHECK(vgt_hip_nearest_dev(stand_in, occupancy, 4, 4, 4, 1, nearest.data(), d2.data(), nullptr, workspace.size()) ==
        VGT_HIP_ERR_INVALID_ARGUMENT);
  CHECK(vgt_hip_nearest_from_mask_u8(stand_in, nullptr, 4, 4, 4, nearest.data(), nullptr) == VGT_HIP_ERR_INVALID_ARGUMENT);
  CHECK(vgt_hip_cells_nearest(stand_in, nullptr, nullptr, 0, 1, nearest.data(), nullptr, nullptr) ==
        VGT_HIP_ERR_INVALID_ARGUMENT);
  CHECK(std::all_of(nearest.begin(), nearest.end(), [](int32_t v) { return v == 9; }));
  CHECK(std::all_of(d2.begin(), d2.end(), [](int32_t v) { return v == 9; }));
  CHECK(std::all_of(workspace.begin(), workspace.end(), [](uint8_t v) { return v == 0; }));
  return g_failures;
}

// Squared distance of every cell to the nearest cell of the other class, -1 where there is none: three passes of plain
// minima along the lines (no hull), once per class.
static std::vector<int64_t> ReferenceD2(const std::vector<uint8_t>& filled, int64_t nx, int64_t ny, int64_t nz)
{
  const int64_t n = nx * ny * nz, inf = int64_t{1} << 40;
  std::vector<int64_t> result(static_cast<size_t>(n), -1);
  for (int site_class = 0; site_class < 2; site_class++)
  {
    std::vector<int64_t> field(static_cast<size_t>(n)), next(static_cast<size_t>(n));
    for (int64_t i = 0; i < n; i++) field[static_cast<size_t>(i)] = filled[static_cast<size_t>(i)] == site_class ? 0 : inf;
    const int64_t extent[3] = {nx, ny, nz}, stride[3] = {ny * nz, nz, 1};
    for (int axis = 2; axis >= 0; axis--)
    {
      for (int64_t i = 0; i < n; i++)
      {
        const int64_t r = i / stride[axis] % extent[axis], first = i - r * stride[axis];
        int64_t best = inf;
        for (int64_t t = 0; t < extent[axis]; t++)
          best = std::min(best, field[static_cast<size_t>(first + t * stride[axis])] + (t - r) * (t - r));
        next[static_cast<size_t>(i)] = best;
      }
      field.swap(next);
    }
    for (int64_t i = 0; i < n; i++)
      if (filled[static_cast<size_t>(i)] != site_class && field[static_cast<size_t>(i)] < inf)
        result[static_cast<size_t>(i)] = field[static_cast<size_t>(i)];
  }
  return result;
}

// The contract for every cell; `ids`: the cells' object ids when the map is tagged (object_id is then checked too).
static void CheckNearest(const NearestCells& got, const std::vector<uint8_t>& filled, const std::vector<uint32_t>* ids,
                         int64_t nx, int64_t ny, int64_t nz)
{
  const int64_t n = nx * ny * nz;
  CHECK(static_cast<int64_t>(got.index.size()) == n && static_cast<int64_t>(got.squared_distance.size()) == n);
  CHECK(got.object_id.size() == (ids ? static_cast<size_t>(n) : 0u));
  if (static_cast<int64_t>(got.index.size()) != n || static_cast<int64_t>(got.squared_distance.size()) != n) return;
  const std::vector<int64_t> want = ReferenceD2(filled, nx, ny, nz);
  int64_t bad = 0, bad_object = 0;
  for (int64_t c = 0; c < n; c++)
  {
    const size_t i = static_cast<size_t>(c);
    const int64_t t = got.index[i];
    bool ok;
    if (want[i] < 0)
      ok = t == -1 && got.squared_distance[i] == 0x7fffffff;
    else
    {
      ok = t >= 0 && t < n && filled[static_cast<size_t>(t)] != filled[i] && got.squared_distance[i] == want[i];
      if (ok)
      {
        const int64_t dx = t / (ny * nz) - c / (ny * nz), dy = t / nz % ny - c / nz % ny, dz = t % nz - c % nz;
        ok = dx * dx + dy * dy + dz * dz == want[i];
      }
    }
    if (!ok) bad++;
    if (ids && ok && got.object_id.size() == static_cast<size_t>(n))
    {
      const uint32_t expected = filled[i] ? (*ids)[i] : (t >= 0 ? (*ids)[static_cast<size_t>(t)] : 0u);
      if (got.object_id[i] != expected) bad_object++;
    }
  }
  if (bad || bad_object) std::printf("%lld cells break the contract, %lld object ids\n", (long long)bad, (long long)bad_object);
  CHECK(bad == 0);
  CHECK(bad_object == 0);
}

static int RunDevice()
{
  const int64_t n1 = 40;
  // a scene of boxes, a few single cells and unknown cells
  OccupancyMap map(Isometry3::Translation(1.0, -2.0, 0.5), "test_frame", 0.25, n1, n1, n1, 0.0f);
  TaggedObjectOccupancyMap tagged(Isometry3::Identity(), "test_frame", 0.25, n1, n1, n1, TaggedObjectOccupancyCell());
  TaggedObjectOccupancyComponentMap tagged_component(Isometry3::Identity(), "test_frame", 0.25, n1, n1, n1,
                                                     TaggedObjectOccupancyComponentCell());
  const int boxes[3][6] = {{3, 11, 4, 9, 5, 30}, {20, 35, 18, 22, 2, 9}, {14, 18, 28, 39, 20, 38}};
  for (int b = 0; b < 3; b++)
    for (int x = boxes[b][0]; x < boxes[b][1]; x++)
      for (int y = boxes[b][2]; y < boxes[b][3]; y++)
        for (int z = boxes[b][4]; z < boxes[b][5]; z++)
        {
          map.SetIndex(x, y, z, 1.0f);
          tagged.SetIndex(x, y, z, TaggedObjectOccupancyCell{1.0f, static_cast<uint32_t>(b + 1)});
          tagged_component.SetIndex(x, y, z, TaggedObjectOccupancyComponentCell{1.0f, static_cast<uint32_t>(b + 1), 7u, 9u});
        }
  for (int k = 0; k < 12; k++)
  {
    const int x = (k * 17 + 5) % 40, y = (k * 11 + 30) % 40, z = (k * 29 + 3) % 40;
    map.SetIndex(x, y, z, k % 3 == 0 ? 0.5f : 1.0f);
    tagged.SetIndex(x, y, z, TaggedObjectOccupancyCell{k % 3 == 0 ? 0.5f : 1.0f, 0u});
    tagged_component.SetIndex(x, y, z, TaggedObjectOccupancyComponentCell{k % 3 == 0 ? 0.5f : 1.0f, 0u, 0u, 0u});
  }
  const size_t n = static_cast<size_t>(n1 * n1 * n1);
  for (const bool unknown_is_filled : {true, false})
  {
    std::vector<uint8_t> filled(n);
    for (size_t i = 0; i < n; i++)
    {
      const float occ = map.GetImmutableRawData()[i];
      filled[i] = occ > 0.5f || (unknown_is_filled && occ == 0.5f);
    }
    const NearestCells got = ExtractNearestCells(map, unknown_is_filled);
    CheckNearest(got, filled, nullptr, n1, n1, n1);
    const NearestCells again = ExtractNearestCells(map, unknown_is_filled);
    CHECK(again.index == got.index && again.squared_distance == got.squared_distance);
  }
  // tagged: every object, then objects 1 and 3 only
  std::vector<uint32_t> ids(n);
  for (size_t i = 0; i < n; i++) ids[i] = tagged.GetImmutableRawData()[i].object_id;
  for (const std::vector<uint32_t>& objects : {std::vector<uint32_t>{}, std::vector<uint32_t>{3u, 1u}})
  {
    std::vector<uint8_t> filled(n);
    for (size_t i = 0; i < n; i++)
    {
      const TaggedObjectOccupancyCell& cell = tagged.GetImmutableRawData()[i];
      filled[i] = cell.occupancy >= 0.5f &&
                  (objects.empty() || std::find(objects.begin(), objects.end(), cell.object_id) != objects.end());
    }
    const NearestCells got = ExtractNearestCells(tagged, objects);
    CheckNearest(got, filled, &ids, n1, n1, n1);
    const NearestCells wide = ExtractNearestCells(tagged_component, objects);
    CHECK(wide.index == got.index && wide.squared_distance == got.squared_distance && wide.object_id == got.object_id);
  }
  // a map of one class
  const NearestCells none = ExtractNearestCells(OccupancyMap(Isometry3::Identity(), "f", 1.0, 3, 2, 5, 0.0f));
  CHECK(std::all_of(none.index.begin(), none.index.end(), [](int32_t v) { return v == -1; }));
  CHECK(std::all_of(none.squared_distance.begin(), none.squared_distance.end(), [](int32_t v) { return v == 0x7fffffff; }));
  return g_failures;
}

int main(int argc, char** argv)
{
  const bool no_device = argc > 1 && std::strcmp(argv[1], "--no-device") == 0;
  const int failures = no_device ? RunNoDevice() : (RunNoDevice(), RunDevice());
  if (failures == 0) std::printf("PASSED\n");
  return failures == 0 ? 0 : 1;
}
