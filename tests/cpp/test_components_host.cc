// The component entry points of the C++ host layer (include/vgt_hip/hip_pointcloud_voxelizer.hpp) against a flood fill
// coded here: the reference's ComputeConnectedComponents (topology_computation.hpp:59-196) -- start cells in X-major
// order, a FIFO queue, the six face neighbours.
//   test_components_host              needs a HIP device
//   test_components_host --no-device  only the argument errors that are raised before a device is touched
#include <vgt_hip.h>
#include <vgt_hip/hip_pointcloud_voxelizer.hpp>

#include <cmath>
#include <cstdio>
#include <cstring>
#include <deque>
#include <functional>
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

// labels[i] = 0 for inactive cells, else the component number; returns the number of components
static uint32_t FloodFill(int64_t nx, int64_t ny, int64_t nz, const std::function<bool(int64_t)>& active,
                          const std::function<bool(int64_t, int64_t)>& connected, std::vector<uint32_t>& labels)
{
  const int64_t total = nx * ny * nz;
  labels.assign(static_cast<size_t>(total), 0u);
  std::vector<uint8_t> queued(static_cast<size_t>(total), 0);
  uint32_t count = 0;
  for (int64_t start = 0; start < total; start++)
  {
    if (!active(start) || labels[static_cast<size_t>(start)] != 0u) continue;
    count++;
    std::deque<int64_t> queue{start};
    queued[static_cast<size_t>(start)] = 1;
    while (!queue.empty())
    {
      const int64_t cur = queue.front();
      queue.pop_front();
      labels[static_cast<size_t>(cur)] = count;
      const int64_t x = cur / (ny * nz), y = (cur / nz) % ny, z = cur % nz;
      const int64_t nb[6] = {x > 0 ? cur - ny * nz : -1, x + 1 < nx ? cur + ny * nz : -1, y > 0 ? cur - nz : -1,
                             y + 1 < ny ? cur + nz : -1,  z > 0 ? cur - 1 : -1,          z + 1 < nz ? cur + 1 : -1};
      for (const int64_t n : nb)
      {
        if (n < 0 || !active(n) || labels[static_cast<size_t>(n)] != 0u || queued[static_cast<size_t>(n)]) continue;
        if (!connected(cur, n)) continue;
        queued[static_cast<size_t>(n)] = 1;
        queue.push_back(n);
      }
    }
  }
  return count;
}

static bool SameClass(float a, float b)
{
  return (a > 0.5f && b > 0.5f) || (a < 0.5f && b < 0.5f) || (a == 0.5f && b == 0.5f);
}

// a deterministic scene: blobs of filled / unknown cells, a NaN, object ids in blocks
static uint32_t Mix(uint32_t v)
{
  v ^= v >> 16;
  v *= 0x7feb352dU;
  v ^= v >> 15;
  v *= 0x846ca68bU;
  v ^= v >> 16;
  return v;
}
static float SceneOccupancy(int64_t x, int64_t y, int64_t z)
{
  const uint32_t h = Mix(static_cast<uint32_t>((x / 2) * 73856093 ^ (y / 3) * 19349663 ^ (z / 2) * 83492791));
  if (x == 5 && y == 4 && z == 3) return std::nanf("");
  return (h % 7 < 2) ? 1.0f : ((h % 7 == 2) ? 0.5f : 0.0f);
}
static uint32_t SceneObject(int64_t x, int64_t y, int64_t z)
{
  return Mix(static_cast<uint32_t>((x / 4) * 31 + (y / 4) * 17 + (z / 4) * 7 + 1)) % 3;
}

static int RunNoDevice()
{
  CHECK(ThrowsInvalidArgument([] { OccupancyComponentMap m; UpdateConnectedComponents(m); }));
  CHECK(ThrowsInvalidArgument([] { TaggedObjectOccupancyComponentMap m; UpdateConnectedComponents(m, false); }));
  CHECK(ThrowsInvalidArgument([] {
    TaggedObjectOccupancyComponentMap m;
    UpdateSpatialSegments(m, 1.0, SignedDistanceFieldGenerationParameters());
  }));
  TaggedObjectOccupancyComponentMap tagged(Isometry3::Identity(), "f", 0.5, 3, 3, 3, TaggedObjectOccupancyComponentCell());
  CHECK(ThrowsInvalidArgument([&] { UpdateSpatialSegments(tagged, -1.0, SignedDistanceFieldGenerationParameters()); }));
  CHECK(ThrowsInvalidArgument([&] { UpdateSpatialSegments(tagged, std::nan(""), SignedDistanceFieldGenerationParameters()); }));
  CHECK(ThrowsInvalidArgument([] { ExtractComponentSurfaces(OccupancyComponentMap(), FILLED_COMPONENTS); }));
  CHECK(ThrowsInvalidArgument([] { ExtractComponentSurfaces(TaggedObjectOccupancyComponentMap(), FILLED_COMPONENTS); }));
  OccupancyComponentMap plain(Isometry3::Identity(), "f", 0.5, 3, 3, 3, OccupancyComponentCell());
  CHECK(ThrowsInvalidArgument([&] { ExtractComponentSurfaces(plain, 0); }));
  CHECK(ThrowsInvalidArgument([&] { ExtractComponentSurfaces(tagged, 8); }));
  // the C ABI rejects the same before any HIP call
  uint32_t count = 0, label = 0;
  float occupancy = 0.0f;
  CHECK(vgt_hip_connected_components(nullptr, &occupancy, 1, 1, 1, &label, &count) == VGT_HIP_ERR_INVALID_ARGUMENT);
  CHECK(vgt_hip_connected_components(nullptr, &occupancy, 0, 1, 1, &label, &count) == VGT_HIP_ERR_INVALID_ARGUMENT);
  CHECK(std::strstr(vgt_hip_last_error(), "positive") != nullptr);
  return g_failures;
}

template <typename Map>
static void CheckSurfaces(const Map& map, int64_t nx, int64_t ny, int64_t nz)
{
  const auto& data = map.GetImmutableRawData();
  const auto index = [&](int64_t x, int64_t y, int64_t z) { return static_cast<size_t>((x * ny + y) * nz + z); };
  for (int types = 1; types <= 7; types++)
  {
    const ComponentSurfaces surfaces = ExtractComponentSurfaces(map, static_cast<uint8_t>(types));
    std::vector<uint8_t> listed(data.size(), 0);
    for (const auto& kv : surfaces)
    {
      int64_t previous = -1;
      for (const auto& cell : kv.second)
      {
        const size_t i = index(cell[0], cell[1], cell[2]);
        CHECK(static_cast<int64_t>(i) > previous);  // ascending linear order
        previous = static_cast<int64_t>(i);
        CHECK(data[i].component == kv.first);
        listed[i] = 1;
      }
    }
    for (int64_t x = 0; x < nx; x++)
      for (int64_t y = 0; y < ny; y++)
        for (int64_t z = 0; z < nz; z++)
        {
          const size_t i = index(x, y, z);
          const float o = data[i].occupancy;
          const int bit = o > 0.5f ? 1 : (o < 0.5f ? 2 : 4);
          bool surface = x == 0 || y == 0 || z == 0 || x == nx - 1 || y == ny - 1 || z == nz - 1;
          if (!surface)
          {
            const uint32_t own = data[i].component;
            surface = data[index(x, y, z - 1)].component != own || data[index(x, y, z + 1)].component != own ||
                      data[index(x, y - 1, z)].component != own || data[index(x, y + 1, z)].component != own ||
                      data[index(x - 1, y, z)].component != own || data[index(x + 1, y, z)].component != own;
          }
          if (listed[i] != (((types & bit) && surface) ? 1 : 0))
          {
            CHECK(!"surface list differs from the rule");
            return;
          }
        }
  }
}

static int RunDevice()
{
  const int64_t nx = 13, ny = 11, nz = 70;
  const double res = 0.25;
  OccupancyComponentMap plain(Isometry3::Translation(-1.0, 0.5, 0.0), "f", res, nx, ny, nz, OccupancyComponentCell());
  TaggedObjectOccupancyComponentMap tagged(Isometry3::Translation(-1.0, 0.5, 0.0), "f", res, nx, ny, nz,
                                           TaggedObjectOccupancyComponentCell());
  for (int64_t x = 0; x < nx; x++)
    for (int64_t y = 0; y < ny; y++)
      for (int64_t z = 0; z < nz; z++)
      {
        OccupancyComponentCell a;
        a.occupancy = SceneOccupancy(x, y, z);
        a.component = 12345u;
        plain.SetIndex(x, y, z, a);
        TaggedObjectOccupancyComponentCell b;
        b.occupancy = a.occupancy;
        b.object_id = SceneObject(x, y, z);
        b.component = 777u;
        b.spatial_segment = 0xdeadbeefu;
        tagged.SetIndex(x, y, z, b);
      }
  const auto& pd = plain.GetImmutableRawData();
  const auto& td = tagged.GetImmutableRawData();
  const auto all = [](int64_t) { return true; };
  std::vector<uint32_t> want;

  // OccupancyComponentMap::UpdateConnectedComponents
  uint32_t want_count = FloodFill(nx, ny, nz, all, [&](int64_t a, int64_t b) {
    return SameClass(pd[static_cast<size_t>(a)].occupancy, pd[static_cast<size_t>(b)].occupancy);
  }, want);
  CHECK(UpdateConnectedComponents(plain) == want_count);
  CHECK(want_count > 3);
  for (size_t i = 0; i < pd.size(); i++)
    if (pd[i].component != want[i])
    {
      CHECK(!"component differs (OccupancyComponentMap)");
      break;
    }
  CheckSurfaces(plain, nx, ny, nz);

  // TaggedObjectOccupancyComponentMap::UpdateConnectedComponents, both ways
  for (const bool across : {true, false})
  {
    want_count = FloodFill(nx, ny, nz, all, [&](int64_t a, int64_t b) {
      const auto& ca = td[static_cast<size_t>(a)];
      const auto& cb = td[static_cast<size_t>(b)];
      return SameClass(ca.occupancy, cb.occupancy) && (across || ca.object_id == cb.object_id);
    }, want);
    CHECK(UpdateConnectedComponents(tagged, across) == want_count);
    for (size_t i = 0; i < td.size(); i++)
      if (td[i].component != want[i] || td[i].spatial_segment != 0xdeadbeefu)
      {
        CHECK(!"component differs (TaggedObjectOccupancyComponentMap)");
        break;
      }
  }
  CheckSurfaces(tagged, nx, ny, nz);

  // UpdateSpatialSegments: the flood fill runs on the extrema map the layer itself computes for the same field
  for (const bool border : {false, true})
    for (const double factor : {0.5, 1.75, 3.3, 1.0e6})
    {
      SignedDistanceFieldGenerationParameters params;
      params.add_virtual_border = border;
      const DeviceTaggedObjectMap device_map(tagged);
      const SignedDistanceField sdf = border ? device_map.ExtractSignedDistanceField({}, params)
                                             : device_map.ExtractFreeAndNamedObjectsSignedDistanceField(params);
      const std::vector<double> extrema = ComputeLocalExtremaMap(sdf);
      const double threshold = factor * res;
      const auto active = [&](int64_t i) {
        const auto& c = td[static_cast<size_t>(i)];
        const double* e = &extrema[static_cast<size_t>(3 * i)];
        return (c.occupancy < 0.5f || c.object_id > 0u) && !std::isinf(e[0]) && !std::isinf(e[1]) && !std::isinf(e[2]);
      };
      want_count = FloodFill(nx, ny, nz, active, [&](int64_t a, int64_t b) {
        if (td[static_cast<size_t>(a)].object_id != td[static_cast<size_t>(b)].object_id) return false;
        const double* ea = &extrema[static_cast<size_t>(3 * a)];
        const double* eb = &extrema[static_cast<size_t>(3 * b)];
        const double dx = ea[0] - eb[0], dy = ea[1] - eb[1], dz = ea[2] - eb[2];
        return std::sqrt((dx * dx + dy * dy) + dz * dz) < threshold;
      }, want);
      const std::vector<uint32_t> components_before = [&] {
        std::vector<uint32_t> c;
        for (const auto& cell : td) c.push_back(cell.component);
        return c;
      }();
      CHECK(UpdateSpatialSegments(tagged, threshold, params) == want_count);
      const ComponentLabels again = device_map.SpatialSegments(threshold, params);
      CHECK(again.count == want_count && again.labels == want);
      for (size_t i = 0; i < td.size(); i++)
        if (td[i].spatial_segment != want[i] || td[i].component != components_before[i])
        {
          CHECK(!"spatial segment differs");
          break;
        }
    }
  return g_failures;
}

int main(int argc, char** argv)
{
  const bool no_device = argc > 1 && std::strcmp(argv[1], "--no-device") == 0;
  const int failures = no_device ? RunNoDevice() : (RunNoDevice(), RunDevice());
  if (failures == 0) std::printf("PASSED\n");
  return failures == 0 ? 0 : 1;
}
