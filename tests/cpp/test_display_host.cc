// SurfaceIndices, the display exports and ExtractComponentSurfaces of the C++ host layer
// (include/vgt_hip/hip_pointcloud_voxelizer.hpp) against plain triple loops coded here: ExportVoxelGridToRViz's loop
// (ros_interface.hpp:92-148) with the colour function applied to every cell, and IsSurfaceIndex's literal loop.
//   test_display_host [nx ny nz resolution x0 x1 y0 y1 z0 z1]   needs a HIP device; the arguments describe the SDF
//                                                                scene (a filled box on a free grid), which
//                                                                tests/test_cpp_display.py takes from
//                                                                tests/golden/sdf_reference_kats.json
//   test_display_host --no-device                               only the argument errors raised before a device is touched
#include <vgt_hip.h>
#include <vgt_hip/hip_pointcloud_voxelizer.hpp>

#include <cmath>
#include <cstdio>
#include <cstdlib>
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

static float OccupancyOf(float cell) { return cell; }
template <typename Cell>
static float OccupancyOf(const Cell& cell)
{
  return cell.occupancy;
}

// IsSurfaceIndex, S/occupancy_map.cpp:201-246
template <typename Map>
static bool IsSurfaceIndex(const Map& map, int64_t x, int64_t y, int64_t z)
{
  const float our = OccupancyOf(map.GetIndexImmutable(x, y, z));
  const int64_t min_x = std::max<int64_t>(0, x - 1), max_x = std::min(map.NumXVoxels() - 1, x + 1);
  const int64_t min_y = std::max<int64_t>(0, y - 1), max_y = std::min(map.NumYVoxels() - 1, y + 1);
  const int64_t min_z = std::max<int64_t>(0, z - 1), max_z = std::min(map.NumZVoxels() - 1, z + 1);
  for (int64_t xi = min_x; xi <= max_x; xi++)
    for (int64_t yi = min_y; yi <= max_y; yi++)
      for (int64_t zi = min_z; zi <= max_z; zi++)
      {
        if (xi == x && yi == y && zi == z) continue;
        const float other = OccupancyOf(map.GetIndexImmutable(xi, yi, zi));
        if (our < 0.5 && other >= 0.5) return true;
        if (our > 0.5 && other <= 0.5) return true;
        if (our == 0.5 && other != 0.5) return true;
      }
  return false;
}

// ExportVoxelGridToRViz: every cell in X, Y, Z order, coloured, kept when alpha > 0
template <typename Map, typename ColorFn>
static DisplayCubes LoopExport(const Map& map, const ColorFn& color_fn)
{
  DisplayCubes cubes;
  for (int64_t x = 0; x < map.NumXVoxels(); x++)
    for (int64_t y = 0; y < map.NumYVoxels(); y++)
      for (int64_t z = 0; z < map.NumZVoxels(); z++)
      {
        const ColorRGBA color = color_fn(map.GetIndexImmutable(x, y, z), x, y, z);
        if (color[3] > 0.0f)
        {
          cubes.points.push_back({(static_cast<double>(x) + 0.5) * map.Resolution(),
                                  (static_cast<double>(y) + 0.5) * map.Resolution(),
                                  (static_cast<double>(z) + 0.5) * map.Resolution()});
          cubes.colors.push_back(color);
        }
      }
  return cubes;
}

static bool Same(const DisplayCubes& a, const DisplayCubes& b)
{
  return a.points.size() == a.colors.size() && a.points == b.points && a.colors == b.colors;
}

static const ColorRGBA kRed{{1.0f, 0.0f, 0.0f, 1.0f}}, kGreen{{0.0f, 1.0f, 0.0f, 0.25f}}, kGrey{{0.5f, 0.5f, 0.5f, 0.5f}};
static const ColorRGBA kNone{{0.0f, 0.0f, 0.0f, 0.0f}}, kNegative{{1.0f, 1.0f, 1.0f, -1.0f}};

template <typename Map>
static void CheckOccupancyExports(const Map& map, const char* what)
{
  // colours with alpha > 0, == 0 and < 0 in every position
  const ColorRGBA sets[][3] = {{kRed, kGreen, kGrey},   {kRed, kNone, kNone},     {kNone, kGreen, kNone},
                               {kNone, kNone, kGrey},   {kRed, kNegative, kGrey}, {kNone, kNone, kNegative},
                               {kNegative, kGreen, kGrey}};
  for (const auto& set : sets)
  {
    const auto by_class = [&](float occupancy) {
      return occupancy > 0.5 ? set[0] : (occupancy < 0.5 ? set[1] : set[2]);
    };
    const DisplayCubes all = LoopExport(map, [&](const auto& cell, int64_t, int64_t, int64_t) {
      return by_class(OccupancyOf(cell));
    });
    const DisplayCubes surfaces = LoopExport(map, [&](const auto& cell, int64_t x, int64_t y, int64_t z) {
      return IsSurfaceIndex(map, x, y, z) ? by_class(OccupancyOf(cell)) : kNone;
    });
    if (!Same(ExportForDisplay(map, set[0], set[1], set[2]), all))
    {
      std::printf("ExportForDisplay differs (%s)\n", what);
      CHECK(!"ExportForDisplay");
    }
    if (!Same(ExportSurfacesForDisplay(map, set[0], set[1], set[2]), surfaces))
    {
      std::printf("ExportSurfacesForDisplay differs (%s)\n", what);
      CHECK(!"ExportSurfacesForDisplay");
    }
  }
  const std::array<DisplayCubes, 3> separate = ExportForSeparateDisplay(map, kRed, kGreen, kGrey);
  CHECK(Same(separate[0], ExportForDisplay(map, kRed, kNone, kNone)));
  CHECK(Same(separate[1], ExportForDisplay(map, kNone, kGreen, kNone)));
  CHECK(Same(separate[2], ExportForDisplay(map, kNone, kNone, kGrey)));
  CHECK(separate[0].points.size() + separate[1].points.size() + separate[2].points.size() ==
        map.GetImmutableRawData().size());
  // SurfaceIndices against the literal loop
  GridIndices want;
  for (int64_t x = 0; x < map.NumXVoxels(); x++)
    for (int64_t y = 0; y < map.NumYVoxels(); y++)
      for (int64_t z = 0; z < map.NumZVoxels(); z++)
        if (IsSurfaceIndex(map, x, y, z)) want.push_back({x, y, z});
  CHECK(SurfaceIndices(map) == want);
  CHECK(!want.empty() && want.size() < map.GetImmutableRawData().size());
}

static ColorRGBA Palette(uint32_t component)
{
  // a palette with a transparent entry: every third component is not displayed
  const float v = static_cast<float>(component % 7) / 7.0f;
  return ColorRGBA{{v, 1.0f - v, 0.25f, component % 3 == 0 ? 0.0f : 1.0f}};
}

template <typename Map>
static void CheckComponentExports(const Map& map)
{
  for (const bool color_unknown : {false, true})
  {
    const DisplayCubes want = LoopExport(map, [&](const auto& cell, int64_t, int64_t, int64_t) {
      if (cell.occupancy != 0.5) return Palette(cell.component);
      return color_unknown ? Palette(cell.component) : ColorRGBA{{0.5f, 0.5f, 0.5f, 1.0f}};
    });
    CHECK(Same(ExportConnectedComponentsForDisplay(map, color_unknown, Palette), want));
    CHECK(!want.points.empty());
    // (with the palette alone some components are transparent)
    if (color_unknown) CHECK(want.points.size() < map.GetImmutableRawData().size());
  }
  CHECK(ThrowsInvalidArgument([&] { ExportConnectedComponentsForDisplay(map, true, ComponentPalette()); }));
  // ExtractComponentSurfaces against the dense mask of the C ABI sorted into lists here (the route it took before)
  const auto& data = map.GetImmutableRawData();
  std::vector<float> occupancy(data.size());
  std::vector<uint32_t> labels(data.size());
  for (size_t i = 0; i < data.size(); i++)
  {
    occupancy[i] = data[i].occupancy;
    labels[i] = data[i].component;
  }
  vgt_hip_ctx* ctx = nullptr;
  CHECK(vgt_hip_create(0, -1, &ctx) == VGT_HIP_OK);
  const int64_t ny = map.NumYVoxels(), nz = map.NumZVoxels();
  for (int types = 1; types <= 7; types++)
  {
    std::vector<uint8_t> mask(data.size());
    CHECK(vgt_hip_component_surface_mask(ctx, occupancy.data(), labels.data(), map.NumXVoxels(), ny, nz, types,
                                         mask.data()) == VGT_HIP_OK);
    ComponentSurfaces want;
    for (size_t i = 0; i < mask.size(); i++)
      if (mask[i])
      {
        const int64_t index = static_cast<int64_t>(i);
        want[labels[i]].push_back({index / (ny * nz), (index / nz) % ny, index % nz});
      }
    CHECK(ExtractComponentSurfaces(map, static_cast<uint8_t>(types)) == want);
    CHECK(!want.empty());
  }
  vgt_hip_destroy(ctx);
}

static void CheckSdfExports(const SignedDistanceField& sdf)
{
  for (const float alpha : {0.01f, 0.5f, 1.0f, 7.0f, 0.0f, -1.0f})
  {
    const float clamped = alpha < 0.0f ? 0.0f : (alpha > 1.0f ? 1.0f : alpha);
    const auto scale_color_value = [](float distance, float distance_extrema) {
      const float distance_ratio = static_cast<float>(std::abs(distance / distance_extrema));
      return (distance_ratio * 0.8f) + 0.2f;
    };
    const DisplayCubes want = LoopExport(sdf.grid, [&](float distance, int64_t, int64_t, int64_t) {
      ColorRGBA color{{0.0f, 0.0f, 0.0f, clamped}};
      if (distance > 0.0)
        color[1] = scale_color_value(distance, sdf.maximum);
      else if (distance < 0.0)
        color[0] = scale_color_value(distance, sdf.minimum);
      else
        color[2] = 1.0f;
      return color;
    });
    CHECK(Same(ExportSDFForDisplay(sdf, alpha), want));
    CHECK(want.points.size() == (clamped > 0.0f ? sdf.grid.GetImmutableRawData().size() : 0u));
    const DisplayCubes collision = LoopExport(sdf.grid, [&](float distance, int64_t, int64_t, int64_t) {
      return distance <= 0.0 ? ColorRGBA{{1.0f, 0.0f, 0.0f, alpha}} : kNone;
    });
    CHECK(Same(ExportSDFForDisplayCollisionOnly(sdf, alpha), collision));
  }
}

static uint32_t Mix(uint32_t v)
{
  v ^= v >> 16;
  v *= 0x7feb352dU;
  v ^= v >> 15;
  v *= 0x846ca68bU;
  v ^= v >> 16;
  return v;
}

// the grid pointcloud_voxelization_test.cpp expects from its two cameras (test/pointcloud_voxelization_test.cpp:84-158):
// a filled floor, free space in front of the two walls, the walls, unknown space behind them
static float VoxelizedScene(int64_t x, int64_t y, int64_t z)
{
  if (z == 0) return 1.0f;
  if ((x == 4 && y >= 4) || (y == 4 && x >= 4)) return 1.0f;
  if (x >= 5 && y >= 5) return 0.5f;
  return 0.0f;
}

// blobs of filled and unknown cells and a NaN, on lines that are no multiple of a wave
static float BlobScene(int64_t x, int64_t y, int64_t z)
{
  const uint32_t h = Mix(static_cast<uint32_t>((x / 2) * 73856093 ^ (y / 3) * 19349663 ^ (z / 2) * 83492791));
  if (x == 5 && y == 4 && z == 3) return std::nanf("");
  return (h % 7 < 2) ? 1.0f : ((h % 7 == 2) ? 0.5f : 0.0f);
}

template <typename SceneFn>
static void CheckScene(int64_t nx, int64_t ny, int64_t nz, double resolution, const SceneFn& scene, const char* what)
{
  const Isometry3 origin = Isometry3::Translation(-1.0, -1.0, -1.0);
  OccupancyMap plain(origin, "world", resolution, nx, ny, nz, 0.0f);
  OccupancyComponentMap component(origin, "world", resolution, nx, ny, nz, OccupancyComponentCell());
  TaggedObjectOccupancyMap tagged(origin, "world", resolution, nx, ny, nz, TaggedObjectOccupancyCell());
  TaggedObjectOccupancyComponentMap tagged_component(origin, "world", resolution, nx, ny, nz,
                                                     TaggedObjectOccupancyComponentCell());
  for (int64_t x = 0; x < nx; x++)
    for (int64_t y = 0; y < ny; y++)
      for (int64_t z = 0; z < nz; z++)
      {
        const float occupancy = scene(x, y, z);
        const uint32_t object = Mix(static_cast<uint32_t>((x / 4) * 31 + (y / 4) * 17 + (z / 4) * 7 + 1)) % 3;
        plain.SetIndex(x, y, z, occupancy);
        component.SetIndex(x, y, z, OccupancyComponentCell{occupancy, 0u});
        tagged.SetIndex(x, y, z, TaggedObjectOccupancyCell{occupancy, object});
        tagged_component.SetIndex(x, y, z, TaggedObjectOccupancyComponentCell{occupancy, object, 0u, 0xdeadbeefu});
      }
  CHECK(UpdateConnectedComponents(component) > 1);
  CHECK(UpdateConnectedComponents(tagged_component, false) > 1);
  CheckOccupancyExports(plain, what);
  CheckOccupancyExports(component, what);
  CheckOccupancyExports(tagged, what);
  CheckOccupancyExports(tagged_component, what);
  CheckComponentExports(component);
  CheckComponentExports(tagged_component);
}

static int RunNoDevice()
{
  CHECK(ThrowsInvalidArgument([] { SurfaceIndices(OccupancyMap()); }));
  CHECK(ThrowsInvalidArgument([] { SurfaceIndices(OccupancyComponentMap()); }));
  CHECK(ThrowsInvalidArgument([] { SurfaceIndices(TaggedObjectOccupancyMap()); }));
  CHECK(ThrowsInvalidArgument([] { SurfaceIndices(TaggedObjectOccupancyComponentMap()); }));
  CHECK(ThrowsInvalidArgument([] { ExportForDisplay(OccupancyMap(), kRed, kGreen, kGrey); }));
  CHECK(ThrowsInvalidArgument([] { ExportSurfacesForDisplay(TaggedObjectOccupancyMap(), kRed, kGreen, kGrey); }));
  CHECK(ThrowsInvalidArgument([] { ExportForSeparateDisplay(OccupancyComponentMap(), kRed, kGreen, kGrey); }));
  CHECK(ThrowsInvalidArgument([] { ExportConnectedComponentsForDisplay(OccupancyComponentMap(), true, Palette); }));
  CHECK(ThrowsInvalidArgument([] { ExportSDFForDisplay(SignedDistanceField()); }));
  CHECK(ThrowsInvalidArgument([] { ExportSDFForDisplayCollisionOnly(SignedDistanceField()); }));
  CHECK(ThrowsInvalidArgument([] { ExtractComponentSurfaces(OccupancyComponentMap(), FILLED_COMPONENTS); }));
  // no colour with alpha > 0: nothing to select, no device needed
  const OccupancyMap map(Isometry3::Identity(), "f", 0.5, 3, 3, 3, 1.0f);
  CHECK(ExportForDisplay(map, kNone, kNegative, kNone).points.empty());
  CHECK(ExportSurfacesForDisplay(map, kNone, kNone, kNone).colors.empty());
  SignedDistanceField sdf;
  sdf.grid = map;
  CHECK(ExportSDFForDisplay(sdf, 0.0f).points.empty() && ExportSDFForDisplayCollisionOnly(sdf, -1.0f).points.empty());
  // the C ABI rejects bad arguments before any HIP call
  int64_t count = -7;
  float value = 0.0f;
  CHECK(vgt_hip_select_cells(nullptr, &value, nullptr, 1, 1, 1, VGT_HIP_SELECT_ALL, 15, 0.5f, nullptr, nullptr, nullptr, 0,
                             &count) == VGT_HIP_ERR_INVALID_ARGUMENT);
  CHECK(vgt_hip_cells_select(nullptr, nullptr, nullptr, VGT_HIP_SELECT_ALL, 15, nullptr, nullptr, nullptr,
                             VGT_HIP_CELL_MEMBER_NONE, 0, &count) == VGT_HIP_ERR_INVALID_ARGUMENT);
  CHECK(count == -7);
  return g_failures;
}

static int RunDevice(int argc, char** argv)
{
  CheckScene(8, 8, 8, 0.25, VoxelizedScene, "voxelized 8^3");
  CheckScene(9, 7, 67, 0.125, BlobScene, "blobs 9x7x67");
  // the SDF scene: CenterObstacle of the reference's sdf_generation_test.cpp unless the command line says otherwise
  int64_t dims[9] = {4, 8, 12, 1, 3, 2, 6, 3, 9};
  double resolution = 0.25;
  if (argc == 11)
  {
    for (int k = 0; k < 3; k++) dims[k] = std::atoll(argv[1 + k]);
    resolution = std::atof(argv[4]);
    for (int k = 0; k < 6; k++) dims[3 + k] = std::atoll(argv[5 + k]);
  }
  OccupancyMap map(Isometry3::Identity(), "world", resolution, dims[0], dims[1], dims[2], 0.0f);
  for (int64_t x = dims[3]; x < dims[4]; x++)
    for (int64_t y = dims[5]; y < dims[6]; y++)
      for (int64_t z = dims[7]; z < dims[8]; z++) map.SetIndex(x, y, z, 1.0f);
  SignedDistanceField sdf = ExtractSignedDistanceField(map, SignedDistanceFieldGenerationParameters());
  CHECK(sdf.IsLocked() && sdf.minimum < 0.0f && sdf.maximum > 0.0f);
  CheckSdfExports(sdf);
  // zeros of both signs and a NaN; an unlocked field's extrema are those of its values
  sdf.grid.SetIndex(0, 0, 0, 0.0f);
  sdf.grid.SetIndex(0, 0, 1, -0.0f);
  sdf.grid.SetIndex(0, 1, 0, std::nanf(""));
  CheckSdfExports(sdf);
  SignedDistanceField unlocked = sdf;
  unlocked.locked = false;
  unlocked.minimum = unlocked.maximum = 123.0f;
  CHECK(Same(ExportSDFForDisplay(unlocked, 0.5f), ExportSDFForDisplay(sdf, 0.5f)));
  return g_failures;
}

int main(int argc, char** argv)
{
  const bool no_device = argc > 1 && std::strcmp(argv[1], "--no-device") == 0;
  const int failures = no_device ? RunNoDevice() : (RunNoDevice(), RunDevice(argc, argv));
  if (failures == 0) std::printf("PASSED\n");
  return failures == 0 ? 0 : 1;
}
