// The mesh rasterizer of the C++ host layer (include/vgt_hip/mesh_rasterizer.hpp): the two cases of the reference's
// test/mesh_rasterization_test.cpp (TestOccupancyMap, TestOccupancyComponentMap) and the reference's two exceptions.
//   test_mesh_host              needs a HIP device
//   test_mesh_host --no-device  only the errors that are raised before a device is touched
#include <vgt_hip.h>
#include <vgt_hip/hip_pointcloud_voxelizer.hpp>  // ReleaseCachedDeviceMemory
#include <vgt_hip/mesh_rasterizer.hpp>

#include <cstdio>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

using namespace vgt_hip;
using mesh_rasterizer::Vector3d;
using mesh_rasterizer::Vector3i;

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

template <typename Fn>
static std::string RuntimeErrorMessage(const Fn& fn)
{
  try
  {
    fn();
  }
  catch (const std::invalid_argument&)
  {
    return "(invalid_argument)";
  }
  catch (const std::runtime_error& e)
  {
    return e.what();
  }
  return "";
}

static float Occupancy(const OccupancyMap& map, int64_t x, int64_t y, int64_t z) { return map.GetIndexImmutable(x, y, z); }
static float Occupancy(const OccupancyComponentMap& map, int64_t x, int64_t y, int64_t z)
{
  return map.GetIndexImmutable(x, y, z).occupancy;
}

// the expectations of test/mesh_rasterization_test.cpp:38-65
template <typename Map>
static void CheckReferenceTriangle(const Map& map)
{
  CHECK(map.NumXVoxels() == 10 && map.NumYVoxels() == 10 && map.NumZVoxels() == 2);
  for (int64_t x = 0; x < map.NumXVoxels(); x++)
    for (int64_t y = 0; y < map.NumYVoxels(); y++)
    {
      CHECK(Occupancy(map, x, y, 0) == 0.0f);
      if (x == 0 || y == 0)
        CHECK(Occupancy(map, x, y, 1) == 0.0f);
      else if (y >= map.NumYVoxels() - x)
        CHECK(Occupancy(map, x, y, 1) == 0.0f);
      else
        CHECK(Occupancy(map, x, y, 1) == 1.0f);
    }
}

int main(int argc, char** argv)
{
  const bool no_device = argc > 1 && std::strcmp(argv[1], "--no-device") == 0;
  const std::vector<Vector3d> vertices = {{0.0, 0.0, 0.0}, {1.0, 0.0, 0.0}, {0.0, 1.0, 0.0}};
  const std::vector<Vector3i> triangles = {{0, 1, 2}};
  const double resolution = 0.125;

  // raised before a device is touched
  CHECK(ThrowsInvalidArgument([&] { mesh_rasterizer::RasterizeMeshIntoOccupancyMap(vertices, triangles, 0.0); }));
  CHECK(ThrowsInvalidArgument([&] { mesh_rasterizer::RasterizeMeshIntoOccupancyMap(vertices, triangles, -1.0); }));
  CHECK(ThrowsInvalidArgument([&] { mesh_rasterizer::RasterizeMeshIntoOccupancyComponentMap(vertices, triangles, 0.0); }));
  {
    OccupancyMap empty_map;
    OccupancyComponentMap empty_component_map;
    CHECK(ThrowsInvalidArgument([&] { mesh_rasterizer::RasterizeMesh(vertices, triangles, empty_map); }));
    CHECK(ThrowsInvalidArgument([&] { mesh_rasterizer::RasterizeTriangle(vertices, triangles, 0, empty_component_map); }));
  }
  if (!no_device)
  {
    CheckReferenceTriangle(mesh_rasterizer::RasterizeMeshIntoOccupancyMap(vertices, triangles, resolution));
    const OccupancyComponentMap component_map =
        mesh_rasterizer::RasterizeMeshIntoOccupancyComponentMap(vertices, triangles, resolution);
    CheckReferenceTriangle(component_map);
    for (const OccupancyComponentCell& cell : component_map.GetImmutableRawData()) CHECK(cell.component == 0u);

    // RasterizeTriangle / RasterizeMesh into a caller's map; a map that does not contain the triangle
    OccupancyMap map(Isometry3::Translation(-0.125, -0.125, -0.125), "mesh", resolution, 10, 10, 2, 0.0f);
    mesh_rasterizer::RasterizeTriangle(vertices, triangles, 0, map);
    CheckReferenceTriangle(map);
    OccupancyMap small(Isometry3::Translation(0.25, 0.25, -0.125), "mesh", resolution, 4, 4, 2, 0.5f);
    const std::string message =
        RuntimeErrorMessage([&] { mesh_rasterizer::RasterizeMesh(vertices, triangles, small, true); });
    CHECK(message.find("Triangle is not contained by occupancy map") == 0);
    for (const float value : small.GetImmutableRawData()) CHECK(value == 0.5f);
    OccupancyComponentMap small_components(Isometry3::Translation(0.25, 0.25, -0.125), "mesh", resolution, 4, 4, 2,
                                           OccupancyComponentCell{0.5f, 9u});
    CHECK(RuntimeErrorMessage([&] { mesh_rasterizer::RasterizeTriangle(vertices, triangles, 0, small_components, true); })
              .find("Triangle is not contained by occupancy map") == 0);
    mesh_rasterizer::RasterizeMesh(vertices, triangles, small_components, false);
    bool any = false;
    for (const OccupancyComponentCell& cell : small_components.GetImmutableRawData())
    {
      CHECK(cell.component == 9u && (cell.occupancy == 0.5f || cell.occupancy == 1.0f));
      any = any || cell.occupancy == 1.0f;
    }
    CHECK(any);

    // mesh -> SDF: zero-crossing where the map is filled
    SignedDistanceFieldGenerationParameters parameters;
    const SignedDistanceField sdf = mesh_rasterizer::MeshToSignedDistanceField(vertices, triangles, resolution, parameters);
    CHECK(sdf.grid.NumXVoxels() == 10 && sdf.grid.NumZVoxels() == 2);
    for (int64_t x = 0; x < 10; x++)
      for (int64_t y = 0; y < 10; y++)
        for (int64_t z = 0; z < 2; z++) CHECK((sdf.GetIndexImmutable(x, y, z) < 0.0f) == (Occupancy(map, x, y, z) == 1.0f));

    // The rasterizer's scratch is cached by the process's one context of the device, which ReleaseCachedDeviceMemory()
    // trims: the same mesh into a fresh map afterwards gives the same cells, and mesh -> SDF the same field bit for bit.
    ReleaseCachedDeviceMemory();
    OccupancyMap fresh(Isometry3::Translation(-0.125, -0.125, -0.125), "mesh", resolution, 10, 10, 2, 0.0f);
    mesh_rasterizer::RasterizeMesh(vertices, triangles, fresh);
    const auto same_bits = [](const OccupancyMap& a, const OccupancyMap& b) {
      return a.GetImmutableRawData().size() == b.GetImmutableRawData().size() &&
             std::memcmp(a.GetImmutableRawData().data(), b.GetImmutableRawData().data(),
                         a.GetImmutableRawData().size() * sizeof(float)) == 0;
    };
    CHECK(same_bits(fresh, map));
    ReleaseCachedDeviceMemory();
    const SignedDistanceField sdf_again =
        mesh_rasterizer::MeshToSignedDistanceField(vertices, triangles, resolution, parameters);
    CHECK(same_bits(sdf_again.grid, sdf.grid));
    CHECK(sdf_again.minimum == sdf.minimum && sdf_again.maximum == sdf.maximum);
  }
  if (g_failures == 0) std::printf("PASSED\n");
  return g_failures == 0 ? 0 : 1;
}
