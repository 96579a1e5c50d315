// Enclosed space through the C++ host layer: FillEnclosedSpace (include/vgt_hip/hip_pointcloud_voxelizer.hpp) on both map
// types and the three ...Solid... functions of include/vgt_hip/mesh_rasterizer.hpp against the counts that
// tests/test_fill_ref.py pins for the CPU restatement (box 3080, icosphere 1472).
//   test_fill_host              needs a HIP device
//   test_fill_host --no-device  only the errors that are raised before a device is touched
#include <vgt_hip.h>
#include <vgt_hip/hip_pointcloud_voxelizer.hpp>
#include <vgt_hip/mesh_rasterizer.hpp>

#include <cmath>
#include <cstdio>
#include <cstring>
#include <map>
#include <stdexcept>
#include <utility>
#include <vector>

using namespace vgt_hip;
using mesh_rasterizer::ClosestPointRule;
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

struct Mesh
{
  std::vector<Vector3d> vertices;
  std::vector<Vector3i> triangles;
};

// synthetic.mesh_box
static Mesh Box(const Vector3d& lo, const Vector3d& hi)
{
  Mesh mesh;
  for (int i = 0; i < 8; i++)
    mesh.vertices.push_back({(i & 1) ? hi[0] : lo[0], (i & 2) ? hi[1] : lo[1], (i & 4) ? hi[2] : lo[2]});
  mesh.triangles = {{0, 2, 1}, {1, 2, 3}, {4, 5, 6}, {5, 7, 6}, {0, 1, 4}, {1, 5, 4},
                    {2, 6, 3}, {3, 6, 7}, {0, 4, 2}, {2, 4, 6}, {1, 3, 5}, {3, 7, 5}};
  return mesh;
}

// synthetic.mesh_icosphere round the origin, in its order of operations
static Mesh Icosphere(int subdivisions, double radius)
{
  const double g = (1.0 + std::sqrt(5.0)) / 2.0;
  const double norm = std::sqrt(1.0 + g * g);
  Mesh mesh;
  const double raw[12][3] = {{-1, g, 0}, {1, g, 0}, {-1, -g, 0}, {1, -g, 0}, {0, -1, g}, {0, 1, g},
                             {0, -1, -g}, {0, 1, -g}, {g, 0, -1}, {g, 0, 1}, {-g, 0, -1}, {-g, 0, 1}};
  for (const auto& p : raw) mesh.vertices.push_back({p[0] / norm, p[1] / norm, p[2] / norm});
  mesh.triangles = {{0, 11, 5}, {0, 5, 1}, {0, 1, 7}, {0, 7, 10}, {0, 10, 11}, {1, 5, 9}, {5, 11, 4},
                    {11, 10, 2}, {10, 7, 6}, {7, 1, 8}, {3, 9, 4}, {3, 4, 2}, {3, 2, 6}, {3, 6, 8},
                    {3, 8, 9}, {4, 9, 5}, {2, 4, 11}, {6, 2, 10}, {8, 6, 7}, {9, 8, 1}};
  for (int s = 0; s < subdivisions; s++)
  {
    std::map<std::pair<int32_t, int32_t>, int32_t> middle;
    const auto mid = [&](int32_t a, int32_t b) {
      const std::pair<int32_t, int32_t> key(a < b ? a : b, a < b ? b : a);
      const auto found = middle.find(key);
      if (found != middle.end()) return found->second;
      const Vector3d& va = mesh.vertices[static_cast<size_t>(a)];
      const Vector3d& vb = mesh.vertices[static_cast<size_t>(b)];
      const double m[3] = {(va[0] + vb[0]) * 0.5, (va[1] + vb[1]) * 0.5, (va[2] + vb[2]) * 0.5};
      const double length = std::sqrt((m[0] * m[0] + m[1] * m[1]) + m[2] * m[2]);
      mesh.vertices.push_back({m[0] / length, m[1] / length, m[2] / length});
      const int32_t index = static_cast<int32_t>(mesh.vertices.size()) - 1;
      middle[key] = index;
      return index;
    };
    std::vector<Vector3i> next;
    for (const Vector3i& t : mesh.triangles)
    {
      const int32_t a = t[0], b = t[1], c = t[2];
      const int32_t ab = mid(a, b), ca = mid(c, a), bc = mid(b, c);
      next.push_back({a, ab, ca});
      next.push_back({b, bc, ab});
      next.push_back({c, ca, bc});
      next.push_back({ab, bc, ca});
    }
    mesh.triangles = next;
  }
  for (Vector3d& v : mesh.vertices)
    for (double& c : v) c = c * radius + 0.0;
  return mesh;
}

static int64_t CountFilled(const OccupancyMap& map)
{
  int64_t n = 0;
  for (const float v : map.GetImmutableRawData()) n += v > 0.5f ? 1 : 0;
  return n;
}
static int64_t CountFilled(const OccupancyComponentMap& map)
{
  int64_t n = 0;
  for (const OccupancyComponentCell& c : map.GetImmutableRawData()) n += c.occupancy > 0.5f ? 1 : 0;
  return n;
}

int main(int argc, char** argv)
{
  const bool no_device = argc > 1 && std::strcmp(argv[1], "--no-device") == 0;
  const Mesh box = Box({0.11, -0.2, 0.3}, {0.93, 0.41, 0.77});
  const Mesh sphere = Icosphere(2, 0.4);
  CHECK(sphere.vertices.size() == 162 && sphere.triangles.size() == 320);

  // raised before a device is touched
  {
    OccupancyMap empty_map;
    OccupancyComponentMap empty_component_map;
    CHECK(ThrowsInvalidArgument([&] { FillEnclosedSpace(empty_map); }));
    CHECK(ThrowsInvalidArgument([&] { FillEnclosedSpace(empty_component_map, false); }));
  }
  CHECK(ThrowsInvalidArgument([&] { mesh_rasterizer::RasterizeSolidMeshIntoOccupancyMap(box.vertices, box.triangles, 0.0); }));
  CHECK(ThrowsInvalidArgument(
      [&] { mesh_rasterizer::RasterizeSolidMeshIntoOccupancyComponentMap(box.vertices, box.triangles, -1.0); }));
  CHECK(ThrowsInvalidArgument([&] {
    mesh_rasterizer::SolidMeshToSignedDistanceField(box.vertices, box.triangles, 0.0,
                                                    SignedDistanceFieldGenerationParameters());
  }));

  if (!no_device)
  {
    // FillEnclosedSpace on both map types: a 5 x 5 x 5 shell of 0.7 round a 3 x 3 x 3 cavity whose centre is unknown
    OccupancyMap map(Isometry3::Translation(0.0, 0.0, 0.0), "fill", 0.1, 7, 7, 7, 0.0f);
    OccupancyComponentMap component_map(Isometry3::Translation(0.0, 0.0, 0.0), "fill", 0.1, 7, 7, 7,
                                        OccupancyComponentCell{0.0f, 5u});
    for (int64_t x = 1; x < 6; x++)
      for (int64_t y = 1; y < 6; y++)
        for (int64_t z = 1; z < 6; z++)
        {
          const bool cavity = x > 1 && x < 5 && y > 1 && y < 5 && z > 1 && z < 5;
          const float value = !cavity ? 0.7f : (x == 3 && y == 3 && z == 3 ? 0.5f : 0.25f);
          map.SetIndex(x, y, z, value);
          component_map.SetIndex(x, y, z, OccupancyComponentCell{value, static_cast<uint32_t>(100 * x + 10 * y + z)});
        }
    OccupancyMap passable_unknown = map;
    CHECK(FillEnclosedSpace(map) == 26);  // the unknown centre counts as filled already
    CHECK(FillEnclosedSpace(passable_unknown, false) == 27);
    CHECK(FillEnclosedSpace(component_map, true) == 26);
    for (int64_t x = 0; x < 7; x++)
      for (int64_t y = 0; y < 7; y++)
        for (int64_t z = 0; z < 7; z++)
        {
          const bool outside = x < 1 || x > 5 || y < 1 || y > 5 || z < 1 || z > 5;
          const bool cavity = x > 1 && x < 5 && y > 1 && y < 5 && z > 1 && z < 5;
          const bool centre = x == 3 && y == 3 && z == 3;
          const float want = outside ? 0.0f : (!cavity ? 0.7f : (centre ? 0.5f : 1.0f));
          CHECK(map.GetIndexImmutable(x, y, z) == want);
          CHECK(passable_unknown.GetIndexImmutable(x, y, z) == (centre ? 1.0f : want));
          const OccupancyComponentCell& cell = component_map.GetIndexImmutable(x, y, z);
          CHECK(cell.occupancy == want);
          CHECK(cell.component == (outside ? 5u : static_cast<uint32_t>(100 * x + 10 * y + z)));  // never written
        }
    CHECK(FillEnclosedSpace(map) == 0 && FillEnclosedSpace(component_map) == 0);  // idempotent

    // solid meshes: shell + the cells it encloses
    const OccupancyMap box_shell =
        mesh_rasterizer::RasterizeMeshIntoOccupancyMap(box.vertices, box.triangles, 0.04, 0, ClosestPointRule::NEAREST);
    const OccupancyMap box_solid = mesh_rasterizer::RasterizeSolidMeshIntoOccupancyMap(box.vertices, box.triangles, 0.04);
    CHECK(CountFilled(box_solid) - CountFilled(box_shell) == 3080);
    const OccupancyComponentMap box_components =
        mesh_rasterizer::RasterizeSolidMeshIntoOccupancyComponentMap(box.vertices, box.triangles, 0.04);
    CHECK(CountFilled(box_components) == CountFilled(box_solid));
    for (const OccupancyComponentCell& cell : box_components.GetImmutableRawData()) CHECK(cell.component == 0u);
    const OccupancyMap box_reference = mesh_rasterizer::RasterizeSolidMeshIntoOccupancyMap(
        box.vertices, box.triangles, 0.04, 0, ClosestPointRule::REFERENCE);
    const OccupancyMap box_reference_shell =
        mesh_rasterizer::RasterizeMeshIntoOccupancyMap(box.vertices, box.triangles, 0.04);
    CHECK(CountFilled(box_reference) - CountFilled(box_reference_shell) == 3080);

    const OccupancyMap sphere_shell = mesh_rasterizer::RasterizeMeshIntoOccupancyMap(
        sphere.vertices, sphere.triangles, 0.05, 0, ClosestPointRule::NEAREST);
    const OccupancyMap sphere_solid =
        mesh_rasterizer::RasterizeSolidMeshIntoOccupancyMap(sphere.vertices, sphere.triangles, 0.05);
    CHECK(CountFilled(sphere_solid) - CountFilled(sphere_shell) == 1472);

    // the field: negative at the body's centre, positive there for the hollow shell; zero crossing = the solid map
    SignedDistanceFieldGenerationParameters parameters;
    const SignedDistanceField solid =
        mesh_rasterizer::SolidMeshToSignedDistanceField(sphere.vertices, sphere.triangles, 0.05, parameters);
    const SignedDistanceField hollow = mesh_rasterizer::MeshToSignedDistanceField(
        sphere.vertices, sphere.triangles, 0.05, parameters, ClosestPointRule::NEAREST);
    const int64_t cx = solid.grid.NumXVoxels() / 2, cy = solid.grid.NumYVoxels() / 2, cz = solid.grid.NumZVoxels() / 2;
    CHECK(solid.GetIndexImmutable(cx, cy, cz) < 0.0f && hollow.GetIndexImmutable(cx, cy, cz) > 0.0f);
    CHECK(solid.grid.NumXVoxels() == sphere_solid.NumXVoxels());
    for (int64_t x = 0; x < sphere_solid.NumXVoxels(); x++)
      for (int64_t y = 0; y < sphere_solid.NumYVoxels(); y++)
        for (int64_t z = 0; z < sphere_solid.NumZVoxels(); z++)
          CHECK((solid.GetIndexImmutable(x, y, z) < 0.0f) == (sphere_solid.GetIndexImmutable(x, y, z) == 1.0f));
  }
  if (g_failures == 0) std::printf("PASSED\n");
  return g_failures == 0 ? 0 : 1;
}
