// ExtractSurfaceMesh of the C++ host layer (include/vgt_hip/surface_extraction.hpp) against a restatement of the rules of
// include/vgt_hip.h (vgt_hip_extract_surface) in this program, compared bit for bit.
//   test_surface_host              needs a HIP device
//   test_surface_host --no-device  the restatement against answers derived by hand, and the argument errors that are
//                                  raised before a device is touched (also what runs under the sanitizers)
#include <vgt_hip.h>
#include <vgt_hip/surface_extraction.hpp>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <map>
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

// The rules, one operation at a time (this file is compiled without -ffast-math; x86-64 doubles do not contract).
static SurfaceMesh Restate(const std::vector<float>& f, int64_t nx, int64_t ny, int64_t nz, float iso, bool inside_above,
                           double resolution, const Isometry3& world_from_grid)
{
  const auto at = [&](int64_t i, int64_t j, int64_t k) { return f[static_cast<size_t>((i * ny + j) * nz + k)]; };
  const auto inside = [&](float v) { return inside_above ? v > iso : v < iso; };
  SurfaceMesh mesh;
  std::map<int64_t, int32_t> vertex_of;
  for (int64_t i = 0; i + 1 < nx; i++)
    for (int64_t j = 0; j + 1 < ny; j++)
      for (int64_t k = 0; k + 1 < nz; k++)
      {
        bool finite = true;
        int inside_corners = 0;
        for (int c = 0; c < 8; c++)
        {
          const float v = at(i + (c >> 2), j + ((c >> 1) & 1), k + (c & 1));
          finite = finite && std::isfinite(v);
          inside_corners += inside(v) ? 1 : 0;
        }
        if (!finite || inside_corners == 0 || inside_corners == 8) continue;
        double offset[3] = {0.0, 0.0, 0.0};
        int crossings = 0;
        for (int a = 0; a < 3; a++)
        {
          const int b = (a + 1) % 3, c = (a + 2) % 3;
          for (int db = 0; db < 2; db++)
            for (int dc = 0; dc < 2; dc++)
            {
              int64_t p0[3] = {0, 0, 0}, p1[3];
              p0[b] = db;
              p0[c] = dc;
              std::copy(p0, p0 + 3, p1);
              p1[a] = 1;
              const float v0 = at(i + p0[0], j + p0[1], k + p0[2]), v1 = at(i + p1[0], j + p1[1], k + p1[2]);
              if (inside(v0) == inside(v1)) continue;
              const volatile double t =
                  (static_cast<double>(iso) - static_cast<double>(v0)) / (static_cast<double>(v1) - static_cast<double>(v0));
              offset[a] += t;
              offset[b] += static_cast<double>(db);
              offset[c] += static_cast<double>(dc);
              crossings++;
            }
        }
        const int64_t index[3] = {i, j, k};
        volatile double p[3];
        for (int axis = 0; axis < 3; axis++)
        {
          const volatile double mean = offset[axis] / static_cast<double>(crossings);
          const volatile double in_cells = (static_cast<double>(index[axis]) + 0.5) + mean;
          p[axis] = in_cells * resolution;
        }
        mesh_rasterizer::Vector3d location;
        const auto& m = world_from_grid.m;
        for (size_t r = 0; r < 3; r++)
        {
          const volatile double x = m[r] * p[0], y = m[4 + r] * p[1], z = m[8 + r] * p[2];
          const volatile double xy = x + y;
          const volatile double xyz = xy + z;
          location[r] = xyz + m[12 + r];
        }
        const int64_t cell = (i * ny + j) * nz + k;
        vertex_of[cell] = static_cast<int32_t>(mesh.vertices.size());
        mesh.vertices.push_back(location);
        mesh.vertex_cells.push_back(static_cast<int32_t>(cell));
      }
  const int64_t extent[3] = {nx, ny, nz}, stride[3] = {ny * nz, nz, 1};
  for (int64_t i = 0; i < nx; i++)
    for (int64_t j = 0; j < ny; j++)
      for (int64_t k = 0; k < nz; k++)
        for (int a = 0; a < 3; a++)
        {
          const int b = (a + 1) % 3, c = (a + 2) % 3;
          const int64_t p[3] = {i, j, k};
          if (p[a] + 1 >= extent[a] || p[b] < 1 || p[c] < 1) continue;
          const int64_t linear = (i * ny + j) * nz + k;
          const bool p_inside = inside(f[static_cast<size_t>(linear)]);
          if (p_inside == inside(f[static_cast<size_t>(linear + stride[a])])) continue;
          const int64_t c00 = linear - stride[b] - stride[c], c10 = linear - stride[c], c11 = linear, c01 = linear - stride[b];
          if (!vertex_of.count(c00) || !vertex_of.count(c10) || !vertex_of.count(c11) || !vertex_of.count(c01)) continue;
          const int32_t q0 = vertex_of[c00], q1 = vertex_of[p_inside ? c10 : c01], q2 = vertex_of[c11],
                        q3 = vertex_of[p_inside ? c01 : c10];
          mesh.triangles.push_back({q0, q1, q2});
          mesh.triangles.push_back({q0, q2, q3});
        }
  return mesh;
}

static bool SameBytes(const SurfaceMesh& a, const SurfaceMesh& b)
{
  const auto same = [](const auto& x, const auto& y) {
    return x.size() == y.size() && (x.empty() || std::memcmp(x.data(), y.data(), x.size() * sizeof(x[0])) == 0);
  };
  return same(a.vertices, b.vertices) && same(a.triangles, b.triangles) && same(a.vertex_cells, b.vertex_cells);
}

static double SignedVolume(const SurfaceMesh& mesh)
{
  double six_volumes = 0.0;
  for (const auto& t : mesh.triangles)
  {
    const auto &a = mesh.vertices[static_cast<size_t>(t[0])], &b = mesh.vertices[static_cast<size_t>(t[1])],
               &c = mesh.vertices[static_cast<size_t>(t[2])];
    six_volumes += a[0] * (b[1] * c[2] - b[2] * c[1]) + a[1] * (b[2] * c[0] - b[0] * c[2]) + a[2] * (b[0] * c[1] - b[1] * c[0]);
  }
  return six_volumes / 6.0;
}

static int RunNoDevice()
{
  // the restatement against answers derived by hand: a 3 x 3 x 3 field of +1 with centre -1
  {
    std::vector<float> f(27, 1.0f);
    f[13] = -1.0f;
    const SurfaceMesh mesh = Restate(f, 3, 3, 3, 0.0f, false, 1.0, Isometry3::Identity());
    CHECK(mesh.vertices.size() == 8 && mesh.triangles.size() == 12);
    const double low = 0.5 + 2.5 / 3.0, high = 1.5 + 0.5 / 3.0;  // cube (0, 0, 0): offset 5/6; cube (1, 1, 1): 1/6
    CHECK(mesh.vertices.size() == 8 && mesh.vertices[0] == (mesh_rasterizer::Vector3d{low, low, low}) &&
          mesh.vertices[7] == (mesh_rasterizer::Vector3d{high, high, high}));
    CHECK(mesh.vertex_cells == (std::vector<int32_t>{0, 1, 3, 4, 9, 10, 12, 13}));
    // the x edge from (0, 1, 1), whose lower end is outside: (c00, c01, c11, c10) of the cubes 0, 1, 4, 3
    CHECK(mesh.triangles.size() == 12 && mesh.triangles[0] == (mesh_rasterizer::Vector3i{0, 1, 3}) &&
          mesh.triangles[1] == (mesh_rasterizer::Vector3i{0, 3, 2}));
    CHECK(SignedVolume(mesh) > 0.0);
    // a single cube with one inside corner: a vertex, no face; a NaN corner: a void cube
    std::vector<float> cube(8, 1.0f);
    cube[5] = -3.0f;
    CHECK(Restate(cube, 2, 2, 2, 0.0f, false, 2.0, Isometry3::Identity()).vertices.size() == 1);
    CHECK(Restate(cube, 2, 2, 2, 0.0f, false, 2.0, Isometry3::Identity()).triangles.empty());
    cube[0] = std::numeric_limits<float>::quiet_NaN();
    CHECK(Restate(cube, 2, 2, 2, 0.0f, false, 2.0, Isometry3::Identity()).vertices.empty());
  }
  // the layer's own checks
  CHECK(ThrowsInvalidArgument([] { ExtractSurfaceMesh(SignedDistanceField()); }));
  CHECK(ThrowsInvalidArgument([] { ExtractSurfaceMesh(OccupancyMap()); }));
  CHECK(ThrowsInvalidArgument([] { ExtractSurfaceMesh(OccupancyComponentMap()); }));
  CHECK(ThrowsInvalidArgument([] { ExtractSurfaceMesh(TaggedObjectOccupancyMap()); }));
  CHECK(ThrowsInvalidArgument([] { ExtractSurfaceMesh(TaggedObjectOccupancyComponentMap()); }));
  SignedDistanceField sdf;
  sdf.grid = DenseGrid(Isometry3::Identity(), "f", 1.0, 4, 4, 4, 1.0f);
  CHECK(ThrowsInvalidArgument([&] { ExtractSurfaceMesh(sdf, std::numeric_limits<float>::quiet_NaN()); }));
  CHECK(ThrowsInvalidArgument([&] { ExtractSurfaceMesh(sdf, std::numeric_limits<float>::infinity()); }));
  // the C ABI rejects these before any HIP call and leaves its outputs alone (the grid stands in for a context: a
  // non-null context pointer is not dereferenced before the other checks)
  const float* field = sdf.grid.GetImmutableRawData().data();
  vgt_hip_ctx* stand_in = reinterpret_cast<vgt_hip_ctx*>(const_cast<float*>(field));
  std::vector<double> vertices(24, 9.0);
  std::vector<int32_t> cells(8, 9), triangles(24, 9);
  int64_t nv = -7, nt = -7;
  const auto host = [&](vgt_hip_ctx* ctx, const float* values, int64_t nx, float iso, double resolution, double* v,
                        int32_t* t) {
    return vgt_hip_extract_surface(ctx, values, nx, 4, 4, iso, 0, resolution, nullptr, v, v ? cells.data() : nullptr,
                                   v ? 8 : 0, t, t ? 8 : 0, &nv, &nt);
  };
  CHECK(host(nullptr, field, 4, 0.0f, 1.0, vertices.data(), triangles.data()) == VGT_HIP_ERR_INVALID_ARGUMENT);
  CHECK(std::strstr(vgt_hip_last_error(), "null") != nullptr);
  CHECK(host(stand_in, nullptr, 4, 0.0f, 1.0, vertices.data(), triangles.data()) == VGT_HIP_ERR_INVALID_ARGUMENT);
  CHECK(host(stand_in, field, 0, 0.0f, 1.0, vertices.data(), triangles.data()) == VGT_HIP_ERR_INVALID_ARGUMENT);
  CHECK(std::strstr(vgt_hip_last_error(), "positive") != nullptr);
  CHECK(host(stand_in, field, int64_t{1} << 31, 0.0f, 1.0, vertices.data(), triangles.data()) == VGT_HIP_ERR_INVALID_ARGUMENT);
  CHECK(std::strstr(vgt_hip_last_error(), "2^31") != nullptr);
  CHECK(host(stand_in, field, 4, 0.0f, 0.0, vertices.data(), triangles.data()) == VGT_HIP_ERR_INVALID_ARGUMENT);
  CHECK(std::strstr(vgt_hip_last_error(), "resolution") != nullptr);
  CHECK(host(stand_in, field, 4, 0.0f, std::numeric_limits<double>::infinity(), vertices.data(), triangles.data()) ==
        VGT_HIP_ERR_INVALID_ARGUMENT);
  CHECK(host(stand_in, field, 4, std::numeric_limits<float>::quiet_NaN(), 1.0, vertices.data(), triangles.data()) ==
        VGT_HIP_ERR_INVALID_ARGUMENT);
  CHECK(std::strstr(vgt_hip_last_error(), "iso") != nullptr);
  CHECK(host(stand_in, field, 4, 0.0f, 1.0, nullptr, triangles.data()) == VGT_HIP_ERR_INVALID_ARGUMENT);
  CHECK(std::strstr(vgt_hip_last_error(), "needs a vertex buffer") != nullptr);
  CHECK(vgt_hip_extract_surface_dev(stand_in, field, 4, 4, 4, 0.0f, 0, 1.0, nullptr, nullptr, nullptr, 8, nullptr, 0, &nv,
                                    &nt) == VGT_HIP_ERR_INVALID_ARGUMENT);
  CHECK(vgt_hip_cells_extract_surface(stand_in, nullptr, 1.0, nullptr, nullptr, nullptr, 0, nullptr, 0, &nv, &nt) ==
        VGT_HIP_ERR_INVALID_ARGUMENT);
  CHECK(nv == -7 && nt == -7);
  // an extent of 1: no cubes, success with 0 and 0 and nothing launched
  CHECK(vgt_hip_extract_surface(stand_in, field, 4, 1, 4, 0.0f, 0, 1.0, nullptr, nullptr, nullptr, 0, nullptr, 0, &nv,
                                &nt) == VGT_HIP_OK && nv == 0 && nt == 0);
  CHECK(std::all_of(vertices.begin(), vertices.end(), [](double v) { return v == 9.0; }));
  CHECK(std::all_of(cells.begin(), cells.end(), [](int32_t v) { return v == 9; }));
  CHECK(std::all_of(triangles.begin(), triangles.end(), [](int32_t v) { return v == 9; }));
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

template <typename Map>
static void CheckRasterizes(const SurfaceMesh& mesh, const Map& like)
{
  // the mesh goes into the rasterizer as it is: formats only, the frames agree because both use the map's transform
  OccupancyMap target(like.OriginTransform(), "test_frame", like.Resolution(), like.NumXVoxels(), like.NumYVoxels(),
                      like.NumZVoxels(), 0.0f);
  mesh_rasterizer::RasterizeMesh(mesh.vertices, mesh.triangles, target, false, 0, mesh_rasterizer::ClosestPointRule::NEAREST);
  const auto& cells = target.GetImmutableRawData();
  CHECK(std::count(cells.begin(), cells.end(), 1.0f) > 0);
}

static int RunDevice()
{
  const Isometry3 origin = Isometry3::FromQuaternion(0.9238795325112867, 0.0, 0.3826834323650898, 0.0, 1.0, -2.0, 0.5);
  const int64_t shapes[2][3] = {{9, 7, 70}, {20, 33, 17}};
  for (const auto& shape : shapes)
  {
    const int64_t nx = shape[0], ny = shape[1], nz = shape[2], n = nx * ny * nz;
    // a signed field: a sphere's distance with some noise, a few non-finite values
    SignedDistanceField sdf;
    sdf.grid = DenseGrid(origin, "test_frame", 0.25, nx, ny, nz, 0.0f);
    std::vector<float> field(static_cast<size_t>(n));
    for (int64_t i = 0; i < n; i++)
    {
      const double x = static_cast<double>(i / (ny * nz)) - 0.5 * nx, y = static_cast<double>(i / nz % ny) - 0.5 * ny,
                   z = static_cast<double>(i % nz) - 0.5 * nz;
      float v = static_cast<float>(std::sqrt(x * x + y * y + z * z) - 0.3 * static_cast<double>(std::min({nx, ny, nz}))) +
                0.5f * Noise(i, 1);
      if (i % 397 == 11) v = std::numeric_limits<float>::quiet_NaN();
      if (i % 1013 == 5) v = -std::numeric_limits<float>::infinity();
      field[static_cast<size_t>(i)] = v;
      sdf.grid.GetMutableRawData()[static_cast<size_t>(i)] = v;
    }
    for (const float iso : {0.0f, 0.37f})
    {
      const SurfaceMesh got = ExtractSurfaceMesh(sdf, iso);
      const SurfaceMesh want = Restate(field, nx, ny, nz, iso, false, 0.25, origin);
      CHECK(!want.vertices.empty() && !want.triangles.empty());
      CHECK(SameBytes(got, want));
      CHECK(SameBytes(ExtractSurfaceMesh(sdf, iso), got));
      if (iso == 0.0f) CheckRasterizes(got, sdf.grid);
    }
    // occupancy in {0, 0.5, 1}: the four map types
    OccupancyMap map(origin, "test_frame", 0.25, nx, ny, nz, 0.0f);
    OccupancyComponentMap component(origin, "test_frame", 0.25, nx, ny, nz, OccupancyComponentCell());
    TaggedObjectOccupancyMap tagged(origin, "test_frame", 0.25, nx, ny, nz, TaggedObjectOccupancyCell());
    TaggedObjectOccupancyComponentMap wide(origin, "test_frame", 0.25, nx, ny, nz, TaggedObjectOccupancyComponentCell());
    std::vector<float> occupancy(static_cast<size_t>(n));
    for (int64_t i = 0; i < n; i++)
    {
      const float r = Noise(i, 2);
      const float occ = r < 0.55f ? 0.0f : (r < 0.65f ? 0.5f : 1.0f);
      const uint32_t id = static_cast<uint32_t>(i % 5);
      const size_t at = static_cast<size_t>(i);
      occupancy[at] = occ;
      map.GetMutableRawData()[at] = occ;
      component.GetMutableRawData()[at] = OccupancyComponentCell{occ, id + 7u};
      tagged.GetMutableRawData()[at] = TaggedObjectOccupancyCell{occ, id};
      wide.GetMutableRawData()[at] = TaggedObjectOccupancyComponentCell{occ, id, id + 7u, 0xDEADBEEFu};
    }
    const SurfaceMesh want = Restate(occupancy, nx, ny, nz, 0.5f, true, 0.25, origin);
    CHECK(!want.vertices.empty() && !want.triangles.empty());
    CHECK(SameBytes(ExtractSurfaceMesh(map), want));
    CHECK(SameBytes(ExtractSurfaceMesh(component), want));
    CHECK(SameBytes(ExtractSurfaceMesh(tagged), want));
    CHECK(SameBytes(ExtractSurfaceMesh(wide), want));
    CheckRasterizes(want, map);
  }
  // a grid without cubes, and a field without a surface
  CHECK(ExtractSurfaceMesh(OccupancyMap(Isometry3::Identity(), "f", 1.0, 3, 1, 5, 1.0f)).vertices.empty());
  const SurfaceMesh none = ExtractSurfaceMesh(OccupancyMap(Isometry3::Identity(), "f", 1.0, 3, 2, 5, 0.0f));
  CHECK(none.vertices.empty() && none.triangles.empty() && none.vertex_cells.empty());
  return g_failures;
}

int main(int argc, char** argv)
{
  const bool no_device = argc > 1 && std::strcmp(argv[1], "--no-device") == 0;
  const int failures = no_device ? RunNoDevice() : (RunNoDevice(), RunDevice());
  if (failures == 0) std::printf("PASSED\n");
  return failures == 0 ? 0 : 1;
}
