// ComputeComponentTopology of the C++ host layer (include/vgt_hip/hip_pointcloud_voxelizer.hpp) on shapes whose holes and
// voids are known: a torus (a slab with a hole), a shell round a cavity, a double torus.
//   test_topology_host              needs a HIP device
//   test_topology_host --no-device  only the argument errors that are raised before a device is touched
#include <vgt_hip.h>
#include <vgt_hip/hip_pointcloud_voxelizer.hpp>

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
  CHECK(ThrowsInvalidArgument([] { NumberOfHolesAndVoids(-1, 0); }));
  CHECK(ThrowsInvalidArgument([] { NumberOfHolesAndVoids(0, -1); }));
  const NumberOfHolesAndVoids two_one(2, 1), none;
  CHECK(two_one.NumHoles() == 2 && two_one.NumVoids() == 1 && none.NumHoles() == 0 && none.NumVoids() == 0);
  CHECK(ThrowsInvalidArgument([] { OccupancyComponentMap m; ComputeComponentTopology(m, FILLED_COMPONENTS); }));
  CHECK(ThrowsInvalidArgument([] { TaggedObjectOccupancyComponentMap m; ComputeComponentTopology(m, FILLED_COMPONENTS, false); }));
  OccupancyComponentMap plain(Isometry3::Identity(), "f", 0.5, 3, 3, 3, OccupancyComponentCell());
  TaggedObjectOccupancyComponentMap tagged(Isometry3::Identity(), "f", 0.5, 3, 3, 3, TaggedObjectOccupancyComponentCell());
  CHECK(ThrowsInvalidArgument([&] { ComputeComponentTopology(plain, 0); }));
  CHECK(ThrowsInvalidArgument([&] { ComputeComponentTopology(plain, 8); }));
  CHECK(ThrowsInvalidArgument([&] { ComputeComponentTopology(tagged, 0, true); }));
  CHECK(ThrowsInvalidArgument([&] { ComputeComponentTopology(tagged, 8, false); }));
  // the C ABI rejects the same before any HIP call, and leaves its outputs alone
  uint32_t count = 77, label = 5;
  float occupancy = 0.0f;
  vgt_hip_component_topology_t entry[2];
  std::memset(entry, 0x5a, sizeof(entry));
  const vgt_hip_component_topology_t before = entry[0];
  CHECK(vgt_hip_component_topology(nullptr, &occupancy, 1, 1, 1, 7, &label, &count, entry, 2) == VGT_HIP_ERR_INVALID_ARGUMENT);
  CHECK(std::strstr(vgt_hip_last_error(), "null") != nullptr);
  CHECK(vgt_hip_component_topology(nullptr, &occupancy, 0, 1, 1, 7, &label, &count, entry, 2) == VGT_HIP_ERR_INVALID_ARGUMENT);
  CHECK(std::strstr(vgt_hip_last_error(), "positive") != nullptr);
  CHECK(vgt_hip_component_topology(nullptr, &occupancy, 1, 1, 1, 9, &label, &count, entry, 2) == VGT_HIP_ERR_INVALID_ARGUMENT);
  CHECK(std::strstr(vgt_hip_last_error(), "component types") != nullptr);
  CHECK(vgt_hip_component_topology_dev(nullptr, &occupancy, &label, 1, 1, (int64_t{1} << 31) - 2, 7, 1, entry) ==
        VGT_HIP_ERR_INVALID_ARGUMENT);
  CHECK(std::strstr(vgt_hip_last_error(), "lattice") != nullptr);
  CHECK(vgt_hip_cells_component_topology(nullptr, nullptr, 0, 7, &label, &count, entry, 2) == VGT_HIP_ERR_INVALID_ARGUMENT);
  CHECK(count == 77 && label == 5 && std::memcmp(&before, &entry[0], sizeof(before)) == 0);
  return g_failures;
}

struct Box
{
  int64_t x0, x1, y0, y1, z0, z1;
  float occupancy;
};
struct Shape
{
  const char* name;
  int64_t nx, ny, nz;
  std::vector<Box> boxes;  // painted in order over an empty grid
  int64_t at[3];           // a cell of the filled component
  int32_t holes, voids;
};

// Both map types; object ids in two halves along x, so that without connect_across_objects the shape falls apart.
static void CheckShape(const Shape& s)
{
  OccupancyComponentMap plain(Isometry3::Identity(), "f", 0.25, s.nx, s.ny, s.nz, OccupancyComponentCell());
  TaggedObjectOccupancyComponentMap tagged(Isometry3::Identity(), "f", 0.25, s.nx, s.ny, s.nz,
                                           TaggedObjectOccupancyComponentCell());
  for (int64_t x = 0; x < s.nx; x++)
    for (int64_t y = 0; y < s.ny; y++)
      for (int64_t z = 0; z < s.nz; z++)
      {
        float occupancy = 0.0f;
        for (const Box& b : s.boxes)
          if (x >= b.x0 && x < b.x1 && y >= b.y0 && y < b.y1 && z >= b.z0 && z < b.z1) occupancy = b.occupancy;
        OccupancyComponentCell a;
        a.occupancy = occupancy;
        a.component = 12345u;
        plain.SetIndex(x, y, z, a);
        TaggedObjectOccupancyComponentCell t;
        t.occupancy = occupancy;
        t.object_id = x < s.nx / 2 ? 1u : 2u;
        t.component = 777u;
        t.spatial_segment = 0xdeadbeefu;
        tagged.SetIndex(x, y, z, t);
      }
  const size_t at = static_cast<size_t>((s.at[0] * s.ny + s.at[1]) * s.nz + s.at[2]);

  // OccupancyComponentMap: the labels are written back, exactly UpdateConnectedComponents' ones
  const TopologicalInvariants filled = ComputeComponentTopology(plain, FILLED_COMPONENTS);
  OccupancyComponentMap relabelled = plain;
  const uint32_t count = UpdateConnectedComponents(relabelled);
  bool same = true;
  for (size_t i = 0; i < plain.GetImmutableRawData().size(); i++)
    same = same && plain.GetImmutableRawData()[i].component == relabelled.GetImmutableRawData()[i].component;
  CHECK(same);
  const uint32_t label = plain.GetImmutableRawData()[at].component;
  CHECK(label >= 1 && label <= count);
  CHECK(filled.size() == 1 && filled.count(label) == 1);  // (one filled component; the empty ones are not selected)
  if (filled.count(label))
  {
    if (filled.at(label).NumHoles() != s.holes || filled.at(label).NumVoids() != s.voids)
      std::printf("%s: holes %d voids %d\n", s.name, filled.at(label).NumHoles(), filled.at(label).NumVoids());
    CHECK(filled.at(label).NumHoles() == s.holes && filled.at(label).NumVoids() == s.voids);
  }
  const TopologicalInvariants all = ComputeComponentTopology(plain, FILLED_COMPONENTS | EMPTY_COMPONENTS | UNKNOWN_COMPONENTS);
  CHECK(all.size() == count);

  // TaggedObjectOccupancyComponentMap across objects: the same components and numbers
  const TopologicalInvariants across = ComputeComponentTopology(tagged, FILLED_COMPONENTS, true);
  same = true;
  for (size_t i = 0; i < tagged.GetImmutableRawData().size(); i++)
  {
    const auto& cell = tagged.GetImmutableRawData()[i];
    same = same && cell.component == relabelled.GetImmutableRawData()[i].component && cell.spatial_segment == 0xdeadbeefu;
  }
  CHECK(same);
  CHECK(across.size() == 1 && across.count(label) == 1 && across.at(label).NumHoles() == s.holes &&
        across.at(label).NumVoids() == s.voids);
  // ... and by object: the two halves are components of their own, labelled as UpdateConnectedComponents does
  const TopologicalInvariants by_object = ComputeComponentTopology(tagged, FILLED_COMPONENTS, false);
  TaggedObjectOccupancyComponentMap tagged_relabelled = tagged;
  UpdateConnectedComponents(tagged_relabelled, false);
  same = true;
  for (size_t i = 0; i < tagged.GetImmutableRawData().size(); i++)
    same = same && tagged.GetImmutableRawData()[i].component == tagged_relabelled.GetImmutableRawData()[i].component;
  CHECK(same);
  CHECK(by_object.size() >= 2);
  // the device-resident map gives the same table without touching a map
  ComponentLabels labels;
  const TopologicalInvariants resident = DeviceTaggedObjectMap(tagged).ComponentTopology(true, FILLED_COMPONENTS, &labels);
  CHECK(labels.count == count && resident.size() == 1 && resident.count(label) == 1);
}

static int RunDevice()
{
  const std::vector<Shape> shapes = {
      {"torus", 12, 11, 6, {{2, 9, 2, 9, 2, 4, 1.0f}, {4, 7, 4, 7, 2, 4, 0.0f}}, {2, 2, 2}, 1, 0},
      {"shell", 12, 11, 11, {{2, 9, 2, 9, 2, 9, 1.0f}, {4, 7, 4, 7, 4, 7, 0.0f}}, {2, 2, 2}, 0, 1},
      {"double torus", 12, 18, 6,
       {{2, 9, 2, 15, 2, 4, 1.0f}, {4, 7, 4, 7, 2, 4, 0.0f}, {4, 7, 10, 13, 2, 4, 0.0f}}, {2, 2, 2}, 2, 0},
  };
  for (const Shape& s : shapes) CheckShape(s);
  return g_failures;
}

int main(int argc, char** argv)
{
  const bool no_device = argc > 1 && std::strcmp(argv[1], "--no-device") == 0;
  const int failures = no_device ? RunNoDevice() : (RunNoDevice(), RunDevice());
  if (failures == 0) std::printf("PASSED\n");
  return failures == 0 ? 0 : 1;
}
