// Lists of cells of include/vgt_hip/hip_pointcloud_voxelizer.hpp -- SurfaceIndices, the display exports and
// ExtractComponentSurfaces -- on the C ABI's cell selection (vgt_hip_select_cells, vgt_hip_cells_select): the device
// selects, the host colours the compact list with the reference's colour arithmetic (I/ros_interface.hpp:336-375,
// S/ros_interface.cpp) and never loops over the voxels.
#include "../../../include/vgt_hip/hip_pointcloud_voxelizer.hpp"
#include "host_internal.hpp"

#include <cmath>
#include <limits>

namespace vgt_hip
{
namespace
{
using detail::SharedSdfContext;
using detail::ThrowForCode;

// The selected cells of a map: linear indices in ascending order, their values and -- for a cell member -- one uint32 each.
struct Selection
{
  std::vector<int32_t> indices;
  std::vector<float> values;
  std::vector<uint32_t> payload;
};

// A float grid (OccupancyMap, the grid of a SignedDistanceField): the values go up with the call.
Selection Select(const DenseGrid& grid, int rule, int class_mask, float threshold, int /* payload_member */, int hip_device)
{
  if (!grid.IsInitialized()) throw std::invalid_argument("Grid must be initialized");
  vgt_hip_ctx* const ctx = SharedSdfContext(hip_device);
  const float* const values = grid.GetImmutableRawData().data();
  const int64_t nx = grid.NumXVoxels(), ny = grid.NumYVoxels(), nz = grid.NumZVoxels();
  Selection s;
  int64_t count = 0;
  int rc = vgt_hip_select_cells(ctx, values, nullptr, nx, ny, nz, rule, class_mask, threshold, nullptr, nullptr, nullptr,
                                0, &count);
  if (rc != VGT_HIP_OK) ThrowForCode(rc, vgt_hip_last_error());
  if (count == 0) return s;
  s.indices.resize(static_cast<size_t>(count));
  s.values.resize(static_cast<size_t>(count));
  rc = vgt_hip_select_cells(ctx, values, nullptr, nx, ny, nz, rule, class_mask, threshold, s.indices.data(),
                            s.values.data(), nullptr, count, &count);
  if (rc != VGT_HIP_OK) ThrowForCode(rc, vgt_hip_last_error());
  return s;
}

template <typename Cell>
constexpr int ObjectIdOffset()
{
  return -1;
}
template <>
constexpr int ObjectIdOffset<TaggedObjectOccupancyCell>()
{
  return 4;
}
template <>
constexpr int ObjectIdOffset<TaggedObjectOccupancyComponentCell>()
{
  return 4;
}

// A grid of cell records: uploaded once, selected on the device.  (threshold: 0.5, the occupancy's.)
template <typename Cell>
Selection Select(const CellGrid<Cell>& map, int rule, int class_mask, float /* threshold */, int payload_member,
                 int hip_device)
{
  if (!map.IsInitialized()) throw std::invalid_argument("Grid must be initialized");
  vgt_hip_ctx* const ctx = SharedSdfContext(hip_device);
  vgt_hip_cells* cells = nullptr;
  int rc = vgt_hip_cells_create(ctx, map.GetImmutableRawData().data(), map.NumXVoxels(), map.NumYVoxels(),
                                map.NumZVoxels(), static_cast<int32_t>(sizeof(Cell)), ObjectIdOffset<Cell>(), &cells);
  if (rc != VGT_HIP_OK) ThrowForCode(rc, vgt_hip_last_error());
  Selection s;
  int64_t count = 0;
  rc = vgt_hip_cells_select(ctx, cells, nullptr, rule, class_mask, nullptr, nullptr, nullptr, VGT_HIP_CELL_MEMBER_NONE, 0,
                            &count);
  if (rc == VGT_HIP_OK && count > 0)
  {
    s.indices.resize(static_cast<size_t>(count));
    s.values.resize(static_cast<size_t>(count));
    if (payload_member != VGT_HIP_CELL_MEMBER_NONE) s.payload.resize(static_cast<size_t>(count));
    rc = vgt_hip_cells_select(ctx, cells, nullptr, rule, class_mask, s.indices.data(), s.values.data(),
                              s.payload.empty() ? nullptr : s.payload.data(), payload_member, count, &count);
  }
  const std::string msg = (rc == VGT_HIP_OK) ? std::string() : std::string(vgt_hip_last_error());
  vgt_hip_cells_destroy(cells);
  if (rc != VGT_HIP_OK) ThrowForCode(rc, msg);
  return s;
}

struct Extents
{
  int64_t ny, nz;
  double voxel_size;
};
template <typename Map>
Extents ExtentsOf(const Map& map)
{
  return Extents{map.NumYVoxels(), map.NumZVoxels(), map.Resolution()};
}

std::array<int64_t, 3> GridIndexOf(const Extents& e, int32_t linear)
{
  const int64_t index = static_cast<int64_t>(linear);
  return {index / (e.ny * e.nz), (index / e.nz) % e.ny, index % e.nz};
}

// The centre of a cell in the grid frame (NOT PINNED, see the header): (index + 0.5) * voxel size per axis, in double.
std::array<double, 3> CellCentre(const Extents& e, int32_t linear)
{
  const std::array<int64_t, 3> index = GridIndexOf(e, linear);
  return {(static_cast<double>(index[0]) + 0.5) * e.voxel_size, (static_cast<double>(index[1]) + 0.5) * e.voxel_size,
          (static_cast<double>(index[2]) + 0.5) * e.voxel_size};
}

// ExportVoxelGridToRViz over a selection: colour every listed cell, keep those with alpha > 0.
template <typename ColorFn>
DisplayCubes Colour(const Selection& s, const Extents& e, const ColorFn& color_fn)
{
  DisplayCubes cubes;
  cubes.points.reserve(s.indices.size());
  cubes.colors.reserve(s.indices.size());
  for (size_t k = 0; k < s.indices.size(); k++)
  {
    const ColorRGBA color = color_fn(k);
    if (color[3] > 0.0f)
    {
      cubes.points.push_back(CellCentre(e, s.indices[k]));
      cubes.colors.push_back(color);
    }
  }
  return cubes;
}

// collision / free / unknown colours by occupancy class; classes whose colour would be dropped are not selected at all
template <typename Map>
DisplayCubes OccupancyDisplay(const Map& map, int rule, const ColorRGBA& collision_color, const ColorRGBA& free_color,
                              const ColorRGBA& unknown_color, int hip_device)
{
  if (!map.IsInitialized()) throw std::invalid_argument("Grid must be initialized");
  const int class_mask = (collision_color[3] > 0.0f ? VGT_HIP_CLASS_ABOVE : 0) |
                         (free_color[3] > 0.0f ? VGT_HIP_CLASS_BELOW : 0) |
                         (unknown_color[3] > 0.0f ? (VGT_HIP_CLASS_EQUAL | VGT_HIP_CLASS_UNORDERED) : 0);
  if (class_mask == 0) return DisplayCubes();
  const Selection s = Select(map, rule, class_mask, 0.5f, VGT_HIP_CELL_MEMBER_NONE, hip_device);
  return Colour(s, ExtentsOf(map), [&](size_t k) {
    const float occupancy = s.values[k];
    return occupancy > 0.5f ? collision_color : (occupancy < 0.5f ? free_color : unknown_color);
  });
}

template <typename Map>
std::array<DisplayCubes, 3> SeparateDisplay(const Map& map, const ColorRGBA& collision_color, const ColorRGBA& free_color,
                                            const ColorRGBA& unknown_color, int hip_device)
{
  const ColorRGBA no_color{{0.0f, 0.0f, 0.0f, 0.0f}};
  return {OccupancyDisplay(map, VGT_HIP_SELECT_ALL, collision_color, no_color, no_color, hip_device),
          OccupancyDisplay(map, VGT_HIP_SELECT_ALL, no_color, free_color, no_color, hip_device),
          OccupancyDisplay(map, VGT_HIP_SELECT_ALL, no_color, no_color, unknown_color, hip_device)};
}

template <typename Map>
GridIndices Surfaces(const Map& map, int hip_device)
{
  const Selection s = Select(map, VGT_HIP_SELECT_SURFACE_26, 15, 0.5f, VGT_HIP_CELL_MEMBER_NONE, hip_device);
  const Extents e = ExtentsOf(map);
  GridIndices indices;
  indices.reserve(s.indices.size());
  for (const int32_t linear : s.indices) indices.push_back(GridIndexOf(e, linear));
  return indices;
}

template <typename Map>
DisplayCubes ComponentsDisplay(const Map& map, bool color_unknown_components, const ComponentPalette& palette_fn,
                               int hip_device)
{
  if (!palette_fn) throw std::invalid_argument("a component palette is needed");
  const Selection s = Select(map, VGT_HIP_SELECT_ALL, 15, 0.5f, VGT_HIP_CELL_MEMBER_COMPONENT, hip_device);
  const ColorRGBA unknown_color{{0.5f, 0.5f, 0.5f, 1.0f}};
  return Colour(s, ExtentsOf(map), [&](size_t k) {
    if (s.values[k] != 0.5f || color_unknown_components) return palette_fn(s.payload[k]);
    return unknown_color;
  });
}

template <typename Map>
ComponentSurfaces ExtractSurfaces(const Map& map, uint8_t component_types, int hip_device)
{
  if (!map.IsInitialized()) throw std::invalid_argument("Grid must be initialized");
  if (component_types < 1 || component_types > 7)
    throw std::invalid_argument("component types must be a combination of FILLED_, EMPTY_ and UNKNOWN_COMPONENTS");
  // "unknown" is whatever is neither > 0.5 nor < 0.5: equal or unordered
  const int class_mask = (component_types & (FILLED_COMPONENTS | EMPTY_COMPONENTS)) |
                         ((component_types & UNKNOWN_COMPONENTS) ? (VGT_HIP_CLASS_EQUAL | VGT_HIP_CLASS_UNORDERED) : 0);
  const Selection s =
      Select(map, VGT_HIP_SELECT_COMPONENT_SURFACE, class_mask, 0.5f, VGT_HIP_CELL_MEMBER_COMPONENT, hip_device);
  const Extents e = ExtentsOf(map);
  ComponentSurfaces surfaces;
  for (size_t k = 0; k < s.indices.size(); k++) surfaces[s.payload[k]].push_back(GridIndexOf(e, s.indices[k]));
  return surfaces;
}

float ClampAlpha(float alpha) { return alpha < 0.0f ? 0.0f : (alpha > 1.0f ? 1.0f : alpha); }
}  // namespace

#define VGT_HIP_FOR_EACH_MAP_TYPE(X) \
  X(OccupancyMap) X(OccupancyComponentMap) X(TaggedObjectOccupancyMap) X(TaggedObjectOccupancyComponentMap)

#define VGT_HIP_DEFINE_DISPLAY(Map)                                                                                  \
  GridIndices SurfaceIndices(const Map& map, int hip_device) { return Surfaces(map, hip_device); }                  \
  DisplayCubes ExportForDisplay(const Map& map, const ColorRGBA& collision_color, const ColorRGBA& free_color,      \
                                const ColorRGBA& unknown_color, int hip_device)                                     \
  {                                                                                                                  \
    return OccupancyDisplay(map, VGT_HIP_SELECT_ALL, collision_color, free_color, unknown_color, hip_device);       \
  }                                                                                                                  \
  std::array<DisplayCubes, 3> ExportForSeparateDisplay(const Map& map, const ColorRGBA& collision_color,            \
                                                       const ColorRGBA& free_color, const ColorRGBA& unknown_color, \
                                                       int hip_device)                                              \
  {                                                                                                                  \
    return SeparateDisplay(map, collision_color, free_color, unknown_color, hip_device);                            \
  }                                                                                                                  \
  DisplayCubes ExportSurfacesForDisplay(const Map& map, const ColorRGBA& collision_color,                           \
                                        const ColorRGBA& free_color, const ColorRGBA& unknown_color, int hip_device) \
  {                                                                                                                  \
    return OccupancyDisplay(map, VGT_HIP_SELECT_SURFACE_26, collision_color, free_color, unknown_color, hip_device); \
  }
VGT_HIP_FOR_EACH_MAP_TYPE(VGT_HIP_DEFINE_DISPLAY)
#undef VGT_HIP_DEFINE_DISPLAY
#undef VGT_HIP_FOR_EACH_MAP_TYPE

DisplayCubes ExportConnectedComponentsForDisplay(const OccupancyComponentMap& map, bool color_unknown_components,
                                                 const ComponentPalette& palette_fn, int hip_device)
{
  return ComponentsDisplay(map, color_unknown_components, palette_fn, hip_device);
}

DisplayCubes ExportConnectedComponentsForDisplay(const TaggedObjectOccupancyComponentMap& map,
                                                 bool color_unknown_components, const ComponentPalette& palette_fn,
                                                 int hip_device)
{
  return ComponentsDisplay(map, color_unknown_components, palette_fn, hip_device);
}

DisplayCubes ExportSDFForDisplay(const SignedDistanceField& sdf, float alpha, int hip_device)
{
  if (!sdf.grid.IsInitialized()) throw std::invalid_argument("Grid must be initialized");
  const float clamped_alpha = ClampAlpha(alpha);
  if (!(clamped_alpha > 0.0f)) return DisplayCubes();  // (every cell would be dropped)
  float minimum = sdf.minimum, maximum = sdf.maximum;
  if (!sdf.IsLocked())
  {
    minimum = std::numeric_limits<float>::infinity();
    maximum = -std::numeric_limits<float>::infinity();
    for (const float distance : sdf.grid.GetImmutableRawData())
    {
      if (distance < minimum) minimum = distance;
      if (distance > maximum) maximum = distance;
    }
  }
  const auto scale_color_value = [](float distance, float distance_extrema) {
    constexpr float color_scaling = 0.8f;
    constexpr float min_color_value = 0.2f;
    const float distance_ratio = static_cast<float>(std::abs(distance / distance_extrema));
    const float color_value = (distance_ratio * color_scaling) + min_color_value;
    return color_value;
  };
  // every cell is listed: each of them has the alpha above
  const Selection s = Select(sdf.grid, VGT_HIP_SELECT_ALL, 15, 0.0f, VGT_HIP_CELL_MEMBER_NONE, hip_device);
  return Colour(s, ExtentsOf(sdf.grid), [&](size_t k) {
    const float distance = s.values[k];
    ColorRGBA color{{0.0f, 0.0f, 0.0f, clamped_alpha}};
    if (distance > 0.0f)
      color[1] = scale_color_value(distance, maximum);
    else if (distance < 0.0f)
      color[0] = scale_color_value(distance, minimum);
    else
      color[2] = 1.0f;
    return color;
  });
}

DisplayCubes ExportSDFForDisplayCollisionOnly(const SignedDistanceField& sdf, float alpha, int hip_device)
{
  if (!sdf.grid.IsInitialized()) throw std::invalid_argument("Grid must be initialized");
  if (!(alpha > 0.0f)) return DisplayCubes();
  // distance <= 0.0: below or equal; a NaN compares false and gets the free colour, whose alpha is 0
  const Selection s = Select(sdf.grid, VGT_HIP_SELECT_ALL, VGT_HIP_CLASS_BELOW | VGT_HIP_CLASS_EQUAL, 0.0f,
                             VGT_HIP_CELL_MEMBER_NONE, hip_device);
  const ColorRGBA filled_color{{1.0f, 0.0f, 0.0f, alpha}};
  return Colour(s, ExtentsOf(sdf.grid), [&](size_t) { return filled_color; });
}

ComponentSurfaces ExtractComponentSurfaces(const OccupancyComponentMap& map, uint8_t component_types, int hip_device)
{
  return ExtractSurfaces(map, component_types, hip_device);
}

ComponentSurfaces ExtractComponentSurfaces(const TaggedObjectOccupancyComponentMap& map, uint8_t component_types,
                                           int hip_device)
{
  return ExtractSurfaces(map, component_types, hip_device);
}
}  // namespace vgt_hip
