// ComputeTravelCost / TracePaths of include/vgt_hip/travel_cost.hpp on the C ABI (vgt_hip_travel_cost,
// vgt_hip_cells_travel_cost, vgt_hip_trace_paths).
#include "../../../include/vgt_hip/travel_cost.hpp"
#include "host_internal.hpp"

#include <cmath>

namespace vgt_hip
{
namespace
{
using detail::SharedSdfContext;
using detail::ThrowForCode;

std::vector<int32_t> LinearIndices(const TravelCostField& shape, const std::vector<GridIndex>& indices)
{
  std::vector<int32_t> linear(indices.size());
  for (size_t i = 0; i < indices.size(); i++) linear[i] = static_cast<int32_t>(shape.LinearIndex(indices[i]));
  return linear;
}

// What the C ABI would refuse, refused before a device is asked for; then the outputs sized for the grid.
template <typename Grid>
TravelCostField Prepare(const Grid& grid, const std::vector<GridIndex>& sources, const TravelCostOptions& options)
{
  if (!grid.IsInitialized()) throw std::invalid_argument("Grid must be initialized");
  if (!options.source_costs.empty() && options.source_costs.size() != sources.size())
    throw std::invalid_argument("source_costs must be empty or hold one cost per source");
  if (options.weights[0] == 0u) throw std::invalid_argument("weights[0] (the axis moves) must be greater than zero");
  for (const uint32_t w : options.weights)
    if (w > 65535u) throw std::invalid_argument("a move weight must be at most 65535");
  if (options.cost_limit == VGT_HIP_TRAVEL_UNREACHED)
    throw std::invalid_argument("the cost limit must be at most 0xfffffffe (which means no limit)");
  TravelCostField field;
  field.nx = grid.NumXVoxels();
  field.ny = grid.NumYVoxels();
  field.nz = grid.NumZVoxels();
  if (field.nx * field.ny * field.nz >= (int64_t{1} << 31))
    throw std::invalid_argument("travel costs support grids below 2^31 cells");
  const size_t n = static_cast<size_t>(field.nx * field.ny * field.nz);
  field.cost.resize(n);
  if (options.with_toward) field.toward.resize(n);
  return field;
}

TravelCostField FromFloats(const DenseGrid& grid, int32_t mode, double threshold, const std::vector<GridIndex>& sources,
                           const TravelCostOptions& o)
{
  TravelCostField field = Prepare(grid, sources, o);
  const std::vector<int32_t> linear = LinearIndices(field, sources);
  const int rc = vgt_hip_travel_cost(
      SharedSdfContext(o.hip_device), grid.GetImmutableRawData().data(), field.nx, field.ny, field.nz, mode,
      o.unknown_is_filled ? 1 : 0, threshold, o.weights.data(), o.no_corner_cutting ? VGT_HIP_TRAVEL_NO_CORNER_CUTTING : 0u,
      linear.data(), o.source_costs.empty() ? nullptr : o.source_costs.data(), static_cast<int64_t>(linear.size()),
      o.cost_limit, field.cost.data(), o.with_toward ? field.toward.data() : nullptr, &field.num_reached);
  if (rc != VGT_HIP_OK) ThrowForCode(rc, vgt_hip_last_error());
  return field;
}

// A grid of cell records: uploaded, the predicate runs on the device copy.
template <typename Cell>
TravelCostField FromCells(const CellGrid<Cell>& map, int object_id_offset, const std::vector<GridIndex>& sources,
                          const TravelCostOptions& o)
{
  TravelCostField field = Prepare(map, sources, o);
  if (!o.objects_to_use.empty() && object_id_offset < 0)
    throw std::invalid_argument("this map type carries no object ids: objects_to_use must be empty");
  const std::vector<int32_t> linear = LinearIndices(field, sources);
  vgt_hip_ctx* const ctx = SharedSdfContext(o.hip_device);
  vgt_hip_cells* cells = nullptr;
  const int created = vgt_hip_cells_create(ctx, map.GetImmutableRawData().data(), field.nx, field.ny, field.nz,
                                           static_cast<int32_t>(sizeof(Cell)), object_id_offset, &cells);
  if (created != VGT_HIP_OK) ThrowForCode(created, vgt_hip_last_error());
  struct Destroy
  {
    vgt_hip_cells* cells;
    ~Destroy() { vgt_hip_cells_destroy(cells); }
  } destroy{cells};
  const int rc = vgt_hip_cells_travel_cost(
      ctx, cells, o.objects_to_use.empty() ? nullptr : o.objects_to_use.data(),
      static_cast<int64_t>(o.objects_to_use.size()), o.unknown_is_filled ? 1 : 0, o.weights.data(),
      o.no_corner_cutting ? VGT_HIP_TRAVEL_NO_CORNER_CUTTING : 0u, linear.data(),
      o.source_costs.empty() ? nullptr : o.source_costs.data(), static_cast<int64_t>(linear.size()), o.cost_limit,
      field.cost.data(), o.with_toward ? field.toward.data() : nullptr, &field.num_reached);
  if (rc != VGT_HIP_OK) ThrowForCode(rc, vgt_hip_last_error());
  return field;
}
}  // namespace

TravelCostField ComputeTravelCost(const OccupancyMap& map, const std::vector<GridIndex>& sources,
                                  const TravelCostOptions& options)
{
  if (!options.objects_to_use.empty())
    throw std::invalid_argument("this map type carries no object ids: objects_to_use must be empty");
  return FromFloats(map, VGT_HIP_TRAVEL_OCCUPANCY, 0.0, sources, options);
}
TravelCostField ComputeTravelCost(const OccupancyComponentMap& map, const std::vector<GridIndex>& sources,
                                  const TravelCostOptions& options)
{
  return FromCells(map, -1, sources, options);
}
TravelCostField ComputeTravelCost(const TaggedObjectOccupancyMap& map, const std::vector<GridIndex>& sources,
                                  const TravelCostOptions& options)
{
  return FromCells(map, 4, sources, options);
}
TravelCostField ComputeTravelCost(const TaggedObjectOccupancyComponentMap& map, const std::vector<GridIndex>& sources,
                                  const TravelCostOptions& options)
{
  return FromCells(map, 4, sources, options);
}

TravelCostField ComputeTravelCost(const SignedDistanceField& sdf, double minimum_distance,
                                  const std::vector<GridIndex>& sources, const TravelCostOptions& options)
{
  if (std::isnan(minimum_distance)) throw std::invalid_argument("minimum_distance must not be NaN");
  if (!options.objects_to_use.empty())
    throw std::invalid_argument("a distance field carries no object ids: objects_to_use must be empty");
  return FromFloats(sdf.grid, VGT_HIP_TRAVEL_SDF_ABOVE, minimum_distance, sources, options);
}

TracedPaths TracePaths(const TravelCostField& field, const std::vector<GridIndex>& starts, int32_t max_cells,
                       int hip_device)
{
  if (max_cells < 1) throw std::invalid_argument("max_cells must be at least 1");
  if (field.toward.empty() || field.toward.size() != static_cast<size_t>(field.nx * field.ny * field.nz))
    throw std::invalid_argument("the field holds no toward entries (computed without with_toward?)");
  TracedPaths paths;
  paths.max_cells = max_cells;
  paths.cells.assign(starts.size() * static_cast<size_t>(max_cells), -1);
  paths.lengths.assign(starts.size(), 0);
  paths.status.assign(starts.size(), static_cast<uint8_t>(VGT_HIP_TRACE_INVALID));
  if (starts.empty()) return paths;  // (nothing to do: no device is needed)
  const std::vector<int32_t> linear = LinearIndices(field, starts);
  const int rc = vgt_hip_trace_paths(SharedSdfContext(hip_device), field.toward.data(),
                                     static_cast<int64_t>(field.toward.size()), linear.data(),
                                     static_cast<int64_t>(linear.size()), max_cells, paths.cells.data(),
                                     paths.lengths.data(), paths.status.data());
  if (rc != VGT_HIP_OK) ThrowForCode(rc, vgt_hip_last_error());
  return paths;
}
}  // namespace vgt_hip
