// Host drivers of the HIP backend:
//   HipPointCloudVoxelizer     the sibling of CudaPointCloudVoxelizer / OpenCLPointCloudVoxelizer
//                              (device_pointcloud_voxelization.hpp:73-91), running
//                              DevicePointCloudVoxelizer::DoVoxelizePointClouds
//                              (device_pointcloud_voxelization.cpp:65-181) over the HIP helper;
//   ExtractSignedDistanceField the device implementation of
//                              OccupancyMap::ExtractSignedDistanceField<float>
//                              (occupancy_map.hpp:174-210).
#pragma once

#include <array>
#include <functional>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

struct vgt_hip_ctx;
struct vgt_hip_cells;

#include "hip_voxelization_helpers.h"
#include "host_types.hpp"

namespace vgt_hip
{
using voxelized_geometry_tools::pointcloud_voxelization::DeviceVoxelizationHelperInterface;
using voxelized_geometry_tools::pointcloud_voxelization::LoggingFunction;

// Host-clock phases of one VoxelizePointClouds call (seconds), for benchmarks: what VoxelizerRuntime's two numbers are made of.
struct VoxelizePhases
{
  double prepare_tracking_grids_s = 0;       // device buffer (pooled) + zeroing enqueued
  double filter_grid_enqueue_s = 0;          // page-locking the static environment + enqueueing its upload (not waited for)
  double raycast_s = 0;                      // per-cloud upload + raycast kernels, all clouds, dispatch threads joined
  double filter_grid_blocking_upload_s = 0;  // only with helpers that cannot defer the upload
  double filter_enqueue_s = 0;               // filter kernel enqueued
  double filter_and_download_s = 0;          // rest of the upload, filter kernel, download of the filtered grid (blocking)
  double release_s = 0;                      // device buffers back to the pool
  double total_s = 0;
  // by-value overload only: making the returned map (no cell touched) and waiting, before the download, for the threads
  // that fault its pages in
  double output_allocate_s = 0;
  double output_pages_wait_s = 0;
};

class HipPointCloudVoxelizer
{
public:
  // Options: DISPATCH_PARALLELIZE (1), DISPATCH_NUM_THREADS (-1 = hardware concurrency), plus
  // the helper's HIP_* options.  Throws std::runtime_error when no device can be used, like
  // CudaPointCloudVoxelizer's constructor (device_pointcloud_voxelization.cpp:183-192).
  explicit HipPointCloudVoxelizer(const std::map<std::string, int32_t>& options,
                                  const LoggingFunction& logging_fn = {});

  // PointCloudVoxelizationInterface::VoxelizePointClouds
  // (pointcloud_voxelization_interface.hpp:246-292), both overloads.
  OccupancyMap VoxelizePointClouds(
      const OccupancyMap& static_environment,
      const PointCloudVoxelizationFilterOptions& filter_options,
      const std::vector<PointCloudWrapperSharedPtr>& pointclouds,
      const std::function<void(const VoxelizerRuntime&)>& runtime_log_fn = {}) const;

  VoxelizerRuntime VoxelizePointClouds(
      const OccupancyMap& static_environment,
      const PointCloudVoxelizationFilterOptions& filter_options,
      const std::vector<PointCloudWrapperSharedPtr>& pointclouds,
      OccupancyMap& output_environment) const;

  // Phases of the most recent call that finished on this object (any thread).
  VoxelizePhases LastPhases() const
  {
    std::lock_guard<std::mutex> lock(phases_mutex_);
    return last_phases_;
  }

private:
  void EnforceAvailable() const;
  // both overloads; before_download (optional) runs after the filter kernel is enqueued and before the download starts
  VoxelizerRuntime DoVoxelizePointClouds(const OccupancyMap& static_environment,
                                         const PointCloudVoxelizationFilterOptions& filter_options,
                                         const std::vector<PointCloudWrapperSharedPtr>& pointclouds,
                                         OccupancyMap& output_environment,
                                         const std::function<void()>& before_download) const;
  std::unique_ptr<DeviceVoxelizationHelperInterface> helper_interface_;
  std::string device_name_ = "HipPointCloudVoxelizer";
  int dispatch_threads_ = 1;
  mutable std::mutex phases_mutex_;
  mutable VoxelizePhases last_phases_;
};

// OccupancyMap::ExtractSignedDistanceField<float>.  Throws std::invalid_argument for grids the
// reference rejects, std::runtime_error when no HIP device can be used (no CPU fallback).
SignedDistanceField ExtractSignedDistanceField(
    const OccupancyMap& map, const SignedDistanceFieldGenerationParameters& parameters);
// The same for a batch of maps of one size (e.g. the per-object or per-frame maps of a planner): one batched extraction
// (vgt_hip_sdf_batch_from_occupancy_f32) instead of a loop of calls; fields[i] belongs to maps[i] and is what the single
// call returns for it, bit for bit.  Throws std::invalid_argument when the maps' sizes differ.
std::vector<SignedDistanceField> ExtractSignedDistanceFields(
    const std::vector<const OccupancyMap*>& maps, const SignedDistanceFieldGenerationParameters& parameters);
// The free-standing SDF entry points share one context per device for the life of the process; that
// context keeps its device buffers between calls (no hipMalloc / hipFree per extraction).  This
// returns the memory (e.g. after one very large grid).
void ReleaseCachedDeviceMemory();

// ---- SDF consumers on the device, batched: one call for many query points / all voxels ----
// Results carry the reference's query semantics: has_value[i] == 0 <=> the reference's query object is empty.
struct DistanceEstimates
{
  std::vector<double> distance;     // EstimateDistanceQuery::Value()
  std::vector<uint8_t> has_value;   // EstimateDistanceQuery::HasValue()
};
struct Gradients
{
  std::vector<double> gradient;     // 3 per query / voxel: GradientQuery::Value().head<3>()
  std::vector<uint8_t> has_value;
};
// SignedDistanceField::EstimateLocationDistance for every point of `locations_xyz` (3 doubles per point, in the
// frame the field's origin transform maps to), signed_distance_field.hpp:808-833.
DistanceEstimates EstimateLocationDistances(const SignedDistanceField& sdf, const std::vector<double>& locations_xyz,
                                            int hip_device = 0);
// SignedDistanceField::ProjectLocationOutOfCollisionToMinimumDistance (:1111-1203) for every point of `locations_xyz`,
// with the field's inverse origin transform and rotation.  A batch reports per-point outcomes instead of throwing:
// status[i] is one of the VGT_HIP_PROJECT_* values of vgt_hip.h (0 clear of minimum_distance, 1 the start is outside
// the grid and returned unchanged, 2 flat gradient, 3 a step left the grid -- where the reference throws --, 4 still in
// collision after max_iterations steps), has_value[i] == 0 and a NaN position for 2, 3 and 4.  max_iterations == 0
// selects ceil(2 * (nx + ny + nz) / stepsize_multiplier); the reference's loop has no limit.
struct ProjectedPositions
{
  std::vector<double> position;     // 3 per point, in the frame of `locations_xyz`
  std::vector<uint8_t> has_value;
  std::vector<uint8_t> status;
  std::vector<int32_t> iterations;  // steps taken
};
ProjectedPositions ProjectLocationsOutOfCollision(const SignedDistanceField& sdf, const std::vector<double>& locations_xyz,
                                                  double minimum_distance = 0.0, double stepsize_multiplier = 0.1,
                                                  int32_t max_iterations = 0, int hip_device = 0);
// SignedDistanceField::GetLocationFineGradient (:1050-1091); throws std::runtime_error("Window size for fine
// gradient is too large for SDF") exactly when the reference does for one of the points.
Gradients GetLocationFineGradients(const SignedDistanceField& sdf, const std::vector<double>& locations_xyz,
                                   double nominal_window_size, int hip_device = 0);
// SignedDistanceField::GetIndexCoarseGradient at every voxel (:906-1016), X-major / Z fastest.
Gradients GetIndexCoarseGradients(const SignedDistanceField& sdf, bool enable_edge_gradients = false,
                                  int hip_device = 0);
// SignedDistanceField::ComputeLocalExtremaMap (:1205-1231): 3 doubles per voxel.
std::vector<double> ComputeLocalExtremaMap(const SignedDistanceField& sdf, int hip_device = 0);

// ---- connected components, spatial segments, component surfaces ----
struct ComponentLabels
{
  std::vector<uint32_t> labels;  // one per voxel, X-major / Z fastest; 0 = not labelled
  uint32_t count = 0;            // the largest label
};
// ExtractComponentSurfaces' component_types_to_extract (occupancy_component_map.hpp)
enum COMPONENT_TYPES : uint8_t { FILLED_COMPONENTS = 0x01, EMPTY_COMPONENTS = 0x02, UNKNOWN_COMPONENTS = 0x04 };
// component number -> grid indices (x, y, z) of its surface cells, in ascending linear order
using ComponentSurfaces = std::map<uint32_t, std::vector<std::array<int64_t, 3>>>;

// Holes and voids of one component (topology_computation.hpp:23-48): refuses negative numbers like the reference's class.
class NumberOfHolesAndVoids
{
public:
  NumberOfHolesAndVoids() = default;
  NumberOfHolesAndVoids(int32_t num_holes, int32_t num_voids);  // std::invalid_argument when either is negative
  int32_t NumHoles() const { return holes_; }
  int32_t NumVoids() const { return voids_; }

private:
  int32_t holes_ = 0;
  int32_t voids_ = 0;
};
// component number -> its holes and voids, for the components of the selected classes
using TopologicalInvariants = std::map<uint32_t, NumberOfHolesAndVoids>;

// ---- the other three map types ----
// OccupancyComponentMap::ExtractSignedDistanceField<float> (occupancy_component_map.hpp:270-306).
SignedDistanceField ExtractSignedDistanceField(
    const OccupancyComponentMap& map, const SignedDistanceFieldGenerationParameters& parameters);

// A tagged map's cells on the device, for any number of extractions.  The methods are the
// reference's (tagged_object_occupancy_map.hpp:199-378 and
// tagged_object_occupancy_component_map.hpp:361-540), float instantiation.
class DeviceTaggedObjectMap
{
public:
  DeviceTaggedObjectMap(const TaggedObjectOccupancyMap& map, int hip_device = 0);
  DeviceTaggedObjectMap(const TaggedObjectOccupancyComponentMap& map, int hip_device = 0);
  ~DeviceTaggedObjectMap();
  DeviceTaggedObjectMap(const DeviceTaggedObjectMap&) = delete;
  DeviceTaggedObjectMap& operator=(const DeviceTaggedObjectMap&) = delete;

  SignedDistanceField ExtractSignedDistanceField(
      const std::vector<uint32_t>& objects_to_use,
      const SignedDistanceFieldGenerationParameters& parameters) const;
  std::map<uint32_t, SignedDistanceField> MakeSeparateObjectSDFs(
      const std::vector<uint32_t>& object_ids,
      const SignedDistanceFieldGenerationParameters& parameters) const;
  std::map<uint32_t, SignedDistanceField> MakeAllObjectSDFs(
      const SignedDistanceFieldGenerationParameters& parameters) const;
  SignedDistanceField ExtractFreeAndNamedObjectsSignedDistanceField(
      const SignedDistanceFieldGenerationParameters& parameters) const;
  // distinct object ids > 0, ascending
  std::vector<uint32_t> ObjectIds() const;
  // The labels of UpdateConnectedComponents / UpdateSpatialSegments for the uploaded cells (one uint32 per voxel,
  // X-major / Z fastest) and their number: the same upload serves fields and labels.  The map itself is not written;
  // the free functions below do that.  `rotation`: of the map's origin transform (what the extrema map follows).
  ComponentLabels ConnectedComponents(bool connect_across_objects) const;
  ComponentLabels SpatialSegments(double connected_threshold,
                                  const SignedDistanceFieldGenerationParameters& parameters) const;
  // ComputeComponentTopology for the uploaded cells (vgt_hip_cells_component_topology): the invariants of the components
  // whose class component_types selects; `labels` (optional) receives the labelling it ran first.
  TopologicalInvariants ComponentTopology(bool connect_across_objects, uint8_t component_types,
                                          ComponentLabels* labels = nullptr) const;

private:
  void Upload(const void* cells, int cell_bytes, int object_id_offset, int hip_device);
  SignedDistanceField EmptyField(const SignedDistanceFieldGenerationParameters& parameters) const;
  ::vgt_hip_ctx* ctx_ = nullptr;  // the process's context of the device (not owned)
  ::vgt_hip_cells* cells_ = nullptr;
  DenseGrid shape_;  // origin / frame / sizes of the map, for the fields handed back
};

// OccupancyComponentMap::UpdateConnectedComponents (occupancy_component_map.cpp:447-509) and
// TaggedObjectOccupancyComponentMap::UpdateConnectedComponents (tagged_object_occupancy_component_map.cpp:689-773): the
// cells' `component` members receive the reference's numbers (1, 2, 3 ... in ascending order of the components' smallest
// linear index); returns their number.  std::invalid_argument for an uninitialised map or one of 2^31 cells and more.
uint32_t UpdateConnectedComponents(OccupancyComponentMap& map, int hip_device = 0);
uint32_t UpdateConnectedComponents(TaggedObjectOccupancyComponentMap& map, bool connect_across_objects,
                                   int hip_device = 0);
// Enclosed space (an extension; include/vgt_hip.h, vgt_hip_fill_enclosed): every cell that is not filled -- occupancy
// > 0.5, or == 0.5 when unknown_is_filled -- and that no chain of face-adjacent such cells joins to a face of the grid
// gets occupancy 1.0f, in place; nothing else of the map is written.  Returns the number of cells filled.
// The OccupancyComponentMap overload leaves the cells' `component` members as they are: they describe the map before
// the fill and are invalid after a fill that returns more than 0 (this layer's map types keep no validity flag of
// their own to clear: call UpdateConnectedComponents again, as after any other change of an occupancy).
// std::invalid_argument for an uninitialised map or one of 2^31 cells and more.
int64_t FillEnclosedSpace(OccupancyMap& map, bool unknown_is_filled = true, int hip_device = 0);
int64_t FillEnclosedSpace(OccupancyComponentMap& map, bool unknown_is_filled = true, int hip_device = 0);
// TaggedObjectOccupancyComponentMap::UpdateSpatialSegments (:775-868) as one device chain (SDF -> local extrema map,
// rotated by the map's origin transform -> segments); writes the cells' `spatial_segment` members.  Runs on
// sdf_parameters.hip_device.
uint32_t UpdateSpatialSegments(TaggedObjectOccupancyComponentMap& map, double connected_threshold,
                               const SignedDistanceFieldGenerationParameters& sdf_parameters);
// ExtractComponentSurfaces (occupancy_component_map.cpp:511-571, tagged variant :485-541) from the cells' current
// `component` members: the device selects the surface cells into one compact ordered list with their components
// (vgt_hip_cells_select, VGT_HIP_SELECT_COMPONENT_SURFACE), the host splits that list by component.  No dense mask
// comes back.
ComponentSurfaces ExtractComponentSurfaces(const OccupancyComponentMap& map, uint8_t component_types,
                                           int hip_device = 0);
ComponentSurfaces ExtractComponentSurfaces(const TaggedObjectOccupancyComponentMap& map, uint8_t component_types,
                                           int hip_device = 0);
// ComputeComponentTopology (occupancy_component_map.cpp:594-653, tagged_object_occupancy_component_map.cpp:566-625):
// labels the map like UpdateConnectedComponents -- the cells' `component` members are written, as by the reference's
// method -- and returns holes and voids of every component whose class component_types selects (csrc/topology_kernels.hip;
// include/vgt_hip.h defines the numbers and names the one deliberate difference from the reference, Z + 1).
// std::invalid_argument for an uninitialised map, component_types outside 1..7, a map whose vertex lattice
// (nx + 1)(ny + 1)(nz + 1) reaches 2^31, and -- from NumberOfHolesAndVoids -- a component whose count comes out negative.
TopologicalInvariants ComputeComponentTopology(OccupancyComponentMap& map, uint8_t component_types, int hip_device = 0);
TopologicalInvariants ComputeComponentTopology(TaggedObjectOccupancyComponentMap& map, uint8_t component_types,
                                               bool connect_across_objects, int hip_device = 0);
// ---- surface cells and display exports as compact lists (csrc/host/hip_display.cc) ----
// IsSurfaceIndex (occupancy_map.cpp:201-246 and the same text in the other three map types) as a list: the grid indices
// (x, y, z) of every cell for which it is true, in ascending linear order.  The device selects
// (VGT_HIP_SELECT_SURFACE_26, include/vgt_hip.h); std::invalid_argument for an uninitialised map or one of 2^31 cells
// and more.
using GridIndices = std::vector<std::array<int64_t, 3>>;
GridIndices SurfaceIndices(const OccupancyMap& map, int hip_device = 0);
GridIndices SurfaceIndices(const OccupancyComponentMap& map, int hip_device = 0);
GridIndices SurfaceIndices(const TaggedObjectOccupancyMap& map, int hip_device = 0);
GridIndices SurfaceIndices(const TaggedObjectOccupancyComponentMap& map, int hip_device = 0);

// What ros_interface::ExportVoxelGridToRViz (ros_interface.hpp:92-148) puts into a CUBE_LIST marker: the cells whose
// colour has alpha > 0, in X, Y, Z loop order; points[i] is the cell's centre in the grid frame, colors[i] its colour.
// The marker's pose is the map's OriginTransform(), its scale the voxel size, its frame the map's Frame().
// NOT PINNED by the reference's sources available here: the centre is (index + 0.5) * voxel size per axis,
// in double (GridIndexToLocationInGridFrame lives in common_robotics_utilities).
using ColorRGBA = std::array<float, 4>;  // r, g, b, a
struct DisplayCubes
{
  std::vector<std::array<double, 3>> points;
  std::vector<ColorRGBA> colors;
};
// ros_interface.cpp's ExportForDisplay / ExportForSeparateDisplay / ExportSurfacesForDisplay: > 0.5 collision_color,
// < 0.5 free_color, everything else unknown_color; the surface variant keeps IsSurfaceIndex cells only.  A class whose
// colour has alpha <= 0 is left out of the device's selection.  ExportForSeparateDisplay: {collision only, free only,
// unknown only}.
DisplayCubes ExportForDisplay(const OccupancyMap& map, const ColorRGBA& collision_color, const ColorRGBA& free_color,
                              const ColorRGBA& unknown_color, int hip_device = 0);
DisplayCubes ExportForDisplay(const OccupancyComponentMap& map, const ColorRGBA& collision_color,
                              const ColorRGBA& free_color, const ColorRGBA& unknown_color, int hip_device = 0);
DisplayCubes ExportForDisplay(const TaggedObjectOccupancyMap& map, const ColorRGBA& collision_color,
                              const ColorRGBA& free_color, const ColorRGBA& unknown_color, int hip_device = 0);
DisplayCubes ExportForDisplay(const TaggedObjectOccupancyComponentMap& map, const ColorRGBA& collision_color,
                              const ColorRGBA& free_color, const ColorRGBA& unknown_color, int hip_device = 0);
std::array<DisplayCubes, 3> ExportForSeparateDisplay(const OccupancyMap& map, const ColorRGBA& collision_color,
                                                     const ColorRGBA& free_color, const ColorRGBA& unknown_color,
                                                     int hip_device = 0);
std::array<DisplayCubes, 3> ExportForSeparateDisplay(const OccupancyComponentMap& map, const ColorRGBA& collision_color,
                                                     const ColorRGBA& free_color, const ColorRGBA& unknown_color,
                                                     int hip_device = 0);
std::array<DisplayCubes, 3> ExportForSeparateDisplay(const TaggedObjectOccupancyMap& map,
                                                     const ColorRGBA& collision_color, const ColorRGBA& free_color,
                                                     const ColorRGBA& unknown_color, int hip_device = 0);
std::array<DisplayCubes, 3> ExportForSeparateDisplay(const TaggedObjectOccupancyComponentMap& map,
                                                     const ColorRGBA& collision_color, const ColorRGBA& free_color,
                                                     const ColorRGBA& unknown_color, int hip_device = 0);
DisplayCubes ExportSurfacesForDisplay(const OccupancyMap& map, const ColorRGBA& collision_color,
                                      const ColorRGBA& free_color, const ColorRGBA& unknown_color, int hip_device = 0);
DisplayCubes ExportSurfacesForDisplay(const OccupancyComponentMap& map, const ColorRGBA& collision_color,
                                      const ColorRGBA& free_color, const ColorRGBA& unknown_color, int hip_device = 0);
DisplayCubes ExportSurfacesForDisplay(const TaggedObjectOccupancyMap& map, const ColorRGBA& collision_color,
                                      const ColorRGBA& free_color, const ColorRGBA& unknown_color, int hip_device = 0);
DisplayCubes ExportSurfacesForDisplay(const TaggedObjectOccupancyComponentMap& map, const ColorRGBA& collision_color,
                                      const ColorRGBA& free_color, const ColorRGBA& unknown_color, int hip_device = 0);
// ExportConnectedComponentsForDisplay (ros_interface.cpp:356-389, 1030-1063): a cell whose occupancy != 0.5 (a NaN too)
// gets palette_fn(component); a cell == 0.5 the same with color_unknown_components, else grey (0.5, 0.5, 0.5, 1).
// NOT PINNED: the reference's palette is common_robotics_utilities' LookupUniqueColor, which is not available here; the
// palette is the caller's function.  It is called once per listed cell, on the host.
using ComponentPalette = std::function<ColorRGBA(uint32_t component)>;
DisplayCubes ExportConnectedComponentsForDisplay(const OccupancyComponentMap& map, bool color_unknown_components,
                                                 const ComponentPalette& palette_fn, int hip_device = 0);
DisplayCubes ExportConnectedComponentsForDisplay(const TaggedObjectOccupancyComponentMap& map,
                                                 bool color_unknown_components, const ComponentPalette& palette_fn,
                                                 int hip_device = 0);
// ExportSDFForDisplay (ros_interface.hpp:332-381): alpha clamped to [0, 1]; distance > 0 green, < 0 red, each
// |distance / extremum| * 0.8f + 0.2f in float, else blue.  The extrema are the field's cached minimum / maximum when it
// is locked, else those of its values.  ExportSDFForDisplayCollisionOnly (:383-411): the cells with distance <= 0 in
// (1, 0, 0, alpha).
DisplayCubes ExportSDFForDisplay(const SignedDistanceField& sdf, float alpha = 0.01f, int hip_device = 0);
DisplayCubes ExportSDFForDisplayCollisionOnly(const SignedDistanceField& sdf, float alpha = 0.01f, int hip_device = 0);
}  // namespace vgt_hip
