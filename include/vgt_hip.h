/*
 * vgt_hip.h -- C ABI of libvgt_hip.so, the MI355X (gfx950) backend for the SDF/EDT and
 * pointcloud-raycast-voxelization hot path of calderpg/voxelized_geometry_tools.
 *
 * This is the drop-in boundary: plain pointers and sizes, no C++ or torch types.
 * Each entry point names the reference interface it stands in for (paths relative to
 * the reference checkout; I/ = include/voxelized_geometry_tools/,
 * S/ = src/voxelized_geometry_tools/).  The reference-side binding a maintainer would
 * add is shown in INTEGRATION.md; include/vgt_hip/ holds the C++ glue that implements
 * the reference's DeviceVoxelizationHelperInterface on top of these calls.
 *
 * Conventions
 *   - every function returns 0 on success, non-zero on failure; the message is then
 *     available from vgt_hip_last_error() (thread-local).  No exception crosses the ABI.
 *   - dense grids are X-major / Z fastest: index = x*(ny*nz) + y*nz + z
 *     (S/cuda_voxelization_helpers.cu:683-684).
 *   - "host" pointers are ordinary process memory; "dev" pointers are HIP device memory
 *     on the context's device.  The caller owns every buffer it passes in; the library
 *     owns what it hands out behind the opaque handles.
 *   - there is no CPU fallback: without a usable HIP device vgt_hip_create() fails.
 */
#ifndef VGT_HIP_H_
#define VGT_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
/* The library is built with -fvisibility=hidden: the functions declared between this push and the pop at the end
 * of the header are its whole dynamic symbol table (tests/test_capi_symbols.py checks `nm -D`). */
#if defined(__GNUC__) || defined(__clang__)
#pragma GCC visibility push(default)
#endif

#define VGT_HIP_ABI_VERSION 2

typedef struct vgt_hip_ctx vgt_hip_ctx;       /* one context <-> one device + one stream */
typedef struct vgt_hip_grids vgt_hip_grids;   /* tracking grids (TrackingGridsHandle)    */
typedef struct vgt_hip_filter vgt_hip_filter; /* filter grid (FilterGridHandle)          */

/* Error codes (also the return values). */
enum {
  VGT_HIP_OK = 0,
  VGT_HIP_ERR_INVALID_ARGUMENT = 1, /* maps to std::invalid_argument in the C++ glue */
  VGT_HIP_ERR_RUNTIME = 2,          /* HIP error; maps to std::runtime_error          */
  VGT_HIP_ERR_UNAVAILABLE = 3       /* no device / device index out of range           */
};

int vgt_hip_abi_version(void);
const char* vgt_hip_last_error(void);

/* ---- device enumeration: hip_helpers::GetAvailableDevices()
 *      (sibling of cuda_helpers::GetAvailableDevices, S/cuda_voxelization_helpers.cu:791-821) */
int vgt_hip_device_count(int* count);
int vgt_hip_device_name(int device, char* buffer, size_t buffer_size);

/* ---- context: the state behind hip_helpers::MakeHipVoxelizationHelper(options, log)
 *      (I/cuda_voxelization_helpers.h:19-24; ctor S/cuda_voxelization_helpers.cu:562-639).
 *      threads_per_block <= 0 selects the defaults: 256 for the filter and the small-cloud raycast
 *      kernel, and the size the direction-sorted raycast kernel is tuned for (512: its LDS table, the
 *      re-deal of rays by walk length and the flush scale with the workgroup); a positive value (a
 *      multiple of 64, at most 1024) is used for all of them.  Options HIP_DEVICE /
 *      HIP_THREADS_PER_BLOCK of the C++ glue land here. */
int vgt_hip_create(int device, int threads_per_block, vgt_hip_ctx** out_ctx);
void vgt_hip_destroy(vgt_hip_ctx* ctx);
/* A context keeps the device buffers of its host-pointer entry points (SDF input / field /
 * workspace, point-cloud staging) across calls, growing them on demand, so that repeated calls do
 * not pay for hipMalloc / hipFree (the reference allocates per call, S/cuda_voxelization_helpers.cu:
 * 676-680).  vgt_hip_trim gives that memory back (waits for the context's stream first). */
int vgt_hip_trim(vgt_hip_ctx* ctx);
/* Run all work of this context on an externally owned hipStream_t (e.g. the caller's
 * framework stream); NULL is HIP's legacy default stream.  vgt_hip_reset_stream goes back to the
 * context's own (non-blocking) stream.  Both drain the stream in use first. */
int vgt_hip_set_stream(vgt_hip_ctx* ctx, void* hip_stream);
int vgt_hip_reset_stream(vgt_hip_ctx* ctx);
int vgt_hip_synchronize(vgt_hip_ctx* ctx);
int vgt_hip_device_of(const vgt_hip_ctx* ctx);

/* =====================  pointcloud raycast voxelization  ===================== */

/* DeviceVoxelizationHelperInterface::PrepareTrackingGrids
 * (I/device_voxelization_interface.hpp:148-149; S/cuda_voxelization_helpers.cu:641-658):
 * num_grids zeroed grids of int32[2*num_cells] = (seen_free, seen_filled) per cell,
 * grid g starting at element offset g*num_cells*2. */
int vgt_hip_tracking_grids_create(vgt_hip_ctx* ctx, int64_t num_cells, int32_t num_grids,
                                  vgt_hip_grids** out_grids);
void vgt_hip_tracking_grids_destroy(vgt_hip_grids* grids);
int64_t vgt_hip_tracking_grids_num_cells(const vgt_hip_grids* grids);
int32_t vgt_hip_tracking_grids_num_grids(const vgt_hip_grids* grids);
int64_t vgt_hip_tracking_grids_offset(const vgt_hip_grids* grids, size_t grid_index);
void* vgt_hip_tracking_grids_dev_ptr(const vgt_hip_grids* grids, size_t grid_index);
int vgt_hip_tracking_grids_clear(vgt_hip_ctx* ctx, vgt_hip_grids* grids);

/* DeviceVoxelizationHelperInterface::RaycastPoints
 * (I/device_voxelization_interface.hpp:151-158; kernel S/cuda_voxelization_helpers.cu:73-356):
 * float32 DDA of num_points xyz points (AoS, cloud frame) through the grid, transform =
 * 16 floats column-major (grid <- cloud).  Safe to call concurrently from several host
 * threads on one context with distinct grid_index
 * (S/device_pointcloud_voxelization.cpp:147-149).  Returns after the kernel has been
 * enqueued AND the host point buffer has been consumed. */
int vgt_hip_raycast_points_f32(vgt_hip_ctx* ctx, vgt_hip_grids* grids, size_t grid_index,
                               const float* points_xyz_host, int64_t num_points,
                               float max_range, const float* grid_pointcloud_transform,
                               float voxel_size, float inverse_voxel_size,
                               float grid_x_size, float grid_y_size, float grid_z_size,
                               int32_t num_x_voxels, int32_t num_y_voxels,
                               int32_t num_z_voxels);
/* PointCloud2 ingestion: the message's data buffer is uploaded as it is and the
 * kernel reads x, y, z in place -- instead of the per-point virtual
 * CopyPointLocationIntoFloatPtr gather of S/device_pointcloud_voxelization.cpp:130-136 over
 * PointCloud2Wrapper (I/pointcloud_voxelization_ros_interface.hpp:68-91).
 *   cloud_data_host  sensor_msgs/PointCloud2::data, num_points = width * height records
 *   point_step       bytes per record;  xyz_offset = offset of field "x" (y and z follow, FLOAT32;
 *                    S/pointcloud_voxelization_ros_interface.cpp:49-78).  Both multiples of 4. */
int vgt_hip_raycast_pointcloud2_f32(vgt_hip_ctx* ctx, vgt_hip_grids* grids, size_t grid_index,
                                    const uint8_t* cloud_data_host, int64_t num_points,
                                    int64_t point_step, int64_t xyz_offset, float max_range,
                                    const float* grid_pointcloud_transform, float voxel_size,
                                    float inverse_voxel_size, float grid_x_size,
                                    float grid_y_size, float grid_z_size, int32_t num_x_voxels,
                                    int32_t num_y_voxels, int32_t num_z_voxels);
/* Same, points already resident on the device (bench / device-resident pipelines). */
int vgt_hip_raycast_points_f32_dev(vgt_hip_ctx* ctx, vgt_hip_grids* grids, size_t grid_index,
                                   const float* points_xyz_dev, int64_t num_points,
                                   float max_range, const float* grid_pointcloud_transform,
                                   float voxel_size, float inverse_voxel_size,
                                   float grid_x_size, float grid_y_size, float grid_z_size,
                                   int32_t num_x_voxels, int32_t num_y_voxels,
                                   int32_t num_z_voxels);
/* HIP_EXACT_FP64 mode: float64 DDA with the arithmetic of the reference's CPU voxelizer
 * (CpuPointCloudVoxelizer::DoRaycastSinglePoint, S/cpu_pointcloud_voxelization.cpp:208-436);
 * points and transform are doubles. */
int vgt_hip_raycast_points_f64(vgt_hip_ctx* ctx, vgt_hip_grids* grids, size_t grid_index,
                               const double* points_xyz_host, int64_t num_points,
                               double max_range, const double* grid_pointcloud_transform,
                               double voxel_size, double inverse_voxel_size,
                               double grid_x_size, double grid_y_size, double grid_z_size,
                               int32_t num_x_voxels, int32_t num_y_voxels,
                               int32_t num_z_voxels);

/* DeviceVoxelizationHelperInterface::PrepareFilterGrid
 * (I/device_voxelization_interface.hpp:160-161; S/cuda_voxelization_helpers.cu:701-708):
 * device copy of the static environment's float occupancy. */
int vgt_hip_filter_grid_create(vgt_hip_ctx* ctx, int64_t num_cells,
                               const float* occupancy_host, vgt_hip_filter** out_filter);
/* The same without waiting for the copy: the upload runs on a copy stream beside whatever the context does next (the
 * raycasts of HipPointCloudVoxelizer, which prepares the filter grid first), and the calls that use the grid --
 * filter, retrieve, destroy -- are ordered behind it.  `occupancy_host` must stay valid and unchanged until one of
 * vgt_hip_retrieve_filtered_grid / vgt_hip_filter_grid_destroy has returned for this grid (it is page-locked by the
 * library for that time). */
int vgt_hip_filter_grid_create_deferred(vgt_hip_ctx* ctx, int64_t num_cells,
                                        const float* occupancy_host, vgt_hip_filter** out_filter);
void vgt_hip_filter_grid_destroy(vgt_hip_filter* filter);
int64_t vgt_hip_filter_grid_num_cells(const vgt_hip_filter* filter);
/* The grid's device buffer.  Waits for a deferred upload first (the pointer is then usable on any stream); NULL, with the
 * reason in vgt_hip_last_error(), when that wait fails. */
void* vgt_hip_filter_grid_dev_ptr(const vgt_hip_filter* filter);

/* DeviceVoxelizationHelperInterface::FilterTrackingGrids
 * (I/device_voxelization_interface.hpp:163-166; kernel S/cuda_voxelization_helpers.cu:358-426).
 * ratio_in_double = 0: float ratio as the reference device kernels; 1: double ratio as
 * PointCloudVoxelizationFilterOptions::CountsSeenAs (I/pointcloud_voxelization_interface.hpp:55-86). */
int vgt_hip_filter_tracking_grids(vgt_hip_ctx* ctx, const vgt_hip_grids* grids,
                                  float percent_seen_free, int32_t outlier_points_threshold,
                                  int32_t num_cameras_seen_free, vgt_hip_filter* filter);
int vgt_hip_filter_tracking_grids_f64(vgt_hip_ctx* ctx, const vgt_hip_grids* grids,
                                      double percent_seen_free,
                                      int32_t outlier_points_threshold,
                                      int32_t num_cameras_seen_free, vgt_hip_filter* filter);

/* DeviceVoxelizationHelperInterface::RetrieveTrackingGrid / RetrieveFilteredGrid
 * (I/device_voxelization_interface.hpp:168-173; S/cuda_voxelization_helpers.cu:734-767):
 * blocking copies of num_cells*8 / num_cells*4 bytes; all earlier work of the context
 * has finished when they return. */
int vgt_hip_retrieve_tracking_grid(vgt_hip_ctx* ctx, const vgt_hip_grids* grids,
                                   size_t grid_index, void* host_out);
int vgt_hip_retrieve_filtered_grid(vgt_hip_ctx* ctx, const vgt_hip_filter* filter,
                                   void* host_out);

/* ==========================  signed distance field  ========================== */

/* OccupancyMap::ExtractSignedDistanceField<float>(params)
 * (I/occupancy_map.hpp:174-210 -> I/signed_distance_field_generation.hpp:39-285 ->
 *  S/signed_distance_field_generation.cpp:258-391).  occupancy_host / sdf_host are
 * float[nx*ny*nz]; out_min / out_max receive what SignedDistanceField::Lock() caches
 * (I/signed_distance_field.hpp:765-787) and may be NULL.  Blocking.  The two host arrays are
 * page-locked for the call, the context keeps its device buffers between calls (vgt_hip_trim
 * returns them), and grids of 2^27 voxels and more overlap upload, kernels and download chunk
 * by chunk on three streams (the threshold is fixed in the product library; testing builds can move
 * it with vgt_hip_testing_set_host_pipeline_min_voxels); the result does not depend on it. */
int vgt_hip_sdf_from_occupancy_f32(vgt_hip_ctx* ctx, const float* occupancy_host,
                                   int64_t nx, int64_t ny, int64_t nz, double resolution,
                                   int unknown_is_filled, int add_virtual_border,
                                   float* sdf_host, float* out_min, float* out_max);
/* Same for the map types whose predicate is not a pure occupancy threshold
 * (I/occupancy_component_map.hpp:270-306, I/tagged_object_occupancy_map.hpp:199-247):
 * the caller evaluates is_filled on the host into one byte per voxel. */
int vgt_hip_sdf_from_mask_u8(vgt_hip_ctx* ctx, const uint8_t* filled_mask_host, int64_t nx,
                             int64_t ny, int64_t nz, double resolution,
                             int add_virtual_border, float* sdf_host, float* out_min,
                             float* out_max);

/* Device-resident form (bench, device pipelines): input and output stay
 * in HBM, the caller provides the scratch workspace.  minmax_dev, if non-NULL, receives
 * {min, max} as two floats on the device after the call (stream-ordered). */
size_t vgt_hip_sdf_workspace_bytes(int64_t nx, int64_t ny, int64_t nz);
/* As above for a context set to EDT variant `variant` (0 = the default pipeline = vgt_hip_sdf_workspace_bytes; the
 * cross-check variant 1 exists in testing builds only, the product library returns 0 for it).  The default
 * workspace holds the class records of pass 1 (0.25 bytes per voxel), the int32 intermediate field (4 bytes per voxel)
 * and the line passes' scratch, which grows with the axis lengths, not with the volume (the spilled stack entries and
 * sign words of the at most 4096 waves in flight: 1.1 GB for a 1024^3 grid, 4.4 GB at 2048 x 2048 x 1024; the launches
 * use as many workgroups as the scratch they are given holds).  5.8 GB in all at 1024^3. */
size_t vgt_hip_sdf_workspace_bytes_for_variant(int64_t nx, int64_t ny, int64_t nz, int variant);
int vgt_hip_sdf_dev(vgt_hip_ctx* ctx, const float* occupancy_dev, int64_t nx, int64_t ny,
                    int64_t nz, double resolution, int unknown_is_filled,
                    int add_virtual_border, float* sdf_dev, void* workspace_dev,
                    size_t workspace_bytes, float* minmax_dev);
/* As vgt_hip_sdf_dev, bracketing each kernel with HIP events on the context's stream.
 * kernel_ms[0..2] = pass 1 (class records), Y-pass, X-pass(+finalize) durations of this call. Blocking. */
int vgt_hip_sdf_dev_timed(vgt_hip_ctx* ctx, const float* occupancy_dev, int64_t nx,
                          int64_t ny, int64_t nz, double resolution, int unknown_is_filled,
                          int add_virtual_border, float* sdf_dev, void* workspace_dev,
                          size_t workspace_bytes, float* minmax_dev, float* kernel_ms);
/* ---- Batches: `batch` grids of the same extents in one call (many small maps, or many masks of one map).
 * The reference extracts one field per call and loops -- TaggedObjectOccupancyMap::MakeSeparateObjectSDFs /
 * MakeAllObjectSDFs run one whole ExtractSignedDistanceField per object id
 * (I/tagged_object_occupancy_map.hpp:249-290) -- and on the grid sizes of its own examples and tests (8^3 - 40^3)
 * one extraction is a few hundred work items for a GPU that holds 16 384 waves.  Here the three passes run ONCE
 * over the whole batch: the grids lie one after the other, [batch][nx][ny][nz], in the input, in the output and in
 * every intermediate buffer; pass 1 and the Y pass see one grid of batch * nx slices (their lines never leave a
 * slice), the X pass deals (grid, y, z segment) items to the same persistent workgroups, every grid has its own
 * extrema.  Results are bit-identical to `batch` single calls.
 *   limits      the per-axis limit of every SDF entry point for nx, ny, nz; batch * nx * ny < 2^28
 *   minmax_dev  NULL or 2 * batch floats: {min, max} of grid 0, of grid 1, ...
 * vgt_hip_sdf_batch_from_occupancy_f32 takes `batch` host arrays (any addresses) and hands back `batch` fields and
 * their extrema (out_min / out_max: NULL or `batch` floats each); it cuts batches that exceed the limits or 2 GiB of
 * device buffers into several launches by itself.  Blocking. */
size_t vgt_hip_sdf_batch_workspace_bytes(int64_t batch, int64_t nx, int64_t ny, int64_t nz);
int vgt_hip_sdf_batch_dev(vgt_hip_ctx* ctx, const float* occupancy_dev, int64_t batch, int64_t nx, int64_t ny,
                          int64_t nz, double resolution, int unknown_is_filled, int add_virtual_border,
                          float* sdf_dev, void* workspace_dev, size_t workspace_bytes, float* minmax_dev);
int vgt_hip_sdf_batch_from_occupancy_f32(vgt_hip_ctx* ctx, const float* const* occupancy_host, int64_t batch,
                                         int64_t nx, int64_t ny, int64_t nz, double resolution,
                                         int unknown_is_filled, int add_virtual_border, float* const* sdf_host,
                                         float* out_min, float* out_max);
#ifdef VGT_HIP_TESTING
/* ---- Testing builds only: libvgt_hip_testing.so (make -C voxelized_geometry_tools_amd/csrc testing), which the parity
 * tests load next to the product library.  The product library exports none of these and contains none of the
 * cross-check implementations. ----
 * Selects the EDT pipeline (both exact): 0 = default (pass 1 writes class records, lane-per-line sweeps: one lane runs
 * the Felzenszwalb-Huttenlocher stack of one line, stack tops in LDS, any extent); 1 = the independent cross-check: an
 * int16 distance field along Z as pass 1, then a pruned outward search per voxel straight from HBM (any size). */
int vgt_hip_set_edt_variant(vgt_hip_ctx* ctx, int variant);
/* The final conversion float(sqrt(double(d2)) * resolution) has a fast evaluation with an exact fallback
 * (csrc/edt_device.hpp); this runs both over d2 in [first_d2, first_d2 + count) on the device and reports how many
 * results differ (must be 0) and the first differing d2 (UINT64_MAX if none). */
int vgt_hip_debug_finalize_check(vgt_hip_ctx* ctx, int64_t first_d2, int64_t count,
                                 double resolution, uint64_t* mismatches,
                                 uint64_t* first_mismatch);
/* Smallest grid (voxels) that the host-pointer SDF entry points pipeline (upload / kernels / download overlapped);
 * default 2^27, negative = never.  Lets the tests run that path on small grids. */
int vgt_hip_testing_set_host_pipeline_min_voxels(int64_t min_voxels);
/* Lines of at most `rows` rows (0 - 128) take the short-line kernels (csrc/edt_short_kernels.hip) instead of the sweeps,
 * whatever the number of items: lets the tests and benches run either formulation on any length.  Negative: back to the
 * product's rule (64 rows; the Y pass of launches of at most 1024 items: 128). */
int vgt_hip_testing_set_short_line_rows(int rows);
/* After a vgt_hip_sdf_dev call with `workspace_dev` (waits for the stream): counts[0] = Z lines of one class among the
 * counts[1] lines that pass 1's counting workgroups saw (one workgroup in 32): the ratio the X pass chose its kernel by. */
int vgt_hip_testing_one_class_counts(vgt_hip_ctx* ctx, const void* workspace_dev, int64_t nx, int64_t ny, int64_t nz,
                                     uint32_t* counts);
/* At most `slots` workgroups per launch of the sweep passes (process-wide), so that a small grid is a launch of several rounds
 * of items; 0 or negative: back to the product's 4096. */
int vgt_hip_testing_set_sweep_slots(int slots);
/* Which kernel the plain X pass with 32-bit stack entries runs on a whole single grid (csrc/edt_sweep_kernels.hip, kCoarse;
 * process-wide): 0 = by scene, the product's rule -- where the launch qualifies (lines of 512 rows and more, two rounds of
 * items) both kernels are enqueued and pass 1's count of one-class lines decides on the device; 1 = the coarse-hull kernel
 * wherever it applies (lines of more than 64 rows), whatever it costs; 2 = never.  Results are bit-identical. */
int vgt_hip_testing_set_coarse_hull(int mode);
/* After a vgt_hip_sdf_dev call with `workspace_dev` (waits for the stream): which plain X kernel did the work, as the kernel
 * itself wrote it to its scratch head.  0 = neither (another kernel), 1 = plain, 2 = coarse hull; + 4 when both were
 * enqueued and the device chose. */
int vgt_hip_testing_x_pass_choice(vgt_hip_ctx* ctx, const void* workspace_dev, int64_t nx, int64_t ny, int64_t nz,
                                  int32_t* choice);
/* At most `workgroups` workgroups per launch of vgt_hip_check_spheres[_dev] (process-wide), so that a few configurations
 * already make its persistent waves stride; 0 or negative: back to the product's limit. */
int vgt_hip_testing_set_check_spheres_workgroups(int workgroups);
/* The same for the launches of vgt_hip_rasterize_spheres[_dev] and vgt_hip_spheres_cover_points[_dev], so that small
 * inputs already make their persistent waves and workgroups take several trips. */
int vgt_hip_testing_set_sphere_volume_workgroups(int workgroups);
/* The same for the evaluation launches of vgt_hip_align_points[_dev], so that a few (pose, 4096-point block) items
 * already make its persistent workgroups take several trips. */
int vgt_hip_testing_set_align_workgroups(int workgroups);
/* The same for the launches of vgt_hip_forward_kinematics[_dev] (workgroups of 64 configurations) and
 * vgt_hip_clearance_joint_gradient[_dev], so that a few hundred configurations already make their persistent waves
 * stride.  It caps the launch of vgt_hip_solve_ik[_dev] (workgroups of 64 problems) in the same way. */
int vgt_hip_testing_set_kinematics_workgroups(int workgroups);
/* The same for the launches of vgt_hip_check_motions[_dev] (one workgroup per motion), so that a few motions already make
 * its persistent waves stride. */
int vgt_hip_testing_set_motion_workgroups(int workgroups);
/* The same for the launches of vgt_hip_clearance_cost[_dev] (one workgroup per tile of configurations), so that a few
 * hundred configurations already make its persistent waves stride. */
int vgt_hip_testing_set_cost_workgroups(int workgroups);
/* What a launch of vgt_hip_check_motions[_dev] for a tree of num_links links and a model of num_spheres spheres is made
 * of, computed by the function the launcher itself takes it from: the samples of a tile (vgt_hip_motion_tile_samples)
 * and whether the sphere table sits in LDS (1) or is read through the cache (0).  Lets the tests pick shapes on both
 * sides of that choice whatever the kernel's constants are.  VGT_HIP_ERR_INVALID_ARGUMENT: a NULL output, a negative
 * sphere count, or a tree the kernel does not take. */
int vgt_hip_testing_motion_launch_geometry(int64_t num_links, int64_t num_spheres, int32_t* tile_samples,
                                           int32_t* table_in_lds);
/* The same for vgt_hip_clearance_cost[_dev], in the gradient form (gradient_form != 0: joint_gradient or
 * num_without_gradient is asked for) or the cost-only form: the configurations of a tile (vgt_hip_cost_tile_samples),
 * the passes of phase B buffered in front of phase C, and whether the sphere table and what the walk reads of the links
 * sit in LDS (1) or are read through the cache (0). */
int vgt_hip_testing_cost_launch_geometry(int64_t num_links, int64_t num_spheres, int gradient_form, int32_t* tile_samples,
                                         int32_t* passes, int32_t* table_in_lds, int32_t* links_in_lds);
/* The same for the launches of vgt_hip_check_self_collision[_poses][_dev] (one workgroup per tile of configurations). */
int vgt_hip_testing_set_self_collision_workgroups(int workgroups);
/* The same for the launches of vgt_hip_check_motions_with_self[_dev] (one workgroup per motion). */
int vgt_hip_testing_set_motion_self_workgroups(int workgroups);
/* Counting runs of vgt_hip_rasterize_spheres[_dev] (process-wide): while counters_dev is not NULL every launch adds to
 * its three uint64, on the device, the (cell, sphere) tests it made, those that covered, and the atomics it issued (a
 * counting variant of the kernel; the answers are the same).  The caller zeroes and reads them.  NULL: back to the
 * product's kernel. */
int vgt_hip_testing_set_sphere_volume_counters(uint64_t* counters_dev);
/* Pass 1 alone, for a test of the record format itself (csrc/vgt_internal.hpp, ClassRecord): the class records of a
 * device-resident occupancy grid, [x][64-voxel word][y] x 4 uint32 (mask_lo, mask_hi, below2, above2), into records_dev
 * (vgt_hip_testing_class_record_bytes bytes); summary_dev (optional): the 4-byte slab summaries per line, in which case the
 * records carry no one-class marks (a slab cannot know).  Blocking. */
size_t vgt_hip_testing_class_record_bytes(int64_t nx, int64_t ny, int64_t nz);
int vgt_hip_testing_class_records_dev(vgt_hip_ctx* ctx, const float* occupancy_dev, int64_t nx, int64_t ny, int64_t nz,
                                      int unknown_is_filled, int64_t z_offset, void* records_dev, void* summary_dev);
#endif /* VGT_HIP_TESTING */

/* ---- SDFs of the map types whose cells carry more than an occupancy ----
 * Replaces the per-voxel `is_filled_fn` + EDT of
 *   OccupancyComponentMap::ExtractSignedDistanceField            occupancy_component_map.hpp:270-306
 *   TaggedObjectOccupancyMap::ExtractSignedDistanceField         tagged_object_occupancy_map.hpp:199-247
 *     ::MakeSeparateObjectSDFs / ::MakeAllObjectSDFs             :249-290
 *     ::ExtractFreeAndNamedObjectsSignedDistanceField            :292-378
 *   TaggedObjectOccupancyComponentMap (same four)                tagged_object_occupancy_component_map.hpp:361-540
 * The raw cell store (`GetImmutableRawData().data()`) is uploaded once; every extraction after that
 * evaluates its predicate on the device and runs the same exact EDT.
 *   cell_bytes        sizeof the cell: 8 (OccupancyComponentCell, TaggedObjectOccupancyCell) or
 *                     16 (TaggedObjectOccupancyComponentCell); 4 (plain OccupancyCell) also works.
 *                     The float occupancy is the first member of all of them.
 *   object_id_offset  byte offset of the uint32 object id inside a cell (4 for both tagged types),
 *                     or -1 for a type without one (OccupancyComponentCell: the component is not
 *                     used by its SDF). */
typedef struct vgt_hip_cells vgt_hip_cells;
int vgt_hip_cells_create(vgt_hip_ctx* ctx, const void* cells_host, int64_t nx, int64_t ny,
                         int64_t nz, int32_t cell_bytes, int32_t object_id_offset,
                         vgt_hip_cells** out_cells);
void vgt_hip_cells_destroy(vgt_hip_cells* cells);
/* Distinct object ids > 0 in ascending order (what MakeAllObjectSDFs collects in a std::set).
 * Writes at most `capacity` ids; *count receives the number found. */
int vgt_hip_cells_object_ids(vgt_hip_ctx* ctx, vgt_hip_cells* cells, uint32_t* ids_out,
                             int64_t capacity, int64_t* count);
/* ExtractSignedDistanceField(objects_to_use, parameters): a cell is filled when its occupancy is
 * (> 0.5, or == 0.5 with unknown_is_filled) AND (num_objects == 0 or its object id is listed).
 * One call per object id = MakeSeparateObjectSDFs. */
int vgt_hip_cells_sdf(vgt_hip_ctx* ctx, vgt_hip_cells* cells, const uint32_t* objects_to_use,
                      int64_t num_objects, double resolution, int unknown_is_filled,
                      int add_virtual_border, float* sdf_host, float* out_min, float* out_max);
/* MakeSeparateObjectSDFs(object_ids) / MakeAllObjectSDFs (:249-290) as ONE batch: sdf_host[k] receives
 * ExtractSignedDistanceField({object_ids[k]}) -- the field of vgt_hip_cells_sdf with that one id, bit for bit --
 * and out_min[k] / out_max[k] (NULL or num_objects floats each) its extrema.  One pass over the cells writes every
 * object's mask, the EDT passes run once over all of them (see "Batches" above), the fields come back through
 * page-locked copies.  Object lists that exceed the limits of a batch or 4 GiB of device buffers are cut into several
 * launches.  Blocking. */
int vgt_hip_cells_object_sdfs(vgt_hip_ctx* ctx, vgt_hip_cells* cells, const uint32_t* object_ids,
                              int64_t num_objects, double resolution, int unknown_is_filled, int add_virtual_border,
                              float* const* sdf_host, float* out_min, float* out_max);
/* ExtractFreeAndNamedObjectsSignedDistanceField: the field of all filled cells where it is >= 0,
 * the field of the filled cells of named objects (id > 0) where that is <= 0, else 0. */
int vgt_hip_cells_free_and_named_objects_sdf(vgt_hip_ctx* ctx, vgt_hip_cells* cells,
                                             double resolution, int unknown_is_filled,
                                             int add_virtual_border, float* sdf_host,
                                             float* out_min, float* out_max);

/* ---- deferred per-kernel timing (benchmarks) ----
 * Between start and stop every vgt_hip_sdf_dev call (or vgt_hip_sdf_slab_begin_dev /
 * _finish_dev pair called with kernel_ms == NULL) on this context records HIP events around its
 * kernels on the stream they run on, WITHOUT synchronising; stop waits for the stream once and
 * returns, per call, the milliseconds of {pass 1 (+ slab record fix-up), Y pass, X pass}.  Calls beyond
 * max_calls are not recorded. */
int vgt_hip_timing_start(vgt_hip_ctx* ctx, int32_t max_calls);
int vgt_hip_timing_stop(vgt_hip_ctx* ctx, float* kernel_ms /* [max_calls][3] */,
                        int32_t* num_calls);

/* ---- SDF consumers ----
 * SignedDistanceField<float>::GetGridAlignedIndexCoarseGradient
 * (I/signed_distance_field.hpp:923-1016) for every voxel of a field at once: gradient[3 * i + a]
 * (double), i = x*ny*nz + y*nz + z.  Voxels on a face of the grid get one-sided differences when
 * enable_edge_gradients is set, otherwise NaN and has_value[i] = 0 (has_value may be NULL).
 * rotation (NULL or 9 doubles, row-major) = the rotation of OriginTransform(): with it the
 * result is GetIndexCoarseGradient's (:906-921). */
int vgt_hip_sdf_coarse_gradient(vgt_hip_ctx* ctx, const float* sdf_host, int64_t nx, int64_t ny,
                                int64_t nz, double resolution, int enable_edge_gradients,
                                const double* rotation, double* gradient_host,
                                uint8_t* has_value_host);
/* Same on device buffers (e.g. straight after vgt_hip_sdf_dev, without leaving the device). */
int vgt_hip_sdf_coarse_gradient_dev(vgt_hip_ctx* ctx, const float* sdf_dev, int64_t nx, int64_t ny,
                                    int64_t nz, double resolution, int enable_edge_gradients,
                                    const double* rotation, double* gradient_dev,
                                    uint8_t* has_value_dev);

/* Batched point queries against a float SDF (x, y, z as 3 doubles per query, in the frame
 * `grid_from_world` maps from: 16 doubles column-major = InverseOriginTransform, NULL = the grid
 * frame itself).
 *   vgt_hip_sdf_estimate_distance   SignedDistanceField::EstimateLocationDistance (trilinear estimate
 *                                   over the eight surrounding cell centres, I/signed_distance_field.hpp:
 *                                   808-833 over :259-378); distance[i] = NaN and has_value[i] = 0 for a
 *                                   query outside the grid.
 *   vgt_hip_sdf_fine_gradient       ::GetLocationFineGradient (:1050-1091 over :214-254): differences of
 *                                   seven estimates at +-|nominal_window_size| along the query frame's
 *                                   axes; 3 doubles per query.  A query in the grid whose window leaves it
 *                                   on both sides of an axis is the reference's std::runtime_error
 *                                   "Window size for fine gradient is too large for SDF": the call then
 *                                   returns VGT_HIP_ERR_INVALID_ARGUMENT with that message.
 * The one operation whose order the reference takes from common_robotics_utilities
 * (TrilinearInterpolate) is evaluated along x, then y, then z, each as a*(1-t) + b*t in double
 * (csrc/cell_kernels.hip); results therefore agree with the reference to rounding (tests: 1e-5). */
int vgt_hip_sdf_estimate_distance(vgt_hip_ctx* ctx, const float* sdf_host, int64_t nx, int64_t ny, int64_t nz,
                                  double resolution, const double* grid_from_world, const double* query_xyz_host,
                                  int64_t num_queries, double* distance_host, uint8_t* has_value_host);
int vgt_hip_sdf_estimate_distance_dev(vgt_hip_ctx* ctx, const float* sdf_dev, int64_t nx, int64_t ny, int64_t nz,
                                      double resolution, const double* grid_from_world, const double* query_xyz_dev,
                                      int64_t num_queries, double* distance_dev, uint8_t* has_value_dev);
int vgt_hip_sdf_fine_gradient(vgt_hip_ctx* ctx, const float* sdf_host, int64_t nx, int64_t ny, int64_t nz,
                              double resolution, const double* grid_from_world, const double* query_xyz_host,
                              int64_t num_queries, double nominal_window_size, double* gradient_host,
                              uint8_t* has_value_host);

/* SignedDistanceField::ProjectLocationOutOfCollisionToMinimumDistance (I/signed_distance_field.hpp:1111-1203;
 * ProjectLocationOutOfCollision is minimum_distance = 0) for N points at once, one lane per point, the whole loop in
 * one kernel.  Frames as above: queries and results are in the frame `grid_from_world` maps from (16 doubles
 * column-major, NULL = the grid frame); `rotation` (9 doubles row-major = the rotation of OriginTransform(), NULL =
 * none) turns the grid-aligned gradient into that frame, and the step is taken there.  Per point:
 *   1. not in the grid (the has_value test of vgt_hip_sdf_estimate_distance; NaN and infinite coordinates too): the
 *      point is returned unchanged, with a value.
 *   2. margin = minimum_distance + resolution * stepsize_multiplier * 1e-3, max_step = resolution *
 *      stepsize_multiplier, d = the estimate of vgt_hip_sdf_estimate_distance.
 *   3. while d <= minimum_distance: g = the coarse gradient (edge gradients on, rotated) of the cell the point is in;
 *      no value, or norm <= resolution * 0.25: no result; else point += (g / norm) * min(max_step, margin - d) and
 *      d is estimated again.  (A NaN estimate ends the loop like the reference's comparison does.)
 * The operation order of the step, which the reference takes from Eigen's norm() / normalized(), is, in double and
 * without contraction:
 *   norm = sqrt((gx*gx + gy*gy) + gz*gz);   n_a = g_a / norm;   loc_a = loc_a + n_a * step
 * so results agree with the reference to rounding and are bit-identical to a restatement in this order.
 * Outputs per point (has_value, status and iterations may each be NULL):
 *   status               meaning                                                        position      has_value
 *   0 OK                 clear of minimum_distance, possibly after 0 steps              projected     1
 *   1 OUTSIDE            the start is not in the grid                                   the input     1
 *   2 FLAT_GRADIENT      norm <= resolution * 0.25, or the gradient has no value        NaN x3        0
 *   3 LEFT_GRID          a step left the grid                                           NaN x3        0
 *   4 ITERATION_LIMIT    still d <= minimum_distance after max_iterations steps         NaN x3        0
 *   iterations[i] = the steps taken (int32).
 * Two divergences from the reference, both where it leaves the outcome open:
 *   - The reference's loop has no iteration limit and does not end where the gradients of neighbouring cells point at
 *     each other while the estimate stays <= minimum_distance (a free corridor narrower than twice the clearance).
 *     Here the loop ends after max_iterations steps with status 4; max_iterations == 0 selects
 *     ceil(2 * (nx + ny + nz) / stepsize_multiplier), twice the full-size steps of a straight path across the grid:
 *     a safety limit, not a tuning number.
 *   - A step can carry the point off the grid (edge gradients are on); the reference then takes .Value() of an empty
 *     estimate, which throws.  Here that point gets status 3 and the call succeeds.
 * VGT_HIP_ERR_INVALID_ARGUMENT before any device work: stepsize_multiplier not positive and finite, minimum_distance
 * NaN, max_iterations < 0, resolution not positive, a grid of 2^31 cells or more, a NULL required pointer. */
#define VGT_HIP_PROJECT_OK 0
#define VGT_HIP_PROJECT_OUTSIDE 1
#define VGT_HIP_PROJECT_FLAT_GRADIENT 2
#define VGT_HIP_PROJECT_LEFT_GRID 3
#define VGT_HIP_PROJECT_ITERATION_LIMIT 4
int vgt_hip_sdf_project_out_of_collision(vgt_hip_ctx* ctx, const float* sdf_host, int64_t nx, int64_t ny, int64_t nz,
                                         double resolution, const double* grid_from_world, const double* rotation,
                                         const double* query_xyz_host, int64_t num_queries, double minimum_distance,
                                         double stepsize_multiplier, int32_t max_iterations, double* position_host,
                                         uint8_t* has_value_host, uint8_t* status_host, int32_t* iterations_host);
/* Same on device buffers (e.g. straight after vgt_hip_sdf_dev); enqueued on the context's stream, not blocking. */
int vgt_hip_sdf_project_out_of_collision_dev(vgt_hip_ctx* ctx, const float* sdf_dev, int64_t nx, int64_t ny, int64_t nz,
                                             double resolution, const double* grid_from_world, const double* rotation,
                                             const double* query_xyz_dev, int64_t num_queries, double minimum_distance,
                                             double stepsize_multiplier, int32_t max_iterations, double* position_dev,
                                             uint8_t* has_value_dev, uint8_t* status_dev, int32_t* iterations_dev);

/* N segments a -> b cast through a float occupancy map or a float SDF, one lane per segment: is the segment free, and
 * if not, which voxel does it hit first and how far along; for an SDF also how close it comes to an obstacle.  The edge
 * check of a sampling planner, a line-of-sight test, a depth image of a map.  Read-only.
 * A segment is 6 doubles (a, b) in the frame `grid_from_world` maps from (16 doubles column-major; NULL = the grid
 * frame: the coordinates are then used as they are, without a multiplication by an identity).  With a transform X,
 * A = X a and B = X b, each row evaluated as ((m0*x + m4*y) + m8*z) + m12.  Everything is done in double without
 * contraction, inverse_voxel_size = 1.0 / resolution, grid_size[a] = n[a] * resolution.
 * Cells examined, in order: the cells the reference's f64 voxelizer walk (S/cpu_pointcloud_voxelization.cpp:208-436,
 * the walk of vgt_hip_raycast_points_f64) visits for origin A, point B and max_range = +infinity -- the ray is never
 * clipped and tmax of the slab test starts at +infinity; the origin's index and the in-grid test are taken per
 * segment; the slab entry with its `t2 > tmax` quirk, the 1e-10 nudge, the walk's index conversion, the tie order
 * X, then Y, then Z, the `cur[a] == end[a]` break and leaving the walk at the first out-of-grid cell are the walk's.
 * The in-grid cells of the walk come first, in walk order; the final cell (which the reference marks first) comes
 * last, if it is in the grid.  No cell appears twice.  So a segment cast through a map that the voxelizer carved sees
 * exactly the cells the voxelizer would have marked free.
 * One divergence from the reference's walk: when the origin is outside the grid and tmin + 1e-10 > length (tmin of the
 * slab test, length = the norm the walk computes), the segment ends before it reaches the grid and examines nothing.
 * (The reference there walks backwards from the grid's entry point, over cells that are not on the segment.)  A
 * segment of length zero outside the grid (direction 0 / 0) examines nothing by the same rule.
 * Predicate (`mode`):
 *   VGT_HIP_SEGMENT_OCCUPANCY  the field is float occupancy; a cell is a hit when occ > 0.5f || (unknown_is_filled &&
 *                              occ == 0.5f), the SDF's own predicate.  NaN is never a hit.
 *   VGT_HIP_SEGMENT_SDF_BELOW  the field is a float SDF; a cell is a hit when (double)value <= threshold, the
 *                              projection's comparison.  NaN is never a hit, +-infinity compare as they are.
 * Examination stops at the first hit, unless flags & VGT_HIP_SEGMENT_WALK_THROUGH: then all cells are examined, and
 * the hit outputs still describe the first hit.
 * Outputs per segment (`status` is required, every other output may be NULL):
 *   status (uint8)          0 CLEAR: at least one cell examined, none a hit;  1 HIT;  2 MISSED_GRID: no cell examined;
 *                           3 INVALID: one of the 6 coordinates is not finite, nothing is examined.  A segment of
 *                           length zero inside the grid examines exactly its own cell.
 *   hit_index (int32)       the linear index x*ny*nz + y*nz + z of the first hit, or -1
 *   cells_examined (int32)  the number of cells examined; without WALK_THROUGH the hit cell is the last of them
 *   hit_fraction (double)   where the segment A -> B enters the hit cell's box, as a fraction of the segment, in double:
 *                             lo_a = idx_a * resolution, hi_a = (idx_a + 1) * resolution;
 *                             for each axis with d_a = B_a - A_a != 0: ta = (lo_a - A_a) / d_a, tb = (hi_a - A_a) / d_a;
 *                             enter = 0.0, raised by m = min(ta, tb) of each such axis in the order x, y, z
 *                             (if (m > enter) enter = m);  the result is enter > 1.0 ? 1.0 : enter;  NaN without a hit
 *   min_value (float), min_index (int32)   SDF mode only (with VGT_HIP_SEGMENT_OCCUPANCY either is an invalid
 *                           argument): the least non-NaN value among the examined cells and its index, ties to the
 *                           first cell in examination order; NaN and -1 when no non-NaN value was examined.  With
 *                           WALK_THROUGH: the clearance of the whole segment at cell centres.
 * VGT_HIP_ERR_INVALID_ARGUMENT before any device work: a NULL required pointer, a resolution that is not positive and
 * finite, an unknown mode or flag bit, a NaN threshold in SDF mode, a grid of 2^31 cells or more, a negative extent,
 * num_segments < 0.  num_segments == 0 and an empty grid succeed and touch nothing. */
#define VGT_HIP_SEGMENT_OCCUPANCY 0
#define VGT_HIP_SEGMENT_SDF_BELOW 1
#define VGT_HIP_SEGMENT_WALK_THROUGH 1u
#define VGT_HIP_SEGMENT_CLEAR 0
#define VGT_HIP_SEGMENT_HIT 1
#define VGT_HIP_SEGMENT_MISSED_GRID 2
#define VGT_HIP_SEGMENT_INVALID 3
int vgt_hip_cast_segments(vgt_hip_ctx* ctx, const float* field_host, int64_t nx, int64_t ny, int64_t nz,
                          double resolution, int32_t mode, int unknown_is_filled, double threshold, uint32_t flags,
                          const double* grid_from_world, const double* segments_host, int64_t num_segments,
                          uint8_t* status_host, int32_t* hit_index_host, double* hit_fraction_host,
                          int32_t* cells_examined_host, float* min_value_host, int32_t* min_index_host);
/* Same with the field, the segments and the outputs on the device (e.g. straight after vgt_hip_sdf_dev); enqueued on
 * the context's stream, not blocking.  The transform is a host array. */
int vgt_hip_cast_segments_dev(vgt_hip_ctx* ctx, const float* field_dev, int64_t nx, int64_t ny, int64_t nz,
                              double resolution, int32_t mode, int unknown_is_filled, double threshold, uint32_t flags,
                              const double* grid_from_world, const double* segments_dev, int64_t num_segments,
                              uint8_t* status_dev, int32_t* hit_index_dev, double* hit_fraction_dev,
                              int32_t* cells_examined_dev, float* min_value_dev, int32_t* min_index_dev);

/* ---- Sphere models checked against an SDF ----
 * B configurations of a body modelled as S spheres attached to L links: for every configuration, how close the worst
 * sphere comes to an obstacle, which sphere that is, and which way is out.  The collision check of a planner whose robot
 * is not a point; forward kinematics stays with the caller (the call takes link poses, not joint angles).  Read-only.
 * Inputs:
 *   sphere_xyzr   4 doubles per sphere: the centre in its link's frame and the radius
 *   sphere_link   one int32 per sphere, a value in [0, L); in any order
 *   link_poses    [B][L][16] doubles, column-major: world_from_link, the memory of a std::vector<Eigen::Isometry3d> per
 *                 configuration.  Only the elements 0-2, 4-6, 8-10 and 12-14 are read.
 *   grid_from_world, rotation   as for vgt_hip_sdf_project_out_of_collision: 16 doubles column-major and 9 doubles
 *                 row-major, each may be NULL, both host arrays in both forms.
 * Per (configuration b, sphere s), in double and without contraction:
 *   w_r       = ((m[r]*x + m[4+r]*y) + m[8+r]*z) + m[12+r] for r = 0, 1, 2, with m the pose of sphere_link[s] in
 *               configuration b: the order of vgt_hip_cast_segments' transform.
 *   d         = the estimate of vgt_hip_sdf_estimate_distance at w: the same code, grid_from_world applied as that
 *               function applies it, the same has-value test (a non-finite w therefore has no value).
 *   clearance = d - radius.
 *   gradient  = the coarse gradient, edge gradients on and rotated by `rotation`, of the cell w lies in: what step 3 of
 *               vgt_hip_sdf_project_out_of_collision takes.  NaN x3 where the sphere has no value or the gradient has none.
 * Outputs per configuration (`status` is required, every other output may be NULL):
 *   num_outside (int32)    spheres without a value (not in the grid)
 *   num_below (int32)      spheres with a value and clearance <= minimum_clearance (the projection's comparison: NaN is
 *                          never below, +-infinity compare as they are)
 *   min_clearance (double), min_sphere (int32)   the least non-NaN clearance among the spheres with a value and the index
 *                          of its sphere, ties to the lowest index; NaN and -1 when there is none
 *   min_gradient (3 doubles)   `gradient` of min_sphere; NaN x3 when min_sphere == -1
 *   status (uint8)         1 COLLISION: num_below > 0, or flags & VGT_HIP_SPHERES_OUTSIDE_IS_COLLISION and
 *                          num_outside > 0;  otherwise 0 CLEAR when min_sphere != -1;  otherwise 2 NO_VALUE: nothing was
 *                          comparable.
 * Outputs per sphere (each may be NULL): sphere_clearance [B][S], NaN without a value; sphere_gradient [B][S][3].
 * VGT_HIP_ERR_INVALID_ARGUMENT before any device work: a NULL required pointer (ctx, sdf, status; the model's two arrays
 * when S > 0; link_poses when S > 0 and B > 0), a resolution that is not positive and finite, a NaN minimum_clearance,
 * an unknown flag bit, a negative extent or count, num_links == 0 with num_spheres > 0, a grid of 2^31 cells or more,
 * 2^31 or more spheres, links or configurations, B * S >= 2^31; and, for the host form only, a sphere_link outside
 * [0, L) or a radius that is negative or NaN: the message names the first such sphere ("sphere 17: ...").
 * The device form cannot look at device memory: there a link outside [0, L) makes that sphere one "without a value",
 * counted in num_outside, and the kernel forms no address from it; a negative or NaN radius is used as it is.
 * B == 0, S == 0 and an empty grid succeed.  With S == 0 or an empty grid nothing is comparable: every configuration gets
 * NaN and -1, num_below 0, num_outside 0 resp. S, and the status the rules above give (NO_VALUE; COLLISION for an empty
 * grid with S > 0 under VGT_HIP_SPHERES_OUTSIDE_IS_COLLISION); the host form then needs no device. */
#define VGT_HIP_SPHERES_OUTSIDE_IS_COLLISION 1u
#define VGT_HIP_SPHERES_CLEAR 0
#define VGT_HIP_SPHERES_COLLISION 1
#define VGT_HIP_SPHERES_NO_VALUE 2
int vgt_hip_check_spheres(vgt_hip_ctx* ctx, const float* sdf_host, int64_t nx, int64_t ny, int64_t nz, double resolution,
                          const double* grid_from_world, const double* rotation, const double* sphere_xyzr_host,
                          const int32_t* sphere_link_host, int64_t num_spheres, const double* link_poses_host,
                          int64_t num_links, int64_t num_configurations, double minimum_clearance, uint32_t flags,
                          uint8_t* status_host, double* min_clearance_host, int32_t* min_sphere_host,
                          int32_t* num_below_host, int32_t* num_outside_host, double* min_gradient_host,
                          double* sphere_clearance_host, double* sphere_gradient_host);
/* Same with every array on the device except the two transforms (e.g. the field straight after vgt_hip_sdf_dev, the
 * poses straight out of a batched forward kinematics); enqueued on the context's stream, not blocking. */
int vgt_hip_check_spheres_dev(vgt_hip_ctx* ctx, const float* sdf_dev, int64_t nx, int64_t ny, int64_t nz,
                              double resolution, const double* grid_from_world, const double* rotation,
                              const double* sphere_xyzr_dev, const int32_t* sphere_link_dev, int64_t num_spheres,
                              const double* link_poses_dev, int64_t num_links, int64_t num_configurations,
                              double minimum_clearance, uint32_t flags, uint8_t* status_dev, double* min_clearance_dev,
                              int32_t* min_sphere_dev, int32_t* num_below_dev, int32_t* num_outside_dev,
                              double* min_gradient_dev, double* sphere_clearance_dev, double* sphere_gradient_dev);

/* ---- Sphere models into voxel grids and onto point clouds: swept volumes, self-filter ----
 * The same body the other way round: which cells of a grid, or which points of a cloud, the spheres of B configurations
 * cover, and the least configuration that does.  Over the cells of a grid that is the swept volume of a motion (a
 * reservation, the overlap of two plans, a time-stamped occupancy); over the points of a depth cloud it is the
 * self-filter in front of the voxelizer.  The model and the poses are those of vgt_hip_check_spheres: sphere_xyzr [S][4]
 * doubles, sphere_link [S] int32, link_poses [B][L][16] doubles column-major of which only the elements 0-2, 4-6, 8-10 and
 * 12-14 are read.  Everything in double and without contraction:
 *   w_r       = ((m[r]*x + m[4+r]*y) + m[8+r]*z) + m[12+r] for r = 0, 1, 2, with m the pose of sphere_link[s] in
 *               configuration b: the expression of vgt_hip_check_spheres.
 *   R         = radius + padding; `padding` is one double per call, finite, possibly negative.
 *   usable    a sphere with a link in [0, L), a finite w and a finite R >= 0 (in the grid form also a finite centre c in
 *             the grid frame).  A sphere that is not usable covers nothing: this rule, and not the comparison below,
 *             decides every non-finite case.
 *   covers(q) ((dx*dx + dy*dy) + dz*dz) <= R*R with d_a = q_a - c_a.  R == 0 covers a location that equals the centre.
 * The answer is a minimum over a set, so it does not depend on the order of the work.
 *
 * Grid form.  nx x ny x nz cells at `resolution`, linear index x*ny*nz + y*nz + z, fewer than 2^31 cells.
 *   grid_from_world   16 doubles column-major, or NULL for the grid's own frame (a host array in both forms)
 *   c_a               = M[a]*w0 + M[4+a]*w1 + M[8+a]*w2 + M[12+a], left to right (the order of the SDF queries'
 *                     grid_from_world); c = w with NULL
 *   q_a               = (i_a + 0.5) * resolution: the centre of cell (i_x, i_y, i_z)
 *   first_configuration [cell] (int32)   first_configuration_base + b for the least b with a sphere that covers the
 *                     cell, -1 where there is none.  first_configuration_base >= 0 and base + B <= 2^31 - 1.
 *   Without VGT_HIP_SPHERES_KEEP the call first sets every entry to -1.  With it the array is input and output: an entry
 *   ends as the UNSIGNED minimum of what it held and what this call finds (-1 is the greatest unsigned value), so a
 *   motion can be rasterised in several calls with rising bases, in any order, with the same result.  The host form
 *   uploads the array first.
 *
 * Point form.  points_xyz [N][3] float32, the voxelizer's format; world_from_points 16 doubles column-major (the cloud's
 * origin transform, a host array in both forms) or NULL.  Each coordinate is converted to double, then
 *   q_r = ((T[r]*px + T[4+r]*py) + T[8+r]*pz) + T[12+r], or q = p with NULL,
 * and covers(q) is tested against c = w in the world frame; no grid is involved.  A point with a non-finite coordinate
 * or a non-finite q is covered by nothing.  Every output may be NULL, but not all of them:
 *   first_configuration [N] (int32)   the least b that covers the point, or -1 (no base here)
 *   first_sphere [N] (int32)          the least s of that b that covers it, or -1
 *   filtered_xyz [N][3] (float32)     the point's own three floats bit for bit where nothing covers it, a quiet NaN in
 *                                     all three where something does; may be the input array itself.  The raycast entry
 *                                     points skip non-finite points, so this is a self-filtered cloud as it stands.
 *
 * VGT_HIP_ERR_INVALID_ARGUMENT before any device work, outputs untouched: a NULL required pointer (ctx; the model's two
 * arrays when S > 0; link_poses when S > 0 and B > 0; first_configuration in the grid form; points when N > 0 and at
 * least one output in the point form), a resolution that is not positive and finite, a NaN or infinite padding, an
 * unknown flag bit (the point form knows none), a negative extent or count, num_links == 0 with num_spheres > 0, a grid
 * of 2^31 cells or more, 2^31 or more spheres, links, configurations or points, B * S >= 2^31, a
 * first_configuration_base that is negative or with base + B > 2^31 - 1; and, for the host forms only, a sphere_link
 * outside [0, L) or a radius that is negative or NaN: the message names the first such sphere ("sphere 17: ...").
 * The device forms cannot look at device memory: there a radius that makes R negative or NaN, or a link outside
 * [0, L), makes the sphere not usable by the rule above, and the kernel forms no address from such a link.
 * B == 0, S == 0, N == 0 and an empty grid succeed.  With B == 0 or S == 0 the grid form still writes -1 everywhere
 * unless VGT_HIP_SPHERES_KEEP, the point form still writes -1 and the plain copy (the host forms then need no device). */
#define VGT_HIP_SPHERES_KEEP 1u
int vgt_hip_rasterize_spheres(vgt_hip_ctx* ctx, int64_t nx, int64_t ny, int64_t nz, double resolution,
                              const double* grid_from_world, const double* sphere_xyzr_host,
                              const int32_t* sphere_link_host, int64_t num_spheres, const double* link_poses_host,
                              int64_t num_links, int64_t num_configurations, double padding,
                              int64_t first_configuration_base, uint32_t flags, int32_t* first_configuration_host);
/* Same with the model, the poses and the output on the device; enqueued on the context's stream, not blocking. */
int vgt_hip_rasterize_spheres_dev(vgt_hip_ctx* ctx, int64_t nx, int64_t ny, int64_t nz, double resolution,
                                  const double* grid_from_world, const double* sphere_xyzr_dev,
                                  const int32_t* sphere_link_dev, int64_t num_spheres, const double* link_poses_dev,
                                  int64_t num_links, int64_t num_configurations, double padding,
                                  int64_t first_configuration_base, uint32_t flags, int32_t* first_configuration_dev);
int vgt_hip_spheres_cover_points(vgt_hip_ctx* ctx, const float* points_xyz_host, int64_t num_points,
                                 const double* world_from_points, const double* sphere_xyzr_host,
                                 const int32_t* sphere_link_host, int64_t num_spheres, const double* link_poses_host,
                                 int64_t num_links, int64_t num_configurations, double padding, uint32_t flags,
                                 int32_t* first_configuration_host, int32_t* first_sphere_host, float* filtered_xyz_host);
/* Same with the cloud, the model, the poses and the outputs on the device (e.g. filtered_xyz_dev straight into
 * vgt_hip_raycast_points_f32_dev); enqueued on the context's stream, not blocking. */
int vgt_hip_spheres_cover_points_dev(vgt_hip_ctx* ctx, const float* points_xyz_dev, int64_t num_points,
                                     const double* world_from_points, const double* sphere_xyzr_dev,
                                     const int32_t* sphere_link_dev, int64_t num_spheres, const double* link_poses_dev,
                                     int64_t num_links, int64_t num_configurations, double padding, uint32_t flags,
                                     int32_t* first_configuration_dev, int32_t* first_sphere_dev,
                                     float* filtered_xyz_dev);

/* ---- Point clouds aligned to an SDF, batched over pose hypotheses ----
 * Where is the sensor with respect to the map?  A cloud of N points, B initial poses, a signed distance field: every
 * pose is evaluated (how far from `target_distance` the field is at the transformed points), refined by up to K damped
 * Gauss-Newton steps on that residual, and returned with its score.  K = 0 only scores: the measurement model of a
 * particle filter.  Read-only on the field and the cloud; nothing is synchronised with the host between iterations.
 * Inputs:
 *   points_xyz    [N][3] float32, the voxelizer's format (as vgt_hip_spheres_cover_points takes it).  A point with a
 *                 non-finite coordinate is skipped: it is counted nowhere and contributes +0.0.
 *   poses         [B][16] doubles, column-major: world_from_points per hypothesis (as link_poses of
 *                 vgt_hip_check_spheres).  Elements 0-2, 4-6, 8-10 and 12-14 are read and refined; 3, 7, 11 and 15 are
 *                 handed through to poses_out as they came.
 *   grid_from_world, rotation   as for vgt_hip_check_spheres: 16 doubles column-major and 9 doubles row-major, each may
 *                 be NULL, host arrays in both forms.
 *   pivot         3 doubles (host array in both forms), the point about which rotations are taken, in the poses' frame;
 *                 NULL = the origin.  The grid's centre keeps translation and rotation decoupled.
 *
 * THE DEFINITION.  Everything in double, without contraction, every operator rounded on its own.
 * evaluate(m): per point p = (x, y, z), widened to double:
 *   w_r   = ((m[r]*x + m[4+r]*y) + m[8+r]*z) + m[12+r] for r = 0, 1, 2: the expression of vgt_hip_check_spheres.
 *   d     = the estimate of vgt_hip_sdf_estimate_distance at w (the same code; grid_from_world applied as there).  A
 *           finite point without a value (w not in the grid, or not finite) counts in num_outside.
 *   g     = the gradient OF THAT INTERPOLANT, from its eight corner values c_abc (a, b, c in {m, p}: lower / upper index
 *           along x, y, z, after the half-cell correction) and its weights tx, ty, tz, with
 *           Lerp(a, b, t) = a*(1 - t) + b*t, low_x = (lower_x + 0.5)*resolution, ex = (low_x + resolution) - low_x,
 *           tx = (g_x - low_x)/ex (g_x: w in the grid frame), likewise along y and z -- all as the estimate forms them:
 *             gx = Lerp(Lerp(c_pmm - c_mmm, c_ppm - c_mpm, ty), Lerp(c_pmp - c_mmp, c_ppp - c_mpp, ty), tz) / ex
 *             gy = Lerp(Lerp(c_mpm - c_mmm, c_ppm - c_pmm, tx), Lerp(c_mpp - c_mmp, c_ppp - c_pmp, tx), tz) / ey
 *             gz = Lerp(Lerp(c_mmp - c_mmm, c_pmp - c_pmm, tx), Lerp(c_mpp - c_mpm, c_ppp - c_ppm, tx), ty) / ez
 *           An axis whose two indices coincide (the grid's faces) gives a component of 0.  With `rotation`:
 *           g <- (R[0]*gx + R[1]*gy + R[2]*gz, R[3]*gx + ..., R[6]*gx + ...), as the coarse gradient is rotated.
 *   r     = d - target_distance.
 *   used  iff the point has a value, r, gx, gy and gz are finite and |r| <= max_residual.  A point with a value that is
 *           not used counts in num_rejected.  num_used + num_outside + num_rejected = the number of finite points.
 *   q     = w - pivot (pivot = 0 when NULL).
 *   J     = (gx, gy, gz, q_y*gz - q_z*gy, q_z*gx - q_x*gz, q_x*gy - q_y*gx): the derivative of d under the left
 *           perturbation T' = Exp(v, omega) T about the pivot.
 *   terms 28 per used point: H_jk = J_j*J_k for j <= k, row-major (21); b_j = J_j*r (6); e = r*r (1).  A point that is
 *           not used, or skipped, contributes +0.0 to each.
 * tree_sum: each of the 28 terms is summed over the points, in point order, by ONE tree, whatever the launch geometry
 *   and the device: the list is cut into groups of 64 consecutive entries, the last padded with +0.0; a group is
 *   reduced by  for h in 32, 16, 8, 4, 2, 1: v[i] = v[i] + v[i + h] for i < h;  while more than one group sum is left,
 *   the procedure repeats on the list of group sums.  No floating-point atomics.
 * solve: A = H (symmetric) with A_jj = H_jj*(1 + damping); A = L D L^T without pivoting, column by column:
 *   for j = 0..5:  D_j = A_jj, then for k = 0..j-1 in turn D_j = D_j - (L_jk*L_jk)*D_k;
 *                  for i = j+1..5:  L_ij = A_ij, then for k = 0..j-1 in turn L_ij = L_ij - (L_ik*L_jk)*D_k; L_ij = L_ij/D_j
 *   y_i = b_i, then for k = 0..i-1 in turn y_i = y_i - L_ik*y_k  (i = 0..5);   z_i = y_i/D_i;
 *   x_i = z_i, then for k = i+1..5 in turn x_i = x_i - L_ki*x_k  (i = 5..0);   delta = (v, omega) = -x.
 *   A D_j that is not > 0, or a delta with a component that is not finite: VGT_HIP_ALIGN_DEGENERATE.
 * update (a Cayley retraction: no sin / cos): a = omega*0.5, s = 1 + ((a_x*a_x + a_y*a_y) + a_z*a_z), f = 2/s,
 *   D = I + f*([a]x + [a]x^2), formed as
 *     D00 = 1 - f*(a_y*a_y + a_z*a_z)   D01 = f*(a_x*a_y - a_z)           D02 = f*(a_x*a_z + a_y)
 *     D10 = f*(a_x*a_y + a_z)           D11 = 1 - f*(a_x*a_x + a_z*a_z)   D12 = f*(a_y*a_z - a_x)
 *     D20 = f*(a_x*a_z - a_y)           D21 = f*(a_y*a_z + a_x)           D22 = 1 - f*(a_x*a_x + a_y*a_y)
 *   m'[4c+r] = (D_r0*m[4c] + D_r1*m[4c+1]) + D_r2*m[4c+2] for c = 0, 1, 2;  u = t - pivot (t_r = m[12+r]);
 *   m'[12+r] = (((D_r0*u_0 + D_r1*u_1) + D_r2*u_2) + pivot_r) + v_r.
 * loop, per pose: evaluate the initial pose; then up to K = max_iterations times: solve, update, evaluate.  After EVERY
 *   evaluation, in this order: num_used < min_points stops the pose as VGT_HIP_ALIGN_TOO_FEW; a pose whose last update
 *   had max|v_r| <= translation_tolerance and max|omega_r| <= rotation_tolerance stops as VGT_HIP_ALIGN_CONVERGED (it
 *   has then been evaluated once more, at the pose it returns); a pose that has taken its K steps stops as
 *   VGT_HIP_ALIGN_ITERATION_LIMIT (with K = 0: straight after the first evaluation); otherwise it is solved, which may
 *   stop it as VGT_HIP_ALIGN_DEGENERATE.  A pose that stops is returned exactly as it stood at that evaluation, and
 *   costs no further gathers.
 * Outputs per pose (`status` is required, every other output may be NULL):
 *   poses_out [16] (may be the input array), status (uint8), num_used / num_outside / num_rejected (int32),
 *   sum_squared (double: e), evaluations (int32), normal_equations [27] (H's 21 entries, then b), last_step [6] (the
 *   last delta applied; zeros when none was).  The counts, sum_squared and normal_equations are those of the last
 *   evaluation, which is the one AT the returned pose.
 * VGT_HIP_ERR_INVALID_ARGUMENT before any HIP call, outputs untouched: a NULL required pointer (ctx, sdf, points, poses,
 * status; the workspace in the device form), N == 0, B == 0 or an empty grid, a negative extent or count, a grid of 2^31
 * cells or more, N or B of 2^31 or more, B * ceil(N / 4096) >= 2^31, a resolution that is not positive and finite,
 * max_iterations outside [0, 10000], min_points < 6, a damping that is negative or not finite, a max_residual that is
 * NaN or not positive (+infinity is allowed), a target_distance or a pivot that is not finite, a tolerance that is
 * negative or NaN, a workspace that is too small.
 * The device form takes vgt_hip_align_points_workspace_bytes(N, B) bytes of scratch (0 for sizes the call refuses): the
 * poses in progress, a flag per pose, and the partial sums [B][ceil(N / 4096)][32] doubles. */
#define VGT_HIP_ALIGN_CONVERGED 0
#define VGT_HIP_ALIGN_ITERATION_LIMIT 1
#define VGT_HIP_ALIGN_DEGENERATE 2
#define VGT_HIP_ALIGN_TOO_FEW 3
int vgt_hip_align_points(vgt_hip_ctx* ctx, const float* sdf_host, int64_t nx, int64_t ny, int64_t nz, double resolution,
                         const double* grid_from_world, const double* rotation, const float* points_xyz_host,
                         int64_t num_points, const double* poses_host, int64_t num_poses, const double* pivot,
                         int32_t max_iterations, int32_t min_points, double damping, double max_residual,
                         double target_distance, double translation_tolerance, double rotation_tolerance,
                         double* poses_out_host, uint8_t* status_host, int32_t* num_used_host, int32_t* num_outside_host,
                         int32_t* num_rejected_host, double* sum_squared_host, int32_t* evaluations_host,
                         double* normal_equations_host, double* last_step_host);
/* Same with the field, the cloud, the poses and the outputs on the device (the two transforms and the pivot stay host
 * arrays); enqueued on the context's stream, not blocking.  The workspace must stay untouched until the call is done. */
size_t vgt_hip_align_points_workspace_bytes(int64_t num_points, int64_t num_poses);
int vgt_hip_align_points_dev(vgt_hip_ctx* ctx, const float* sdf_dev, int64_t nx, int64_t ny, int64_t nz,
                             double resolution, const double* grid_from_world, const double* rotation,
                             const float* points_xyz_dev, int64_t num_points, const double* poses_dev,
                             int64_t num_poses, const double* pivot, int32_t max_iterations, int32_t min_points,
                             double damping, double max_residual, double target_distance,
                             double translation_tolerance, double rotation_tolerance, double* poses_out_dev,
                             uint8_t* status_dev, int32_t* num_used_dev, int32_t* num_outside_dev,
                             int32_t* num_rejected_dev, double* sum_squared_dev, int32_t* evaluations_dev,
                             double* normal_equations_dev, double* last_step_dev, void* workspace_dev,
                             size_t workspace_bytes);

/* ---- Forward kinematics: joint values to link poses, and clearance gradients back to joint space ----
 * The producer of the link_poses [B][L][16] that vgt_hip_check_spheres, vgt_hip_rasterize_spheres and
 * vgt_hip_spheres_cover_points take, and the way back: what the check says about the worst sphere (or about every
 * sphere) as a gradient with respect to the joint values.
 *
 * A kinematic tree of L links, described once by host arrays (validated and uploaded by vgt_hip_kinematics_create; the
 * handle serves any number of calls and is destroyed by vgt_hip_kinematics_destroy, before or after its context):
 *   parent [L] (int32)       -1: the link hangs on the base; otherwise a value in [0, i): links are topologically ordered
 *   joint_type [L] (int32)   VGT_HIP_JOINT_FIXED 0, VGT_HIP_JOINT_REVOLUTE 1, VGT_HIP_JOINT_PRISMATIC 2
 *   joint_index [L] (int32)  the column of joint_values the link reads, in [0, J); ignored for FIXED links; several links
 *                            may read one column (mimic joints)
 *   axis [L][3] (double)     in the joint frame, used as it is (unit length is the caller's business)
 *   origin [L][16] (double)  parent_from_joint, column-major (the URDF <origin>); only the elements 0-2, 4-6, 8-10 and
 *                            12-14 are read
 * VGT_HIP_ERR_INVALID_ARGUMENT, *out_tree NULL, before any device work: a NULL pointer, L <= 0 or L >= 2^31, J < 0, and
 * -- the message names the first offending link, e.g. "link 5: parent 7 is not below 5" -- a parent outside [-1, i), an
 * unknown joint type, a joint_index outside [0, J) on a link that is not FIXED (so also J == 0 with such a link).
 * A floating base needs no special case: three prismatic and three revolute links.
 *
 * vgt_hip_forward_kinematics.  joint_values [B][J] doubles; world_from_base 16 doubles column-major (elements 0-2, 4-6,
 * 8-10, 12-14 are read), a host array in both forms, may be NULL; joint_limits [J][2] doubles (lower, upper), a host array
 * in both forms, may be NULL.  THE DEFINITION, everything in double, without contraction, every operator rounded on its
 * own:
 * sin / cos of a revolute value q (plain arithmetic, so that every implementation gives the same bits):
 *   k     = rint(q * 0x1.45f306dc9c883p-1)                     (round to nearest even; 2/pi)
 *   r     = ((q - k*P1) - k*P2) - k*P3   with P1 = 0x1.921fb54400000p+0, P2 = 0x1.0b4611a600000p-34,
 *           P3 = 0x1.3198a2e037073p-69   (pi/2 in two pieces of 33 bits and the rounded rest)
 *   z     = r*r
 *   ps    = S17; ps = ps*z + S15; ... ; ps = ps*z + S3         S_n = (-1)^((n-1)/2) / n!, correctly rounded
 *   sin_r = r + (r*z)*ps
 *   pc    = C16; pc = pc*z + C14; ... ; pc = pc*z + C2         C_n = (-1)^(n/2) / n!, correctly rounded
 *   cos_r = 1 + z*pc
 *   (sin, cos) by k & 3 with k as int64: 0 (sin_r, cos_r); 1 (cos_r, -sin_r); 2 (-sin_r, -cos_r); 3 (-cos_r, sin_r).
 *   q = 0 gives exactly (0, 1): a zero joint leaves the pose untouched bit for bit.  Within 4 * 2^-53 absolute of a
 *   correctly rounded sin / cos for |q| <= 2^20 (tests/test_kinematics_ref.py measures 2 * 2^-53).
 * rotation of a revolute link about axis (x, y, z), v = 1 - c:
 *   R00 = c + (x*x)*v      R01 = (x*y)*v - z*s    R02 = (x*z)*v + y*s
 *   R10 = (x*y)*v + z*s    R11 = c + (y*y)*v      R12 = (y*z)*v - x*s
 *   R20 = (x*z)*v - y*s    R21 = (y*z)*v + x*s    R22 = c + (z*z)*v          the translation is zero
 * product A.B of two 3 x 4 transforms:
 *   rotation (A_r0*B_0c + A_r1*B_1c) + A_r2*B_2c;  translation ((A_r0*t_0 + A_r1*t_1) + A_r2*t_2) + tA_r  (t: B's)
 * pose of link i:  F = P . origin_i, with P the pose of parent[i], or world_from_base for parent -1; with a NULL base F
 *   is origin_i's twelve elements as they are, no arithmetic.
 *   FIXED      T_i = F
 *   REVOLUTE   the rotation of T_i is that of F . (R, 0) by the product rule; the translation is F's own, unchanged
 *   PRISMATIC  the rotation is F's, unchanged; the translation is the product rule applied to t = (x*q, y*q, z*q)
 * Every pose is this one fixed sequence of operations: the answer does not depend on the launch geometry.
 * Outputs:
 *   link_poses [B][L][16] doubles column-major; the elements 3, 7, 11, 15 are written as 0, 0, 0, 1: the memory of a
 *              std::vector<Eigen::Isometry3d>, and what the three sphere-model calls take as it stands
 *   status [B] uint8, may be NULL: bit VGT_HIP_FK_NOT_COMPUTABLE 1: a link that is not FIXED read a value that is not
 *              finite, or a REVOLUTE link read |q| > 2^20; the twelve elements of that link are NaN, and so are those
 *              of every descendant (NaN by arithmetic); every other link is computed.  vgt_hip_check_spheres counts the
 *              spheres of such links as "without a value".  Bit VGT_HIP_FK_OUTSIDE_LIMITS 2: with limits given, some
 *              joint_values[b][j] < lower_j or > upper_j for a j in [0, J) (NaN compares false); the poses are computed
 *              all the same.
 * VGT_HIP_ERR_INVALID_ARGUMENT before any device work: a NULL required pointer (ctx, tree, link_poses; joint_values
 * when J > 0), a negative B, B >= 2^31, B * L >= 2^31, a tree of another context.  B == 0 succeeds, and the host form
 * then needs no device.  The host form blocks; the device form (joint values, poses and status on the device) is
 * enqueued on the context's stream.  Calls that use one tree are serialised by the context.
 *
 * vgt_hip_clearance_joint_gradient.  Inputs: the tree, link_poses as the forward kinematics wrote them, the sphere model
 * of vgt_hip_check_spheres (sphere_xyzr [S][4], sphere_link [S]) and what the check returned, as exactly one of two pairs
 * (the other pair NULL):
 *   worst-sphere form   min_sphere [B] (int32) and min_gradient [B][3]
 *   summed form         sphere_weight [B][S] (double) and sphere_gradient [B][S][3]
 * Output: joint_gradient [B][J] doubles.  For sphere s on link k with gradient g: p = the sphere's world centre by
 * vgt_hip_check_spheres' expression w_r.  Walk i = k, parent[k], ... up to the base; for each link on the way that is
 * not FIXED, with m the pose of link i:
 *   a_r  = (m[r]*x + m[4+r]*y) + m[8+r]*z          (x, y, z): axis_i
 *   REVOLUTE   d_r = p_r - m[12+r];  u = (a1*d2 - a2*d1, a2*d0 - a0*d2, a0*d1 - a1*d0);  term = (g0*u0 + g1*u1) + g2*u2
 *   PRISMATIC  term = (g0*a0 + g1*a1) + g2*a2
 * Worst-sphere form: every acc_j starts at +0.0, then acc_j = acc_j + term in walk order for j = joint_index[i], for the
 *   sphere min_sphere[b].  The whole row is NaN when min_sphere[b] is outside [0, S) or that sphere's link outside
 *   [0, L).  The result is d min_clearance / d q wherever the worst sphere does not change (for revolute axes of unit
 *   length: with another length R above is no rotation, and the term is the definition, not a derivative).
 * Summed form: the spheres in ascending s, each sphere's terms in walk order, acc_j = acc_j + w*term with
 *   w = sphere_weight[b][s].  A sphere with w == 0, or with a link outside [0, L), is skipped entirely: its NaN gradient
 *   then does no harm.
 * That fixed order is the definition.
 * VGT_HIP_ERR_INVALID_ARGUMENT before any device work: a NULL required pointer (ctx, tree; link_poses, the model's two
 * arrays and joint_gradient when B > 0 and J > 0), not exactly one complete pair, a negative count, B, S, B * L, B * J
 * or B * S of 2^31 or more, a tree of another context.  B == 0 and J == 0 succeed without a device; S == 0 gives NaN
 * rows (worst-sphere form) or +0.0 (summed form). */
#define VGT_HIP_JOINT_FIXED 0
#define VGT_HIP_JOINT_REVOLUTE 1
#define VGT_HIP_JOINT_PRISMATIC 2
#define VGT_HIP_FK_NOT_COMPUTABLE 1
#define VGT_HIP_FK_OUTSIDE_LIMITS 2
typedef struct vgt_hip_kinematics vgt_hip_kinematics;
int vgt_hip_kinematics_create(vgt_hip_ctx* ctx, int64_t num_links, int64_t num_joints, const int32_t* parent,
                              const int32_t* joint_type, const int32_t* joint_index, const double* axis,
                              const double* origin, vgt_hip_kinematics** out_tree);
void vgt_hip_kinematics_destroy(vgt_hip_kinematics* tree);
int64_t vgt_hip_kinematics_num_links(const vgt_hip_kinematics* tree);
int64_t vgt_hip_kinematics_num_joints(const vgt_hip_kinematics* tree);
/* How many links' poses the forward kinematics keeps in LDS for their descendants: those of the first so many links
 * that are the parent of a link other than the next one.  A link whose parent is a later such link reads its own
 * earlier output back; the answer is the same.  A constant of the kernel (csrc/kinematics_kernels.hip), exposed so that
 * tests build trees on both sides of it. */
int32_t vgt_hip_kinematics_lds_links(void);
int vgt_hip_forward_kinematics(vgt_hip_ctx* ctx, const vgt_hip_kinematics* tree, const double* joint_values_host,
                               int64_t num_configurations, const double* world_from_base, const double* joint_limits,
                               double* link_poses_host, uint8_t* status_host);
int vgt_hip_forward_kinematics_dev(vgt_hip_ctx* ctx, const vgt_hip_kinematics* tree, const double* joint_values_dev,
                                   int64_t num_configurations, const double* world_from_base,
                                   const double* joint_limits, double* link_poses_dev, uint8_t* status_dev);
int vgt_hip_clearance_joint_gradient(vgt_hip_ctx* ctx, const vgt_hip_kinematics* tree, const double* link_poses_host,
                                     int64_t num_configurations, const double* sphere_xyzr_host,
                                     const int32_t* sphere_link_host, int64_t num_spheres, const int32_t* min_sphere_host,
                                     const double* min_gradient_host, const double* sphere_weight_host,
                                     const double* sphere_gradient_host, double* joint_gradient_host);
int vgt_hip_clearance_joint_gradient_dev(vgt_hip_ctx* ctx, const vgt_hip_kinematics* tree, const double* link_poses_dev,
                                         int64_t num_configurations, const double* sphere_xyzr_dev,
                                         const int32_t* sphere_link_dev, int64_t num_spheres,
                                         const int32_t* min_sphere_dev, const double* min_gradient_dev,
                                         const double* sphere_weight_dev, const double* sphere_gradient_dev,
                                         double* joint_gradient_dev);
/* The three in one call, host arrays in and out: vgt_hip_forward_kinematics on joint_values, vgt_hip_check_spheres on
 * its poses, and -- when joint_gradient_host is not NULL -- the worst-sphere form of vgt_hip_clearance_joint_gradient
 * on what the check found.  The poses are made and used on the device and never visit the host; every output is what
 * the three calls give one after the other.  Arguments, outputs and errors as theirs (num_links is the tree's);
 * fk_status_host (the forward kinematics' status) may be NULL.  B == 0 succeeds without a device.  Blocking. */
int vgt_hip_check_spheres_from_joints(vgt_hip_ctx* ctx, const float* sdf_host, int64_t nx, int64_t ny, int64_t nz,
                                      double resolution, const double* grid_from_world, const double* rotation,
                                      const double* sphere_xyzr_host, const int32_t* sphere_link_host,
                                      int64_t num_spheres, const vgt_hip_kinematics* tree,
                                      const double* joint_values_host, int64_t num_configurations,
                                      const double* world_from_base, const double* joint_limits,
                                      double minimum_clearance, uint32_t flags, uint8_t* status_host,
                                      double* min_clearance_host, int32_t* min_sphere_host, int32_t* num_below_host,
                                      int32_t* num_outside_host, double* min_gradient_host,
                                      double* sphere_clearance_host, double* sphere_gradient_host,
                                      uint8_t* fk_status_host, double* joint_gradient_host);

/* ---- Inverse kinematics: tip poses to joint values, batched over targets and seeds ----
 * The step in front of every joint-driven call: a task arrives as the pose of a tool frame, and a planner turns it into
 * goal configurations -- many of them, from many seeds -- before it keeps those that pass
 * vgt_hip_check_spheres_from_joints and vgt_hip_check_self_collision.  B problems (a target pose and a seed row of joint
 * values) in, one row of joint values per problem out, after up to K damped least-squares steps that bring one chosen
 * link (the tip) of a vgt_hip_kinematics tree to its target.  Everything happens on the device, in one launch
 * (csrc/ik_kernels.hip); nothing is synchronised with the host between iterations.
 * Inputs:
 *   tree, tip_link   the tree as it is, and a link in [0, L).  The chain is the set of links on the way from the tip to
 *                    the base; the call finds it from the tree.
 *   targets          [T][16] doubles, column-major world_from_tip; elements 0-2, 4-6, 8-10 and 12-14 are read.
 *   seeds_per_target R >= 1: B = T * R, and problem b aims at target b / R (a planner's restarts need no tiled copy of
 *                    the targets).
 *   seeds            [B][J] doubles.
 *   world_from_base, joint_limits [J][2]   as for vgt_hip_forward_kinematics: host arrays in both forms, each may be NULL.
 *   task_weights     6 doubles w (a host array in both forms, NULL = all 1) for (x, y, z, rx, ry, rz), each finite and
 *                    >= 0.  A weight of 0 removes that component from both the step and the convergence test:
 *                    (1, 1, 1, 0, 0, 0) is position-only IK.
 *   max_iterations   K in [0, 10000]; K = 0 evaluates the seeds only.  damping lambda >= 0, finite.  max_step > 0,
 *                    +infinity is allowed.  position_tolerance, rotation_tolerance >= 0.
 *
 * THE DEFINITION.  Everything in double, without contraction, every operator rounded on its own.
 * evaluate(q): the poses of the chain's links exactly as vgt_hip_forward_kinematics defines them for the row q (links off
 *   the chain are not computed); m is the tip's.  With t* and r*_c the target's translation and rotation columns and r_c
 *   those of m, cross(a, b) = (a1*b2 - a2*b1, a2*b0 - a0*b2, a0*b1 - a1*b0) and dot(a, b) = (a0*b0 + a1*b1) + a2*b2:
 *     e_r = t*_r - m[12+r] for r = 0, 1, 2;   x_c = cross(r_c, r*_c);   (e_3, e_4, e_5) = ((x_0 + x_1) + x_2) * 0.5
 *     componentwise;   trace = (dot(r_0, r*_0) + dot(r_1, r*_1)) + dot(r_2, r*_2).
 *   The orientation error is sin(theta) times the axis of the rotation that is left: no inverse trigonometry, exact to
 *   first order.
 * converged: every |e_i| with w_i != 0 is <= its tolerance (position_tolerance for i < 3, rotation_tolerance for i >= 3;
 *   NaN compares false); and, when all three rotational weights are non-zero, trace > 1 -- which excludes the half turn,
 *   where the cross products vanish.
 * columns: for every chain link i that is not FIXED, walked from the tip to the base, with a the expression a_r of
 *   vgt_hip_clearance_joint_gradient for the pose of link i, o the translation of that pose and p the translation of m:
 *     REVOLUTE   d = p - o;  c = (cross(a, d), a)      (the translational half is that call's expression u)
 *     PRISMATIC  c = (a, +0.0, +0.0, +0.0)
 *   then c_k <- w_k * c_k.  As there, the columns are derivatives only for revolute axes of unit length; with another
 *   length they are the definition, not a derivative.
 * step:
 *   A = sum of c c^T over the chain in walk order: the 21 entries j <= k each start at +0.0, then A_jk = A_jk + c_j*c_k;
 *   A_jj = A_jj + lambda*lambda;
 *   A y = (w_i * e_i) by the L D L^T sequence of vgt_hip_align_points' "solve" with b = the weighted e, without its
 *   damping line and without its final negation (y is its x).  A D_j that is not > 0, or a y with a component that is
 *   not finite: VGT_HIP_IK_DEGENERATE.
 *   dq_i = ((((c_0*y_0 + c_1*y_1) + c_2*y_2) + c_3*y_3) + c_4*y_4) + c_5*y_5 per moving chain link;
 *   mx = +0.0, then in walk order mx = |dq_i| where |dq_i| > mx;  if mx > max_step: s = max_step / mx, dq_i = dq_i * s;
 *   q_j = q_j + dq_i for j = joint_index[i];  with limits: q_j = lower_j where q_j < lower_j, then q_j = upper_j where
 *   q_j > upper_j.
 * loop, per problem: evaluate the seed; after EVERY evaluation, in this order: a chain link that is not computable (the
 *   forward kinematics' bit 1) stops the problem as VGT_HIP_IK_NOT_COMPUTABLE; a converged problem stops as
 *   VGT_HIP_IK_CONVERGED; a problem that has taken K steps stops as VGT_HIP_IK_ITERATION_LIMIT; otherwise it takes a
 *   step, which may stop it as VGT_HIP_IK_DEGENERATE, and is evaluated again.  A problem that stops is returned exactly
 *   as it stood at its last evaluation and costs nothing further.  Every output is this one fixed sequence of
 *   operations: the answer does not depend on the launch geometry.
 * Two moving links on one chain that read one column (a mimic joint on the chain) would need a column sum per joint:
 * such a (tree, tip) is refused, and the message names both links.  A mimic joint off the chain is fine.
 * Outputs per problem (`status` is required, every other output may be NULL):
 *   joints_out [J]     the row at the last evaluation; columns that no chain link reads are the seed's, bit for bit.  It
 *                      may be the seed array.
 *   status (uint8), iterations (int32: the steps taken), error [6] (the unweighted e at the returned row),
 *   tip_pose [16]      m, written with 0, 0, 0, 1 like link_poses;
 *   fk_status (uint8)  VGT_HIP_FK_NOT_COMPUTABLE from the chain's links, VGT_HIP_FK_OUTSIDE_LIMITS by the forward
 *                      kinematics' test over all J columns of the returned row.
 * VGT_HIP_ERR_INVALID_ARGUMENT before any device work, outputs untouched: a NULL required pointer (ctx, tree, targets,
 * status; seeds when J > 0), T <= 0 or R <= 0, B >= 2^31, a tip outside [0, L), a tree of another context, K, lambda,
 * max_step, a tolerance or a weight outside the ranges above, a mimic joint on the chain, a chain with more than
 * vgt_hip_ik_max_chain_joints() moving links (a constant of the kernel, which keeps six doubles per moving link and lane
 * in LDS; at least 16: a 7-joint arm on a lift on a 6-joint floating base), and in the device form a missing or too
 * small workspace.  The host form blocks; the device form (targets, seeds and outputs on the device) is enqueued on the
 * context's stream.  The working rows are those of joints_out; only when joints_out_dev is NULL does the device form
 * need vgt_hip_solve_ik_workspace_bytes(J, B) bytes of scratch (0 for sizes the call refuses), which must stay untouched
 * until the call is done.  Calls that use one tree are serialised by the context. */
#define VGT_HIP_IK_CONVERGED 0
#define VGT_HIP_IK_ITERATION_LIMIT 1
#define VGT_HIP_IK_DEGENERATE 2
#define VGT_HIP_IK_NOT_COMPUTABLE 3
int32_t vgt_hip_ik_max_chain_joints(void);
int vgt_hip_solve_ik(vgt_hip_ctx* ctx, const vgt_hip_kinematics* tree, int32_t tip_link, const double* targets_host,
                     int64_t num_targets, int64_t seeds_per_target, const double* seeds_host,
                     const double* world_from_base, const double* joint_limits, const double* task_weights,
                     int32_t max_iterations, double damping, double max_step, double position_tolerance,
                     double rotation_tolerance, double* joints_out_host, uint8_t* status_host, int32_t* iterations_host,
                     double* error_host, double* tip_pose_host, uint8_t* fk_status_host);
size_t vgt_hip_solve_ik_workspace_bytes(int64_t num_joints, int64_t num_problems);
int vgt_hip_solve_ik_dev(vgt_hip_ctx* ctx, const vgt_hip_kinematics* tree, int32_t tip_link, const double* targets_dev,
                         int64_t num_targets, int64_t seeds_per_target, const double* seeds_dev,
                         const double* world_from_base, const double* joint_limits, const double* task_weights,
                         int32_t max_iterations, double damping, double max_step, double position_tolerance,
                         double rotation_tolerance, double* joints_out_dev, uint8_t* status_dev, int32_t* iterations_dev,
                         double* error_dev, double* tip_pose_dev, uint8_t* fk_status_dev, void* workspace_dev,
                         size_t workspace_bytes);

/* ---- Motions between joint configurations checked against an SDF ----
 * The question a sampling planner asks of an edge: is the straight joint-space motion from q_a to q_b free, where does it
 * first collide, how close does it come.  A batch of E motions in, one verdict per motion out; the link poses of the
 * samples are made and used on the device and are never written to memory (csrc/motion_kernels.hip).  Read-only.
 *
 * THE DEFINITION.  Motion e has the endpoints a = joint_from[e] and b = joint_to[e] (J doubles each, J the tree's) and a
 * step count n = num_steps[e], or uniform_steps when num_steps is NULL.  It has n + 1 samples k = 0 ... n, in double,
 * every operator rounded on its own:
 *   k == 0       q = a, the bits as given.  With n == 0 this is the only sample and b is not read.
 *   k == n > 0   q = b, the bits as given (not a + 1*(b - a)).
 *   otherwise    t = (double)k / (double)n;  q_j = a_j + t * (b_j - a_j).
 * Interpolation is plain linear: there is no wrap-around for continuous revolute joints.
 * Per sample: vgt_hip_check_spheres_from_joints with joint_values = q and the same field, grid_from_world, rotation,
 * model, tree, world_from_base, joint_limits, minimum_clearance and VGT_HIP_SPHERES_OUTSIDE_IS_COLLISION bit would return
 * status, min_clearance, min_sphere, num_below, num_outside, min_gradient and fk_status; every bit of those seven values
 * is what that call gives.  Nothing of the kinematics or of the check is restated here.
 * Considered samples: all of them; with flags & VGT_HIP_MOTION_STOP_AT_COLLISION only the samples 0 ... first_collision
 * when there is a collision: the later samples then do not exist for any output.
 * Outputs, one entry per motion; status is required, every other output may be NULL:
 *   status (uint8)           VGT_HIP_MOTION_COLLISION 1 when a considered sample's status is COLLISION; otherwise
 *                            VGT_HIP_MOTION_NO_VALUE 2 when one is NO_VALUE (a motion is not clear when a sample could
 *                            not be judged); otherwise VGT_HIP_MOTION_CLEAR 0.  VGT_HIP_MOTION_INVALID 3: the device
 *                            form only, below.
 *   first_collision (int32)  the least k whose sample status is COLLISION, or -1
 *   min_clearance (double), min_sample (int32), min_sphere (int32)
 *                            the least non-NaN sample min_clearance among the considered samples; ties under == go to
 *                            the lowest k (so -0.0 and 0.0 tie); the value written is that sample's own bits, and
 *                            min_sphere is that sample's.  NaN, -1, -1 when there is no such sample.
 *   min_gradient [3] (double)  the min_gradient of sample min_sample; NaN x 3 when min_sample == -1
 *   fk_status (uint8)        the OR of the considered samples' fk_status
 * Both reductions are total orders on distinct k: the answer does not depend on the launch geometry.
 * VGT_HIP_ERR_INVALID_ARGUMENT before any device work: a NULL required pointer (ctx, sdf, tree, status; the model's two
 * arrays when S > 0; the two joint arrays when E > 0 and J > 0); a resolution that is not positive and finite; a NaN
 * minimum_clearance; an unknown flag bit; negative extents or counts; a negative uniform_steps when num_steps is NULL; a
 * grid of 2^31 cells or more; E, E * J or S of 2^31 or more; a tree of another context; a tree of more links than the
 * kernel takes (vgt_hip_motion_tile_samples gives 0; the message gives both numbers).  The host form also looks at its
 * arrays and names the first offender -- "motion 12: num_steps -3", "sphere 17: ..." --: a num_steps[e] < 0, a
 * sphere_link outside [0, L), a negative or NaN radius.  The device form cannot look: a motion with n < 0 gets status
 * INVALID, first_collision -1, min_clearance NaN, min_sample -1, min_sphere -1, min_gradient NaN x 3 and fk_status 0, and
 * forms no address; a link outside [0, L) makes its sphere "without a value", as in vgt_hip_check_spheres_dev.
 * E == 0 succeeds without a device.  The host form stages its arrays and blocks; the device form (field, model, joint
 * arrays, num_steps and outputs on the device; the three transforms / limits are host arrays) is enqueued on the context's
 * stream, not blocking.  Calls that use one tree are serialised by the context. */
#define VGT_HIP_MOTION_STOP_AT_COLLISION 2u
#define VGT_HIP_MOTION_CLEAR 0
#define VGT_HIP_MOTION_COLLISION 1
#define VGT_HIP_MOTION_NO_VALUE 2
#define VGT_HIP_MOTION_INVALID 3
int vgt_hip_check_motions(vgt_hip_ctx* ctx, const float* sdf_host, int64_t nx, int64_t ny, int64_t nz, double resolution,
                          const double* grid_from_world, const double* rotation, const double* sphere_xyzr_host,
                          const int32_t* sphere_link_host, int64_t num_spheres, const vgt_hip_kinematics* tree,
                          const double* joint_from_host, const double* joint_to_host, const int32_t* num_steps_host,
                          int32_t uniform_steps, int64_t num_motions, const double* world_from_base,
                          const double* joint_limits, double minimum_clearance, uint32_t flags, uint8_t* status_host,
                          int32_t* first_collision_host, double* min_clearance_host, int32_t* min_sample_host,
                          int32_t* min_sphere_host, double* min_gradient_host, uint8_t* fk_status_host);
int vgt_hip_check_motions_dev(vgt_hip_ctx* ctx, const float* sdf_dev, int64_t nx, int64_t ny, int64_t nz,
                              double resolution, const double* grid_from_world, const double* rotation,
                              const double* sphere_xyzr_dev, const int32_t* sphere_link_dev, int64_t num_spheres,
                              const vgt_hip_kinematics* tree, const double* joint_from_dev, const double* joint_to_dev,
                              const int32_t* num_steps_dev, int32_t uniform_steps, int64_t num_motions,
                              const double* world_from_base, const double* joint_limits, double minimum_clearance,
                              uint32_t flags, uint8_t* status_dev, int32_t* first_collision_dev,
                              double* min_clearance_dev, int32_t* min_sample_dev, int32_t* min_sphere_dev,
                              double* min_gradient_dev, uint8_t* fk_status_dev);
/* The samples per tile the kernel uses for a tree of so many links: a power of two, at most 64, with 96 * L * T <= 60 KiB
 * of LDS for the poses of a tile (the build keeps them within 12 KiB where more than one sample fits that: DESIGN.md 4n);
 * 0: more links than the kernel takes (640), or none.  Exposed so that tests put step counts on both sides of it. */
int32_t vgt_hip_motion_tile_samples(int64_t num_links);

/* ---- The obstacle cost of configurations given as joint values, and its gradient with respect to the joints ----
 * What an optimiser asks per configuration (CHOMP, STOMP or MPPI roll-outs, collision-aware IK, path smoothing): a cost
 * that counts EVERY sphere inside a safety margin, not only the worst one, and that cost's gradient in joint space.  B
 * configurations in, one cost and optionally one gradient row [J] per configuration out; link poses and per-sphere
 * values are made and used on the device and are never written to memory (csrc/cost_kernels.hip).  A trajectory is
 * nothing special: [N][W][J] is B = N * W configurations.  Read-only.
 *
 * Inputs: as vgt_hip_check_spheres_from_joints -- the field and its extents, resolution, grid_from_world, rotation, the
 * model, the tree, joint_values [B][J], world_from_base, joint_limits --, then margin and flags (no bit is defined yet).
 *
 * THE DEFINITION.  Per (configuration b, sphere s): clearance d and gradient g are exactly what vgt_hip_check_spheres
 * defines for the poses that vgt_hip_forward_kinematics defines for row b; nothing of either is restated here.  A sphere
 * "without a value" is one whose d is NaN: a sphere not in the grid, a non-finite centre, a NaN pose from a link that is
 * not computable, an estimate that is itself NaN (a NaN in the field, infinity minus infinity) and, in the device form, a
 * link outside [0, L).
 * The hinge, in double, every operator rounded on its own, with eps = margin; the comparisons in this order:
 *   d is NaN       no contribution, w = 0
 *   d < 0          c = (eps * 0.5) - d                        w = -1.0
 *   d <= eps       t = d - eps;  c = ((t * t) * 0.5) / eps    w = t / eps
 *   otherwise      c = +0.0                                   w = 0
 * +-infinity compare as they are.  c is the CHOMP obstacle potential and w = dc/dd; both are continuous at 0 and at eps,
 * but the bits of the two branches at d == 0 need not agree, which is why the order of the comparisons is part of the
 * definition (-0.0 < 0 is false: it takes the second branch).
 * Outputs per configuration; cost is required, every other output may be NULL:
 *   cost (double)                 acc = +0.0; acc = acc + c_s for s ascending, over the spheres with a value
 *   joint_gradient [J] (double)   the summed form of vgt_hip_clearance_joint_gradient, to the bit, with
 *                                 sphere_weight[b][s] = w_s and sphere_gradient = g: the walk, the term and the order are
 *                                 exactly as the summed form defines them (s ascending, walk order within a sphere, a
 *                                 sphere skipped when its weight is 0).  One addition: a sphere with w != 0 whose g has a
 *                                 NaN component is given weight 0 for the gradient; it still counts in cost.
 *   num_active (int32)            spheres with a value and w != 0
 *   num_outside (int32)           spheres without a value
 *   num_without_gradient (int32)  spheres that are active but were skipped in the gradient by the rule above
 *   fk_status (uint8)             the forward kinematics' status
 * The order is fixed: no output depends on the launch geometry.  With joint_gradient and num_without_gradient both NULL
 * (roll-out scoring) no gradient is loaded at all.
 * VGT_HIP_ERR_INVALID_ARGUMENT before any device work: a NULL required pointer (ctx, sdf, tree, cost; the model's two
 * arrays when S > 0; joint_values when B > 0 and J > 0); a resolution that is not positive and finite; a margin that is
 * not positive and finite; an unknown flag bit (any bit); negative extents or counts; a grid of 2^31 cells or more; B, S,
 * B * J, B * S or B * L of 2^31 or more; a tree of another context; a tree of more links than the kernel takes
 * (vgt_hip_cost_tile_samples gives 0; the message gives both numbers).  The host form also looks at the model and names
 * the first offending sphere -- "sphere 17: ..." --: a sphere_link outside [0, L), a negative or NaN radius.  The device
 * form cannot look: such a link makes its sphere "without a value" and forms no address; a bad radius is used as it is.
 * B == 0 succeeds without a device.  S == 0 gives cost +0.0, a gradient row of +0.0 and counts 0.  The host form stages
 * its arrays and blocks; the device form (field, model, joint values and outputs on the device; the three transforms /
 * limits are host arrays) is enqueued on the context's stream, not blocking.  Calls that use one tree are serialised by
 * the context. */
int vgt_hip_clearance_cost(vgt_hip_ctx* ctx, const float* sdf_host, int64_t nx, int64_t ny, int64_t nz, double resolution,
                           const double* grid_from_world, const double* rotation, const double* sphere_xyzr_host,
                           const int32_t* sphere_link_host, int64_t num_spheres, const vgt_hip_kinematics* tree,
                           const double* joint_values_host, int64_t num_configurations, const double* world_from_base,
                           const double* joint_limits, double margin, uint32_t flags, double* cost_host,
                           double* joint_gradient_host, int32_t* num_active_host, int32_t* num_outside_host,
                           int32_t* num_without_gradient_host, uint8_t* fk_status_host);
int vgt_hip_clearance_cost_dev(vgt_hip_ctx* ctx, const float* sdf_dev, int64_t nx, int64_t ny, int64_t nz,
                               double resolution, const double* grid_from_world, const double* rotation,
                               const double* sphere_xyzr_dev, const int32_t* sphere_link_dev, int64_t num_spheres,
                               const vgt_hip_kinematics* tree, const double* joint_values_dev,
                               int64_t num_configurations, const double* world_from_base, const double* joint_limits,
                               double margin, uint32_t flags, double* cost_dev, double* joint_gradient_dev,
                               int32_t* num_active_dev, int32_t* num_outside_dev, int32_t* num_without_gradient_dev,
                               uint8_t* fk_status_dev);
/* The configurations per tile the kernel uses for a tree of so many links: a power of two, at most 64, with
 * 96 * L * T <= 48 KiB of LDS for the poses of a tile (the build keeps them within 6 KiB where more than one
 * configuration fits that: DESIGN.md 4o); 0: more links than the kernel takes (512), or none.  Exposed so that tests put
 * batch sizes on both sides of it. */
int32_t vgt_hip_cost_tile_samples(int64_t num_links);

/* ---- Self-collision of a sphere model, batched over configurations ----
 * The calls above ask whether the robot touches the ENVIRONMENT; this one asks whether it touches ITSELF: B
 * configurations and a list of P sphere pairs in; per configuration a verdict, two counts, the worst pair with its
 * clearance and direction, and that clearance's gradient with respect to the joints out.  Link poses and sphere centres
 * are made and used on the device and are never written to memory (csrc/self_collision_kernels.hip).  No field is
 * involved.  Read-only.  A caller combines this verdict with the environment's.
 *
 * The model (sphere_xyzr [S][4], sphere_link [S]) and the tree are exactly those of vgt_hip_check_spheres /
 * vgt_hip_forward_kinematics.  The pair list is pairs [P][2] int32, each row (a, b) with 0 <= a < b < S; duplicates are
 * allowed and the order is the caller's (vgt_hip_self_collision_pairs below makes one).
 *
 * THE DEFINITION.  Per (configuration, pair p = (a, b)), in double, without contraction, every operator rounded on its
 * own: ca, cb are the world centres of the spheres a and b -- vgt_hip_check_spheres' expression w_r on the pose that
 * vgt_hip_forward_kinematics defines (or on the link pose given, in the poses form); nothing of either is restated --,
 *   e_r = ca_r - cb_r      d2 = (e0 * e0 + e1 * e1) + e2 * e2      dist = sqrt(d2), correctly rounded
 *   clearance = (dist - ra) - rb
 * A pair is "without a value" when its clearance is NaN: a NaN pose from a link that is not computable, a NaN centre,
 * infinity minus infinity and, in the device forms, a sphere index outside [0, S) or a sphere_link outside [0, L) (no
 * address is formed from such a value).  +-infinity compare as they are.
 * Outputs per configuration; status is required, every other output may be NULL:
 *   num_below (int32)           pairs with a value and clearance <= minimum_clearance
 *   num_without_value (int32)   pairs without a value
 *   min_clearance (double), min_pair (int32, an index into pairs)
 *                               the least non-NaN clearance and the index of its pair; ties under == go to the lowest p;
 *                               NaN and -1 when there is none
 *   min_direction [3] (double)  n_r = e_r / dist of min_pair: three divisions, as arithmetic gives them (coincident
 *                               centres: NaN); NaN x3 when min_pair == -1
 *   joint_gradient [J] (double) the summed form of vgt_hip_clearance_joint_gradient, to the bit, with every weight 0 but
 *                               sphere_weight[a] = sphere_weight[b] = 1.0 and sphere_gradient[a] = n, sphere_gradient[b]
 *                               = -n: acc_j = +0.0, then sphere a's walk with g = n, then sphere b's with g = -n.  A NaN
 *                               row when min_pair == -1.  It is d min_clearance / d q wherever the worst pair does not
 *                               change.
 *   status (uint8)              VGT_HIP_SELF_COLLISION when num_below > 0, or flags & VGT_HIP_SELF_NO_VALUE_IS_COLLISION
 *                               and num_without_value > 0; otherwise VGT_HIP_SELF_CLEAR when min_pair != -1; otherwise
 *                               VGT_HIP_SELF_NO_VALUE
 *   fk_status (uint8)           the forward kinematics' status (the joint-value forms only)
 * and per pair, optional: pair_clearance [B][P], NaN without a value.
 * The worst pair is a total order and the counts are integer sums: no output depends on the launch geometry.
 *
 * vgt_hip_check_self_collision takes joint values (the tree, joint_values [B][J], world_from_base, joint_limits, as
 * vgt_hip_forward_kinematics takes them); vgt_hip_check_self_collision_poses takes link_poses [B][L][16] as
 * vgt_hip_check_spheres takes them, with num_links given, and a tree only for joint_gradient (NULL with a NULL
 * joint_gradient; otherwise a tree of num_links links whose J gives the row length).
 * VGT_HIP_ERR_INVALID_ARGUMENT before any device work: a NULL required pointer (ctx, status; the tree in the joint-value
 * forms; the model's arrays when S > 0; pairs when P > 0 and S > 0; joint_values when B > 0 and J > 0; link_poses when
 * B > 0); joint_gradient without a tree; a NaN minimum_clearance; an unknown flag bit; negative counts; B, S, P, B * J or
 * B * L of 2^31 or more, or B * P of 2^31 or more when pair_clearance is given; a tree of another context, or of another
 * number of links than num_links; a tree or model larger than the kernel takes (vgt_hip_self_collision_tile_samples
 * gives 0; the message gives both numbers).  The host forms also look at their arrays and name the first offender:
 * "sphere 17: link 9 is not in [0, num_links)", "sphere 17: the radius must not be negative or NaN", "pair 3: sphere 300
 * is outside [0, 200)", "pair 12: (5, 5) is not ascending".  The device forms cannot look.
 * B == 0 succeeds without a device.  P == 0 or S == 0 give NaN, -1, counts 0 and NO_VALUE (with S == 0 the pair list is
 * not looked at in either form, and pair_clearance is not written).  The host forms stage their arrays and block; the
 * device forms (model, pairs, joint values or link poses and outputs on the device; world_from_base and joint_limits
 * are host arrays) are enqueued on the context's stream, not blocking.  Calls that use one tree are serialised by the
 * context. */
#define VGT_HIP_SELF_NO_VALUE_IS_COLLISION 1u
#define VGT_HIP_SELF_CLEAR 0
#define VGT_HIP_SELF_COLLISION 1
#define VGT_HIP_SELF_NO_VALUE 2
int vgt_hip_check_self_collision(vgt_hip_ctx* ctx, const double* sphere_xyzr_host, const int32_t* sphere_link_host,
                                 int64_t num_spheres, const int32_t* pairs_host, int64_t num_pairs,
                                 const vgt_hip_kinematics* tree, const double* joint_values_host,
                                 int64_t num_configurations, const double* world_from_base, const double* joint_limits,
                                 double minimum_clearance, uint32_t flags, uint8_t* status_host, int32_t* num_below_host,
                                 int32_t* num_without_value_host, double* min_clearance_host, int32_t* min_pair_host,
                                 double* min_direction_host, double* joint_gradient_host, uint8_t* fk_status_host,
                                 double* pair_clearance_host);
int vgt_hip_check_self_collision_dev(vgt_hip_ctx* ctx, const double* sphere_xyzr_dev, const int32_t* sphere_link_dev,
                                     int64_t num_spheres, const int32_t* pairs_dev, int64_t num_pairs,
                                     const vgt_hip_kinematics* tree, const double* joint_values_dev,
                                     int64_t num_configurations, const double* world_from_base,
                                     const double* joint_limits, double minimum_clearance, uint32_t flags,
                                     uint8_t* status_dev, int32_t* num_below_dev, int32_t* num_without_value_dev,
                                     double* min_clearance_dev, int32_t* min_pair_dev, double* min_direction_dev,
                                     double* joint_gradient_dev, uint8_t* fk_status_dev, double* pair_clearance_dev);
int vgt_hip_check_self_collision_poses(vgt_hip_ctx* ctx, const double* sphere_xyzr_host, const int32_t* sphere_link_host,
                                       int64_t num_spheres, const int32_t* pairs_host, int64_t num_pairs,
                                       const double* link_poses_host, int64_t num_configurations, int64_t num_links,
                                       const vgt_hip_kinematics* tree, double minimum_clearance, uint32_t flags,
                                       uint8_t* status_host, int32_t* num_below_host, int32_t* num_without_value_host,
                                       double* min_clearance_host, int32_t* min_pair_host, double* min_direction_host,
                                       double* joint_gradient_host, double* pair_clearance_host);
int vgt_hip_check_self_collision_poses_dev(vgt_hip_ctx* ctx, const double* sphere_xyzr_dev,
                                           const int32_t* sphere_link_dev, int64_t num_spheres, const int32_t* pairs_dev,
                                           int64_t num_pairs, const double* link_poses_dev, int64_t num_configurations,
                                           int64_t num_links, const vgt_hip_kinematics* tree, double minimum_clearance,
                                           uint32_t flags, uint8_t* status_dev, int32_t* num_below_dev,
                                           int32_t* num_without_value_dev, double* min_clearance_dev,
                                           int32_t* min_pair_dev, double* min_direction_dev, double* joint_gradient_dev,
                                           double* pair_clearance_dev);
/* The pair list of a model, on the host (no context, no device): in lexicographic order every (a, b) with a < b whose
 * spheres sit on different links that are not an ignored pair and -- with flags & VGT_HIP_SELF_PAIRS_SKIP_ADJACENT and
 * `parent` given -- of which neither is the other's direct parent.  sphere_link [S]; parent [L] (each in [-1, L)) or
 * NULL; ignored_link_pairs [K][2], unordered, or NULL with K == 0.  Writes at most `capacity` rows to pairs_out (NULL
 * with capacity == 0 only counts); *count always receives the full number.  VGT_HIP_ERR_INVALID_ARGUMENT, naming the
 * first offender: "sphere 3: link 9 is not in [0, num_links)", "link 3: parent 9 is not in [-1, num_links)", "ignored
 * pair 2: link 9 is not in [0, num_links)"; also a NULL count or sphere_link (S > 0), negative numbers, an unknown flag
 * bit. */
#define VGT_HIP_SELF_PAIRS_SKIP_ADJACENT 1u
int vgt_hip_self_collision_pairs(const int32_t* sphere_link, int64_t num_spheres, const int32_t* parent,
                                 int64_t num_links, const int32_t* ignored_link_pairs, int64_t num_ignored,
                                 uint32_t flags, int32_t* pairs_out, int64_t capacity, int64_t* count);
/* The configurations per tile the kernel uses for a tree of so many links carrying so many spheres: a power of two, at
 * most 64, whose poses and centres take (96 L + 24 S) T <= 16 KiB of LDS where more than one configuration fits that
 * (DESIGN.md 4p); 0: no links, or one configuration does not fit a launch's 64 KiB (96 L + 32 S + 256 bytes: 680 links
 * without spheres, 2037 spheres on one link).  Exposed so that tests put batch sizes and models on both sides of it. */
int32_t vgt_hip_self_collision_tile_samples(int64_t num_links, int64_t num_spheres);

/* ---- Motions checked against the field and against the robot itself in one call ----
 * What a sampling planner asks of an edge in full: is the straight joint-space motion free of the environment AND of the
 * robot itself, where does it first collide and with which of the two, how close does it come to either.  E motions in,
 * one verdict per motion out; every sample's link poses and sphere centres are made once, used for both questions and
 * never written to memory (csrc/motion_self_kernels.hip).  Read-only.
 *
 * Arguments: those of vgt_hip_check_motions, with pairs [P][2] and num_pairs behind the model as
 * vgt_hip_check_self_collision takes them, self_minimum_clearance beside minimum_clearance, and the flag bit
 * VGT_HIP_MOTION_SELF_NO_VALUE_IS_COLLISION beside VGT_HIP_SPHERES_OUTSIDE_IS_COLLISION 1u and
 * VGT_HIP_MOTION_STOP_AT_COLLISION 2u.  The field may be NULL (pass the extents as 0): its extents, resolution,
 * grid_from_world, rotation and minimum_clearance are then not looked at.
 *
 * THE DEFINITION.  Nothing of the kinematics, of the sphere check or of the pair check is restated here.
 * Samples: exactly vgt_hip_check_motions' (k == 0 and k == n > 0 take the given bits, otherwise a + t * (b - a)).
 * The environment part is there iff the field is not NULL: per sample what vgt_hip_check_spheres_from_joints returns, as
 * vgt_hip_check_motions says.
 * The self part is there iff P > 0: per sample what vgt_hip_check_self_collision returns for joint_values = q with the
 * same model, pairs, tree, world_from_base and joint_limits, minimum_clearance = self_minimum_clearance and its
 * NO_VALUE_IS_COLLISION bit set iff flags & VGT_HIP_MOTION_SELF_NO_VALUE_IS_COLLISION: status, min_clearance, min_pair
 * and fk_status, every bit.
 * Neither part: VGT_HIP_ERR_INVALID_ARGUMENT.
 * A sample COLLIDES when a part that is there says COLLISION; its cause is VGT_HIP_MOTION_CAUSE_ENVIRONMENT 1 |
 * VGT_HIP_MOTION_CAUSE_SELF 2.  A sample is WITHOUT A VALUE when it does not collide and a part that is there says
 * NO_VALUE.
 * Considered samples: all of them; with flags & VGT_HIP_MOTION_STOP_AT_COLLISION only the samples 0 ... first_collision
 * of this combined verdict: the later samples then do not exist for any output.
 * Outputs, one entry per motion; status is required, every other output may be NULL:
 *   status (uint8)            VGT_HIP_MOTION_COLLISION when a considered sample collides; otherwise
 *                             VGT_HIP_MOTION_NO_VALUE when one is without a value; otherwise VGT_HIP_MOTION_CLEAR.
 *                             VGT_HIP_MOTION_INVALID: the device form only, below.
 *   first_collision (int32)   the least colliding k, or -1
 *   collision_cause (uint8)   the cause bits of sample first_collision, or 0
 *   min_clearance, min_sample, min_sphere, min_gradient [3]
 *                             vgt_hip_check_motions' reduction of the environment part over the considered samples; NaN,
 *                             -1, -1, NaN x 3 without an environment part
 *   self_min_clearance (double), self_min_sample (int32), self_min_pair (int32)
 *                             the least non-NaN self min_clearance among the considered samples; ties under == go to the
 *                             lowest k; the value written is that sample's own bits and self_min_pair is that sample's
 *                             min_pair.  NaN, -1, -1 when there is no such sample or no self part.
 *   fk_status (uint8)         the OR of the considered samples' fk_status
 * All reductions are total orders on distinct k: no output depends on the launch geometry.  Two consequences:
 *   - without a self part every output this call shares with vgt_hip_check_motions equals that call's to the bit
 *     (collision_cause is then 1 where first_collision is not -1);
 *   - without VGT_HIP_MOTION_STOP_AT_COLLISION min_clearance, min_sample, min_sphere and min_gradient equal
 *     vgt_hip_check_motions' to the bit, whatever the self part finds.
 * VGT_HIP_ERR_INVALID_ARGUMENT before any device work: what vgt_hip_check_motions rejects (the field's own arguments
 * only with a field) and, for the pair list, what vgt_hip_check_self_collision rejects: NULL pairs with P > 0 and S > 0, a
 * negative P, P of 2^31 or more, a NaN self_minimum_clearance with P > 0; a tree or model larger than the kernel takes
 * (vgt_hip_motion_self_tile_samples gives 0; the message gives both numbers).  The host form also looks at its arrays and
 * names the first offender as the two calls do (num_steps, radii, pairs, links).  The device form cannot look: a motion
 * with n < 0 gets status INVALID, first_collision -1, collision_cause 0, NaN, -1, -1, NaN x 3, NaN, -1, -1 and fk_status
 * 0, and forms no address; a sphere_link outside [0, L) makes its sphere "without a value" for both parts and a sphere
 * index outside [0, S) its pair, and no address is formed from such a value.
 * E == 0 succeeds without a device.  With S == 0 the pair list is not looked at in either form (the self part, when P > 0,
 * is NO_VALUE at every sample).  The host form stages its arrays and blocks; the device form (field, model, pairs, joint
 * arrays, num_steps and outputs on the device; the three transforms / limits are host arrays) is enqueued on the context's
 * stream, not blocking.  Calls that use one tree are serialised by the context. */
#define VGT_HIP_MOTION_SELF_NO_VALUE_IS_COLLISION 4u
#define VGT_HIP_MOTION_CAUSE_ENVIRONMENT 1
#define VGT_HIP_MOTION_CAUSE_SELF 2
int vgt_hip_check_motions_with_self(
    vgt_hip_ctx* ctx, const float* sdf_host, int64_t nx, int64_t ny, int64_t nz, double resolution,
    const double* grid_from_world, const double* rotation, const double* sphere_xyzr_host,
    const int32_t* sphere_link_host, int64_t num_spheres, const int32_t* pairs_host, int64_t num_pairs,
    const vgt_hip_kinematics* tree, const double* joint_from_host, const double* joint_to_host,
    const int32_t* num_steps_host, int32_t uniform_steps, int64_t num_motions, const double* world_from_base,
    const double* joint_limits, double minimum_clearance, double self_minimum_clearance, uint32_t flags,
    uint8_t* status_host, int32_t* first_collision_host, uint8_t* collision_cause_host, double* min_clearance_host,
    int32_t* min_sample_host, int32_t* min_sphere_host, double* min_gradient_host, double* self_min_clearance_host,
    int32_t* self_min_sample_host, int32_t* self_min_pair_host, uint8_t* fk_status_host);
int vgt_hip_check_motions_with_self_dev(
    vgt_hip_ctx* ctx, const float* sdf_dev, int64_t nx, int64_t ny, int64_t nz, double resolution,
    const double* grid_from_world, const double* rotation, const double* sphere_xyzr_dev, const int32_t* sphere_link_dev,
    int64_t num_spheres, const int32_t* pairs_dev, int64_t num_pairs, const vgt_hip_kinematics* tree,
    const double* joint_from_dev, const double* joint_to_dev, const int32_t* num_steps_dev, int32_t uniform_steps,
    int64_t num_motions, const double* world_from_base, const double* joint_limits, double minimum_clearance,
    double self_minimum_clearance, uint32_t flags, uint8_t* status_dev, int32_t* first_collision_dev,
    uint8_t* collision_cause_dev, double* min_clearance_dev, int32_t* min_sample_dev, int32_t* min_sphere_dev,
    double* min_gradient_dev, double* self_min_clearance_dev, int32_t* self_min_sample_dev, int32_t* self_min_pair_dev,
    uint8_t* fk_status_dev);
/* The samples per tile the kernel uses for a tree of so many links carrying so many spheres: a power of two, at most 64,
 * whose poses and centres take (96 L + 24 S) T <= 16 KiB of LDS where more than one sample fits that; 0: no
 * links, or one sample does not fit a launch's 64 KiB (96 L + 32 S + 1792 bytes: 664 links without spheres, 1989 spheres
 * on one link).  Exposed so that tests put step counts, models and pair lists on both sides of it. */
int32_t vgt_hip_motion_self_tile_samples(int64_t num_links, int64_t num_spheres);

/* ---- Nearest cell of the other class per voxel (the feature transform of the signed EDT) ----
 * The SDF says how far every voxel is from the other class; this says WHICH voxel that distance is measured to: the
 * vector to the obstacle surface, a contact cell for a penetrating point, the partition of free space by nearest object.
 * The one definition (every entry point below, Python and the C++ layer refer to it):
 *   filled      exactly the predicate of vgt_hip_sdf_dev: occupancy > 0.5f, or == 0.5f with unknown_is_filled; NaN is
 *               free, +infinity filled, as that call classes them.  A mask byte is filled when non-zero.
 *   nearest[c]  (int32) for the cell c = x*ny*nz + y*nz + z: the linear index of a cell of the OTHER class whose centre is
 *               at minimal Euclidean distance from c's centre; -1 where the grid holds no cell of the other class.
 *   d2[c]       (int32, optional output) that minimal squared distance in cells, an exact integer; 0x7fffffff goes with
 *               -1.  sqrt(d2) * resolution, negated in filled cells, is the field of vgt_hip_sdf_dev without a border.
 *   ties        among equidistant candidates any one may be returned, but the choice is a pure function of the input:
 *               the same call on the same grid returns the same array (no atomics, nothing depends on launch order).
 *               As built: the lower z wins on a Z line, then the lower y among the lines' winners, then the lower x.
 *   border      there is NO virtual border (add_virtual_border of the SDF calls): a border cell has no index.
 *   limits      1 .. 16384 cells per axis (the SDF entry points' limit) and fewer than 2^31 cells; beyond them, for an
 *               empty grid, a NULL required pointer or a workspace that is too small: VGT_HIP_ERR_INVALID_ARGUMENT
 *               before any device work, nothing launched, outputs untouched.
 * Three separable passes Z, Y, X carry the site instead of the distance; everything that decides a winner is integer
 * arithmetic (csrc/nearest_kernels.hip).  The workspace holds 6 bytes per voxel (2 after the Z pass, 4 after the Y
 * pass) plus the line passes' hull stacks, which grow with the axis lengths, not with the volume (at most 131072
 * lanes in flight and at most 1 GiB: 7 GiB in all at 1024^3).  vgt_hip_nearest_workspace_bytes returns 0 for an empty
 * or over-limit grid.
 * vgt_hip_nearest_dev: everything on the device, enqueued on the context's stream, copies nothing, not blocking.
 * The host-pointer forms are blocking. */
size_t vgt_hip_nearest_workspace_bytes(int64_t nx, int64_t ny, int64_t nz);
int vgt_hip_nearest_dev(vgt_hip_ctx* ctx, const float* occupancy_dev, int64_t nx, int64_t ny, int64_t nz,
                        int unknown_is_filled, int32_t* nearest_dev, int32_t* d2_dev_or_null, void* workspace_dev,
                        size_t workspace_bytes);
int vgt_hip_nearest_from_occupancy_f32(vgt_hip_ctx* ctx, const float* occupancy_host, int64_t nx, int64_t ny, int64_t nz,
                                       int unknown_is_filled, int32_t* nearest_host, int32_t* d2_host_or_null);
int vgt_hip_nearest_from_mask_u8(vgt_hip_ctx* ctx, const uint8_t* filled_mask_host, int64_t nx, int64_t ny, int64_t nz,
                                 int32_t* nearest_host, int32_t* d2_host_or_null);
/* The same for uploaded cell records, with the filled predicate of vgt_hip_cells_sdf: occupancy AND (num_objects == 0
 * or the object id is listed).  object_host_or_null (uint32 per cell; tagged cell types only): the cell's own object id
 * where it is filled, elsewhere the id stored at nearest[c], 0 where nearest[c] is -1 -- with every object listed, the
 * partition of free space by nearest object in one extraction.  Blocking. */
int vgt_hip_cells_nearest(vgt_hip_ctx* ctx, vgt_hip_cells* cells, const uint32_t* objects_to_use, int64_t num_objects,
                          int unknown_is_filled, int32_t* nearest_host, int32_t* d2_host_or_null,
                          uint32_t* object_host_or_null);

/* SignedDistanceField::ComputeLocalExtremaMap (I/signed_distance_field.hpp:1205-1231 over :385-541; consumed by
 * TaggedObjectOccupancyComponentMap::UpdateSpatialSegments, S/tagged_object_occupancy_component_map.cpp:775-868):
 * for every voxel the grid-frame location (3 doubles) of the cell its gradient chain ends at -- the chain follows
 * the coarse gradient with edge gradients (rotated by `rotation`, 9 doubles row-major, NULL = none; the
 * reference applies the origin transform's rotation) uphill outside obstacles and downhill inside, one of
 * the 26 neighbours at a time -- or +infinity x3 when the chain leaves the grid.  Where chains run into a
 * cycle the reference's answer depends on its X-major visiting order (the first walk that reaches the cycle fixes
 * the cell every later walk inherits); the device formulation reproduces it: bit-identical results
 * (csrc/cell_kernels.hip).  Grids below 2^31 cells. */
int vgt_hip_sdf_local_extrema_map(vgt_hip_ctx* ctx, const float* sdf_host, int64_t nx, int64_t ny, int64_t nz,
                                  double resolution, const double* rotation, double* extrema_host);
int vgt_hip_sdf_local_extrema_map_dev(vgt_hip_ctx* ctx, const float* sdf_dev, int64_t nx, int64_t ny, int64_t nz,
                                      double resolution, const double* rotation, double* extrema_dev);

/* ---- connected components, spatial segments and component surfaces of the component map types ----
 *   OccupancyComponentMap::UpdateConnectedComponents()                        S/occupancy_component_map.cpp:447-509
 *   TaggedObjectOccupancyComponentMap::UpdateConnectedComponents(across)      S/tagged_object_occupancy_component_map.cpp:689-773
 *   TaggedObjectOccupancyComponentMap::UpdateSpatialSegments(threshold, p)    same file :775-868
 * all of which are topology_computation::ComputeConnectedComponents (I/topology_computation.hpp:59-196), a flood fill
 * over the six face neighbours started from every still-unlabelled cell in X-major / Z-fastest order.  The result is
 * therefore fully determined: a cell outside the labelling gets 0, every other cell the number of its component, and
 * components are numbered 1, 2, 3 ... in ascending order of the smallest linear index they contain.  The device
 * labelling (a union-find whose roots are the smallest index of their set, csrc/component_kernels.hip) returns exactly
 * these numbers, one uint32 per voxel; *num_components / *num_segments receive the largest label.  Grids below 2^31
 * cells.  Blocking (the count is read back).  Two face-adjacent cells are connected when
 *   vgt_hip_connected_components[_dev]   both occupancies are > 0.5, or both < 0.5, or both == 0.5 as floats (a NaN cell
 *                                        is a component of its own);
 *   vgt_hip_cells_connected_components   the same and, unless connect_across_objects, their object ids are equal
 *                                        (cells without object ids: connect_across_objects is ignored);
 *   vgt_hip_cells_spatial_segments[_dev] only cells with (occupancy < 0.5 or object id > 0) and no infinite component in
 *                                        their entry of the local-extrema map (vgt_hip_sdf_local_extrema_map, 3 doubles
 *                                        per voxel) are labelled; two of them are connected when their object ids are
 *                                        equal and the distance of their entries, evaluated in double as
 *                                        sqrt((dx*dx + dy*dy) + dz*dz), is < connected_threshold.  Cells with object ids
 *                                        only.
 * vgt_hip_cells_update_spatial_segments is UpdateSpatialSegments as one call: with add_virtual_border the field of
 * vgt_hip_cells_sdf without an object list, otherwise the one of vgt_hip_cells_free_and_named_objects_sdf; its local-
 * extrema map under `rotation` (9 doubles row-major or NULL); the segments.  Field and map never leave the device. */
int vgt_hip_connected_components(vgt_hip_ctx* ctx, const float* occupancy_host, int64_t nx, int64_t ny, int64_t nz,
                                 uint32_t* labels_host, uint32_t* num_components);
int vgt_hip_connected_components_dev(vgt_hip_ctx* ctx, const float* occupancy_dev, int64_t nx, int64_t ny, int64_t nz,
                                     uint32_t* labels_dev, uint32_t* num_components);
int vgt_hip_cells_connected_components(vgt_hip_ctx* ctx, vgt_hip_cells* cells, int connect_across_objects,
                                       uint32_t* labels_host, uint32_t* num_components);
int vgt_hip_cells_spatial_segments(vgt_hip_ctx* ctx, vgt_hip_cells* cells, const double* extrema_host,
                                   double connected_threshold, uint32_t* labels_host, uint32_t* num_segments);
int vgt_hip_cells_spatial_segments_dev(vgt_hip_ctx* ctx, vgt_hip_cells* cells, const double* extrema_dev,
                                       double connected_threshold, uint32_t* labels_dev, uint32_t* num_segments);
int vgt_hip_cells_update_spatial_segments(vgt_hip_ctx* ctx, vgt_hip_cells* cells, double connected_threshold,
                                          double resolution, int unknown_is_filled, int add_virtual_border,
                                          const double* rotation, uint32_t* labels_host, uint32_t* num_segments);
/* The dense form of ExtractComponentSurfaces (S/occupancy_component_map.cpp:290-350,531-567; the tagged variant
 * S/tagged_object_occupancy_component_map.cpp:485-541): mask[i] = 1 when the class of cell i is selected by
 * component_types -- 0x01 filled (> 0.5) | 0x02 empty (< 0.5) | 0x04 unknown (everything else, NaN included) -- and the
 * cell lies on a face of the grid or one of its six face neighbours has another label; else 0. */
int vgt_hip_component_surface_mask(vgt_hip_ctx* ctx, const float* occupancy_host, const uint32_t* labels_host,
                                   int64_t nx, int64_t ny, int64_t nz, int component_types, uint8_t* mask_host);
int vgt_hip_component_surface_mask_dev(vgt_hip_ctx* ctx, const float* occupancy_dev, const uint32_t* labels_dev,
                                       int64_t nx, int64_t ny, int64_t nz, int component_types, uint8_t* mask_dev);

/* ---- selected cells as compact ordered lists (csrc/select_kernels.hip) ----
 * A per-cell predicate, then the selected cells in ascending linear index (X-major, Z fastest: the order of the
 * reference's loops), with the cell's value and one uint32 per cell on request.  What the reference obtains with a host
 * loop over every voxel: IsSurfaceIndex (S/occupancy_map.cpp:201-246 and the same text in the other map types),
 * the display exports of I/ros_interface.hpp:92-148, the lists of ExtractComponentSurfaces.
 * The class of a value v against `threshold` t (0.5 for occupancy, 0.0 for a signed distance) is one of four bits:
 *   VGT_HIP_CLASS_ABOVE 0x01  v > t      VGT_HIP_CLASS_EQUAL     0x04  v == t
 *   VGT_HIP_CLASS_BELOW 0x02  v < t      VGT_HIP_CLASS_UNORDERED 0x08  none of them (NaN)
 * (The "unknown" bit 0x04 of vgt_hip_component_surface_mask and of the topology is 0x04 | 0x08 here.)
 * A cell is selected when its class is in class_mask (1 .. 15) and the rule holds:
 *   VGT_HIP_SELECT_ALL                no further condition.
 *   VGT_HIP_SELECT_SURFACE_26         IsSurfaceIndex, literally; threshold must be 0.5f.  A cell < 0.5 is a surface cell
 *                                     when one of its (up to 26) neighbours inside the grid is >= 0.5; a cell > 0.5 when
 *                                     one is <= 0.5; a cell == 0.5 when one is != 0.5.  A NaN cell never is one; a NaN
 *                                     neighbour satisfies != 0.5 only.  Cells outside the grid do not exist: a face of
 *                                     the grid is no surface by itself.
 *   VGT_HIP_SELECT_COMPONENT_SURFACE  the rule of vgt_hip_component_surface_mask: the cell lies on a face of the grid or
 *                                     one of its six face neighbours has another label.  Needs `labels`.
 * *count always receives the number of selected cells.  indices_out == NULL with capacity == 0 only counts.  When the
 * number exceeds `capacity` the call fails with VGT_HIP_ERR_INVALID_ARGUMENT (the message names both numbers) and writes
 * nothing to the outputs.  values_out / labels_out may be NULL; labels_out needs `labels`.  Grids below 2^31 cells
 * (indices are int32).  Blocking: the count is read back.  The _dev form takes device pointers for the grids and the
 * outputs and runs on the context's stream.  Scratch the context keeps: 1 bit per voxel + 4 bytes per 1024 voxels. */
#define VGT_HIP_CLASS_ABOVE 0x01
#define VGT_HIP_CLASS_BELOW 0x02
#define VGT_HIP_CLASS_EQUAL 0x04
#define VGT_HIP_CLASS_UNORDERED 0x08
#define VGT_HIP_SELECT_ALL 0
#define VGT_HIP_SELECT_SURFACE_26 1
#define VGT_HIP_SELECT_COMPONENT_SURFACE 2
int vgt_hip_select_cells(vgt_hip_ctx* ctx, const float* values_host, const uint32_t* labels_host, int64_t nx, int64_t ny,
                         int64_t nz, int rule, int class_mask, float threshold, int32_t* indices_out, float* values_out,
                         uint32_t* labels_out, int64_t capacity, int64_t* count);
int vgt_hip_select_cells_dev(vgt_hip_ctx* ctx, const float* values_dev, const uint32_t* labels_dev, int64_t nx,
                             int64_t ny, int64_t nz, int rule, int class_mask, float threshold, int32_t* indices_out,
                             float* values_out, uint32_t* labels_out, int64_t capacity, int64_t* count);
/* The same for uploaded cells, threshold 0.5f, lists to HOST memory.  labels_dev_or_null: the labels of
 * VGT_HIP_SELECT_COMPONENT_SURFACE on the device (e.g. of vgt_hip_cells_spatial_segments_dev); NULL: the cells' own
 * `component` member, for the layouts that have one.  payload_host (may be NULL) receives the member payload_member of
 * the selected cells, as the cell layout has them:
 *   VGT_HIP_CELL_MEMBER_OBJECT_ID        at object_id_offset (cells created with one)
 *   VGT_HIP_CELL_MEMBER_COMPONENT        at 4 of 8-byte cells without object id (OccupancyComponentCell), at 8 of 16-byte
 *                                        cells (TaggedObjectOccupancyComponentCell)
 *   VGT_HIP_CELL_MEMBER_SPATIAL_SEGMENT  at 12 of 16-byte cells
 * occupancy_host may be NULL. */
#define VGT_HIP_CELL_MEMBER_NONE 0
#define VGT_HIP_CELL_MEMBER_OBJECT_ID 1
#define VGT_HIP_CELL_MEMBER_COMPONENT 2
#define VGT_HIP_CELL_MEMBER_SPATIAL_SEGMENT 3
int vgt_hip_cells_select(vgt_hip_ctx* ctx, vgt_hip_cells* cells, const uint32_t* labels_dev_or_null, int rule,
                         int class_mask, int32_t* indices_host, float* occupancy_host, uint32_t* payload_host,
                         int payload_member, int64_t capacity, int64_t* count);

/* ---- the iso-surface of a field or a map as an indexed triangle mesh (csrc/surface_kernels.hip) ----
 * An extension: the reference offers cubes only (the display exports).  The method is surface nets on the lattice of
 * cell centres: no case table, shared vertices by construction, a closed and consistently oriented mesh wherever the
 * surface stays inside the grid.  The vertex and triangle arrays have the formats of vgt_hip_rasterize_mesh.
 *   field       float values f[i, j, k] on an nx x ny x nz grid, X-major / Z fastest.
 *   inside(v)   v < iso; with inside_above != 0: v > iso (occupancy: iso = 0.5f, inside_above = 1).  A value equal to iso
 *               is outside; a NaN is not inside.
 *   sample      (i, j, k) sits at the cell centre, per axis (index + 0.5) * resolution in double.
 *   cube        (i, j, k) with 0 <= i < nx - 1, 0 <= j < ny - 1, 0 <= k < nz - 1; its corners are the samples
 *               (i + a, j + b, k + c), a, b, c in {0, 1}.  ACTIVE: all 8 corners are finite (no NaN, no +-inf), some
 *               corner is inside and some is not.  A cube with a non-finite corner is void: no vertex, and no face uses it.
 *   vertex      one per active cube, in double without FMA contraction.  The cube's 12 edges in this order: axis x, then
 *               y, then z; with (b, c) the next two axes cyclically after axis a (x -> (y, z), y -> (z, x), z -> (x, y)),
 *               the four edges of axis a have the offsets (db, dc) = (0,0), (0,1), (1,0), (1,1).  An edge runs from its
 *               lower corner p0 to p1 = p0 + e_a and CROSSES when inside(v0) != inside(v1); then
 *               t = ((double)iso - (double)v0) / ((double)v1 - (double)v0), and the edge's offset inside the cube is t on
 *               axis a, db on axis b, dc on axis c.  Per axis component the offsets of the crossing edges are added left
 *               to right in the edge order, starting from 0.0, and divided by their number n (as a double);
 *               location_axis = (((double)index_axis + 0.5) + offset_axis) * resolution.  With world_from_grid (16
 *               doubles, column-major) row r is M[r] * x + M[4 + r] * y + M[8 + r] * z + M[12 + r], left to right: the
 *               rule of csrc/mesh_kernels.hip.  NULL: the grid frame.
 *   order       vertices in ascending linear index (i * ny + j) * nz + k of the cube's lowest corner in the SAMPLE grid;
 *               vertex_cells_out (int32, may be NULL) receives that index (to gather labels, object ids, colours).
 *   face        one quad, two triangles, per crossing lattice edge p -> p + e_a whose four cubes all exist and are all
 *               active (for a = x: 1 <= j <= ny - 2 and 1 <= k <= nz - 2, alike for y and z): an edge on a face of the
 *               lattice gives no quad, a surface that leaves the grid is open there.  With (b, c) as above the cubes, by
 *               lowest corner: c00 = p - e_b - e_c, c10 = p - e_c, c11 = p, c01 = p - e_b; the loop c00, c10, c11, c01 is
 *               counter-clockwise seen from +a.  p inside: the normal is +a, (q0, q1, q2, q3) = (c00, c10, c11, c01);
 *               otherwise (c00, c01, c11, c10).  Triangles (q0, q1, q2) and (q0, q2, q3), as vertex indices.  Normals
 *               point from inside to outside; the signed volume of a closed result is positive.
 *   face order  ascending linear index of p, then axis x, y, z.
 * The result is a function of the input alone (no atomics on the outputs).
 * *num_vertices and *num_triangles are always stored.  vertices_xyz_out == NULL with both capacities 0 only counts.  A
 * count above its capacity (vertex_capacity in vertices, triangle_capacity in triangles) fails with
 * VGT_HIP_ERR_INVALID_ARGUMENT (the message names both numbers) and writes nothing.  triangles_out may be NULL (vertices
 * only).  Grids below 2^31 cells; 3 * num_triangles below 2^31 (else VGT_HIP_ERR_INVALID_ARGUMENT after the count).  A
 * grid with an extent of 1 has no cubes: success, 0 and 0, nothing launched.  Blocking: the counts are read back.
 * Errors before any HIP call (VGT_HIP_ERR_INVALID_ARGUMENT): a null context, field or count, an extent <= 0, a
 * resolution that is not finite and positive, a non-finite iso, triangles_out or vertex_cells_out without
 * vertices_xyz_out, a capacity without its buffer.
 *   vgt_hip_extract_surface        field and mesh in host memory; the outputs are staged at their real size.
 *   vgt_hip_extract_surface_dev    device pointers for the field and the three outputs (the counts go to the host); runs
 *                                  on the context's stream; the vertex and triangle buffers are valid inputs of
 *                                  vgt_hip_rasterize_mesh_dev as they stand.
 *   vgt_hip_cells_extract_surface  the occupancy member of uploaded cells, iso = 0.5f, inside_above; mesh to host memory.
 * Scratch the context keeps: 5 bits per voxel (bit planes) + 4 bytes per 64 voxels + 8 bytes per 1024 voxels. */
int vgt_hip_extract_surface(vgt_hip_ctx* ctx, const float* values_host, int64_t nx, int64_t ny, int64_t nz, float iso,
                            int inside_above, double resolution, const double* world_from_grid, double* vertices_xyz_out,
                            int32_t* vertex_cells_out, int64_t vertex_capacity, int32_t* triangles_out,
                            int64_t triangle_capacity, int64_t* num_vertices, int64_t* num_triangles);
int vgt_hip_extract_surface_dev(vgt_hip_ctx* ctx, const float* values_dev, int64_t nx, int64_t ny, int64_t nz, float iso,
                                int inside_above, double resolution, const double* world_from_grid,
                                double* vertices_xyz_dev, int32_t* vertex_cells_dev, int64_t vertex_capacity,
                                int32_t* triangles_dev, int64_t triangle_capacity, int64_t* num_vertices,
                                int64_t* num_triangles);
int vgt_hip_cells_extract_surface(vgt_hip_ctx* ctx, vgt_hip_cells* cells, double resolution,
                                  const double* world_from_grid, double* vertices_xyz_out, int32_t* vertex_cells_out,
                                  int64_t vertex_capacity, int32_t* triangles_out, int64_t triangle_capacity,
                                  int64_t* num_vertices, int64_t* num_triangles);

/* ---- cost-to-go through free space, the neighbour to step to, and path tracing (csrc/travel_kernels.hip) ----
 * An extension: how far every cell is from a set of sources THROUGH passable cells -- the navigation function of a grid
 * planner, an admissible heuristic, "reachable within this budget".  This comment is the definition; the numpy
 * restatement (tests/travel_ref.py), the kernels and every binding refer to it.
 *   grid      nx x ny x nz, linear index c = x * ny * nz + y * nz + z, fewer than 2^31 cells.
 *   passable  a cell is passable exactly when vgt_hip_cast_segments in the corresponding mode would NOT call it a hit:
 *               VGT_HIP_TRAVEL_OCCUPANCY  float occupancy; blocked when occ > 0.5f || (unknown_is_filled && occ == 0.5f).
 *                                         A NaN is passable, +inf is blocked.
 *               VGT_HIP_TRAVEL_SDF_ABOVE  float SDF; blocked when (double)value <= threshold (NaN passable, +-inf
 *                                         compare as they are).  A NaN threshold is an invalid argument.  With the
 *                                         threshold at the robot's radius this is the inflated map.
 *             vgt_hip_cells_travel_cost: blocked is the filled predicate of vgt_hip_cells_sdf, occupancy (with
 *             unknown_is_filled) AND (num_objects == 0 or the cell's object id is listed).
 *   moves     the 26 neighbour offsets d fall into three classes by their number k = 1, 2, 3 of non-zero components.
 *             weights[k - 1] (uint32) is the cost of a move of class k; 0 disables the class.  weights[0] > 0, every
 *             weight <= 65535.  {1,0,0}: 6-connected step counts; {2,3,0}: 18-connected; {10,14,17}: the usual
 *             quasi-Euclidean 26-connected costs.  A move a -> b = a + d is ALLOWED when its class is enabled, b is in
 *             the grid and both cells are passable; with flags & VGT_HIP_TRAVEL_NO_CORNER_CUTTING additionally every
 *             cell a + s, s_i in {0, d_i}, must be passable (the 2 x 2 or 2 x 2 x 2 block the move spans).  Both rules
 *             are symmetric: cost-to-go and cost-from coincide.
 *   sources   int32 sources[num_sources], linear indices; uint32 source_costs[num_sources] or NULL (all 0).  A source
 *             outside [0, cells), on a blocked cell, or with an initial cost above cost_limit contributes nothing (not
 *             an error).  Duplicates: the least initial cost.
 *   cost      uint32 cost[c]: the least init(s) + sum of weights over all contributing sources s and all paths of
 *             allowed moves from s to c, without wrap-around; VGT_HIP_TRAVEL_UNREACHED where c is blocked, unreachable,
 *             or that least value exceeds cost_limit.  cost_limit <= 0xfffffffe, and that value means no limit.
 *             Candidates are formed in 64 bits and dropped when above the limit, so nothing overflows, and the result
 *             is exact (every prefix of a shortest path within the limit is within the limit).
 *   toward    int32 toward[c], optional, built from the CONVERGED cost in a pass of its own: -1 where cost[c] is
 *             UNREACHED; else the first b, over the offsets (dx, dy, dz) in ascending lexicographic order of -1, 0, 1,
 *             such that the move c -> b is allowed and cost[b] + weight == cost[c]; -1 when there is none; and, applied
 *             last, c itself where c is a contributing source with init(c) == cost[c] (a ROOT).  Enabled weights are
 *             positive, so following toward strictly lowers the cost and ends at a root.
 *   num_reached  int64, optional: the number of cells with cost != VGT_HIP_TRAVEL_UNREACHED.
 * The cost field is the unique fixed point of the relaxation and toward a pure function of it: no output depends on
 * launch order, on where atomics land or on how often a tile is revisited.
 *   method    cost is relaxed by tiles of 8 x 8 x 16 cells (Z fastest) in rounds, one launch each; after a round the
 *             host reads ONE word, "some tile is active", and stops when it is zero.  A round in which anything fell
 *             lowers at least one cell of a field of integers bounded below, so the rounds end.  How many there are
 *             depends on the grid, not on the number of tiles: a tile is flagged only by a seed or by one of its at
 *             most 26 neighbours, but by the same neighbour once for EVERY round in which that one lowers a cell they
 *             share, and a corridor may cross one face between two tiles dozens of times.  The loop is bounded by
 *             cells + 2 rounds.  Proof: call a reached cell of order h when h is the least number of moves from one
 *             tile into another on any of its least-cost paths (from a contributing source, initial cost included).
 *             After round k every cell of order below k holds its final cost.  k = 1: a cell of order 0 has a
 *             least-cost path inside its tile from a source there, the seed flagged that tile, and a run relaxes its
 *             tile to the fixed point over what it read.  k -> k + 1: on such a path of a cell c of order k let u -> v
 *             be the last move into another tile; u has order below k and lies in the halo of c's tile T.  The round
 *             r <= k that stored u's final cost (or the seed, r = 0) flagged T for round r + 1 <= k + 1, which reads
 *             that cost -- a kernel boundary lies between -- and lowers v and the rest of the path, all inside T, to
 *             their final costs; no later run raises anything.  A path with a repeated cell is not least-cost
 *             (weights are positive), so it has fewer moves than the grid has cells: every order is at most cells - 1,
 *             every cell is final after cells rounds, and one more round, flagged by the last stores, lowers nothing
 *             and flags nobody.  With something still active after cells + 2 rounds the call ends with
 *             VGT_HIP_ERR_RUNTIME: only a defect gets there, and the bound ends the call instead of spinning.
 *   vgt_hip_travel_cost        field, sources and outputs in host memory; blocking.
 *   vgt_hip_travel_cost_dev    everything in device memory (e.g. the output of vgt_hip_sdf_dev); only num_reached is a
 *                              host pointer.  workspace_dev: what vgt_hip_travel_cost_workspace_bytes says for the grid (0
 *                              for an empty grid or one over the limits): 1 bit per cell, two 4-byte flags per tile,
 *                              32 bytes of status.  A smaller workspace_bytes is an invalid argument.  The call copies nothing but
 *                              one word per round, SYNCHRONISES the context's stream every round, and returns when the
 *                              field has converged and every output is complete.  The first 32 bytes of the workspace
 *                              then hold uint32 {0, 0, rounds, 0}, uint64 reached, uint64 tile runs over all rounds.
 *   vgt_hip_cells_travel_cost  uploaded cell records (all map types), outputs to host memory.
 * Errors, VGT_HIP_ERR_INVALID_ARGUMENT before any device work and with the outputs untouched: a NULL required pointer
 * (context, field, weights, cost; sources when num_sources > 0), a negative extent, 2^31 cells or more, an unknown mode
 * or flag bit, a NaN threshold in SDF mode, weights[0] == 0, a weight above 65535, cost_limit == 0xffffffff,
 * num_sources < 0.  An empty grid succeeds (num_reached = 0, nothing else written); num_sources == 0 succeeds and writes
 * UNREACHED and -1 everywhere.
 *
 * Path tracing follows toward for a batch of starts on the device, so that the 4 B / voxel field need not come home.
 * starts int32[num_starts]; max_cells >= 1; start i writes the cells of its path, start first and root last, to
 * paths[i * max_cells + k], k < lengths[i]; slots beyond lengths[i] are left untouched.  status[i] (uint8):
 *   VGT_HIP_TRACE_OK         ended at a root (toward[c] == c).
 *   VGT_HIP_TRACE_UNREACHED  toward[start] == -1; length 0.
 *   VGT_HIP_TRACE_TRUNCATED  max_cells cells written and no root yet (also what bounds a malformed, cyclic toward).
 *   VGT_HIP_TRACE_INVALID    the start is outside [0, num_cells), or an entry read on the way is outside
 *                            [-1, num_cells) or is -1 after the start; the length is what was written before it.
 * One lane per start.  Errors (VGT_HIP_ERR_INVALID_ARGUMENT, before any device work): a NULL pointer (starts only when
 * num_starts > 0), num_cells < 0 or >= 2^31, num_starts < 0, max_cells < 1.  vgt_hip_trace_paths_dev enqueues on the
 * context's stream and does not wait. */
#define VGT_HIP_TRAVEL_OCCUPANCY 0
#define VGT_HIP_TRAVEL_SDF_ABOVE 1
#define VGT_HIP_TRAVEL_NO_CORNER_CUTTING 1u
#define VGT_HIP_TRAVEL_UNREACHED 0xffffffffu
#define VGT_HIP_TRACE_OK 0
#define VGT_HIP_TRACE_UNREACHED 1
#define VGT_HIP_TRACE_TRUNCATED 2
#define VGT_HIP_TRACE_INVALID 3
size_t vgt_hip_travel_cost_workspace_bytes(int64_t nx, int64_t ny, int64_t nz);
int vgt_hip_travel_cost(vgt_hip_ctx* ctx, const float* field_host, int64_t nx, int64_t ny, int64_t nz, int32_t mode,
                        int unknown_is_filled, double threshold, const uint32_t* weights, uint32_t flags,
                        const int32_t* sources_host, const uint32_t* source_costs_host, int64_t num_sources,
                        uint32_t cost_limit, uint32_t* cost_host, int32_t* toward_host, int64_t* num_reached);
int vgt_hip_travel_cost_dev(vgt_hip_ctx* ctx, const float* field_dev, int64_t nx, int64_t ny, int64_t nz, int32_t mode,
                            int unknown_is_filled, double threshold, const uint32_t* weights, uint32_t flags,
                            const int32_t* sources_dev, const uint32_t* source_costs_dev, int64_t num_sources,
                            uint32_t cost_limit, uint32_t* cost_dev, int32_t* toward_dev, int64_t* num_reached,
                            void* workspace_dev, size_t workspace_bytes);
int vgt_hip_cells_travel_cost(vgt_hip_ctx* ctx, vgt_hip_cells* cells, const uint32_t* objects_to_use,
                              int64_t num_objects, int unknown_is_filled, const uint32_t* weights, uint32_t flags,
                              const int32_t* sources_host, const uint32_t* source_costs_host, int64_t num_sources,
                              uint32_t cost_limit, uint32_t* cost_host, int32_t* toward_host, int64_t* num_reached);
int vgt_hip_trace_paths(vgt_hip_ctx* ctx, const int32_t* toward_host, int64_t num_cells, const int32_t* starts_host,
                        int64_t num_starts, int32_t max_cells, int32_t* paths_host, int32_t* lengths_host,
                        uint8_t* status_host);
int vgt_hip_trace_paths_dev(vgt_hip_ctx* ctx, const int32_t* toward_dev, int64_t num_cells, const int32_t* starts_dev,
                            int64_t num_starts, int32_t max_cells, int32_t* paths_dev, int32_t* lengths_dev,
                            uint8_t* status_dev);

/* ---- holes and voids per component: ComputeComponentTopology (I/topology_computation.hpp:331-670, called from
 * S/occupancy_component_map.cpp:594-653 and S/tagged_object_occupancy_component_map.cpp:566-625).
 * The reference walks hash sets per component; its result is this closed form, computed by csrc/topology_kernels.hip.
 * `labels` as vgt_hip_connected_components* writes them (1 .. num_components; 0 and anything larger is "no component
 * of the table"); a cell outside the grid belongs to no component.  For a label c whose class -- 0x01 filled (> 0.5) |
 * 0x02 empty (< 0.5) | 0x04 unknown (everything else), the rule of vgt_hip_component_surface_mask -- is selected by
 * component_types:
 *   1. lattice vertices are (i, j, k), 0 <= i <= nx etc.; the 8 cells round one are (i-1..i, j-1..j, k-1..k).  V_c =
 *      the vertices where at least one of the 8 is of c and at least one is not;
 *   2. a lattice edge at a vertex of V_c is exposed when, of the 4 cells round the edge, some are of c and some are
 *      not; m3 / m5 / m6 = vertices of V_c with exactly 3 / 5 / 6 exposed edges, num_surface_vertices = |V_c|;
 *   3. num_surfaces = connected components of the graph (V_c, exposed edges);
 *   4. num_voids = num_surfaces - 1;  num_holes = 1 + (m5 + 2 m6 - m3) / 8 + num_voids, the division as in C on int32
 *      (toward zero; a component pinched at an edge or a vertex leaves a remainder).
 * A vertex can lie in V_c of up to 8 components at once; each counts it.  num_holes / num_voids are returned as
 * computed, negative values included.
 * DIFFERENCE FROM THE REFERENCE: when it collects V_c it reads the Z + 1 neighbour at Z - 1 (:388-391), so the inner
 * vertices of a flat +Z face are never inserted and its vertex walk (:257) throws std::out_of_range for any component
 * with a flat top of 2 x 2 cells or more.  This library implements the evident intent, Z + 1.
 * Entry [c] of the table belongs to label c; [0] and the entries of labels whose class is not selected are all zero
 * (present == 0).  The table is written to HOST memory in every variant; out_capacity counts entries and must be at
 * least *num_components + 1, else the call fails after it has stored *num_components.
 *   vgt_hip_component_topology_dev    occupancy and labels already on the device (e.g. straight after
 *                                     vgt_hip_connected_components_dev, no host round trip); out_host has
 *                                     num_components + 1 entries;
 *   vgt_hip_component_topology        labels the grid first, as the reference's method does (it calls
 *                                     UpdateConnectedComponents); labels_host may be NULL, else it receives the labels;
 *   vgt_hip_cells_component_topology  the same for uploaded cells, connect_across_objects as for
 *                                     vgt_hip_cells_connected_components.
 * Grids below 2^31 cells whose vertex lattice (nx + 1)(ny + 1)(nz + 1) is below 2^31 too.  Blocking.
 * Device memory of a call, linear in voxels + surface nodes (a node is a pair of a vertex and a selected component with
 * the vertex in V_c): 4 bytes per lattice vertex, 16 bytes per node, 32 bytes per component; the labelling variants add
 * the labels (4 per voxel) and the labelling scratch the context keeps (4 per voxel).  Nodes below 2^31. */
typedef struct {
  int32_t present, num_holes, num_voids, num_surfaces, m3, m5, m6, num_surface_vertices;
} vgt_hip_component_topology_t;
int vgt_hip_component_topology_dev(vgt_hip_ctx* ctx, const float* occupancy_dev, const uint32_t* labels_dev,
                                   int64_t nx, int64_t ny, int64_t nz, int component_types, uint32_t num_components,
                                   vgt_hip_component_topology_t* out_host);
int vgt_hip_component_topology(vgt_hip_ctx* ctx, const float* occupancy_host, int64_t nx, int64_t ny, int64_t nz,
                               int component_types, uint32_t* labels_host, uint32_t* num_components,
                               vgt_hip_component_topology_t* out_host, uint64_t out_capacity);
int vgt_hip_cells_component_topology(vgt_hip_ctx* ctx, vgt_hip_cells* cells, int connect_across_objects,
                                     int component_types, uint32_t* labels_host, uint32_t* num_components,
                                     vgt_hip_component_topology_t* out_host, uint64_t out_capacity);

/* ---- triangle meshes into occupancy: mesh_rasterizer::RasterizeMesh (I/mesh_rasterizer.hpp,
 * S/mesh_rasterizer.cpp:105-229), csrc/mesh_kernels.hip.  Per triangle the bounding box of its vertices becomes an index
 * range (LocationToGridIndex), every cell of the range is a candidate, and a cell whose centre lies within
 * pow(resolution * 0.5 * sqrt(3.0), 2.0) (squared) of the triangle's "closest point" gets occupancy 1.0f; no other cell
 * and no other byte is written.
 *   vertices_xyz      3 doubles per vertex, in the frame world_from_grid maps to
 *   triangles         3 int32 vertex indices per triangle
 *   cells, cell_bytes the map: records of 4 (OccupancyCell) or 8 bytes (OccupancyComponentCell), the float occupancy at
 *                     offset 0, X-major / Z fastest; modified in place
 *   world_from_grid   OriginTransform, 16 doubles column-major (cell centre -> location); grid_from_world its inverse
 *                     (bounding box -> indices), as the reference's grid holds both.  NULL for both: the grid frame.
 *   enforce_contains  non-zero: an intersecting cell outside the grid fails the call (VGT_HIP_ERR_RUNTIME, "Triangle is
 *                     not contained by occupancy map (triangle N)", N the first such triangle); the host map is not
 *                     written then, a device map's content is unspecified.  Outside cells of a range are evaluated
 *                     literally in this mode.  Zero: ranges are clamped to the grid first (same result: the reference
 *                     skips outside cells).
 *   rule              VGT_HIP_MESH_RULE_REFERENCE: the literal port of CalcClosestPointOnTriangle (:59-102), which ranks
 *                     the three edge candidates by their own squared norm -- their distance to the frame's origin, not
 *                     to the query point (:82-84) --, so its result changes when a mesh is translated and cells along
 *                     slanted edges can be missed.  VGT_HIP_MESH_RULE_NEAREST: the same structure, ranked by the squared
 *                     distance to the query point (an extension: the watertight variant).
 * All geometry in double without FMA contraction, in the operation order stated at the top of csrc/mesh_kernels.hip.
 * Errors (VGT_HIP_ERR_INVALID_ARGUMENT, nothing rasterized): a vertex index out of range, a non-finite vertex, a
 * triangle whose normal has squared norm 0 (the reference's behaviour for the last two depends on code that is not
 * available; rejected here), and index ranges of more than 2^36 candidate cells in total.
 * The _dev form takes device pointers for vertices, triangles and cells and waits for the triangles' validation; without
 * enforce_contains the rasterization itself is left enqueued on the context's stream.
 * vgt_hip_mesh_grid_for: the map RasterizeMeshIntoOccupancyMap builds (:243-269): per-axis lower / upper over ALL
 * vertices, counts = ceil(((upper - lower) + 2 * resolution) / resolution), origin = lower - resolution (a translation).
 * Pure host code. */
#define VGT_HIP_MESH_RULE_REFERENCE 0
#define VGT_HIP_MESH_RULE_NEAREST 1
int vgt_hip_rasterize_mesh(vgt_hip_ctx* ctx, const double* vertices_xyz_host, int64_t num_vertices,
                           const int32_t* triangles_host, int64_t num_triangles, void* cells_host, int cell_bytes,
                           int64_t nx, int64_t ny, int64_t nz, double resolution, const double* world_from_grid,
                           const double* grid_from_world, int enforce_contains, int rule);
int vgt_hip_rasterize_mesh_dev(vgt_hip_ctx* ctx, const double* vertices_xyz_dev, int64_t num_vertices,
                               const int32_t* triangles_dev, int64_t num_triangles, void* cells_dev, int cell_bytes,
                               int64_t nx, int64_t ny, int64_t nz, double resolution, const double* world_from_grid,
                               const double* grid_from_world, int enforce_contains, int rule);
int vgt_hip_mesh_grid_for(const double* vertices_xyz_host, int64_t num_vertices, double resolution, int64_t* nx,
                          int64_t* ny, int64_t* nz, double* origin_xyz);

/* ---- enclosed space: fill what a shell encloses (scipy.ndimage.binary_fill_holes under face connectivity), in place;
 * csrc/component_kernels.hip.  An extension: the reference has no such operation, its rasterized meshes stay hollow
 * shells and their signed distance fields are positive inside the body.
 * `cells` as for vgt_hip_rasterize_mesh: records of cell_bytes = 4 (OccupancyCell) or 8 (OccupancyComponentCell) bytes,
 * the float occupancy at offset 0, X-major / Z fastest.
 *   filled(c)    occupancy > 0.5f || (unknown_is_filled && occupancy == 0.5f): the predicate of the SDF entry points.
 *                passable = !filled, so a NaN cell is passable.
 *   border cell  a cell whose index is 0 or n - 1 on some axis.
 *   outside      every passable cell that a chain of face-adjacent passable cells joins to a passable border cell, the
 *                border cells themselves included.
 * Every passable cell that is not outside gets occupancy 1.0f.  NO OTHER BYTE IS WRITTEN: filled cells and outside cells
 * keep their bit patterns (0.7f, -0.0f, NaN stay what they are), and so do the other four bytes of an 8-byte record.
 * *num_filled receives the number of cells written.  The call is idempotent (a second call writes 0 cells), and the
 * result depends on the input alone, never on the order in which the device's atomics land.  A grid with an extent of 1
 * on some axis consists of border cells: nothing is filled.
 * Which shells are sealed: a closed mesh rasterized under VGT_HIP_MESH_RULE_NEAREST separates inside from outside under
 * face connectivity (every cell the surface passes through has its centre within resolution * sqrt(3) / 2 of it, and a
 * face-connected path from inside to outside crosses the surface inside one of these cells).
 * VGT_HIP_MESH_RULE_REFERENCE can miss cells along slanted edges; such a shell leaks and its interior is filled only
 * where it happens to be sealed.  This call does not repair leaks.
 * Device memory: the labelling scratch the context keeps (4 bytes per voxel + 256, shared with
 * vgt_hip_connected_components*), NOTHING beyond it -- "outside" is a virtual root of the union-find, not a flag array --;
 * the host form adds the device copy of the map.  Grids below 2^31 cells.
 *   vgt_hip_fill_enclosed      host map; blocking; the host map is written only when the call succeeds.
 *   vgt_hip_fill_enclosed_dev  device map.  num_filled == NULL: the work is left enqueued on the context's stream (it can
 *                              stand between vgt_hip_rasterize_mesh_dev and vgt_hip_sdf_dev without a host round trip);
 *                              otherwise the call waits for the count.
 * Errors (VGT_HIP_ERR_INVALID_ARGUMENT, before any HIP call): a null context or map, cell_bytes other than 4 or 8, an
 * extent <= 0, 2^31 cells or more. */
int vgt_hip_fill_enclosed(vgt_hip_ctx* ctx, void* cells_host, int cell_bytes, int64_t nx, int64_t ny, int64_t nz,
                          int unknown_is_filled, int64_t* num_filled);
int vgt_hip_fill_enclosed_dev(vgt_hip_ctx* ctx, void* cells_dev, int cell_bytes, int64_t nx, int64_t ny, int64_t nz,
                              int unknown_is_filled, int64_t* num_filled /* host, may be NULL */);

/* ---- multi-GPU: the grid is cut into Z slabs, one device per slab (BASELINE.json config 5).
 * Lines along Y and X are local to a slab; only the first pass (nearest voxel of the other class
 * along Z) crosses slabs, and all it needs from the other slabs is, per (x, y) line, the nearest
 * filled / free voxel below and above.  So:
 *   1. vgt_hip_sdf_slab_begin_dev   local pass 1 (class records) + per-line summary of this slab: 4 bytes per line.  A slab's
 *                                    first voxel is filled or free, so the record holds, for the slab's first and
 *                                    for its last voxel, the class (bit 15: filled) and the global z of the first /
 *                                    last voxel of the OTHER class inside the slab (bits 0-14, 0x7fff when absent)
 *   2. the caller all-gathers the summaries (one RCCL all-gather; torch.distributed in
 *      voxelized_geometry_tools_amd/multi_gpu.py) into [world][lines] records and
 *      vgt_hip_sdf_slab_carries_dev reduces them to this slab's per-line carries
 *      (4 x int16: prev_filled, next_filled, prev_free, next_free as global z, -1 when absent)
 *   3. vgt_hip_sdf_slab_finish_dev  folds the carries in, then Y pass and X pass + finalize.
 * The slabs must be the ranges of vgt_hip_sdf_slab_range (equal shares of nz_global, earlier slabs take the
 * remainder): the carries are decoded with them.  As a guard against the likeliest mistake,
 * vgt_hip_sdf_slab_finish_dev rejects carries that vgt_hip_sdf_slab_carries_dev computed ON THE SAME CONTEXT for
 * another (z_offset, nz_local, nz_global) than the one it is given (VGT_HIP_ERR_INVALID_ARGUMENT; ABI version 2.
 * Version 1 exchanged 8-byte records with absolute positions and accepted any partition).  The guard is
 * best-effort: it goes by the address of the carries buffer, one finish consumes it, and carries that were written
 * by another context, a copy or a collective are not checked -- the partition rule above is the contract.
 * The workspace is the one of vgt_hip_sdf_dev for the slab's extents and must be the same buffer
 * in both calls.  kernel_ms (optional): begin -> [scan]; finish -> [fix-up, Y pass, X pass];
 * when given, the call blocks until the work has finished.
 * Limits: summaries and carries hold GLOBAL z in 15 / 16 bits, so the whole grid's Z extent (nz_global,
 * and z_offset + nz_local of every slab) must not exceed 16384 -- the per-axis limit of every SDF
 * entry point; larger values are rejected with VGT_HIP_ERR_INVALID_ARGUMENT. */
int vgt_hip_sdf_slab_range(int64_t nz_global, int32_t world, int32_t rank, int64_t* z_offset, int64_t* nz_local);
size_t vgt_hip_sdf_slab_summary_bytes(int64_t nx, int64_t ny);
int vgt_hip_sdf_slab_begin_dev(vgt_hip_ctx* ctx, const float* occupancy_dev, int64_t nx, int64_t ny,
                               int64_t nz_local, int64_t z_offset, int unknown_is_filled,
                               void* workspace_dev, size_t workspace_bytes, void* summary_dev,
                               float* kernel_ms);
size_t vgt_hip_sdf_slab_carries_bytes(int64_t nx, int64_t ny);
int vgt_hip_sdf_slab_carries_dev(vgt_hip_ctx* ctx, const void* gathered_summaries_dev, int32_t world,
                                 int32_t rank, int64_t nx, int64_t ny, int64_t nz_global, void* carries_dev);
int vgt_hip_sdf_slab_finish_dev(vgt_hip_ctx* ctx, int64_t nx, int64_t ny, int64_t nz_local,
                                int64_t z_offset, int64_t nz_global, double resolution,
                                int add_virtual_border, const void* carries_dev, float* sdf_dev,
                                void* workspace_dev, size_t workspace_bytes, float* minmax_dev,
                                float* kernel_ms);

/* ---- multi-GPU from ONE process, host buffers in and out: the large-grid branch of
 *      OccupancyMap::ExtractSignedDistanceFieldFloat (S/occupancy_map.cpp:256-260;
 *      I/occupancy_map.hpp:174-210).  The grid is cut into min(num_devices, nz) Z slabs, slab r runs
 *      on devices[r]: strided upload of occupancy[:, :, z0:z1], the slab pipeline above, ONE exchange
 *      of the per-line summaries (rccl ncclAllGather, one call per device in a group), download.
 *      The N uploads / pipelines / downloads run concurrently on per-device streams; the caller's
 *      arrays are page-locked for the duration of the call when possible.  A device may be listed
 *      more than once (several slabs on one GPU); rccl cannot form a communicator then, and the
 *      summaries are copied slab to slab instead.  Result and extrema are bit-identical to
 *      vgt_hip_sdf_from_occupancy_f32 on one device.  Blocking. */
int vgt_hipx_sdf_multi(const int* devices, int num_devices, const float* occupancy_host, int64_t nx,
                       int64_t ny, int64_t nz, double resolution, int unknown_is_filled,
                       int add_virtual_border, float* sdf_host, float* out_min, float* out_max);
/* vgt_hipx_sdf_multi keeps the per-slab contexts, streams and device buffers of the last (device list, grid shape)
 * it served for the next call with the same key (one extraction at a time per process); this frees them. */
void vgt_hipx_release(void);
/* Phases of the last vgt_hipx_sdf_multi call, milliseconds: [0] set-up (slab set on a miss + page-locking),
 * [1] slowest slab's upload, [2] its scan + exchange + passes, [3] its download (events on the slab streams; the
 * phases of different slabs overlap), [4] the whole call. */
int vgt_hipx_last_timing(float* ms5);


/* ---- ONE point cloud over several devices (the reference dispatches whole clouds,
 *      S/device_pointcloud_voxelization.cpp:147-149, so a single large cloud uses one device there).
 *      DeviceVoxelizationHelperInterface::RaycastPoints (I/device_voxelization_interface.hpp:151-158) with the
 *      points cut into 1 + num_helpers contiguous shares (vgt_hipx_point_share: equal shares, earlier shares take
 *      the remainder): share 0 is cast on `ctx`'s device straight into grid `grid_index`, share k on
 *      helper_devices[k-1] into a private tracking grid, and the private grids are then ADDED into grid
 *      `grid_index` -- rccl ncclReduce(sum, int32, root = ctx's device) when all the devices are distinct,
 *      copy + add otherwise (a device listed twice, or the caller's own: the one-GPU test of this path).
 *      Tracking counts are integers, so the result equals vgt_hip_raycast_points_f32 on the whole cloud bit for
 *      bit, whatever the split; counts already in the grid are kept.  Blocking; the sum is ordered on ctx's
 *      stream, so the filter that follows sees it.  Helper contexts and grids are kept for the next call with
 *      the same (device, helper list, cell count); vgt_hipx_release frees them.  num_helpers = 0 is the plain call. */
int vgt_hipx_point_share(int64_t num_points, int32_t shares, int32_t share, int64_t* first, int64_t* count);
int vgt_hipx_raycast_points_split(vgt_hip_ctx* ctx, vgt_hip_grids* grids, size_t grid_index,
                                  const int* helper_devices, int num_helpers, const float* points_xyz_host,
                                  int64_t num_points, float max_range, const float* grid_pointcloud_transform,
                                  float voxel_size, float inverse_voxel_size, float grid_x_size,
                                  float grid_y_size, float grid_z_size, int32_t num_x_voxels,
                                  int32_t num_y_voxels, int32_t num_z_voxels);

#if defined(__GNUC__) || defined(__clang__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif /* VGT_HIP_H_ */
