// Internal declarations shared by the HIP translation units of libvgt_hip.so.
// Not part of the public ABI (that is include/vgt_hip.h).
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include <string>

namespace vgt
{
// Sets the calling thread's vgt_hip_last_error() message (for translation units other than
// vgt_hip_capi.hip that implement parts of the C ABI).
void SetLastError(const std::string& message);
}  // namespace vgt
struct vgt_hip_ctx;
namespace vgt
{
// The stream a context enqueues on (vgt_hip_set_stream's, or its own), for translation units that add work
// which later calls on the context must see (vgt_hipx_multi.hip).
hipStream_t ContextStream(const vgt_hip_ctx* ctx);

// Intermediate encodings of the signed Euclidean distance transform.
//  pass 1 (Z)       -> class records (ClassRecord below): the classes of 64 voxels of a Z line and where the nearest
//                      class change outside them is; the distance along Z to the nearest voxel of the OTHER class
//                      follows from them, kInf16 or more when the line holds no such voxel.
//  pass 2 (Y pass)  -> int32, sign and magnitude: bit 31 = the voxel is filled, bits 0-30 = squared distance in the YZ
//                      plane, kInf32 when none.
//  pass 3 (X pass)  -> float SDF.
// (The testing library's cross-check pipeline has encodings of its own -- an int16 field after pass 1 --: edt_crosscheck.hpp.)
constexpr int16_t kInf16 = 32767;
constexpr int32_t kInf32 = 0x7fffffff;
// Largest supported extent per axis: keeps every squared distance (<= 3*kMaxExtent^2)
// and every parabola value below 2^31.
constexpr int64_t kMaxExtent = 16384;

// Which kernel the plain X pass with 32-bit entries runs (SdfParams::x_kernel): chosen on the device by scene, the coarse-hull
// kernel wherever it applies (whatever it costs), or the plain kernel alone.
constexpr int kXKernelByScene = 0, kXKernelCoarse = 1, kXKernelPlain = 2;
struct SdfParams
{
  int64_t nx, ny, nz;  // extents of the grid held by this device (a Z slab when partitioned)
  double resolution;
  int unknown_is_filled;
  int add_virtual_border;
  // Z-slab partitioning (multi-GPU): this device holds global z in [z_offset, z_offset + nz) of a
  // grid with nz_global voxels along Z.  Single device: z_offset = 0, nz_global = nz.
  int64_t z_offset = 0;
  int64_t nz_global = 0;
  // A batch of `batch` equal grids, one after the other in every buffer (vgt_hip_sdf_batch_dev): pass 1 and the Y pass
  // see it as one grid of batch * nx slices (their lines never leave a slice), only the X pass -- whose lines run along
  // x -- and the extrema need to know.
  int64_t batch = 1;
  // The X pass's kernel by scene (edt_sweep_kernels.hip: the coarse-hull form of the plain X sweep wins on sparse scenes and
  // loses on dense ones).  Pass 1 adds the number of Z lines that hold one class into one_class_lines[0] and the number of
  // lines counted into one_class_lines[1] when it is given (cleared by LaunchInitMinMax: the words kOneClassWord and the
  // next of a single grid's minmax_enc), and the X pass, given the same words, enqueues both kernels and lets the device
  // choose (kXKernelByScene).  The default is the plain kernel alone.
  uint32_t* one_class_lines = nullptr;
  int x_kernel = kXKernelPlain;
};
// minmax_enc of ONE grid: [0] / [1] the extrema, [kOneClassWord] pass 1's count of one-class Z lines among the
// [kOneClassWord + 1] lines that its counting workgroups saw (a sample spread over the grid).
constexpr int kOneClassWord = 2;

// Pass 1 of the default pipeline (edt_record_kernels.hip): the binarised grid as CLASS RECORDS, one 16-byte record per
// 64-voxel word of a Z line, laid out [x][word][y] so that the records a Y-pass wave walks through (one x, one word,
// every y) are contiguous.  A record holds the classes of its 64 voxels and where the nearest class change outside the
// word is; the Y pass derives every voxel's distance along Z from it (0.25 B per voxel instead of a 2-byte distance).
// A class change ("transition") at position t means class(t) != class(t + 1): for every voxel above t (up to the next
// transition) the nearest voxel of the other class below is t, for every voxel at or below t the nearest one above is t + 1.
//   mask:    bit k = voxel 64 w + k is filled; bits past the end of the line repeat the line's last voxel
//   below2:  last transition below the word (t < 64 w), as 2 (t - 64 w) + kRecordBias; kRecordNoneBelow when none
//   above2:  first transition at or after the word's last voxel (t >= 64 w + 63), same encoding; kRecordNoneAbove when
//            none; kRecordNoSite when the whole line -- all slabs of it -- holds one class only (below2 is then
//            kRecordNoneBelow and the word has no transition of its own): no voxel of the word has a distance along Z
// With xq = 2 lane - 1 + kRecordBias, |xq - t2| + 1 is TWICE the distance from voxel `lane` to the other class across
// the transition encoded as t2, whichever side it lies on (one v_sad_u32); the "none" encodings give >= 2 kInf16.
struct ClassRecord
{
  uint32_t mask_lo, mask_hi, below2, above2;
};
constexpr uint32_t kRecordBias = 1u << 17;
constexpr uint32_t kRecordNoneBelow = 0u;
constexpr uint32_t kRecordNoneAbove = 2u * kRecordBias;
constexpr uint32_t kRecordNoSite = 0xfffffff0u;
inline int64_t RecordWords(int64_t nz) { return (nz + 63) / 64; }
// records of a grid (+ padding: the Y pass loads whole 64-row blocks three blocks ahead, so it FETCHES records up to
// 3 * 64 - 1 = 191 rows past the end of the line it works on -- the next lines' records, a later chunk's not yet written
// ones, or this padding, which nobody initialises.  It never USES them: every row is guarded by `row < n`.  Whoever hands
// LaunchPassYSweepRecords a record buffer must keep the padding behind it, or the fetch leaves the allocation.)
constexpr int kRecordPadding = 256;
inline size_t ClassRecordBytes(int64_t nx, int64_t ny, int64_t nz)
{
  return (static_cast<size_t>(nx) * static_cast<size_t>(RecordWords(nz)) * static_cast<size_t>(ny) + kRecordPadding) *
         sizeof(ClassRecord);
}

// Per-line summary of a Z slab, exchanged between devices: 4 bytes.  A slab's first voxel is filled or free, so of
// "first filled" and "first free" one is the slab's first voxel; the record keeps the class of the first voxel and the
// position of the first voxel of the OTHER class (the same for the last voxel):
//   bit 15 = 1: the slab's first / last voxel is filled;  bits 0-14: global z of the first / last voxel of the other
//   class inside the slab, kSlabNone when the slab holds one class only.
// The slabs follow SlabRange (equal shares, earlier slabs take the remainder), which tells the reader where they begin.
struct SlabLineSummary
{
  uint16_t first, last;
};
constexpr uint16_t kSlabFilledBit = 0x8000u;
constexpr uint16_t kSlabNone = 0x7fffu;
// [z0, z0 + count) of slab `rank` of `world` along a Z axis of nz voxels.
inline void SlabRange(int64_t nz, int world, int rank, int64_t* z0, int64_t* count)
{
  const int64_t share = nz / world, extra = nz % world;
  *z0 = rank * share + (rank < extra ? rank : extra);
  *count = share + (rank < extra ? 1 : 0);
}
// Per-line carries derived from the other slabs' summaries: nearest filled / free voxel of the
// line below this slab (largest global z) and above it (smallest global z), -1 when absent.
struct SlabLineCarry
{
  int16_t prev_filled, next_filled, prev_free, next_free;
};

// The pipeline: class records (pass 1, edt_record_kernels.hip) + lane-per-line sweep passes, Felzenszwalb-Huttenlocher
// stacks with their tops in LDS (edt_sweep_kernels.hip; any extent), short-line kernels for lines of few rows
// (edt_short_kernels.hip).  (Earlier rounds' other pipelines -- LDS-tiled envelopes, the int16-fed sweeps -- are in the
// git history and profiles/r2 ... r5/experiments.md.)

// --- launchers of the distance transform.  All asynchronous on `stream`. ---
// Multi-GPU (edt_kernels.hip): per-line carries of slab `rank` from the gathered summaries of all `world` slabs.
hipError_t LaunchSlabCarries(const SlabLineSummary* summaries, int world, int rank, int64_t lines, int64_t nz_global,
                             SlabLineCarry* carries, hipStream_t stream);
// Pass 1 of the default pipeline (edt_record_kernels.hip): occupancy (float) or mask (u8) -> class records
// (ClassRecordBytes bytes).  `summary` (optional, multi-GPU) receives one SlabLineSummary per (x, y) line; lines that
// hold one class are then marked by LaunchSlabRecordFixup, which folds the other slabs' carries into the records.
hipError_t LaunchClassRecordsFromOccupancy(const float* occupancy, ClassRecord* records, const SdfParams& p,
                                           SlabLineSummary* summary, hipStream_t stream);
hipError_t LaunchClassRecordsFromMask(const uint8_t* mask, ClassRecord* records, const SdfParams& p,
                                      SlabLineSummary* summary, hipStream_t stream);
hipError_t LaunchSlabRecordFixup(ClassRecord* records, const SlabLineCarry* carries, const SdfParams& p,
                                 hipStream_t stream);
// Scratch of the sweep passes (work counters, spilled stack entries and sign words of the workgroups in flight): the
// launchers use as many workgroups as its size allows, see SweepPassScratchBytes.
struct SweepScratch
{
  void* ptr;
  size_t bytes;
};
// Y pass of the default pipeline: class records -> int32 signed squared distance (edt_sweep_kernels.hip).
hipError_t LaunchPassYSweepRecords(const ClassRecord* records, int32_t* out32, SweepScratch scratch, const SdfParams& p,
                                   hipStream_t stream);
// X pass + finalize (edt_kernels.hip: the short-line kernels or the sweeps, by the length of the lines): int32 -> float
// SDF, min/max folded into minmax_enc (2 x uint32, order-preserving encoding, must be pre-initialised by InitMinMax).
// `scratch`: SweepPassScratchBytes bytes (part of the SDF workspace).
hipError_t LaunchPassXFinalize(const int32_t* in32, float* sdf, uint32_t* minmax_enc, SweepScratch scratch,
                               const SdfParams& p, hipStream_t stream);
// Lines of at most kShortLineRows rows take the short-line kernels (edt_short_kernels.hip: the whole line in registers,
// exhaustive search) instead of the sweeps; same encodings, same results.  ShortLineRows() is the limit in force for
// the X pass: kShortLineRows, or what a testing build was told (vgt_hip_testing_set_short_line_rows; 0 = sweeps for
// every length); ShortLineLimit(items) the Y pass's.
constexpr int kShortLineRows = 64;
// ... and lines of up to kShortLineRowsFewItems rows when the launch has so few items (at most kFewLineItems bundles of
// 64 lines) that the sweeps would leave most of the chip idle: the search costs O(rows^2) but splits over the waves.
constexpr int kShortLineRowsFewItems = 128;
constexpr int64_t kFewLineItems = 1024;
// What a testing build was told (vgt_hip_testing_set_short_line_rows), -1 = nothing (the product library: always).
// Defined next to that hook, in vgt_hip_capi.hip.
int ShortLineOverride();
// Workgroups (= scratch slots) per sweep launch a testing build was told to stop at (vgt_hip_testing_set_sweep_slots), 0 =
// nothing (the product library: always).  Defined next to that hook, in vgt_hip_capi.hip.
int SweepSlotsOverride();
inline int ShortLineRows()
{
  const int told = ShortLineOverride();
  return told >= 0 ? told : kShortLineRows;
}
inline int ShortLineLimit(int64_t items)
{
  const int told = ShortLineOverride();
  if (told >= 0) return told;  // (a testing build was told: that limit, whatever the item count)
  return items <= kFewLineItems ? kShortLineRowsFewItems : kShortLineRows;
}
hipError_t LaunchPassYShortRecords(const ClassRecord* records, int32_t* out32, const SdfParams& p, hipStream_t stream);
hipError_t LaunchPassXShortFinalizeRange(const int32_t* in32, float* sdf, uint32_t* minmax_enc, const SdfParams& p,
                                         int64_t outer_begin, int64_t outer_count, hipStream_t stream);
// For callers that pipeline parts of a grid: the Y pass treats X slices independently (call LaunchPassYSweepRecords
// with nx = slices of a contiguous part), and the X pass can be launched over a range of Y positions (full-grid
// pointers and extents in `p`; outer_count < 0: the whole axis).
hipError_t LaunchPassXFinalizeRange(const int32_t* in32, float* sdf, uint32_t* minmax_enc, SweepScratch scratch,
                                    const SdfParams& p, int64_t outer_begin, int64_t outer_count, hipStream_t stream);
// The sweeps' own X pass, whatever the length of the lines (edt_sweep_kernels.hip).
hipError_t LaunchPassXSweepFinalizeRange(const int32_t* in32, float* sdf, uint32_t* minmax_enc, SweepScratch scratch,
                                         const SdfParams& p, int64_t outer_begin, int64_t outer_count_or_all,
                                         hipStream_t stream);
hipError_t LaunchPassXSweepFinalize(const int32_t* in32, float* sdf, uint32_t* minmax_enc, SweepScratch scratch,
                                    const SdfParams& p, hipStream_t stream);
// Scratch for the lane-per-line sweep passes (edt_sweep_kernels.hip): work counter, spilled stack entries and sign
// words of the workgroups in flight.
size_t SweepPassScratchBytes(int64_t nx, int64_t ny, int64_t nz, int64_t batch = 1);
// `count` pairs of ordered encodings (one per grid of a batch); one grid: the word kOneClassWord is cleared as well
hipError_t LaunchInitMinMax(uint32_t* minmax_enc, hipStream_t stream, int64_t count = 1);
hipError_t LaunchDecodeMinMax(const uint32_t* minmax_enc, float* minmax_out, hipStream_t stream, int64_t count = 1);

// --- launchers (cell_kernels.hip): map types whose cells carry an object id ---
hipError_t LaunchCellMask(const void* cells_dev, int64_t num_cells, int cell_bytes, int object_id_offset,
                          int mode, const uint32_t* objects_dev, int num_objects, int unknown_is_filled,
                          uint8_t* mask_dev, hipStream_t stream);
// masks_dev[b * num_cells + i] = cell i is filled and belongs to object ids_dev[b]: the byte masks of a batch of
// per-object extractions, one pass over the cells.
hipError_t LaunchCellObjectMasks(const void* cells_dev, int64_t num_cells, int cell_bytes, int object_id_offset,
                                 const uint32_t* ids_dev, int num_ids, int unknown_is_filled, uint8_t* masks_dev,
                                 hipStream_t stream);
// Distinct object ids > 0 in one pass: table_dev = 2^table_log2 zeroed uint32 slots, ids_dev = room for as many ids,
// count_overflow_dev = {number of ids, 1 if the table overflowed} (zeroed by the caller).
hipError_t LaunchDistinctObjectIds(const void* cells_dev, int64_t num_cells, int cell_bytes, int object_id_offset,
                                   uint32_t* table_dev, int table_log2, uint32_t* ids_dev, uint32_t* count_overflow_dev,
                                   hipStream_t stream);
hipError_t LaunchNextObjectId(const void* cells_dev, int64_t num_cells, int cell_bytes, int object_id_offset,
                              uint32_t after, uint32_t* result_dev, hipStream_t stream);
hipError_t LaunchCombineFreeAndNamed(const float* free_sdf_dev, const float* named_sdf_dev, int64_t num_cells,
                                     float* out_dev, uint32_t* minmax_enc, hipStream_t stream);

// SDF consumer: grid-aligned (or rotated) coarse gradient of every voxel, 3 doubles per voxel.
hipError_t LaunchCoarseGradient(const float* sdf_dev, int64_t nx, int64_t ny, int64_t nz, double resolution,
                                int enable_edge_gradients, const double* rotation_host, double* gradient_dev,
                                uint8_t* has_value_dev, hipStream_t stream);

// SDF consumers, batched queries (3 doubles per query point): trilinear distance estimate and fine gradient.
// grid_from_world_host: 16 doubles column-major (InverseOriginTransform) or nullptr = identity.
hipError_t LaunchEstimateDistance(const float* sdf_dev, int64_t nx, int64_t ny, int64_t nz, double resolution,
                                  const double* grid_from_world_host, const double* queries_dev, int64_t num_queries,
                                  double* distance_dev, uint8_t* has_value_dev, hipStream_t stream);
hipError_t LaunchFineGradient(const float* sdf_dev, int64_t nx, int64_t ny, int64_t nz, double resolution,
                              const double* grid_from_world_host, const double* queries_dev, int64_t num_queries,
                              double nominal_window_size, double* gradient_dev, uint8_t* has_value_dev,
                              uint32_t* window_too_large_dev, hipStream_t stream);

// SignedDistanceField::ProjectLocationOutOfCollisionToMinimumDistance for a batch of points, one lane per point
// (statuses and outputs: include/vgt_hip.h).  rotation_host: 9 doubles row-major or nullptr.  has_value_dev, status_dev
// and iterations_dev may be nullptr.  max_iterations == 0 selects DefaultProjectionIterations.
int32_t DefaultProjectionIterations(int64_t nx, int64_t ny, int64_t nz, double stepsize_multiplier);
hipError_t LaunchProjectOutOfCollision(const float* sdf_dev, int64_t nx, int64_t ny, int64_t nz, double resolution,
                                       const double* grid_from_world_host, const double* rotation_host,
                                       const double* queries_dev, int64_t num_queries, double minimum_distance,
                                       double stepsize_multiplier, int32_t max_iterations, double* position_dev,
                                       uint8_t* has_value_dev, uint8_t* status_dev, int32_t* iterations_dev,
                                       hipStream_t stream);

// SignedDistanceField::ComputeLocalExtremaMap: 3 doubles per voxel (grid-frame location of the extremum the
// voxel's gradient chain ends at, +inf when it leaves the grid).  scratch_dev: LocalExtremaScratchBytes bytes.
size_t LocalExtremaScratchBytes(int64_t num_cells);
hipError_t LaunchLocalExtremaMap(const float* sdf_dev, int64_t nx, int64_t ny, int64_t nz, double resolution,
                                 const double* rotation_host, double* extrema_dev, void* scratch_dev,
                                 hipStream_t stream);

// --- launchers (component_kernels.hip): connected components, spatial segments, component surfaces ---
// Which predicate joins two face-adjacent cells:
//   kComponentClasses        both occupancies > 0.5, or both < 0.5, or both == 0.5 (OccupancyComponentMap)
//   kComponentClassesAndIds  the same and equal object ids (TaggedObjectOccupancyComponentMap, not across objects)
//   kComponentSegments       UpdateSpatialSegments: cells that are (free or of a named object) and have a finite entry in
//                            the extrema map; equal object ids and extrema closer than connected_threshold
constexpr int kComponentClasses = 0;
constexpr int kComponentClassesAndIds = 1;
constexpr int kComponentSegments = 2;
//   kComponentFill           enclosed space (LaunchFillEnclosed only): filled cells take no part, two passable cells are
//                            always connected, and passable border cells are united with a virtual root "outside"
constexpr int kComponentFill = 3;
// scratch_dev: ComponentScratchBytes bytes (the int32 union-find labels and the scan's block counts).  labels_dev
// receives 0 for a cell outside the labelling, else the number of its component: 1, 2, 3 ... in ascending order of the
// smallest linear index of the component.  The number of components lies at ComponentCountPtr(scratch_dev) afterwards
// (stream-ordered).  cells_dev: records of cell_bytes bytes with the float occupancy first (a plain float grid: 4, -1).
// Grids below 2^31 cells.
size_t ComponentScratchBytes(int64_t num_cells);
const uint32_t* ComponentCountPtr(const void* scratch_dev, int64_t num_cells);
hipError_t LaunchLabelComponents(const void* cells_dev, int cell_bytes, int object_id_offset, int mode,
                                 const double* extrema_dev, double connected_threshold, int64_t nx, int64_t ny,
                                 int64_t nz, uint32_t* labels_dev, void* scratch_dev, hipStream_t stream);
// Enclosed space (include/vgt_hip.h, vgt_hip_fill_enclosed): every passable cell that no chain of face-adjacent passable
// cells joins to a passable border cell gets occupancy 1.0f, in place; the number of cells written lies at
// FillCountPtr(scratch_dev) afterwards (stream-ordered).  scratch_dev: FillScratchBytes bytes (the int32 union-find
// labels + 256; never more than ComponentScratchBytes).  Grids below 2^31 cells.
size_t FillScratchBytes(int64_t num_cells);
const unsigned long long* FillCountPtr(const void* scratch_dev);
hipError_t LaunchFillEnclosed(void* cells_dev, int cell_bytes, int unknown_is_filled, int64_t nx, int64_t ny, int64_t nz,
                              void* scratch_dev, hipStream_t stream);
// mask_dev[i] = 1 when cell i's occupancy class is selected by component_types (1 filled | 2 empty | 4 unknown) and the
// cell lies on a face of the grid or has a face neighbour with another label.
hipError_t LaunchComponentSurfaceMask(const float* occupancy_dev, const uint32_t* labels_dev, int64_t nx, int64_t ny,
                                      int64_t nz, int component_types, uint8_t* mask_dev, hipStream_t stream);

// block_counts[b] -> exclusive prefix sum in place, *total_dev = the sum (below 2^31): one workgroup, no waiting between
// workgroups.  The scan of the labelling's root counts, shared with the cell selection.
hipError_t LaunchScanBlocks(int32_t* block_counts_dev, int64_t blocks, uint32_t* total_dev, hipStream_t stream);

// --- launchers (select_kernels.hip): selected cells as compact ordered lists ---
// The rules and class bits of include/vgt_hip.h (VGT_HIP_SELECT_*, VGT_HIP_CLASS_*).
constexpr int kSelectAll = 0;
constexpr int kSelectSurface26 = 1;
constexpr int kSelectComponentSurface = 2;
constexpr int kSelectClassAbove = 1, kSelectClassBelow = 2, kSelectClassEqual = 4, kSelectClassUnordered = 8;
// cells_dev: records of cell_bytes bytes with the float value first (a plain float grid: 4).  labels_dev: one uint32
// every label_stride bytes (a plain label grid: 4; a member of the records: cell_bytes), kSelectComponentSurface only.
// Grids below 2^31 cells.
struct SelectGrid
{
  const void* cells_dev;
  int cell_bytes;
  const void* labels_dev;
  int label_stride;
  int nx, ny, nz;
  int rule, class_mask;
  float threshold;
};
// indices_dev receives the linear indices of the selected cells in ascending order; values_dev (or nullptr) their values;
// payload_dev (or nullptr) the uint32 found every payload_stride bytes from payload_source_dev, at the selected cells.
struct SelectOutput
{
  int32_t* indices_dev;
  float* values_dev;
  uint32_t* payload_dev;
  const void* payload_source_dev;
  int payload_stride;
  int64_t capacity;  // entries of each output: at least the number of selected cells
};
// Two steps, because the outputs are sized by what the first one counts:
//   LaunchSelectMark  the bit grid, its block counts and their scan into scratch_dev (SelectScratchBytes bytes: 1 bit per
//                     voxel + 4 bytes per 1024 voxels); the number of selected cells lies at SelectCountPtr afterwards
//                     (stream-ordered);
//   LaunchSelectEmit  the lists, from the scratch of a LaunchSelectMark of the same grid.
size_t SelectScratchBytes(int64_t num_cells);
const uint32_t* SelectCountPtr(const void* scratch_dev, int64_t num_cells);
hipError_t LaunchSelectMark(const SelectGrid& grid, void* scratch_dev, hipStream_t stream);
hipError_t LaunchSelectEmit(const SelectGrid& grid, const SelectOutput& out, const void* scratch_dev,
                            hipStream_t stream);

// --- launchers (surface_kernels.hip): the iso-surface of a field as an indexed triangle mesh ---
// The rules: include/vgt_hip.h, vgt_hip_extract_surface.  values_dev: one float every value_stride bytes (a plain float
// grid: 4; the occupancy of cell records: cell_bytes).  Grids below 2^31 cells.
struct SurfaceGrid
{
  const void* values_dev;
  int value_stride;
  int nx, ny, nz;
  float iso;
  int inside_above;
  double resolution;
  int has_transform;  // 0: the vertices stay in the grid frame
  double world_from_grid[16];
};
// vertices_dev: 3 doubles per vertex; vertex_cells_dev (or nullptr): the linear index of each vertex's cube;
// triangles_dev (or nullptr): 6 int32 per quad.
struct SurfaceOutput
{
  double* vertices_dev;
  int32_t* vertex_cells_dev;
  int32_t* triangles_dev;
};
// quads is exact; quads_scanned is the int32 scan's total, the one the quad offsets are good for: the two differ when
// the quads do not fit the scan (2^31 or more), which the caller must refuse before LaunchSurfaceEmit.
struct SurfaceCounts
{
  uint32_t vertices, quads_scanned;
  unsigned long long quads;
};
// Two steps, because the outputs are sized by what the first one counts:
//   LaunchSurfaceMark  the bit planes, the block counts and their scans into scratch_dev (SurfaceScratchBytes bytes:
//                      5 bits per voxel + 4 bytes per 64 voxels + 8 bytes per 1024 voxels); the counts lie at
//                      SurfaceCountsPtr afterwards (stream-ordered);
//   LaunchSurfaceEmit  the vertices, and the triangles when asked for, from the scratch of a LaunchSurfaceMark of the
//                      same grid (it adds the per-word vertex bases to the scratch).
size_t SurfaceScratchBytes(int64_t num_cells);
const SurfaceCounts* SurfaceCountsPtr(const void* scratch_dev, int64_t num_cells);
hipError_t LaunchSurfaceMark(const SurfaceGrid& grid, void* scratch_dev, hipStream_t stream);
hipError_t LaunchSurfaceEmit(const SurfaceGrid& grid, const SurfaceOutput& out, void* scratch_dev, hipStream_t stream);

// --- launchers (travel_kernels.hip): cost-to-go through free space, `toward`, path tracing ---
// The rules: include/vgt_hip.h, vgt_hip_travel_cost.  Grids below 2^31 cells.
// The tile a workgroup relaxes in LDS (Z fastest); DESIGN.md 4i says why these extents.
constexpr int kTravelTileX = 8, kTravelTileY = 8, kTravelTileZ = 16;
// What the passable bit plane is made from: float occupancy, a float SDF against a threshold, a uint8 filled mask.
constexpr int kTravelFromOccupancy = 0, kTravelFromSdf = 1, kTravelFromMask = 2;
constexpr uint8_t kTraceOk = 0, kTraceUnreached = 1, kTraceTruncated = 2, kTraceInvalid = 3;
struct TravelGrid
{
  int nx, ny, nz;
  uint32_t weights[3];
  uint32_t flags;
  uint32_t cost_limit;
};
// The head of the workspace.  active[r & 1]: some tile must run in round r; reached: cells with a cost, added up by
// LaunchTravelToward; tiles_run: tiles that ran, over all rounds (what a measurement divides by rounds * tiles).
struct TravelStatus
{
  uint32_t active[2];
  uint32_t rounds;  // stored by the host loop when it ends
  uint32_t reserved;
  unsigned long long reached;
  unsigned long long tiles_run;
};
struct TravelWorkspace
{
  size_t status_offset, flags_offset[2], words_offset, bytes;
  int64_t tiles;
};
TravelWorkspace CarveTravelWorkspace(int64_t nx, int64_t ny, int64_t nz);
// Zeroes the workspace's head, fills cost with UNREACHED, classifies `field_dev` (kTravelFrom...) into the bit plane and
// seeds the sources.  Then LaunchTravelRound for round = 0, 1, ... while TravelStatus::active[(round + 1) & 1], read
// after the round, is non-zero; then LaunchTravelToward (toward_dev may be null: it only counts the reached cells).
hipError_t LaunchTravelSeed(const void* field_dev, int source, int unknown_is_filled, double threshold,
                            const TravelGrid& grid, const int32_t* sources_dev, const uint32_t* source_costs_dev,
                            int64_t num_sources, uint32_t* cost_dev, void* workspace_dev, hipStream_t stream);
hipError_t LaunchTravelRound(const TravelGrid& grid, uint32_t* cost_dev, void* workspace_dev, int64_t round,
                             hipStream_t stream);
hipError_t LaunchTravelToward(const TravelGrid& grid, const int32_t* sources_dev, const uint32_t* source_costs_dev,
                              int64_t num_sources, const uint32_t* cost_dev, int32_t* toward_dev, void* workspace_dev,
                              hipStream_t stream);
hipError_t LaunchTracePaths(const int32_t* toward_dev, int64_t cells, const int32_t* starts_dev, int64_t num_starts,
                            int32_t max_cells, int32_t* paths_dev, int32_t* lengths_dev, uint8_t* status_dev,
                            hipStream_t stream);

// --- launchers (topology_kernels.hip): holes and voids per component ---
// One entry per label, the layout of vgt_hip_component_topology_t (include/vgt_hip.h).
struct ComponentTopologyEntry
{
  int32_t present, num_holes, num_voids, num_surfaces, m3, m5, m6, num_surface_vertices;
};
// cells_dev: records of cell_bytes bytes with the float occupancy first (a plain float grid: 4); labels_dev as
// LaunchLabelComponents writes them.  Labels outside 1..num_components count as "another component" and get no entry.
struct TopologyGrid
{
  const void* cells_dev;
  int cell_bytes;
  const uint32_t* labels_dev;
  int64_t nx, ny, nz;
  int component_types;  // 1 filled | 2 empty | 4 unknown
  uint32_t num_components;
};
inline int64_t TopologyVertices(int64_t nx, int64_t ny, int64_t nz) { return (nx + 1) * (ny + 1) * (nz + 1); }
// Two steps, because the node arrays are sized by what the first one counts (nodes = pairs of a lattice vertex and a
// selected component it lies on the surface of: a surface, not a volume):
//   LaunchTopologyCountNodes   vertex_scratch_dev: TopologyVertexScratchBytes bytes (4 per lattice vertex + 4 per 256 of
//                              them); afterwards the number of nodes (64 bits) lies at TopologyNodeCountPtr.
//   LaunchTopologyFromNodes    node_scratch_dev: TopologyNodeScratchBytes(num_nodes) bytes (16 per node), num_nodes
//                              below 2^31; table_dev: num_components + 1 entries, [0] zeroed.
// The lattice (nx + 1)(ny + 1)(nz + 1) must stay below 2^31 vertices.
size_t TopologyVertexScratchBytes(int64_t nx, int64_t ny, int64_t nz);
const unsigned long long* TopologyNodeCountPtr(const void* vertex_scratch_dev, int64_t nx, int64_t ny, int64_t nz);
size_t TopologyNodeScratchBytes(int64_t num_nodes);
hipError_t LaunchTopologyCountNodes(const TopologyGrid& grid, void* vertex_scratch_dev, hipStream_t stream);
hipError_t LaunchTopologyFromNodes(const TopologyGrid& grid, void* vertex_scratch_dev, int64_t num_nodes,
                                   void* node_scratch_dev, ComponentTopologyEntry* table_dev, hipStream_t stream);

// --- launcher (segment_kernels.hip): segments cast through an occupancy map or an SDF ---
// Modes, flags, statuses and outputs: include/vgt_hip.h, vgt_hip_cast_segments.  Grids of 1 to 2^31 - 1 cells.
constexpr int kSegmentOccupancy = 0;
constexpr int kSegmentSdfBelow = 1;
struct SegmentGrid
{
  double xform[16];  // grid_from_world, column-major; unused unless has_xform
  int has_xform;     // 0: the segments are in the grid frame and are used as they are
  double voxel_size, inverse_voxel_size;
  double grid_size[3];
  int32_t counts[3];
};
struct SegmentQuery
{
  int mode;
  int unknown_is_filled;
  double threshold;
  uint32_t flags;
};
// status_dev is required, every other output may be nullptr (min_value_dev / min_index_dev: kSegmentSdfBelow only).
struct SegmentOutputs
{
  uint8_t* status_dev;
  int32_t* hit_index_dev;
  double* hit_fraction_dev;
  int32_t* cells_examined_dev;
  float* min_value_dev;
  int32_t* min_index_dev;
};
hipError_t LaunchCastSegments(const float* field_dev, const SegmentGrid& grid, const SegmentQuery& query,
                              const double* segments_dev, int64_t num_segments, const SegmentOutputs& out,
                              hipStream_t stream);

// --- launcher (body_kernels.hip): sphere models checked against an SDF ---
// Inputs, outputs and statuses: include/vgt_hip.h, vgt_hip_check_spheres.  Grids of 0 to 2^31 - 1 cells, fewer than 2^31
// spheres, links and (configuration, sphere) pairs.  status_dev is required, every other output may be nullptr.
struct BodyOutputs
{
  uint8_t* status;
  double* min_clearance;
  int32_t* min_sphere;
  int32_t* num_below;
  int32_t* num_outside;
  double* min_gradient;
  double* sphere_clearance;
  double* sphere_gradient;
};
// The width of a configuration's lane segment: log2 of the least power of two >= min(num_spheres, 64).
int CheckSpheresWidthLog2(int64_t num_spheres);
// max_workgroups: 0 = the launcher's own limit (a testing build can make it small, so that few configurations already
// stride: vgt_hip_testing_set_check_spheres_workgroups).  The two transforms are host arrays (or nullptr).
hipError_t LaunchCheckSpheres(const float* sdf_dev, int64_t nx, int64_t ny, int64_t nz, double resolution,
                              const double* grid_from_world_host, const double* rotation_host,
                              const double* sphere_xyzr_dev, const int32_t* sphere_link_dev, int64_t num_spheres,
                              const double* link_poses_dev, int64_t num_links, int64_t num_configurations,
                              double minimum_clearance, int outside_is_collision, const BodyOutputs& out,
                              int max_workgroups, hipStream_t stream);

// --- launchers (body_volume_kernels.hip): sphere models into grids and onto point clouds ---
// Rules and outputs: include/vgt_hip.h, vgt_hip_rasterize_spheres / vgt_hip_spheres_cover_points.  The model as above.
struct SphereVolumeModel
{
  const double* xyzr;   // [S][4]
  const int32_t* link;  // [S]
  const double* poses;  // [B][L][16], column-major
  int num_spheres, num_links, num_configurations;
  double padding;
};
// Fills first_configuration_dev with -1 unless `keep`, then lowers it.  Grids of 0 to 2^31 - 1 cells, B * S < 2^31,
// 0 <= base <= 2^31 - 1 - B.  max_workgroups: 0 = the launcher's own limit
// (vgt_hip_testing_set_sphere_volume_workgroups).  grid_from_world_host: 16 doubles or nullptr.  counters_dev: nullptr, or
// (a testing build's counting run, vgt_hip_testing_set_sphere_volume_counters) three uint64 to which the launch adds the
// (cell, sphere) tests it made, those that covered, and the atomics it issued.
hipError_t LaunchRasterizeSpheres(int64_t nx, int64_t ny, int64_t nz, double resolution,
                                  const double* grid_from_world_host, const SphereVolumeModel& model, int64_t base,
                                  bool keep, int32_t* first_configuration_dev, int max_workgroups,
                                  unsigned long long* counters_dev, hipStream_t stream);
// Each output may be nullptr; filtered_xyz_dev may be points_xyz_dev.  world_from_points_host: 16 doubles or nullptr.
hipError_t LaunchCoverPoints(const float* points_xyz_dev, int64_t num_points, const double* world_from_points_host,
                             const SphereVolumeModel& model, int32_t* first_configuration_dev,
                             int32_t* first_sphere_dev, float* filtered_xyz_dev, int max_workgroups,
                             hipStream_t stream);

// --- launcher (align_kernels.hip): point clouds aligned to an SDF ---
// The definition, every output and the statuses: include/vgt_hip.h, vgt_hip_align_points.
struct AlignOptions
{
  int max_iterations, min_points;
  double damping, max_residual, target_distance, translation_tolerance, rotation_tolerance;
  double pivot[3];
};
struct AlignOutputs
{
  double* poses;
  uint8_t* status;
  int32_t *num_used, *num_outside, *num_rejected;
  double* sum_squared;
  int32_t* evaluations;
  double* normal_equations;
  double* last_step;
};
// 0 for sizes the launcher does not take: N or B outside [1, 2^31), B * ceil(N / 4096) >= 2^31.
size_t AlignWorkspaceBytes(int64_t num_points, int64_t num_poses);
// Enqueues the whole loop (1 + max_iterations evaluations, each followed by the solve) on `stream`.  out.status is
// required; out.poses may be poses_dev.  max_workgroups: 0 = the launcher's own limit for the evaluation
// (vgt_hip_testing_set_align_workgroups).  The two transforms are host arrays (or nullptr).
hipError_t LaunchAlignPoints(const float* sdf_dev, int64_t nx, int64_t ny, int64_t nz, double resolution,
                             const double* grid_from_world_host, const double* rotation_host,
                             const float* points_xyz_dev, int64_t num_points, const double* poses_dev,
                             int64_t num_poses, const AlignOptions& options, const AlignOutputs& out,
                             void* workspace_dev, int max_workgroups, hipStream_t stream);

// --- launchers (kinematics_kernels.hip): forward kinematics and the clearance gradient in joint space ---
// The definition of every output: include/vgt_hip.h, vgt_hip_forward_kinematics / vgt_hip_clearance_joint_gradient.
// One record per link, as the kernels read it (the host validates and packs the caller's arrays into these).
struct KinematicLink
{
  int32_t parent, joint_type, joint_index;
  int32_t keep_slot;    // the LDS slot the forward kinematics keeps this link's pose in, -1: none
  int32_t parent_slot;  // the parent's slot when the parent is not the link just before, -1: none
  int32_t reserved;
  double axis[3];
  double origin[12];  // the twelve used elements, column by column: origin[3 c + r]
};
constexpr int kJointFixed = 0, kJointRevolute = 1, kJointPrismatic = 2;
// The LDS budget of the forward kinematics: the poses of at most this many links, 96 B per lane and link, 6 KiB per
// link for a workgroup of one wave: 60 KiB.
constexpr int kKinematicsLdsLinks = 10;
// Fills keep_slot and parent_slot: a slot for every link that is the parent of a link other than the next one (a parent
// that is the link just before its child stays in registers), in link order, for the first kKinematicsLdsLinks of them.
// Returns the number of slots: 0 for a chain.
int AssignKinematicsLdsSlots(KinematicLink* links_host, int64_t num_links);
// Fewer than 2^31 links, configurations and (configuration, link) pairs.  world_from_base_host: 16 doubles or nullptr;
// limits_dev: [J][2] or nullptr; status_dev may be nullptr; lds_links: what AssignKinematicsLdsSlots returned.  max_workgroups: 0 = the launcher's own limit
// (vgt_hip_testing_set_kinematics_workgroups).
hipError_t LaunchForwardKinematics(const KinematicLink* links_dev, int64_t num_links, int64_t num_joints, int lds_links,
                                   const double* joint_values_dev, int64_t num_configurations,
                                   const double* world_from_base_host, const double* limits_dev, double* link_poses_dev,
                                   uint8_t* status_dev, int max_workgroups, hipStream_t stream);
// Exactly one of (min_sphere_dev, min_gradient_dev) and (sphere_weight_dev, sphere_gradient_dev) is given.
hipError_t LaunchClearanceJointGradient(const KinematicLink* links_dev, int64_t num_links, int64_t num_joints,
                                        const double* link_poses_dev, int64_t num_configurations,
                                        const double* sphere_xyzr_dev, const int32_t* sphere_link_dev,
                                        int64_t num_spheres, const int32_t* min_sphere_dev,
                                        const double* min_gradient_dev, const double* sphere_weight_dev,
                                        const double* sphere_gradient_dev, double* joint_gradient_dev,
                                        int max_workgroups, hipStream_t stream);

// --- launcher (ik_kernels.hip): tip poses to joint values ---
// The definition, every output and the statuses: include/vgt_hip.h, vgt_hip_solve_ik.
// The kernel keeps six doubles per lane and moving chain link in LDS: 3 KiB per link for a workgroup of one wave, 48 KiB
// at this many.
constexpr int kIkMaxChainJoints = 16;
struct IkOptions
{
  int max_iterations;
  double damping, max_step, position_tolerance, rotation_tolerance;
  double weights[6];
};
struct IkOutputs
{
  double* joints;  // [B][J]: the working rows, required when J > 0
  uint8_t* status;
  int32_t* iterations;
  double* error;
  double* tip_pose;
  uint8_t* fk_status;
};
// chain_dev: the chain's links, base first (each the parent of the next, the first on the base); moving_links: how many of
// them are not fixed, at most kIkMaxChainJoints, no two reading one column.  Problem b aims at targets_dev[b /
// seeds_per_target].  out.joints may be seeds_dev; every other output but out.status may be nullptr.  max_workgroups:
// 0 = the launcher's own limit (vgt_hip_testing_set_kinematics_workgroups).
hipError_t LaunchSolveIk(const KinematicLink* links_dev, int64_t num_joints, const int32_t* chain_dev, int chain_links,
                         int moving_links, const double* targets_dev, int64_t seeds_per_target, const double* seeds_dev,
                         int64_t num_problems, const double* world_from_base_host, const double* limits_dev,
                         const IkOptions& options, const IkOutputs& out, int max_workgroups, hipStream_t stream);

// --- launcher (motion_kernels.hip): motions between joint configurations checked against an SDF ---
// The definition of every output: include/vgt_hip.h, vgt_hip_check_motions.  status is required, every other output may
// be nullptr.
struct MotionOutputs
{
  uint8_t* status;
  int32_t* first_collision;
  double* min_clearance;
  int32_t* min_sample;
  int32_t* min_sphere;
  double* min_gradient;
  uint8_t* fk_status;
};
// The samples of a tile for a tree of so many links: a power of two T <= 64 with 96 * L * T <= 60 KiB -- the largest one
// within the build's VGT_MOTION_MAX_TILE and VGT_MOTION_TILE_BYTES (12 KiB of poses, where more than one sample fits them);
// 0: more links than the kernel takes (640), or none.
int MotionTileSamples(int64_t num_links);
// The dynamic LDS the poses of a tile may take (under the 64 KiB a launch gets without an attribute), what a link takes of
// it per sample, and so the most links of a tree: 640 (one sample per tile).
constexpr size_t kMotionPoseBudget = 60 * 1024, kMotionPoseBytesPerLink = 96;
constexpr int64_t kMotionMaxLinks = static_cast<int64_t>(kMotionPoseBudget / kMotionPoseBytesPerLink);
// What a launch for a tree of L links and a model of S spheres is made of: the tile (0: a tree MotionTileSamples does
// not take, and nothing else is set), the segment width, whether the sphere table sits in LDS behind the poses, and the
// dynamic LDS.  The launcher takes all of it from here (and so does vgt_hip_testing_motion_launch_geometry).
struct MotionLaunchGeometry
{
  int tile, log2_tile, log2_width, table_in_lds;
  size_t lds_bytes;
};
MotionLaunchGeometry SelectMotionGeometry(int64_t num_links, int64_t num_spheres);
// Grids of 0 to 2^31 - 1 cells; fewer than 2^31 spheres, motions and (motion, joint) pairs; a tree MotionTileSamples
// takes.  Field, model, joint arrays, num_steps (or nullptr: uniform_steps) and outputs on the device; the three
// transforms are host arrays (or nullptr); limits_dev: [J][2] or nullptr.  max_workgroups: 0 = the launcher's own limit
// (vgt_hip_testing_set_motion_workgroups).
hipError_t LaunchCheckMotions(const float* sdf_dev, int64_t nx, int64_t ny, int64_t nz, double resolution,
                              const double* grid_from_world_host, const double* rotation_host,
                              const double* sphere_xyzr_dev, const int32_t* sphere_link_dev, int64_t num_spheres,
                              const KinematicLink* links_dev, int64_t num_links, int64_t num_joints,
                              const double* joint_from_dev, const double* joint_to_dev, const int32_t* num_steps_dev,
                              int32_t uniform_steps, int64_t num_motions, const double* world_from_base_host,
                              const double* limits_dev, double minimum_clearance, int outside_is_collision,
                              int stop_at_collision, const MotionOutputs& out, int max_workgroups, hipStream_t stream);

// --- launcher (cost_kernels.hip): the obstacle cost of configurations given as joint values, and its joint gradient ---
// The definition of every output: include/vgt_hip.h, vgt_hip_clearance_cost.  cost is required, every other output may
// be nullptr.
struct CostOutputs
{
  double* cost;
  double* joint_gradient;
  int32_t* num_active;
  int32_t* num_outside;
  int32_t* num_without_gradient;
  uint8_t* fk_status;
};
// The configurations of a tile for a tree of so many links: a power of two T <= 64 with 96 * L * T <= 48 KiB -- the
// largest one within the build's VGT_COST_MAX_TILE and VGT_COST_TILE_BYTES (6 KiB of poses, where more than one
// configuration fits them); 0: more links than the kernel takes (512), or none.
int CostTileSamples(int64_t num_links);
// The dynamic LDS the poses of a tile may take, what a link takes of it per configuration, and so the most links of a
// tree: 512 (one configuration per tile).  Next to 48 KiB of poses the launch needs one pass of the buffer (64 entries of
// 68 B) and 20 B of resting sums: 53524 B of the 64 KiB a launch gets without an attribute.
constexpr size_t kCostPoseBudget = 48 * 1024, kCostPoseBytesPerLink = 96;
constexpr int64_t kCostMaxLinks = static_cast<int64_t>(kCostPoseBudget / kCostPoseBytesPerLink);
// What a launch for a tree of L links and a model of S spheres is made of, in the gradient form or the cost-only form:
// the tile (0: a tree CostTileSamples does not take, or a launch that does not fit, and nothing else is set), the
// segment width, the buffered passes, whether the sphere table and what the walk reads of the links sit in LDS, and the
// dynamic LDS.  The launcher takes all of it from here (and so does vgt_hip_testing_cost_launch_geometry).
struct CostLaunchGeometry
{
  int tile, log2_tile, log2_width, passes, table_in_lds, links_in_lds;
  size_t lds_bytes;
};
CostLaunchGeometry SelectCostGeometry(int64_t num_links, int64_t num_spheres, bool gradient);
// Grids of 0 to 2^31 - 1 cells; fewer than 2^31 spheres, configurations and (configuration, joint) pairs; a tree
// CostTileSamples takes.  Field, model, joint values and outputs on the device; the three transforms are host arrays (or
// nullptr); limits_dev: [J][2] or nullptr.  Without joint_gradient and num_without_gradient the cost-only kernel runs,
// which loads no gradient.  max_workgroups: 0 = the launcher's own limit (vgt_hip_testing_set_cost_workgroups).
hipError_t LaunchClearanceCost(const float* sdf_dev, int64_t nx, int64_t ny, int64_t nz, double resolution,
                               const double* grid_from_world_host, const double* rotation_host,
                               const double* sphere_xyzr_dev, const int32_t* sphere_link_dev, int64_t num_spheres,
                               const KinematicLink* links_dev, int64_t num_links, int64_t num_joints,
                               const double* joint_values_dev, int64_t num_configurations,
                               const double* world_from_base_host, const double* limits_dev, double margin,
                               const CostOutputs& out, int max_workgroups, hipStream_t stream);

// --- launcher (self_collision_kernels.hip): self-collision of a sphere model over a list of sphere pairs ---
// The definition of every output: include/vgt_hip.h, vgt_hip_check_self_collision.  status is required, every other
// output may be nullptr.
struct SelfCollisionOutputs
{
  uint8_t* status;
  int32_t* num_below;
  int32_t* num_without_value;
  double* min_clearance;
  int32_t* min_pair;
  double* min_direction;   // [B][3]
  double* joint_gradient;  // [B][J]; needs the tree's links
  uint8_t* fk_status;      // the joint-value form only
  double* pair_clearance;  // [B][P]
};
// What a launch may take of dynamic LDS (what it gets without an attribute), and what a link and a sphere take of it per
// configuration of a tile: the twelve used elements of a pose, the three of a centre.  Beside them a launch holds 8 B
// per sphere (the radii) and 256 B (min_pair).
constexpr size_t kSelfLdsLimit = 64 * 1024, kSelfPoseBytesPerLink = 96, kSelfCentreBytes = 24;
// The configurations of a tile for a tree of so many links carrying so many spheres: the largest power of two T <= 64
// whose poses and centres, (96 L + 24 S) T bytes, stay within the build's VGT_SELF_TILE_BYTES (16 KiB), 1 where two
// configurations exceed that; 0: no links, or one configuration does not fit the LDS of a launch
// (96 L + 32 S + 256 > 64 KiB).
int SelfCollisionTileSamples(int64_t num_links, int64_t num_spheres);
// Fewer than 2^31 spheres, pairs, configurations and (configuration, joint / link) pairs; a shape
// SelfCollisionTileSamples takes.  Model, pairs, joint values or link poses and outputs on the device.  Exactly one of
// joint_values_dev (with links_dev; world_from_base_host [16] or nullptr; limits_dev [J][2] or nullptr) and
// link_poses_dev ([B][L][16]; links_dev may be nullptr when out.joint_gradient is) is given -- for a tree without joints
// joint_values_dev is any address, never read, and link_poses_dev nullptr selects the form.  max_workgroups: 0 = the
// launcher's own limit (vgt_hip_testing_set_self_collision_workgroups).
hipError_t LaunchSelfCollision(const double* sphere_xyzr_dev, const int32_t* sphere_link_dev, int64_t num_spheres,
                               const int32_t* pairs_dev, int64_t num_pairs, const KinematicLink* links_dev,
                               int64_t num_links, int64_t num_joints, const double* joint_values_dev,
                               const double* link_poses_dev, int64_t num_configurations,
                               const double* world_from_base_host, const double* limits_dev, double minimum_clearance,
                               int no_value_is_collision, const SelfCollisionOutputs& out, int max_workgroups,
                               hipStream_t stream);

// --- launcher (motion_self_kernels.hip): motions checked against an SDF and against the robot itself in one walk ---
// The definition of every output: include/vgt_hip.h, vgt_hip_check_motions_with_self.  status is required, every other
// output may be nullptr.
struct MotionSelfOutputs
{
  uint8_t* status;
  int32_t* first_collision;
  uint8_t* collision_cause;
  double* min_clearance;
  int32_t* min_sample;
  int32_t* min_sphere;
  double* min_gradient;  // [E][3]
  double* self_min_clearance;
  int32_t* self_min_sample;
  int32_t* self_min_pair;
  uint8_t* fk_status;
};
// What a launch may take of dynamic LDS (what it gets without an attribute), and what a link and a sphere take of it per
// sample of a tile: the twelve used elements of a pose, the three of a centre.  Beside them a launch holds 8 B per sphere
// (the radii) and 1792 B (per slot of a tile the environment part's worst sphere, its clearance and cell, and the status).
constexpr size_t kMotionSelfLdsLimit = 64 * 1024, kMotionSelfPoseBytesPerLink = 96, kMotionSelfCentreBytes = 24,
                 kMotionSelfRecordBytes = 64 * 28;
// The samples of a tile for a tree of so many links carrying so many spheres: the largest power of two T <= 64 whose
// poses and centres, (96 L + 24 S) T bytes, stay within the build's VGT_MOTION_SELF_TILE_BYTES (16 KiB), 1 where two
// samples exceed that; 0: no links, or one sample does not fit the LDS of a launch (96 L + 32 S + 1792 > 64 KiB).
int MotionSelfTileSamples(int64_t num_links, int64_t num_spheres);
// As LaunchCheckMotions, with the pair list of LaunchSelfCollision (pairs_dev [P][2]; P == 0: no self part) and a field
// that may be nullptr (no environment part, the extents are not looked at); one of the two parts must be there.  A shape
// MotionSelfTileSamples takes.  max_workgroups: 0 = the launcher's own limit
// (vgt_hip_testing_set_motion_self_workgroups).
hipError_t LaunchCheckMotionsWithSelf(const float* sdf_dev, int64_t nx, int64_t ny, int64_t nz, double resolution,
                                      const double* grid_from_world_host, const double* rotation_host,
                                      const double* sphere_xyzr_dev, const int32_t* sphere_link_dev, int64_t num_spheres,
                                      const int32_t* pairs_dev, int64_t num_pairs, const KinematicLink* links_dev,
                                      int64_t num_links, int64_t num_joints, const double* joint_from_dev,
                                      const double* joint_to_dev, const int32_t* num_steps_dev, int32_t uniform_steps,
                                      int64_t num_motions, const double* world_from_base_host, const double* limits_dev,
                                      double minimum_clearance, double self_minimum_clearance, int outside_is_collision,
                                      int no_value_is_collision, int stop_at_collision, const MotionSelfOutputs& out,
                                      int max_workgroups, hipStream_t stream);

// --- launchers (voxelizer_kernels.hip) ---
struct RaycastGridF32
{
  float max_range;
  float xform[16];
  float voxel_size, inverse_voxel_size;
  float grid_size[3];
  int32_t counts[3];
};
struct RaycastGridF64
{
  double max_range;
  double xform[16];
  double voxel_size, inverse_voxel_size;
  double grid_size[3];
  int32_t counts[3];
};
// point_stride = floats between consecutive points (3 for packed xyz; PointCloud2: point_step / 4).
// scratch_dev (optional, RaycastScratchBytes(num_points) bytes): lets large clouds be ordered by ray
// direction and counted per workgroup in LDS (same counts, far fewer global atomics).
size_t RaycastScratchBytes(int64_t num_points);
hipError_t LaunchRaycastF32(const float* points_dev, int64_t num_points, int64_t point_stride,
                            const RaycastGridF32& g, int32_t* tracking_dev, int threads_per_block,
                            void* scratch_dev, size_t scratch_bytes, hipStream_t stream);
hipError_t LaunchRaycastF64(const double* points_dev, int64_t num_points, const RaycastGridF64& g,
                            int32_t* tracking_dev, int threads_per_block, void* scratch_dev, size_t scratch_bytes,
                            hipStream_t stream);
// dst[i] += src[i] over `count` int32 counts (both 16-byte aligned): sums the private tracking grids of a split cloud.
hipError_t LaunchAccumulateCounts(int32_t* dst_dev, const int32_t* src_dev, int64_t count, hipStream_t stream);
hipError_t LaunchFilter(const int32_t* tracking_dev, int64_t num_cells, int32_t num_grids,
                        double percent_seen_free, int32_t outlier_points_threshold,
                        int32_t num_cameras_seen_free, bool ratio_in_double, float* occupancy_dev,
                        int threads_per_block, hipStream_t stream);
}  // namespace vgt
