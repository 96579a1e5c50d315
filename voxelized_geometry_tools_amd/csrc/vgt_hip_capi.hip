// extern "C" surface of libvgt_hip.so (declared in include/vgt_hip.h): contexts, handles,
// host<->device staging and the sequencing of the kernels.  No kernel code here.
#include "../../include/vgt_hip.h"

#include "vgt_internal.hpp"
#include "nearest_internal.hpp"
#include "device_memory.hpp"
#include "host_staging.hpp"
#include "mesh_kernels.hpp"
#include "edt_crosscheck.hpp"
#include "host_pages.hpp"

#include <algorithm>
#include <cmath>
#include <limits>
#include <atomic>
#include <cstdio>
#include <cstring>
#include <functional>
#include <map>
#include <memory>
#include <mutex>
#include <vector>
#include <new>
#include <string>
#include <thread>
#ifdef __linux__
#include <sys/mman.h>
#endif
#include <vector>

// Host point clouds are uploaded and raycast on one of a few "upload lanes" (own stream + own staging
// buffer), so that concurrent RaycastPoints calls of the reference's parallel cloud dispatch
// (S/device_pointcloud_voxelization.cpp:147-149) overlap: cloud i+1's H2D copy runs beside cloud
// i's kernel, and kernels into different tracking grids run side by side.
struct UploadLane
{
  std::mutex mutex;
  hipStream_t stream = nullptr;
  hipEvent_t after_ctx = nullptr;  // orders the lane behind what the context's stream holds (grid zeroing)
  vgt::DeviceCache stage;
  // Page-locked host buffer the caller's cloud is copied to first: a 12-MB cloud from pageable memory goes through the
  // runtime's bounce buffers in 5 - 12 ms, page-locking the caller's buffer per call serialises in the driver when
  // several clouds arrive at once; a copy into a buffer that is locked once costs about a millisecond, in parallel
  // across the lanes, and the DMA 0.2 ms.
  void* pinned = nullptr;
  size_t pinned_bytes = 0;
};
constexpr int kUploadLanes = 4;

struct vgt_hip_ctx
{
  int device = -1;
  int threads_per_block = 256;
  int raycast_threads = 0;       // 0: the raycast kernels choose their own workgroup sizes (no HIP_THREADS_PER_BLOCK given)
  hipStream_t own_stream = nullptr;
  hipStream_t stream = nullptr;
  std::mutex mutex;              // serialises enqueues + the staging buffer
  UploadLane lanes[kUploadLanes];
  std::atomic<unsigned> next_lane{0};
  vgt::DeviceCache ray_scratch;  // sort scratch of raycasts of device-resident clouds (context stream)
  vgt::DeviceCache minmax_out;   // 2 floats (device) for host-facing SDF calls
  int variant = 0;               // 0: the default EDT pipeline; 1: the cross-check (vgt_hip_set_edt_variant, testing library)
  // deferred per-kernel timing (vgt_hip_timing_start / _stop): 8 events per SDF call
  std::vector<hipEvent_t> timing_events;
  std::vector<uint8_t> timing_kind;  // 1 = single-device call, 2 = slab begin + finish
  int timing_slots = 0;
  int timing_used = 0;
  // Device buffers of the host-pointer SDF entry points (input, field, workspace), kept across calls
  // and grown on demand: a caller that extracts fields repeatedly pays for hipMalloc / hipFree once.
  // vgt_hip_trim() gives them back.
  vgt::DeviceCache sdf_in, sdf_out, sdf_ws;
  // Scratch of the component labelling (union-find labels + scan counts), kept like the buffers above
  vgt::DeviceCache component_ws;
  // Scratch of the cell selection (bit grid + scan counts), kept likewise
  vgt::DeviceCache select_ws;
  // Scratch of the surface extraction (bit planes, vertex bases, scan counts), kept likewise
  vgt::DeviceCache surface_ws;
  // Scratch of the mesh rasterizer (triangle records, work-list offsets, totals and status), kept likewise
  vgt::DeviceCache mesh_ws;
  // Page-locked staging ring of the batched downloads (DownloadToHostArrays): kStagingSlots slots of kStagingSlotBytes,
  // allocated by the first such call, kept until vgt_hip_trim / vgt_hip_destroy; one event per slot.
  void* host_staging = nullptr;
  std::vector<hipEvent_t> staging_events;
  // Handles created from this context (grids, filter grids, cell grids) point back at it.  A
  // context destroyed while handles are alive releases its device resources at once but keeps this
  // struct until the last handle is gone, so handle destructors never touch freed memory.
  std::atomic<int> children{0};
  std::atomic<bool> destroyed{false};
  // Device buffers of destroyed tracking-grid / filter-grid handles, kept for the next handle of the same size (the
  // voxelizer allocates both per call, S/cuda_voxelization_helpers.cu:641-658,701-708; a hipMalloc + hipFree pair of
  // 128 MiB costs more than the raycast it serves).  Guarded by `mutex`; vgt_hip_trim and vgt_hip_destroy free them.
  std::vector<vgt::DeviceCache> pool;
  size_t pool_bytes = 0;
  bool pool_closed = false;  // set by vgt_hip_destroy: handles destroyed later free their buffers themselves
  // Z-slab calls: which slab a carries buffer was computed for (vgt_hip_sdf_slab_carries_dev decodes the gathered
  // summaries with the slab ranges of vgt_hip_sdf_slab_range; vgt_hip_sdf_slab_finish_dev refuses carries that were
  // made for another slab than the one it is given).  Guarded by `mutex`.
  struct SlabNote
  {
    int64_t z_offset, nz_local, nz_global;
  };
  std::map<const void*, SlabNote> slab_notes;
  // Copy streams and events of the pipelined host-pointer SDF extraction (SdfFromHostPipelined)
  hipStream_t copy_in = nullptr;
  hipStream_t copy_out = nullptr;
  std::vector<hipEvent_t> pipeline_events;
};

struct vgt_hip_grids
{
  vgt_hip_ctx* ctx = nullptr;
  int device = -1;
  vgt::DeviceCache dev;  // int32 counts
  int64_t num_cells = 0;
  int32_t num_grids = 0;
};

struct vgt_hip_filter
{
  vgt_hip_ctx* ctx = nullptr;
  int device = -1;
  vgt::DeviceCache dev;  // floats
  int64_t num_cells = 0;
  // vgt_hip_filter_grid_create_deferred: the upload runs on the context's copy stream; `uploaded` is recorded behind it
  // and the caller's array stays page-locked (`pin`, a ScopedHostPin) until a call has waited for the copy
  hipEvent_t uploaded = nullptr;
  bool upload_pending = false;
  void* pin = nullptr;
};

// A kinematic tree on the device (vgt_hip_kinematics_create): the validated link records and room for one call's joint
// limits.
struct vgt_hip_kinematics
{
  vgt_hip_ctx* ctx = nullptr;
  int device = -1;
  int64_t num_links = 0, num_joints = 0;
  int lds_links = 0;         // the LDS slots of the tree (vgt::AssignKinematicsLdsSlots)
  vgt::DeviceTemp links;     // [num_links] vgt::KinematicLink
  vgt::DeviceTemp limits;    // [num_joints][2] doubles: the joint_limits of the call being enqueued
  vgt::DeviceTemp chain;     // [num_links] int32: the chain of the vgt_hip_solve_ik call being enqueued, base first
  std::vector<vgt::KinematicLink> host_links;  // the records as uploaded: vgt_hip_solve_ik finds its chain here
};

// Device copy of a grid of cell records (occupancy + optional object id) and the buffers the
// per-object SDF extractions reuse.
struct vgt_hip_cells
{
  vgt_hip_ctx* ctx = nullptr;
  int device = -1;
  int64_t nx = 0, ny = 0, nz = 0;
  int cell_bytes = 0;
  int object_id_offset = -1;
  vgt::DeviceTemp records;      // [num_cells] records of cell_bytes bytes
  vgt::DeviceTemp mask;         // [num_cells] uint8 predicate result, the Z scan's input
  vgt::DeviceTemp sdf;          // [num_cells] floats
  vgt::DeviceCache sdf_named;   // [num_cells] floats, allocated by the first free-and-named extraction
  vgt::DeviceCache workspace;
  vgt::DeviceCache objects;     // uint32 object list of the current call
  vgt::DeviceTemp scalar;       // two uint32: result of a reduction + found flag
  // vgt_hip_cells_object_sdfs: masks, fields (+ extrema) and workspace of a batch of per-object extractions (grow-only)
  vgt::DeviceCache batch_masks, batch_sdf, batch_ws;
};

namespace
{
thread_local std::string g_last_error;
// What vgt_hip_testing_set_short_line_rows told the line passes (vgt::ShortLineOverride), -1 = nothing.  Only that hook
// stores to it, and only the testing library has the hook.
std::atomic<int> g_short_line_override{-1};
// What vgt_hip_testing_set_sweep_slots told the sweep launches (vgt::SweepSlotsOverride), 0 = nothing.
std::atomic<int> g_sweep_slots_override{0};
// What vgt_hip_testing_set_coarse_hull told the X pass: vgt::kXKernelByScene (the product's only mode), kXKernelCoarse or
// kXKernelPlain.  Only that hook stores to it.
std::atomic<int> g_coarse_hull_mode{vgt::kXKernelByScene};
// What vgt_hip_testing_set_check_spheres_workgroups told the sphere-model check, 0 = nothing (the launcher's own limit).
std::atomic<int> g_check_spheres_workgroups{0};
// The same from vgt_hip_testing_set_align_workgroups, for the evaluation launches of the cloud alignment.
std::atomic<int> g_align_workgroups{0};
// The same from vgt_hip_testing_set_kinematics_workgroups, for the forward kinematics and the joint gradient.
std::atomic<int> g_kinematics_workgroups{0};
// The same from vgt_hip_testing_set_motion_workgroups, for the motion check.
std::atomic<int> g_motion_workgroups{0};
// The same from vgt_hip_testing_set_cost_workgroups, for the clearance cost.
std::atomic<int> g_cost_workgroups{0};
// The same from vgt_hip_testing_set_self_collision_workgroups, for the self-collision check.
std::atomic<int> g_self_collision_workgroups{0};
// The same from vgt_hip_testing_set_motion_self_workgroups, for the motion check with the self part.
std::atomic<int> g_motion_self_workgroups{0};
// The same from vgt_hip_testing_set_sphere_volume_workgroups, for the sphere rasterizer and the point cover.
std::atomic<int> g_sphere_volume_workgroups{0};
// What vgt_hip_testing_set_sphere_volume_counters gave: three uint64 on the device that the sphere rasterizer adds its
// work counts to (a counting kernel), nullptr = nothing (the product's kernel).
std::atomic<unsigned long long*> g_sphere_volume_counters{nullptr};

int Fail(int code, const std::string& msg)
{
  g_last_error = msg;
  return code;
}

}  // namespace
namespace vgt
{
void SetLastError(const std::string& message) { g_last_error = message; }
hipStream_t ContextStream(const vgt_hip_ctx* ctx) { return ctx->stream; }
int ShortLineOverride() { return g_short_line_override.load(); }
int SweepSlotsOverride() { return g_sweep_slots_override.load(); }
}  // namespace vgt
namespace
{
int FailHip(const char* what, hipError_t err)
{
  g_last_error = std::string("[") + what + "] HIP error [" + hipGetErrorString(err) + "]";
  return VGT_HIP_ERR_RUNTIME;
}

// A handle is being created from / destroyed after its context (see vgt_hip_ctx::children).
void AdoptChild(vgt_hip_ctx* ctx) { ctx->children.fetch_add(1); }
// Waits for the work that may still use the handle's buffers, then drops the handle's reference.
void ReleaseChild(vgt_hip_ctx* ctx, int device)
{
  if (!ctx) return;
  (void)hipSetDevice(device);
  if (ctx->destroyed.load())
    (void)hipDeviceSynchronize();  // the context's stream is gone (vgt_hip_destroy drained it)
  else
    (void)hipStreamSynchronize(ctx->stream);
  if (ctx->children.fetch_sub(1) == 1 && ctx->destroyed.load()) delete ctx;
}

#define VGT_TRY_HIP(expr, what)                          \
  do                                                     \
  {                                                      \
    const hipError_t vgt_err_ = (expr);                  \
    if (vgt_err_ != hipSuccess) return FailHip(what, vgt_err_); \
  } while (0)

int HipResult(const char* what, hipError_t err) { return err == hipSuccess ? VGT_HIP_OK : FailHip(what, err); }

size_t AlignUp(size_t v, size_t a) { return (v + a - 1) / a * a; }

// Handle buffers come from / go back to the context's pool (at most kPoolLimit bytes are kept).
constexpr size_t kPoolLimit = size_t{4} << 30;
hipError_t PoolAllocate(vgt_hip_ctx* ctx, vgt::DeviceCache* buffer, size_t bytes)
{
  {
    std::lock_guard<std::mutex> lock(ctx->mutex);
    for (size_t i = 0; i < ctx->pool.size(); i++)
      if (ctx->pool[i].bytes() == bytes)
      {
        *buffer = std::move(ctx->pool[i]);
        ctx->pool_bytes -= bytes;
        ctx->pool.erase(ctx->pool.begin() + static_cast<std::ptrdiff_t>(i));
        return hipSuccess;
      }
  }
  return buffer->Reserve(bytes);
}
// (the caller has made sure no work uses the buffer any more)
void PoolRelease(vgt_hip_ctx* ctx, vgt::DeviceCache* buffer)
{
  if (!buffer->data()) return;
  if (ctx && !ctx->destroyed.load())
  {
    std::lock_guard<std::mutex> lock(ctx->mutex);
    if (!ctx->pool_closed && ctx->pool_bytes + buffer->bytes() <= kPoolLimit && ctx->pool.size() < 16)
    {
      ctx->pool_bytes += buffer->bytes();
      ctx->pool.push_back(std::move(*buffer));
      return;
    }
  }
  (void)buffer->Release();
}
void FreePool(vgt_hip_ctx* ctx)
{
  ctx->pool.clear();
  ctx->pool_bytes = 0;
}

// Keeps the first error of what was enqueued on `s`, and waits for the stream whatever happened: the buffers that the
// enqueued work uses are about to go.
hipError_t DrainKeepingFirst(hipStream_t s, hipError_t err)
{
  const hipError_t sync = hipStreamSynchronize(s);
  return err == hipSuccess ? sync : err;
}

// Waits for `launched` and for one small value that it left on the device; *value is on the caller's stack.
template <typename T>
hipError_t ReadBack(hipStream_t s, hipError_t launched, T* value, const void* value_dev)
{
  if (launched == hipSuccess) launched = hipMemcpyAsync(value, value_dev, sizeof(T), hipMemcpyDeviceToHost, s);
  return DrainKeepingFirst(s, launched);
}

// A cached buffer that is too small for `need` is regrown (to `grow_to` bytes where the caller wants headroom), once the
// work on `s` that may still use it is done.
int GrowCache(hipStream_t s, vgt::DeviceCache* cache, size_t need, const char* drain_what, const char* allocate_what,
              size_t grow_to = 0)
{
  if (need <= cache->bytes()) return VGT_HIP_OK;
  VGT_TRY_HIP(hipStreamSynchronize(s), drain_what);
  VGT_TRY_HIP(cache->Reserve(grow_to ? grow_to : need), allocate_what);
  return VGT_HIP_OK;
}

void FreeCachedSdfBuffers(vgt_hip_ctx* ctx)
{
  for (vgt::DeviceCache* b : {&ctx->sdf_in, &ctx->sdf_out, &ctx->sdf_ws, &ctx->ray_scratch, &ctx->component_ws,
                             &ctx->select_ws, &ctx->surface_ws, &ctx->mesh_ws})
    (void)b->Release();
  if (ctx->host_staging) (void)hipHostFree(ctx->host_staging);
  ctx->host_staging = nullptr;
  for (hipEvent_t e : ctx->staging_events)
    if (e) (void)hipEventDestroy(e);
  ctx->staging_events.clear();
}

// Page-locks a caller-owned host range for the duration of a call, unless it already is pinned
// (hipHostMalloc / hipHostRegister by the caller): copies from pageable memory go through the
// runtime's bounce buffers at a fraction of the PCIe rate and are not asynchronous.  Best effort:
// when the driver refuses (limits, odd mappings) the copy simply takes the pageable path.
// Two threads may hand the same array to two contexts at once: the registration is shared through a
// process-wide table of the ranges THIS library page-locked, with a use count, so the range stays locked until the
// last call that relies on it has finished.
class ScopedHostPin
{
public:
  ScopedHostPin(const void* ptr, size_t bytes)
  {
    if (!ptr || bytes < (size_t{1} << 20)) return;  // small copies: registration costs more than it saves
    std::lock_guard<std::mutex> lock(TableLock());
    auto& table = Table();
    auto found = table.find(ptr);
    if (found != table.end())
    {
      if (found->second.bytes >= bytes)
      {
        found->second.users++;
        shared_ = ptr;
      }
      return;  // (a larger request on a locked range: the copy takes whatever path the runtime picks)
    }
    hipPointerAttribute_t attr{};
    if (hipPointerGetAttributes(&attr, ptr) == hipSuccess && attr.type == hipMemoryTypeHost) return;  // the caller's pin
    (void)hipGetLastError();
    if (hipHostRegister(const_cast<void*>(ptr), bytes, hipHostRegisterDefault) == hipSuccess)
    {
      table[ptr] = Entry{bytes, 1};
      shared_ = ptr;
    }
    else
      (void)hipGetLastError();
  }
  ~ScopedHostPin()
  {
    if (!shared_) return;
    std::lock_guard<std::mutex> lock(TableLock());
    auto& table = Table();
    auto found = table.find(shared_);
    if (found != table.end() && --found->second.users == 0)
    {
      (void)hipHostUnregister(const_cast<void*>(shared_));
      table.erase(found);
    }
  }
  ScopedHostPin(const ScopedHostPin&) = delete;
  ScopedHostPin& operator=(const ScopedHostPin&) = delete;

private:
  struct Entry
  {
    size_t bytes;
    int users;
  };
  static std::mutex& TableLock()
  {
    static std::mutex lock;
    return lock;
  }
  static std::map<const void*, Entry>& Table()
  {
    static auto* table = new std::map<const void*, Entry>();
    return *table;
  }
  const void* shared_ = nullptr;
};

// The stage helpers from here to LaunchSlabFixup are the only code that knows two EDT pipelines exist: the default one
// and, in the testing library, the cross-check (edt_crosscheck.hpp; variant 1 of vgt_hip_set_edt_variant).  A carved
// workspace says which one it is for -- `records` or `t16` --, so the later stages ask the workspace, not the context.
// The product library links no cross-check: there the arms below are discarded and every workspace has records.
#ifdef VGT_HIP_TESTING
constexpr bool kHaveCrossCheck = true;
#else
constexpr bool kHaveCrossCheck = false;
#endif

struct SdfWorkspace
{
  vgt::ClassRecord* records;  // pass-1 result of the default pipeline ...
  int16_t* t16;               // ... or of the cross-check pipeline (one of the two, the other is null)
  int32_t* t32;
  uint32_t* minmax_enc;
  vgt::SweepScratch sweep_scratch;  // work counters, spilled stack entries and sign words of the line passes
  size_t bytes;
};

// (batch > 1: `batch` grids of nx x ny x nz one after the other -- records and the intermediate field of batch * nx
// slices, a pair of extrema per grid, the line passes' scratch for the batch's items; default pipeline only)
SdfWorkspace CarveWorkspace(void* base, int64_t nx, int64_t ny, int64_t nz, int variant, int64_t batch = 1)
{
  SdfWorkspace ws;
  const size_t n = static_cast<size_t>(batch * nx * ny * nz);
  size_t off = 0;
  ws.records = nullptr;
  ws.t16 = nullptr;
  if (kHaveCrossCheck && variant != 0)
  {
    ws.t16 = reinterpret_cast<int16_t*>(static_cast<char*>(base) + off);
    off = AlignUp(off + vgt::CrossCheckFieldBytes(batch * nx * ny * nz), 256);
  }
  else
  {
    ws.records = reinterpret_cast<vgt::ClassRecord*>(static_cast<char*>(base) + off);
    off = AlignUp(off + vgt::ClassRecordBytes(batch * nx, ny, nz), 256);
  }
  ws.t32 = reinterpret_cast<int32_t*>(static_cast<char*>(base) + off);
  off = AlignUp(off + n * sizeof(int32_t), 256);
  ws.minmax_enc = reinterpret_cast<uint32_t*>(static_cast<char*>(base) + off);
  off += AlignUp(static_cast<size_t>(batch) * 2 * sizeof(uint32_t), 256);
  ws.sweep_scratch.ptr = static_cast<char*>(base) + off;
  ws.sweep_scratch.bytes = vgt::SweepPassScratchBytes(nx, ny, nz, batch);
  off = AlignUp(off + ws.sweep_scratch.bytes, 256);
  ws.bytes = off;
  return ws;
}

// Pass 1 and the Y pass of `slices` X slices that start `first_slice` slices into the grid (the whole grid: 0, p.nx;
// `p` describes the part: p.nx = slices).  `summary`: per-line slab summaries of the part (multi-GPU) or null.
template <typename InT>
hipError_t LaunchPassOne(const InT* input_dev, const SdfWorkspace& ws, const vgt::SdfParams& part, int64_t first_slice,
                         vgt::SlabLineSummary* summary, hipStream_t s)
{
  const int64_t voxel_offset = first_slice * part.ny * part.nz;
  if constexpr (kHaveCrossCheck)
  {
    if (ws.t16)
    {
      if constexpr (std::is_same<InT, float>::value)
        return vgt::LaunchCrossCheckScanZFromOccupancy(input_dev + voxel_offset, ws.t16 + voxel_offset, part, summary, s);
      else
        return vgt::LaunchCrossCheckScanZFromMask(input_dev + voxel_offset, ws.t16 + voxel_offset, part, summary, s);
    }
  }
  vgt::ClassRecord* records = ws.records + first_slice * vgt::RecordWords(part.nz) * part.ny;
  if constexpr (std::is_same<InT, float>::value)
    return vgt::LaunchClassRecordsFromOccupancy(input_dev + voxel_offset, records, part, summary, s);
  else
    return vgt::LaunchClassRecordsFromMask(input_dev + voxel_offset, records, part, summary, s);
}
hipError_t LaunchPassTwo(const SdfWorkspace& ws, const vgt::SdfParams& part, int64_t first_slice, hipStream_t s)
{
  const int64_t voxel_offset = first_slice * part.ny * part.nz;
  if constexpr (kHaveCrossCheck)
  {
    if (ws.t16) return vgt::LaunchCrossCheckPassY(ws.t16 + voxel_offset, ws.t32 + voxel_offset, part, s);
  }
  return vgt::LaunchPassYSweepRecords(ws.records + first_slice * vgt::RecordWords(part.nz) * part.ny,
                                      ws.t32 + voxel_offset, ws.sweep_scratch, part, s);
}
// A whole single grid on the default pipeline: pass 1 counts the grid's one-class lines into the word next to the extrema
// and the X pass chooses its kernel by that count, on the device (edt_sweep_kernels.hip: plain or coarse hull; both are
// enqueued where the launch qualifies and one returns at once).  Every other caller keeps the plain kernel.
vgt::SdfParams WithKernelByScene(const SdfWorkspace& ws, vgt::SdfParams p)
{
  if (p.batch == 1 && ws.records)
  {
    p.one_class_lines = ws.minmax_enc + vgt::kOneClassWord;
    p.x_kernel = g_coarse_hull_mode.load();
  }
  return p;
}
// The X pass and the final conversion of the whole grid `p`, into sdf_dev and the workspace's extrema.
hipError_t LaunchPassThree(const SdfWorkspace& ws, const vgt::SdfParams& p, float* sdf_dev, hipStream_t s)
{
  if constexpr (kHaveCrossCheck)
  {
    if (ws.t16) return vgt::LaunchCrossCheckPassXFinalize(ws.t32, sdf_dev, ws.minmax_enc, p, s);
  }
  return vgt::LaunchPassXFinalize(ws.t32, sdf_dev, ws.minmax_enc, ws.sweep_scratch, p, s);
}
// Multi-GPU: folds the other slabs' carries into the pass-1 result of slab `p`.
hipError_t LaunchSlabFixup(const SdfWorkspace& ws, const vgt::SlabLineCarry* carries, const vgt::SdfParams& p, hipStream_t s)
{
  if constexpr (kHaveCrossCheck)
  {
    if (ws.t16) return vgt::LaunchCrossCheckSlabFixup(ws.t16, carries, p, s);
  }
  return vgt::LaunchSlabRecordFixup(ws.records, carries, p, s);
}

int CheckSdfShape(int64_t nx, int64_t ny, int64_t nz, double resolution)
{
  if (nx <= 0 || ny <= 0 || nz <= 0)
    return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "grid extents must be positive");
  if (nx > vgt::kMaxExtent || ny > vgt::kMaxExtent || nz > vgt::kMaxExtent)
    return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "grid extent exceeds 16384 voxels on an axis");
  if (!(resolution > 0.0) || !std::isfinite(resolution))
    return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "Grid must have uniform, positive resolution");
  return VGT_HIP_OK;
}

// The checks both projection entry points make before any device work.
int CheckProjectionArguments(int64_t nx, int64_t ny, int64_t nz, double resolution, double minimum_distance,
                             double stepsize_multiplier, int32_t max_iterations)
{
  const int rc = CheckSdfShape(nx, ny, nz, resolution);
  if (rc != VGT_HIP_OK) return rc;
  if (nx * ny * nz >= 0x7fffffffLL)
    return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "the projection out of collision supports grids below 2^31 cells");
  if (std::isnan(minimum_distance)) return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "minimum_distance must not be NaN");
  if (!(stepsize_multiplier > 0.0) || !std::isfinite(stepsize_multiplier))
    return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "stepsize_multiplier must be positive and finite");
  if (max_iterations < 0) return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "max_iterations must not be negative");
  return VGT_HIP_OK;
}

// The checks both segment entry points make before any device work; fills in what the kernel is launched with.
int CheckSegmentArguments(const vgt_hip_ctx* ctx, const float* field, int64_t nx, int64_t ny, int64_t nz,
                          double resolution, int32_t mode, int unknown_is_filled, double threshold, uint32_t flags,
                          const double* grid_from_world, const double* segments, int64_t num_segments,
                          const uint8_t* status, const float* min_value, const int32_t* min_index,
                          vgt::SegmentGrid* grid, vgt::SegmentQuery* query)
{
  if (!ctx || !field || !status || num_segments < 0 || (num_segments > 0 && !segments))
    return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "null argument");
  if (nx < 0 || ny < 0 || nz < 0) return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "grid extents must not be negative");
  if (!(resolution > 0.0) || !std::isfinite(resolution))
    return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "Grid must have uniform, positive resolution");
  // (extent by extent: the product of three int64 extents can overflow)
  const int64_t most = 0x7fffffffLL;
  if (nx > most || ny > most || nz > most || (nx > 0 && ny > 0 && nz > 0 && (nx * ny > most || nx * ny * nz > most)))
    return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "segment casts support grids below 2^31 cells");
  if (mode != VGT_HIP_SEGMENT_OCCUPANCY && mode != VGT_HIP_SEGMENT_SDF_BELOW)
    return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "unknown segment cast mode");
  if (flags & ~VGT_HIP_SEGMENT_WALK_THROUGH) return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "unknown segment cast flag");
  if (mode == VGT_HIP_SEGMENT_SDF_BELOW && std::isnan(threshold))
    return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "threshold must not be NaN");
  if (mode == VGT_HIP_SEGMENT_OCCUPANCY && (min_value || min_index))
    return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "min_value and min_index are outputs of the SDF mode");
  grid->has_xform = grid_from_world ? 1 : 0;
  for (int k = 0; k < 16; k++) grid->xform[k] = grid_from_world ? grid_from_world[k] : 0.0;
  grid->voxel_size = resolution;
  grid->inverse_voxel_size = 1.0 / resolution;
  const int64_t counts[3] = {nx, ny, nz};
  for (int a = 0; a < 3; a++)
  {
    grid->counts[a] = static_cast<int32_t>(counts[a]);
    grid->grid_size[a] = static_cast<double>(counts[a]) * resolution;
  }
  query->mode = mode == VGT_HIP_SEGMENT_OCCUPANCY ? vgt::kSegmentOccupancy : vgt::kSegmentSdfBelow;
  query->unknown_is_filled = unknown_is_filled ? 1 : 0;
  query->threshold = threshold;
  query->flags = flags;
  return VGT_HIP_OK;
}

// What both cloud-alignment entry points are called with, and the checks both make before any device work.
struct AlignPointsArguments
{
  const float* sdf;
  int64_t nx, ny, nz;
  double resolution;
  const double *grid_from_world, *rotation;
  const float* points;
  int64_t num_points;
  const double* poses;
  int64_t num_poses;
  const double* pivot;
  int32_t max_iterations, min_points;
  double damping, max_residual, target_distance, translation_tolerance, rotation_tolerance;
  vgt::AlignOutputs out;

  int64_t NumCells() const { return nx * ny * nz; }
  int Check(const vgt_hip_ctx* ctx) const
  {
    if (nx < 0 || ny < 0 || nz < 0 || num_points < 0 || num_poses < 0)
      return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "grid extents and the numbers of points and poses must not be negative");
    if (!ctx || !sdf || !points || !poses || !out.status) return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "null argument");
    if (nx == 0 || ny == 0 || nz == 0 || num_points == 0 || num_poses == 0)
      return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "cloud alignment needs a grid, a cloud and poses that are not empty");
    if (!(resolution > 0.0) || !std::isfinite(resolution))
      return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "Grid must have uniform, positive resolution");
    const int64_t most = 0x7fffffffLL;
    if (nx > most || ny > most || nz > most || nx * ny > most || nx * ny * nz > most)
      return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "cloud alignment supports grids below 2^31 cells");
    if (vgt::AlignWorkspaceBytes(num_points, num_poses) == 0)
      return Fail(VGT_HIP_ERR_INVALID_ARGUMENT,
                  "cloud alignment supports fewer than 2^31 points, poses and (pose, 4096-point block) pairs");
    if (max_iterations < 0 || max_iterations > 10000)
      return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "max_iterations must be in [0, 10000]");
    if (min_points < 6) return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "min_points must be at least 6");
    if (!(damping >= 0.0) || !std::isfinite(damping))
      return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "damping must be finite and not negative");
    if (!(max_residual > 0.0)) return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "max_residual must be positive (or +infinity)");
    if (!std::isfinite(target_distance)) return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "target_distance must be finite");
    if (!(translation_tolerance >= 0.0) || !(rotation_tolerance >= 0.0))
      return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "the tolerances must not be negative or NaN");
    if (pivot && !(std::isfinite(pivot[0]) && std::isfinite(pivot[1]) && std::isfinite(pivot[2])))
      return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "the pivot must be finite");
    return VGT_HIP_OK;
  }
  hipError_t Launch(const float* sdf_dev, const float* points_dev, const double* poses_dev,
                    const vgt::AlignOutputs& out_dev, void* workspace_dev, hipStream_t stream) const
  {
    const vgt::AlignOptions options{max_iterations,        min_points,         damping, max_residual, target_distance,
                                    translation_tolerance, rotation_tolerance,
                                    {pivot ? pivot[0] : 0.0, pivot ? pivot[1] : 0.0, pivot ? pivot[2] : 0.0}};
    return vgt::LaunchAlignPoints(sdf_dev, nx, ny, nz, resolution, grid_from_world, rotation, points_dev, num_points,
                                  poses_dev, num_poses, options, out_dev, workspace_dev, g_align_workgroups.load(),
                                  stream);
  }
};

// What both sphere-model entry points are called with, and the checks both make before any device work.
struct CheckSpheresArguments
{
  const float* sdf;
  int64_t nx, ny, nz;
  double resolution;
  const double *grid_from_world, *rotation;
  const double* sphere_xyzr;
  const int32_t* sphere_link;
  int64_t num_spheres;
  const double* link_poses;
  int64_t num_links, num_configurations;
  double minimum_clearance;
  uint32_t flags;
  vgt::BodyOutputs out;

  int64_t NumCells() const { return nx * ny * nz; }
  int Check(const vgt_hip_ctx* ctx) const
  {
    if (num_spheres < 0 || num_links < 0 || num_configurations < 0)
      return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "the numbers of spheres, links and configurations must not be negative");
    if (!ctx || !sdf || !out.status || (num_spheres > 0 && (!sphere_xyzr || !sphere_link)) ||
        (num_spheres > 0 && num_configurations > 0 && !link_poses))
      return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "null argument");
    if (nx < 0 || ny < 0 || nz < 0) return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "grid extents must not be negative");
    if (!(resolution > 0.0) || !std::isfinite(resolution))
      return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "Grid must have uniform, positive resolution");
    // (extent by extent: the product of three int64 extents can overflow)
    const int64_t most = 0x7fffffffLL;
    if (nx > most || ny > most || nz > most || (nx > 0 && ny > 0 && nz > 0 && (nx * ny > most || nx * ny * nz > most)))
      return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "sphere-model checks support grids below 2^31 cells");
    if (std::isnan(minimum_clearance)) return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "minimum_clearance must not be NaN");
    if (flags & ~VGT_HIP_SPHERES_OUTSIDE_IS_COLLISION)
      return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "unknown sphere-model check flag");
    if (num_links == 0 && num_spheres > 0)
      return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "a model with spheres needs at least one link (num_links == 0)");
    if (num_spheres > most || num_links > most || num_configurations > most ||
        num_configurations * num_spheres > most)
      return Fail(VGT_HIP_ERR_INVALID_ARGUMENT,
                  "sphere-model checks support fewer than 2^31 spheres, links and (configuration, sphere) pairs");
    return VGT_HIP_OK;
  }
  // The host form's own check: it can look at the model.
  int CheckModel() const
  {
    for (int64_t s = 0; s < num_spheres; s++)
    {
      const double radius = sphere_xyzr[4 * s + 3];
      if (sphere_link[s] < 0 || sphere_link[s] >= num_links)
        return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "sphere " + std::to_string(s) + ": link " +
                                                      std::to_string(sphere_link[s]) + " is not in [0, num_links)");
      if (!(radius >= 0.0))
        return Fail(VGT_HIP_ERR_INVALID_ARGUMENT,
                    "sphere " + std::to_string(s) + ": the radius must not be negative or NaN");
    }
    return VGT_HIP_OK;
  }
  hipError_t Launch(const float* sdf_dev, const double* xyzr_dev, const int32_t* link_dev, const double* poses_dev,
                    const vgt::BodyOutputs& out_dev, hipStream_t stream) const
  {
    return vgt::LaunchCheckSpheres(sdf_dev, nx, ny, nz, resolution, grid_from_world, rotation, xyzr_dev, link_dev,
                                   num_spheres, poses_dev, num_links, num_configurations, minimum_clearance,
                                   (flags & VGT_HIP_SPHERES_OUTSIDE_IS_COLLISION) ? 1 : 0, out_dev,
                                   g_check_spheres_workgroups.load(), stream);
  }
};

// What the four sphere-volume entry points share: the model, the poses and the padding, and the checks all of them make
// before any device work.
struct SphereVolumeArguments
{
  const double* sphere_xyzr;
  const int32_t* sphere_link;
  int64_t num_spheres;
  const double* link_poses;
  int64_t num_links, num_configurations;
  double padding;

  // (after the form's own null checks, so that "null" comes first as elsewhere)
  int CheckCounts() const
  {
    if (num_spheres < 0 || num_links < 0 || num_configurations < 0)
      return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "the numbers of spheres, links and configurations must not be negative");
    return VGT_HIP_OK;
  }
  bool MissingModel() const
  {
    return (num_spheres > 0 && (!sphere_xyzr || !sphere_link)) ||
           (num_spheres > 0 && num_configurations > 0 && !link_poses);
  }
  int Check() const
  {
    if (!std::isfinite(padding)) return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "padding must be finite");
    if (num_links == 0 && num_spheres > 0)
      return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "a model with spheres needs at least one link (num_links == 0)");
    const int64_t most = 0x7fffffffLL;
    if (num_spheres > most || num_links > most || num_configurations > most ||
        num_configurations * num_spheres > most)
      return Fail(VGT_HIP_ERR_INVALID_ARGUMENT,
                  "sphere volumes support fewer than 2^31 spheres, links and (configuration, sphere) pairs");
    return VGT_HIP_OK;
  }
  // The host forms' own check: they can look at the model.
  int CheckModel() const
  {
    for (int64_t s = 0; s < num_spheres; s++)
    {
      const double radius = sphere_xyzr[4 * s + 3];
      if (sphere_link[s] < 0 || sphere_link[s] >= num_links)
        return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "sphere " + std::to_string(s) + ": link " +
                                                      std::to_string(sphere_link[s]) + " is not in [0, num_links)");
      if (!(radius >= 0.0))
        return Fail(VGT_HIP_ERR_INVALID_ARGUMENT,
                    "sphere " + std::to_string(s) + ": the radius must not be negative or NaN");
    }
    return VGT_HIP_OK;
  }
  vgt::SphereVolumeModel Model(const double* xyzr_dev, const int32_t* link_dev, const double* poses_dev) const
  {
    return vgt::SphereVolumeModel{xyzr_dev,
                                  link_dev,
                                  poses_dev,
                                  static_cast<int>(num_spheres),
                                  static_cast<int>(num_links),
                                  static_cast<int>(num_configurations),
                                  padding};
  }
};

// The grid form's arguments and checks (both entry points).
struct RasterizeSpheresArguments
{
  int64_t nx, ny, nz;
  double resolution;
  const double* grid_from_world;
  SphereVolumeArguments body;
  int64_t base;
  uint32_t flags;
  int32_t* first_configuration;

  int64_t NumCells() const { return nx * ny * nz; }
  bool Keep() const { return (flags & VGT_HIP_SPHERES_KEEP) != 0; }
  int Check(const vgt_hip_ctx* ctx) const
  {
    int rc = body.CheckCounts();
    if (rc != VGT_HIP_OK) return rc;
    if (!ctx || !first_configuration || body.MissingModel()) return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "null argument");
    if (nx < 0 || ny < 0 || nz < 0) return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "grid extents must not be negative");
    if (!(resolution > 0.0) || !std::isfinite(resolution))
      return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "Grid must have uniform, positive resolution");
    // (extent by extent: the product of three int64 extents can overflow)
    const int64_t most = 0x7fffffffLL;
    if (nx > most || ny > most || nz > most || (nx > 0 && ny > 0 && nz > 0 && (nx * ny > most || nx * ny * nz > most)))
      return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "sphere volumes support grids below 2^31 cells");
    if (flags & ~VGT_HIP_SPHERES_KEEP) return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "unknown sphere-volume flag");
    rc = body.Check();
    if (rc != VGT_HIP_OK) return rc;
    if (base < 0 || base > most - body.num_configurations)
      return Fail(VGT_HIP_ERR_INVALID_ARGUMENT,
                  "first_configuration_base must not be negative, and base + configurations at most 2^31 - 1");
    return VGT_HIP_OK;
  }
  hipError_t Launch(const double* xyzr_dev, const int32_t* link_dev, const double* poses_dev, int32_t* first_dev,
                    hipStream_t stream) const
  {
    return vgt::LaunchRasterizeSpheres(nx, ny, nz, resolution, grid_from_world,
                                       body.Model(xyzr_dev, link_dev, poses_dev), base, Keep(), first_dev,
                                       g_sphere_volume_workgroups.load(), g_sphere_volume_counters.load(), stream);
  }
};

// The point form's arguments and checks (both entry points).
struct CoverPointsArguments
{
  const float* points;
  int64_t num_points;
  const double* world_from_points;
  SphereVolumeArguments body;
  uint32_t flags;
  int32_t *first_configuration, *first_sphere;
  float* filtered;

  int Check(const vgt_hip_ctx* ctx) const
  {
    int rc = body.CheckCounts();
    if (rc != VGT_HIP_OK) return rc;
    if (num_points < 0) return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "the number of points must not be negative");
    if (!ctx || (num_points > 0 && !points) || (!first_configuration && !first_sphere && !filtered) ||
        body.MissingModel())
      return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "null argument");
    if (num_points > 0x7fffffffLL) return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "sphere volumes support fewer than 2^31 points");
    if (flags) return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "unknown sphere-volume flag");
    return body.Check();
  }
  hipError_t Launch(const float* points_dev, const double* xyzr_dev, const int32_t* link_dev, const double* poses_dev,
                    int32_t* first_configuration_dev, int32_t* first_sphere_dev, float* filtered_dev,
                    hipStream_t stream) const
  {
    return vgt::LaunchCoverPoints(points_dev, num_points, world_from_points, body.Model(xyzr_dev, link_dev, poses_dev),
                                  first_configuration_dev, first_sphere_dev, filtered_dev,
                                  g_sphere_volume_workgroups.load(), stream);
  }
};

// Events of the current timing slot (nullptr when no session is active or it is full).
hipEvent_t* TimingSlot(vgt_hip_ctx* ctx)
{
  if (ctx->timing_slots == 0 || ctx->timing_used >= ctx->timing_slots) return nullptr;
  return &ctx->timing_events[static_cast<size_t>(ctx->timing_used) * 8];
}

// Enqueues the three passes.  events (optional) = 4 recorded events bracketing the kernels.
template <typename InT>
int RunSdfPipeline(vgt_hip_ctx* ctx, const InT* input_dev, const vgt::SdfParams& given, float* sdf_dev,
                   void* workspace_dev, size_t workspace_bytes, float* minmax_dev,
                   hipEvent_t* events)
{
  if (given.batch > 1 && ctx->variant != 0)
    return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "batches run on the default EDT pipeline only");
  const SdfWorkspace ws = CarveWorkspace(workspace_dev, given.nx, given.ny, given.nz, ctx->variant, given.batch);
  if (workspace_dev == nullptr || workspace_bytes < ws.bytes)
    return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "SDF workspace too small");
  hipStream_t s = ctx->stream;
  const vgt::SdfParams p = WithKernelByScene(ws, given);
  // A batch of grids (one after the other in every buffer) is ONE grid of batch * nx slices to pass 1 and to the Y
  // pass -- their lines never leave a slice -- and p.batch grids to the X pass, whose lines run along x.
  vgt::SdfParams slices = p;
  slices.nx = p.nx * p.batch;
  slices.batch = 1;
  VGT_TRY_HIP(vgt::LaunchInitMinMax(ws.minmax_enc, s, p.batch), "init min/max");
  if (events) VGT_TRY_HIP(hipEventRecord(events[0], s), "event record");
  VGT_TRY_HIP(LaunchPassOne<InT>(input_dev, ws, slices, 0, nullptr, s), "pass 1");
  if (events) VGT_TRY_HIP(hipEventRecord(events[1], s), "event record");
  VGT_TRY_HIP(LaunchPassTwo(ws, slices, 0, s), "Y pass");
  if (events) VGT_TRY_HIP(hipEventRecord(events[2], s), "event record");
  VGT_TRY_HIP(LaunchPassThree(ws, p, sdf_dev, s), "X pass");
  if (events) VGT_TRY_HIP(hipEventRecord(events[3], s), "event record");
  if (minmax_dev) VGT_TRY_HIP(vgt::LaunchDecodeMinMax(ws.minmax_enc, minmax_dev, s, p.batch), "min/max");
  return VGT_HIP_OK;
}

// Limits of a batch: the stacked grid's lines and voxels must stay inside what pass 1 and the sweeps index with.
int CheckBatch(int64_t batch, int64_t nx, int64_t ny, int64_t nz)
{
  if (batch <= 0) return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "batch must be positive");
  const int64_t zsegs = (nz + 63) / 64;
  if (batch > (int64_t{1} << 20) || batch * nx * ny >= (int64_t{1} << 28) || batch * nx * zsegs > 0x7fffffffLL ||
      batch * ny * zsegs > 0x7fffffffLL)
    return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "batch too large: batch * nx * ny must stay below 2^28 lines");
  return VGT_HIP_OK;
}

// Many device fields into many host arrays the caller has just allocated (the per-object fields of a tagged map, the
// fields of a batch of maps).  Page-locking such arrays costs more than the copy: their pages have never been touched,
// so the registration faults every one of them in, on one thread, and at the end they are unlocked again (32 fields of
// 128^3: 21 ms for 268 MB, a third of the link).  Instead the fields cross the link into a ring of page-locked slots
// that the context keeps, and a few host threads copy every slot's content on into the caller's arrays -- touching the
// arrays' pages in parallel -- while the next slot fills.  `fields`: device pointer and host pointer per array, `bytes`
// each.  The caller holds ctx->mutex; `s` has everything the fields depend on enqueued.
constexpr size_t kStagingSlotBytes = size_t{8} << 20;
constexpr int kStagingSlots = 4;
struct HostArrayCopy
{
  const void* device;
  void* host;
};
// The context's page-locked ring exists (allocated by the first call that wants it).
hipError_t EnsureStaging(vgt_hip_ctx* ctx)
{
  if (ctx->host_staging) return hipSuccess;
  const hipError_t err = hipHostMalloc(&ctx->host_staging, kStagingSlots * kStagingSlotBytes, hipHostMallocDefault);
  if (err != hipSuccess)
  {
    ctx->host_staging = nullptr;
    (void)hipGetLastError();
  }
  return err;
}
// One trip of the ring: a slot's worth of bytes that is either part of ONE array (arrays larger than a slot) or SEVERAL
// whole arrays whose device sides lie one behind the other (small arrays: one DMA and one hand-shake per slot instead of
// one per array -- 64 maps of 64^3 are 8 trips, not 64).
struct RingPiece
{
  size_t first, count;  // arrays [first, first + count)
  size_t offset;        // into the array (count == 1)
  size_t bytes;         // of the whole piece
};
std::vector<RingPiece> RingPieces(const std::vector<HostArrayCopy>& arrays, size_t bytes)
{
  std::vector<RingPiece> pieces;
  if (bytes >= kStagingSlotBytes)
  {
    for (size_t a = 0; a < arrays.size(); a++)
      for (size_t off = 0; off < bytes; off += kStagingSlotBytes)
        pieces.push_back(RingPiece{a, 1, off, std::min(kStagingSlotBytes, bytes - off)});
    return pieces;
  }
  const size_t per_slot = kStagingSlotBytes / bytes;
  for (size_t a = 0; a < arrays.size();)
  {
    size_t count = 1;
    while (count < per_slot && a + count < arrays.size() &&
           static_cast<const char*>(arrays[a + count].device) == static_cast<const char*>(arrays[a].device) + count * bytes)
      count++;
    pieces.push_back(RingPiece{a, count, 0, count * bytes});
    a += count;
  }
  return pieces;
}
// bytes [begin, end) of a piece between its slot and the caller's arrays
void CopyPieceRange(const std::vector<HostArrayCopy>& arrays, size_t bytes, const RingPiece& p, char* slot, size_t begin,
                    size_t end, bool to_host)
{
  while (begin < end)
  {
    const size_t k = p.count == 1 ? 0 : begin / bytes;              // array of the piece
    const size_t in_array = p.count == 1 ? p.offset + begin : begin - k * bytes;
    const size_t array_end = p.count == 1 ? end : std::min(end, (k + 1) * bytes);
    char* const host = static_cast<char*>(arrays[p.first + k].host) + in_array;
    if (to_host)
      std::memcpy(host, slot + begin, array_end - begin);
    else
      std::memcpy(slot + begin, host, array_end - begin);
    begin = array_end;
  }
}

// direction: true = device -> host arrays (the fields of a batch), false = host arrays -> device (its inputs)
hipError_t MoveThroughRing(vgt_hip_ctx* ctx, const std::vector<HostArrayCopy>& arrays, size_t bytes, hipStream_t s, bool to_host)
{
  if (arrays.empty() || bytes == 0) return hipSuccess;
  {
    const hipError_t err = EnsureStaging(ctx);
    if (err != hipSuccess) return err;
  }
  while (static_cast<int>(ctx->staging_events.size()) < kStagingSlots)
  {
    hipEvent_t e = nullptr;
    const hipError_t err = hipEventCreateWithFlags(&e, hipEventDisableTiming);
    if (err != hipSuccess) return err;
    ctx->staging_events.push_back(e);
  }
  const std::vector<RingPiece> pieces = RingPieces(arrays, bytes);
  const unsigned cap = to_host ? 16u : 8u;
  const int workers = static_cast<int>(std::max(1u, std::min(cap, std::thread::hardware_concurrency() / 2)));
#ifdef __linux__
  // (fresh arrays of several MiB: ask for huge pages where the kernel gives them on request -- 2 MiB per fault instead of
  // 4 KiB; a hint, any answer is fine)
  if (to_host && bytes >= (size_t{4} << 20))
    for (const HostArrayCopy& f : arrays)
    {
      const uintptr_t begin = (reinterpret_cast<uintptr_t>(f.host) + 4095) & ~uintptr_t{4095};
      const uintptr_t end = (reinterpret_cast<uintptr_t>(f.host) + bytes) & ~uintptr_t{4095};
      if (end > begin) (void)madvise(reinterpret_cast<void*>(begin), end - begin, MADV_HUGEPAGE);
    }
#endif
  // Download: dma[i] = the copy of piece i into its slot is ENQUEUED (its event recorded); host[i] = workers done with it.
  // Upload: host[i] = workers have filled the slot; dma[i] = its copy to the device is enqueued (event recorded).
  std::vector<std::atomic<int>> dma(pieces.size()), host(pieces.size());
  for (auto& a : dma) a.store(0);
  for (auto& c : host) c.store(0);
  std::atomic<int> failed{0};
  char* const staging = static_cast<char*>(ctx->host_staging);
  const int device = ctx->device;
  std::vector<std::thread> pool;
  for (int w = 0; w < workers; w++)
    pool.emplace_back([&, w]() {
      (void)hipSetDevice(device);
      for (size_t i = 0; i < pieces.size(); i++)
      {
        const int slot = static_cast<int>(i % kStagingSlots);
        // the DMA this piece's slot has to wait for: its own (download) or the one that emptied the slot (upload)
        const bool wait_for_dma = to_host || i >= static_cast<size_t>(kStagingSlots);
        if (wait_for_dma)
        {
          const size_t which = to_host ? i : i - kStagingSlots;
          while (dma[which].load(std::memory_order_acquire) == 0)
          {
            if (failed.load()) return;
            std::this_thread::yield();
          }
          if (hipEventSynchronize(ctx->staging_events[static_cast<size_t>(slot)]) != hipSuccess)
          {
            failed.store(1);
            return;
          }
        }
        const RingPiece& p = pieces[i];
        // (slices on page boundaries: two workers never fault the same page of a fresh array)
        const size_t pages = (p.bytes + 4095) / 4096;
        const size_t begin = std::min(p.bytes, pages * static_cast<size_t>(w) / workers * 4096);
        const size_t end = std::min(p.bytes, pages * static_cast<size_t>(w + 1) / workers * 4096);
        if (end > begin) CopyPieceRange(arrays, bytes, p, staging + static_cast<size_t>(slot) * kStagingSlotBytes, begin, end, to_host);
        host[i].fetch_add(1, std::memory_order_release);
      }
    });
  hipError_t err = hipSuccess;
  for (size_t i = 0; i < pieces.size() && err == hipSuccess; i++)
  {
    const int slot = static_cast<int>(i % kStagingSlots);
    // the host side this DMA has to wait for: the workers that emptied the slot (download) or filled it (upload)
    if (to_host ? i >= static_cast<size_t>(kStagingSlots) : true)
    {
      const size_t which = to_host ? i - kStagingSlots : i;
      while (host[which].load(std::memory_order_acquire) < workers && !failed.load()) std::this_thread::yield();
    }
    if (failed.load()) break;
    const RingPiece& p = pieces[i];
    char* const in_slot = staging + static_cast<size_t>(slot) * kStagingSlotBytes;
    char* const on_device = static_cast<char*>(const_cast<void*>(arrays[p.first].device)) + p.offset;
    err = to_host ? hipMemcpyAsync(in_slot, on_device, p.bytes, hipMemcpyDeviceToHost, s)
                  : hipMemcpyAsync(on_device, in_slot, p.bytes, hipMemcpyHostToDevice, s);
    if (err == hipSuccess) err = hipEventRecord(ctx->staging_events[static_cast<size_t>(slot)], s);
    if (err == hipSuccess) dma[i].store(1, std::memory_order_release);
  }
  if (err != hipSuccess) failed.store(1);
  for (auto& th : pool) th.join();
  if (to_host) err = DrainKeepingFirst(s, err);
  if (err == hipSuccess && failed.load()) err = hipErrorUnknown;
  return err;
}
// Many device fields into many host arrays (synchronises `s`) / many host arrays that hold data into device buffers (at
// return every copy is ENQUEUED on `s`; the ring is only reused by work enqueued on `s` later).  Page-locking a 1 MiB
// array for one copy costs ~0.15 ms (register + unregister) where the copy itself takes 0.02 -- 64 maps of 64^3 spent
// 10 ms there.
hipError_t DownloadToHostArrays(vgt_hip_ctx* ctx, const std::vector<HostArrayCopy>& fields, size_t bytes, hipStream_t s)
{
  return MoveThroughRing(ctx, fields, bytes, s, true);
}
hipError_t UploadFromHostArrays(vgt_hip_ctx* ctx, const std::vector<HostArrayCopy>& arrays, size_t bytes, hipStream_t s)
{
  return MoveThroughRing(ctx, arrays, bytes, s, false);
}

// The largest group of a batch that one launch can take: CheckBatch's limits (2^20 grids, 2^28 lines, 32-bit item counts)
// and `device_bytes` of buffers at `bytes_per_grid` each.  At least 1.
int64_t BatchGroup(int64_t batch, int64_t nx, int64_t ny, int64_t nz, size_t device_bytes, size_t bytes_per_grid)
{
  const int64_t zsegs = (nz + 63) / 64;
  int64_t group = batch;
  const int64_t limits[] = {int64_t{1} << 20, ((int64_t{1} << 28) - 1) / (nx * ny), 0x7fffffffLL / (nx * zsegs),
                            0x7fffffffLL / (ny * zsegs), static_cast<int64_t>(device_bytes / (bytes_per_grid + 1))};
  for (const int64_t limit : limits)
    if (group > limit) group = limit;
  return group < 1 ? 1 : group;
}

// Large grids through the host-pointer entry points: the three phases of a call -- upload, kernels, download --
// overlap.  The grid is uploaded in X chunks (contiguous) on a copy stream and every chunk is scanned along Z and
// swept along Y as soon as it has arrived; the X pass then runs over ranges of Y, and every finished range
// (nx pieces of ny_range * nz floats) goes back on a second copy stream while the next range is computed.  Only
// with the default pipeline (the cross-check's line passes need whole axes per launch).  The caller holds ctx->mutex.
constexpr int kPipelineChunks = 8;
std::atomic<int64_t> g_host_pipeline_min_voxels{int64_t{1} << 27};

template <typename InT>
bool CanPipelineFromHost(const vgt_hip_ctx* ctx, const vgt::SdfParams& p)
{
  // smallest grid that is pipelined: 2^27 voxels (testing builds: vgt_hip_testing_set_host_pipeline_min_voxels lowers
  // it so that small grids take this path, a negative value turns the pipeline off)
  const int64_t min_voxels = g_host_pipeline_min_voxels.load();
  if (min_voxels < 0 || ctx->variant != 0) return false;
  return p.nx >= 4 * kPipelineChunks && p.ny >= 4 * kPipelineChunks && p.nx * p.ny * p.nz >= min_voxels;
}

template <typename InT>
int SdfFromHostPipelined(vgt_hip_ctx* ctx, const InT* input_host, InT* in_dev, const vgt::SdfParams& p,
                         float* sdf_dev, float* sdf_host, const std::function<void()>& before_downloads)
{
  const SdfWorkspace ws = CarveWorkspace(ctx->sdf_ws.data(), p.nx, p.ny, p.nz, ctx->variant);
  if (ctx->sdf_ws.bytes() < ws.bytes) return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "SDF workspace too small");
  if (!ctx->copy_in) VGT_TRY_HIP(hipStreamCreateWithFlags(&ctx->copy_in, hipStreamNonBlocking), "create stream");
  if (!ctx->copy_out) VGT_TRY_HIP(hipStreamCreateWithFlags(&ctx->copy_out, hipStreamNonBlocking), "create stream");
  while (ctx->pipeline_events.size() < static_cast<size_t>(2 * kPipelineChunks + 1))
  {
    hipEvent_t e = nullptr;
    VGT_TRY_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming), "create event");
    ctx->pipeline_events.push_back(e);
  }
  hipEvent_t* const uploaded = ctx->pipeline_events.data();
  hipEvent_t* const computed = uploaded + kPipelineChunks;
  hipEvent_t const start = ctx->pipeline_events[2 * kPipelineChunks];
  hipStream_t s = ctx->stream;
  // the copy streams begin after whatever the context's stream still has to do with these buffers
  VGT_TRY_HIP(hipEventRecord(start, s), "event record");
  VGT_TRY_HIP(hipStreamWaitEvent(ctx->copy_in, start, 0), "order the upload stream");
  VGT_TRY_HIP(hipStreamWaitEvent(ctx->copy_out, start, 0), "order the download stream");
  const int64_t plane = p.ny * p.nz;
  auto x_begin = [&](int c) { return p.nx * c / kPipelineChunks; };
  auto y_begin = [&](int c) { return p.ny * c / kPipelineChunks; };
  for (int c = 0; c < kPipelineChunks; c++)
  {
    const int64_t off = x_begin(c) * plane, count = (x_begin(c + 1) - x_begin(c)) * plane;
    VGT_TRY_HIP(hipMemcpyAsync(in_dev + off, input_host + off, static_cast<size_t>(count) * sizeof(InT),
                               hipMemcpyHostToDevice, ctx->copy_in),
                "copy occupancy to device");
    VGT_TRY_HIP(hipEventRecord(uploaded[c], ctx->copy_in), "event record");
  }
  VGT_TRY_HIP(vgt::LaunchInitMinMax(ws.minmax_enc, s), "init min/max");
  for (int c = 0; c < kPipelineChunks; c++)
  {
    vgt::SdfParams part = p;
    part.nx = x_begin(c + 1) - x_begin(c);
    VGT_TRY_HIP(hipStreamWaitEvent(s, uploaded[c], 0), "wait for a chunk of the upload");
    VGT_TRY_HIP(LaunchPassOne<InT>(in_dev, ws, part, x_begin(c), nullptr, s), "pass 1");
    VGT_TRY_HIP(LaunchPassTwo(ws, part, x_begin(c), s), "Y pass");
  }
  // (everything up to here is enqueued and on its way: the moment to make the output array ready for the downloads)
  before_downloads();
  const size_t pitch = static_cast<size_t>(plane) * sizeof(float);
  for (int c = 0; c < kPipelineChunks; c++)
  {
    const int64_t y0 = y_begin(c), rows = y_begin(c + 1) - y0;
    VGT_TRY_HIP(vgt::LaunchPassXFinalizeRange(ws.t32, sdf_dev, ws.minmax_enc, ws.sweep_scratch, p, y0, rows, s),
                "X pass");
    VGT_TRY_HIP(hipEventRecord(computed[c], s), "event record");
    VGT_TRY_HIP(hipStreamWaitEvent(ctx->copy_out, computed[c], 0), "wait for a range of the field");
    VGT_TRY_HIP(hipMemcpy2DAsync(sdf_host + y0 * p.nz, pitch, sdf_dev + y0 * p.nz, pitch,
                                 static_cast<size_t>(rows * p.nz) * sizeof(float), static_cast<size_t>(p.nx),
                                 hipMemcpyDeviceToHost, ctx->copy_out),
                "copy SDF to host");
  }
  VGT_TRY_HIP(vgt::LaunchDecodeMinMax(ws.minmax_enc, ctx->minmax_out.as<float>(), s), "min/max");
  return VGT_HIP_OK;
}

template <typename InT>
int SdfFromHost(vgt_hip_ctx* ctx, const InT* input_host, const vgt::SdfParams& p, float* sdf_host,
                float* out_min, float* out_max)
{
  if (!ctx || !input_host || !sdf_host)
    return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "null argument");
  const int rc = CheckSdfShape(p.nx, p.ny, p.nz, p.resolution);
  if (rc != VGT_HIP_OK) return rc;
  VGT_TRY_HIP(hipSetDevice(ctx->device), "set device");
  const size_t nvox = static_cast<size_t>(p.nx * p.ny * p.nz);
  const size_t ws_bytes = CarveWorkspace(nullptr, p.nx, p.ny, p.nz, ctx->variant).bytes;
  // The output is usually an array the caller has just allocated: its pages are faulted in by a few threads while the
  // input is page-locked and uploaded, and it is page-locked only when the downloads are about to be enqueued.
  vgt::HostRangePopulator fresh_out(sdf_host, nvox * sizeof(float));
  const ScopedHostPin pin_in(input_host, nvox * sizeof(InT));
  std::unique_ptr<ScopedHostPin> pin_out;
  const auto lock_output = [&]() {
    fresh_out.Wait();
    if (!pin_out) pin_out.reset(new ScopedHostPin(sdf_host, nvox * sizeof(float)));
  };
  std::lock_guard<std::mutex> lock(ctx->mutex);
  hipError_t err = ctx->sdf_in.Reserve(nvox * sizeof(InT));
  if (err == hipSuccess) err = ctx->sdf_out.Reserve(nvox * sizeof(float));
  if (err == hipSuccess) err = ctx->sdf_ws.Reserve(ws_bytes);
  if (err != hipSuccess)
  {
    FreeCachedSdfBuffers(ctx);
    return FailHip("allocate SDF buffers", err);
  }
  InT* in_dev = ctx->sdf_in.as<InT>();
  float* sdf_dev = ctx->sdf_out.as<float>();
  float* const minmax_dev = ctx->minmax_out.as<float>();
  hipStream_t s = ctx->stream;
  int result = VGT_HIP_OK;
  if (CanPipelineFromHost<InT>(ctx, p))
  {
    if (!minmax_dev) return Fail(VGT_HIP_ERR_RUNTIME, "context has no extrema buffer");
    result = SdfFromHostPipelined<InT>(ctx, input_host, in_dev, p, sdf_dev, sdf_host, lock_output);
    float mm[2] = {0.0f, 0.0f};
    if (result == VGT_HIP_OK)
    {
      err = hipMemcpyAsync(mm, minmax_dev, sizeof(mm), hipMemcpyDeviceToHost, s);
      if (err != hipSuccess) result = FailHip("copy extrema to host", err);
    }
    // drain all three streams whatever happened: the caller's arrays are about to be unpinned
    const hipError_t e1 = hipStreamSynchronize(ctx->copy_in);
    const hipError_t e2 = hipStreamSynchronize(s);
    const hipError_t e3 = hipStreamSynchronize(ctx->copy_out);
    if (result == VGT_HIP_OK && (e1 != hipSuccess || e2 != hipSuccess || e3 != hipSuccess))
      result = FailHip("pipelined SDF extraction", e1 != hipSuccess ? e1 : (e2 != hipSuccess ? e2 : e3));
    if (result == VGT_HIP_OK)
    {
      if (out_min) *out_min = mm[0];
      if (out_max) *out_max = mm[1];
    }
    return result;
  }
  // Small maps (the sizes of the reference's own examples and tests; up to 512 KiB) never cross the link as copies: the map
  // is copied into a page-locked slot of the context's ring and the kernels work ON the ring -- pass 1 reads the map from
  // host memory, the X pass writes the field to it, the extrema behind the field -- so a call is one memcpy in, five
  // dispatches, one wait, one memcpy out.  No DMA dispatch in either direction, no pageable copy that the runtime would
  // stage itself, no third copy for two floats: 40^3 0.115 ms per blocking call in round 5, 0.078 - 0.085 with a DMA each
  // way between the ring and the device buffers, 0.060 - 0.072 now; 16^3 0.066 / 0.048 / 0.037
  // (profiles/r6/experiments.md).  A kernel reads host memory slowly, so not beyond 512 KiB (1 MiB: 0.37 ms against
  // 0.13 - 0.36 with page-locked arrays, which is what larger maps get below).
  const size_t in_bytes = nvox * sizeof(InT), out_bytes = nvox * sizeof(float);
  if (in_bytes <= (size_t{1} << 19) && out_bytes + 2 * sizeof(float) <= kStagingSlotBytes && EnsureStaging(ctx) == hipSuccess)
  {
    char* const up = static_cast<char*>(ctx->host_staging);
    char* const down = up + kStagingSlotBytes;
    std::memcpy(up, input_host, in_bytes);
    float* const field = reinterpret_cast<float*>(down);
    result = RunSdfPipeline<InT>(ctx, reinterpret_cast<const InT*>(up), p, field, ctx->sdf_ws.data(),
                                 ctx->sdf_ws.bytes(), field + nvox, nullptr);
    err = hipStreamSynchronize(s);  // (whatever happened: the ring is reused by the next call)
    if (result == VGT_HIP_OK && err != hipSuccess) result = FailHip("small-map SDF extraction", err);
    if (result == VGT_HIP_OK)
    {
      std::memcpy(sdf_host, down, out_bytes);
      float mm[2];
      std::memcpy(mm, down + out_bytes, sizeof(mm));
      if (out_min) *out_min = mm[0];
      if (out_max) *out_max = mm[1];
    }
    return result;
  }
  err = hipMemcpyAsync(in_dev, input_host, nvox * sizeof(InT), hipMemcpyHostToDevice, s);
  if (err != hipSuccess)
    result = FailHip("copy occupancy to device", err);
  else
    result = RunSdfPipeline<InT>(ctx, in_dev, p, sdf_dev, ctx->sdf_ws.data(), ctx->sdf_ws.bytes(), minmax_dev, nullptr);
  if (result == VGT_HIP_OK)
  {
    float mm[2] = {0.0f, 0.0f};
    lock_output();  // (upload and kernels are on their way)
    err = hipMemcpyAsync(sdf_host, sdf_dev, nvox * sizeof(float), hipMemcpyDeviceToHost, s);
    if (err == hipSuccess) err = hipMemcpyAsync(mm, minmax_dev, sizeof(mm), hipMemcpyDeviceToHost, s);
    if (err == hipSuccess) err = hipStreamSynchronize(s);
    if (err != hipSuccess)
      result = FailHip("copy SDF to host", err);
    else
    {
      if (out_min) *out_min = mm[0];
      if (out_max) *out_max = mm[1];
    }
  }
  else
    (void)hipStreamSynchronize(s);
  return result;
}

int CheckRaycastArgs(const vgt_hip_ctx* ctx, const vgt_hip_grids* grids, size_t grid_index,
                     const void* points, int64_t num_points, const void* xform, int32_t nx,
                     int32_t ny, int32_t nz)
{
  if (!ctx || !grids || !xform) return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "null argument");
  if (grids->ctx != ctx)
    return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "tracking grids belong to another context");
  if (grid_index >= static_cast<size_t>(grids->num_grids))
    return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "tracking grid index out of range");
  if (num_points < 0 || (num_points > 0 && !points))
    return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "invalid point buffer");
  if (nx <= 0 || ny <= 0 || nz <= 0 ||
      static_cast<int64_t>(nx) * ny * nz != grids->num_cells)
    return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "voxel counts do not match the tracking grids");
  return VGT_HIP_OK;
}

// Releases the upload lanes' device resources (the caller has made sure nothing runs on them).
void FreeUploadLanes(vgt_hip_ctx* ctx, bool destroy_streams)
{
  for (UploadLane& lane : ctx->lanes)
  {
    std::lock_guard<std::mutex> lock(lane.mutex);
    if (lane.stream) (void)hipStreamSynchronize(lane.stream);
    (void)lane.stage.Release();
    if (lane.pinned) (void)hipHostFree(lane.pinned);
    lane.pinned = nullptr;
    lane.pinned_bytes = 0;
    if (destroy_streams)
    {
      if (lane.after_ctx) (void)hipEventDestroy(lane.after_ctx);
      if (lane.stream) (void)hipStreamDestroy(lane.stream);
      lane.after_ctx = nullptr;
      lane.stream = nullptr;
    }
  }
}

// Uploads `bytes` from host memory on a free upload lane, runs `launch(device_copy, lane_stream)` behind the
// copy and waits for it: the host buffer may be released by the caller as soon as this returns
// (S/cuda_voxelization_helpers.cu:676-699 frees its device copy at scope exit).  Calls on different lanes
// overlap; work queued on the context's stream before the call (the zeroing of new tracking grids) is
// ordered before the lane's work by an event, work queued after it follows the return of this call.
template <typename Launch>
int UploadAndRun(vgt_hip_ctx* ctx, const void* host, size_t bytes, size_t scratch_bytes, Launch launch)
{
  // the first idle lane (a caller that raycasts one cloud after the other keeps using lane 0, whose stream and staging
  // buffer exist; concurrent callers spread over the lanes), or, when all are busy, the next one in turn
  UploadLane* chosen = nullptr;
  std::unique_lock<std::mutex> lane_lock;
  for (int i = 0; i < kUploadLanes && !chosen; i++)
  {
    std::unique_lock<std::mutex> attempt(ctx->lanes[i].mutex, std::try_to_lock);
    if (attempt.owns_lock())
    {
      chosen = &ctx->lanes[i];
      lane_lock = std::move(attempt);
    }
  }
  if (!chosen)
  {
    chosen = &ctx->lanes[ctx->next_lane.fetch_add(1) % kUploadLanes];
    lane_lock = std::unique_lock<std::mutex>(chosen->mutex);
  }
  UploadLane& lane = *chosen;
  if (!lane.stream)
  {
    VGT_TRY_HIP(hipStreamCreateWithFlags(&lane.stream, hipStreamNonBlocking), "create upload stream");
    VGT_TRY_HIP(hipEventCreateWithFlags(&lane.after_ctx, hipEventDisableTiming), "create upload event");
  }
  // staging copy of the cloud, followed by the kernel's scratch (256-byte aligned)
  const size_t scratch_at = AlignUp(bytes, 256);
  const size_t total = scratch_at + scratch_bytes;
  const int grown = GrowCache(lane.stream, &lane.stage, total, "drain before regrowing staging buffer",
                              "allocate staging buffer", AlignUp(total + total / 4, 1 << 20));
  if (grown != VGT_HIP_OK) return grown;
  char* const stage = lane.stage.as<char>();
  {
    std::lock_guard<std::mutex> lock(ctx->mutex);
    VGT_TRY_HIP(hipEventRecord(lane.after_ctx, ctx->stream), "record event");
  }
  VGT_TRY_HIP(hipStreamWaitEvent(lane.stream, lane.after_ctx, 0), "order upload lane");
  const void* source = host;
  {
    hipPointerAttribute_t attr{};
    const bool caller_locked = hipPointerGetAttributes(&attr, host) == hipSuccess && attr.type == hipMemoryTypeHost;
    (void)hipGetLastError();
    if (!caller_locked && bytes >= (size_t{1} << 16))
    {
      if (lane.pinned_bytes < bytes)
      {
        if (lane.pinned) (void)hipHostFree(lane.pinned);
        lane.pinned = nullptr;
        lane.pinned_bytes = 0;
        const size_t want = AlignUp(bytes + bytes / 4, 1 << 20);
        if (hipHostMalloc(&lane.pinned, want, hipHostMallocDefault) == hipSuccess)
          lane.pinned_bytes = want;
        else
          (void)hipGetLastError();  // (no page-locked memory to be had: the copy takes the pageable path)
      }
      if (lane.pinned_bytes >= bytes)
      {
        // (the previous use of the buffer was waited for at the end of its call)  Piece by piece, so that the DMA of one
        // piece runs while the host copies the next: a 12 MB cloud is 0.4 ms of memcpy and 0.2 ms of DMA -- 0.45 ms this
        // way instead of 0.6.
        constexpr size_t kPiece = size_t{2} << 20;
        for (size_t off = 0; off < bytes; off += kPiece)
        {
          const size_t piece = std::min(kPiece, bytes - off);
          std::memcpy(static_cast<char*>(lane.pinned) + off, static_cast<const char*>(host) + off, piece);
          VGT_TRY_HIP(hipMemcpyAsync(stage + off, static_cast<char*>(lane.pinned) + off, piece,
                                     hipMemcpyHostToDevice, lane.stream),
                      "Failed to copy points to the device");
        }
        source = nullptr;  // (uploaded)
      }
    }
  }
  if (source)
    VGT_TRY_HIP(hipMemcpyAsync(stage, source, bytes, hipMemcpyHostToDevice, lane.stream),
                "Failed to copy points to the device");
  VGT_TRY_HIP(launch(stage, stage + scratch_at, lane.stream),
              "Failed to dispatch raycast kernel");
  VGT_TRY_HIP(hipStreamSynchronize(lane.stream), "raycast");
  return VGT_HIP_OK;
}
// Shared body of the batched SDF queries: `run(sdf_dev, queries_dev, out_dev, has_dev, flag_dev)` enqueues the
// kernel.  Host variant: uploads field and queries, downloads the results.  out_doubles = doubles per query.
template <typename Run>
int SdfQueriesHost(vgt_hip_ctx* ctx, const float* sdf_host, int64_t nx, int64_t ny, int64_t nz, double resolution,
                   const double* query_xyz_host, int64_t num_queries, int out_doubles, double* out_host,
                   uint8_t* has_value_host, const char* what, Run run)
{
  if (!ctx || !sdf_host || !out_host || num_queries < 0 || (num_queries > 0 && !query_xyz_host))
    return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "null argument");
  const int rc = CheckSdfShape(nx, ny, nz, resolution);
  if (rc != VGT_HIP_OK) return rc;
  if (num_queries == 0) return VGT_HIP_OK;
  VGT_TRY_HIP(hipSetDevice(ctx->device), "set device");
  const size_t n = static_cast<size_t>(nx * ny * nz), q = static_cast<size_t>(num_queries);
  vgt::HostStaging staging;
  const auto sdf = staging.In(sdf_host, n);
  const auto queries = staging.In(query_xyz_host, q * 3);
  const auto out = staging.Out(out_host, q * out_doubles);
  const auto has = staging.Out(has_value_host, q);
  const auto flag_word = staging.Scratch<uint32_t>(256);
  uint32_t flag = 0;
  const int result = staging.Run(*ctx, what, FailHip, [&](hipStream_t s) {
    VGT_TRY_HIP(hipMemsetAsync(flag_word.dev(), 0, sizeof(uint32_t), s), what);
    VGT_TRY_HIP(run(sdf.dev(), queries.dev(), out.dev(), has.dev(), flag_word.dev(), s), what);
    return HipResult(what, hipMemcpyAsync(&flag, flag_word.dev(), sizeof(flag), hipMemcpyDeviceToHost, s));
  });
  if (result != VGT_HIP_OK) return result;
  if (flag) return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "Window size for fine gradient is too large for SDF");
  return VGT_HIP_OK;
}
}  // namespace

// --- nearest cell of the other class: what the entry points share (templates: outside the C linkage block) ---
namespace
{
// The limits of the nearest-cell transform: the SDF's extent per axis and fewer than 2^31 cells.
bool NearestShapeWithinLimits(int64_t nx, int64_t ny, int64_t nz)
{
  if (nx <= 0 || ny <= 0 || nz <= 0 || nx > vgt::kMaxExtent || ny > vgt::kMaxExtent || nz > vgt::kMaxExtent) return false;
  return nx * ny * nz <= 0x7fffffffLL;  // (each extent is at most 2^14: the product cannot overflow)
}

int CheckNearestShape(int64_t nx, int64_t ny, int64_t nz)
{
  if (nx <= 0 || ny <= 0 || nz <= 0) return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "grid extents must be positive");
  if (nx > vgt::kMaxExtent || ny > vgt::kMaxExtent || nz > vgt::kMaxExtent)
    return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "grid extent exceeds 16384 voxels on an axis");
  if (!NearestShapeWithinLimits(nx, ny, nz))
    return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "the nearest-cell transform supports grids below 2^31 cells");
  return VGT_HIP_OK;
}

vgt::NearestGrid MakeNearestGrid(int64_t nx, int64_t ny, int64_t nz, int unknown_is_filled)
{
  return vgt::NearestGrid{static_cast<int32_t>(nx), static_cast<int32_t>(ny), static_cast<int32_t>(nz),
                          unknown_is_filled ? 1 : 0};
}

// Upload, the three passes, download: the blocking form of both host-pointer entry points.
template <typename InT>
int NearestFromHost(vgt_hip_ctx* ctx, const InT* input_host, int64_t nx, int64_t ny, int64_t nz, int unknown_is_filled,
                    int32_t* nearest_host, int32_t* d2_host)
{
  if (!ctx || !input_host || !nearest_host) return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "null argument");
  const int rc = CheckNearestShape(nx, ny, nz);
  if (rc != VGT_HIP_OK) return rc;
  VGT_TRY_HIP(hipSetDevice(ctx->device), "set device");
  const char* what = "nearest cells";
  const size_t n = static_cast<size_t>(nx * ny * nz);
  vgt::HostStaging staging;
  const auto input = staging.In(input_host, n);
  const auto nearest = staging.Out(nearest_host, n);
  const auto d2 = staging.Out(d2_host, n);
  const auto workspace = staging.Scratch(vgt::CarveNearestWorkspace(nx, ny, nz).bytes);
  return staging.Run(*ctx, what, FailHip, [&](hipStream_t s) {
    return HipResult(what, vgt::LaunchNearest<InT>(input.dev(), MakeNearestGrid(nx, ny, nz, unknown_is_filled),
                                                   nearest.dev(), d2.dev(), workspace.dev(), s));
  });
}
}  // namespace

extern "C" {

int vgt_hip_abi_version(void) { return VGT_HIP_ABI_VERSION; }

const char* vgt_hip_last_error(void) { return g_last_error.c_str(); }

int vgt_hip_device_count(int* count)
{
  if (!count) return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "null argument");
  *count = 0;
  int n = 0;
  const hipError_t err = hipGetDeviceCount(&n);
  if (err != hipSuccess) return FailHip("Failed to get device count", err);
  *count = n;
  return VGT_HIP_OK;
}

int vgt_hip_device_name(int device, char* buffer, size_t buffer_size)
{
  if (!buffer || buffer_size == 0) return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "null argument");
  hipDeviceProp_t prop;
  std::memset(&prop, 0, sizeof(prop));
  VGT_TRY_HIP(hipGetDeviceProperties(&prop, device), "Failed to get device properties");
  std::snprintf(buffer, buffer_size, "%s", prop.name);
  return VGT_HIP_OK;
}

int vgt_hip_create(int device, int threads_per_block, vgt_hip_ctx** out_ctx)
{
  if (!out_ctx) return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "null argument");
  *out_ctx = nullptr;
  int count = 0;
  const hipError_t cerr = hipGetDeviceCount(&count);
  if (cerr != hipSuccess || count <= 0)
  {
    g_last_error = "no usable HIP device (libvgt_hip has no CPU fallback)";
    return VGT_HIP_ERR_UNAVAILABLE;
  }
  if (device < 0 || device >= count)
  {
    g_last_error = "HIP_DEVICE = " + std::to_string(device) + " out of range for " +
                   std::to_string(count) + " devices";
    return VGT_HIP_ERR_UNAVAILABLE;
  }
  const int raycast_threads = threads_per_block > 0 ? threads_per_block : 0;
  if (threads_per_block <= 0) threads_per_block = 256;
  if (threads_per_block > 1024 || (threads_per_block % 64) != 0)
    return Fail(VGT_HIP_ERR_INVALID_ARGUMENT,
                "threads_per_block must be a multiple of 64 and at most 1024");
  VGT_TRY_HIP(hipSetDevice(device), "Failed to set device");
  vgt_hip_ctx* ctx = new (std::nothrow) vgt_hip_ctx();
  if (!ctx) return Fail(VGT_HIP_ERR_RUNTIME, "out of host memory");
  ctx->device = device;
  ctx->threads_per_block = threads_per_block;
  ctx->raycast_threads = raycast_threads;
  hipError_t err = hipStreamCreateWithFlags(&ctx->own_stream, hipStreamNonBlocking);
  if (err == hipSuccess) err = ctx->minmax_out.Reserve(256);
  if (err != hipSuccess)
  {
    if (ctx->own_stream) (void)hipStreamDestroy(ctx->own_stream);
    delete ctx;
    return FailHip("create context", err);
  }
  ctx->stream = ctx->own_stream;
  *out_ctx = ctx;
  return VGT_HIP_OK;
}

void vgt_hip_destroy(vgt_hip_ctx* ctx)
{
  if (!ctx) return;
  (void)hipSetDevice(ctx->device);
  (void)hipStreamSynchronize(ctx->stream);
  FreeUploadLanes(ctx, true);
  (void)ctx->minmax_out.Release();
  FreeCachedSdfBuffers(ctx);
  {
    std::lock_guard<std::mutex> lock(ctx->mutex);
    ctx->pool_closed = true;
    FreePool(ctx);
  }
  for (hipEvent_t e : ctx->timing_events)
    if (e) (void)hipEventDestroy(e);
  for (hipEvent_t e : ctx->pipeline_events)
    if (e) (void)hipEventDestroy(e);
  ctx->pipeline_events.clear();
  if (ctx->copy_in) (void)hipStreamDestroy(ctx->copy_in);
  if (ctx->copy_out) (void)hipStreamDestroy(ctx->copy_out);
  ctx->copy_in = nullptr;
  ctx->copy_out = nullptr;
  if (ctx->own_stream) (void)hipStreamDestroy(ctx->own_stream);
  ctx->timing_events.clear();
  ctx->own_stream = nullptr;
  ctx->stream = nullptr;
  ctx->destroyed.store(true);
  if (ctx->children.load() == 0) delete ctx;  // otherwise the last handle's destroy frees it
}

int vgt_hip_trim(vgt_hip_ctx* ctx)
{
  if (!ctx) return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "null argument");
  {
    std::lock_guard<std::mutex> lock(ctx->mutex);
    VGT_TRY_HIP(hipSetDevice(ctx->device), "set device");
    VGT_TRY_HIP(hipStreamSynchronize(ctx->stream), "drain stream");
    FreeCachedSdfBuffers(ctx);
    FreePool(ctx);
  }
  // Lock order: an upload lane's mutex is taken BEFORE the context's (UploadAndRun holds its lane while it
  // records an event under ctx->mutex), so the lanes are released after ctx->mutex has been dropped; a raycast that
  // is in flight on a lane simply finishes first (FreeUploadLanes takes each lane's mutex and drains its stream).
  FreeUploadLanes(ctx, false);
  return VGT_HIP_OK;
}

int vgt_hip_set_stream(vgt_hip_ctx* ctx, void* hip_stream)
{
  if (!ctx) return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "null argument");
  std::lock_guard<std::mutex> lock(ctx->mutex);
  VGT_TRY_HIP(hipSetDevice(ctx->device), "set device");
  VGT_TRY_HIP(hipStreamSynchronize(ctx->stream), "drain stream");
  ctx->stream = static_cast<hipStream_t>(hip_stream);  // NULL = HIP's legacy default stream
  return VGT_HIP_OK;
}

int vgt_hip_reset_stream(vgt_hip_ctx* ctx)
{
  if (!ctx) return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "null argument");
  std::lock_guard<std::mutex> lock(ctx->mutex);
  VGT_TRY_HIP(hipSetDevice(ctx->device), "set device");
  VGT_TRY_HIP(hipStreamSynchronize(ctx->stream), "drain stream");
  ctx->stream = ctx->own_stream;
  return VGT_HIP_OK;
}

int vgt_hip_synchronize(vgt_hip_ctx* ctx)
{
  if (!ctx) return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "null argument");
  VGT_TRY_HIP(hipSetDevice(ctx->device), "set device");
  VGT_TRY_HIP(hipStreamSynchronize(ctx->stream), "synchronize");
  {
    // deferred filter-grid uploads run on the copy stream: "all work of the context has finished" includes them
    std::lock_guard<std::mutex> lock(ctx->mutex);
    if (ctx->copy_in) VGT_TRY_HIP(hipStreamSynchronize(ctx->copy_in), "synchronize the copy stream");
  }
  return VGT_HIP_OK;
}

int vgt_hip_device_of(const vgt_hip_ctx* ctx) { return ctx ? ctx->device : -1; }

#ifdef VGT_HIP_TESTING
/* Testing builds only (libvgt_hip_testing.so; declared in vgt_hip.h under VGT_HIP_TESTING). */
int vgt_hip_set_edt_variant(vgt_hip_ctx* ctx, int variant)
{
  if (!ctx || variant < 0 || variant > 1) return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "invalid EDT variant");
  ctx->variant = variant;
  return VGT_HIP_OK;
}

int vgt_hip_debug_finalize_check(vgt_hip_ctx* ctx, int64_t first_d2, int64_t count, double resolution,
                                 uint64_t* mismatches, uint64_t* first_mismatch)
{
  if (!ctx || !mismatches || !first_mismatch || first_d2 < 0 || count <= 0 ||
      first_d2 + count > (int64_t{1} << 31))
    return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "invalid finalize-check range");
  VGT_TRY_HIP(hipSetDevice(ctx->device), "set device");
  unsigned long long host[2] = {0ull, ~0ull};
  vgt::HostStaging staging;
  const auto result = staging.InOut(host, 2);
  const int rc = staging.Run(*ctx, "finalize check", FailHip, [&](hipStream_t s) {
    return HipResult("finalize check", vgt::LaunchFinalizeCheck(first_d2, count, resolution, result.dev(), s));
  });
  if (rc != VGT_HIP_OK) return rc;
  *mismatches = host[0];
  *first_mismatch = host[1];
  return VGT_HIP_OK;
}

int vgt_hip_testing_set_host_pipeline_min_voxels(int64_t min_voxels)
{
  g_host_pipeline_min_voxels.store(min_voxels);
  return VGT_HIP_OK;
}

int vgt_hip_testing_set_short_line_rows(int rows)
{
  // 0 ... kShortLineRowsFewItems; negative: back to the defaults
  g_short_line_override.store(rows < 0 ? -1 : (rows > vgt::kShortLineRowsFewItems ? vgt::kShortLineRowsFewItems : rows));
  return VGT_HIP_OK;
}

int vgt_hip_testing_set_sweep_slots(int slots)
{
  g_sweep_slots_override.store(slots > 0 ? slots : 0);
  return VGT_HIP_OK;
}

int vgt_hip_testing_set_coarse_hull(int mode)
{
  if (mode != vgt::kXKernelByScene && mode != vgt::kXKernelCoarse && mode != vgt::kXKernelPlain)
    return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "coarse-hull mode must be 0 (by scene), 1 (always) or 2 (never)");
  g_coarse_hull_mode.store(mode);
  return VGT_HIP_OK;
}

int vgt_hip_testing_x_pass_choice(vgt_hip_ctx* ctx, const void* workspace_dev, int64_t nx, int64_t ny, int64_t nz,
                                  int32_t* choice)
{
  if (!ctx || !workspace_dev || !choice) return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "null argument");
  const int rc = CheckSdfShape(nx, ny, nz, 1.0);
  if (rc != VGT_HIP_OK) return rc;
  VGT_TRY_HIP(hipSetDevice(ctx->device), "set device");
  const SdfWorkspace ws = CarveWorkspace(const_cast<void*>(workspace_dev), nx, ny, nz, ctx->variant);
  std::lock_guard<std::mutex> lock(ctx->mutex);
  VGT_TRY_HIP(hipStreamSynchronize(ctx->stream), "synchronize");
  // (the second int of the sweeps' scratch head: edt_sweep_kernels.hip, kChoiceWord)
  VGT_TRY_HIP(hipMemcpy(choice, static_cast<const char*>(ws.sweep_scratch.ptr) + sizeof(int32_t), sizeof(int32_t),
                        hipMemcpyDeviceToHost),
              "copy");
  return VGT_HIP_OK;
}

int vgt_hip_testing_one_class_counts(vgt_hip_ctx* ctx, const void* workspace_dev, int64_t nx, int64_t ny, int64_t nz,
                                     uint32_t* counts)
{
  if (!ctx || !workspace_dev || !counts) return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "null argument");
  const int rc = CheckSdfShape(nx, ny, nz, 1.0);
  if (rc != VGT_HIP_OK) return rc;
  VGT_TRY_HIP(hipSetDevice(ctx->device), "set device");
  const SdfWorkspace ws = CarveWorkspace(const_cast<void*>(workspace_dev), nx, ny, nz, ctx->variant);
  std::lock_guard<std::mutex> lock(ctx->mutex);
  VGT_TRY_HIP(hipStreamSynchronize(ctx->stream), "synchronize");
  VGT_TRY_HIP(hipMemcpy(counts, ws.minmax_enc + vgt::kOneClassWord, 2 * sizeof(uint32_t), hipMemcpyDeviceToHost), "copy");
  return VGT_HIP_OK;
}

int vgt_hip_testing_set_check_spheres_workgroups(int workgroups)
{
  g_check_spheres_workgroups.store(workgroups > 0 ? workgroups : 0);
  return VGT_HIP_OK;
}

int vgt_hip_testing_set_sphere_volume_workgroups(int workgroups)
{
  g_sphere_volume_workgroups.store(workgroups > 0 ? workgroups : 0);
  return VGT_HIP_OK;
}

int vgt_hip_testing_set_align_workgroups(int workgroups)
{
  g_align_workgroups.store(workgroups > 0 ? workgroups : 0);
  return VGT_HIP_OK;
}

int vgt_hip_testing_set_kinematics_workgroups(int workgroups)
{
  g_kinematics_workgroups.store(workgroups > 0 ? workgroups : 0);
  return VGT_HIP_OK;
}

int vgt_hip_testing_set_motion_workgroups(int workgroups)
{
  g_motion_workgroups.store(workgroups > 0 ? workgroups : 0);
  return VGT_HIP_OK;
}

int vgt_hip_testing_set_cost_workgroups(int workgroups)
{
  g_cost_workgroups.store(workgroups > 0 ? workgroups : 0);
  return VGT_HIP_OK;
}

int vgt_hip_testing_motion_launch_geometry(int64_t num_links, int64_t num_spheres, int32_t* tile_samples,
                                           int32_t* table_in_lds)
{
  if (!tile_samples || !table_in_lds) return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "null argument");
  if (num_spheres < 0) return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "negative sphere count");
  const vgt::MotionLaunchGeometry geometry = vgt::SelectMotionGeometry(num_links, num_spheres);
  if (geometry.tile <= 0) return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "a tree the motion kernel does not take");
  *tile_samples = geometry.tile;
  *table_in_lds = geometry.table_in_lds;
  return VGT_HIP_OK;
}

int vgt_hip_testing_cost_launch_geometry(int64_t num_links, int64_t num_spheres, int gradient_form, int32_t* tile_samples,
                                         int32_t* passes, int32_t* table_in_lds, int32_t* links_in_lds)
{
  if (!tile_samples || !passes || !table_in_lds || !links_in_lds)
    return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "null argument");
  if (num_spheres < 0) return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "negative sphere count");
  const vgt::CostLaunchGeometry geometry = vgt::SelectCostGeometry(num_links, num_spheres, gradient_form != 0);
  if (geometry.tile <= 0) return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "a tree the cost kernel does not take");
  *tile_samples = geometry.tile;
  *passes = geometry.passes;
  *table_in_lds = geometry.table_in_lds;
  *links_in_lds = geometry.links_in_lds;
  return VGT_HIP_OK;
}

int vgt_hip_testing_set_self_collision_workgroups(int workgroups)
{
  g_self_collision_workgroups.store(workgroups > 0 ? workgroups : 0);
  return VGT_HIP_OK;
}

int vgt_hip_testing_set_motion_self_workgroups(int workgroups)
{
  g_motion_self_workgroups.store(workgroups > 0 ? workgroups : 0);
  return VGT_HIP_OK;
}

int vgt_hip_testing_set_sphere_volume_counters(uint64_t* counters_dev)
{
  g_sphere_volume_counters.store(reinterpret_cast<unsigned long long*>(counters_dev));
  return VGT_HIP_OK;
}

size_t vgt_hip_testing_class_record_bytes(int64_t nx, int64_t ny, int64_t nz)
{
  if (nx <= 0 || ny <= 0 || nz <= 0) return 0;
  return vgt::ClassRecordBytes(nx, ny, nz);
}

int vgt_hip_testing_class_records_dev(vgt_hip_ctx* ctx, const float* occupancy_dev, int64_t nx, int64_t ny, int64_t nz,
                                      int unknown_is_filled, int64_t z_offset, void* records_dev, void* summary_dev)
{
  if (!ctx || !occupancy_dev || !records_dev) return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "null argument");
  const int rc = CheckSdfShape(nx, ny, nz, 1.0);
  if (rc != VGT_HIP_OK) return rc;
  VGT_TRY_HIP(hipSetDevice(ctx->device), "set device");
  vgt::SdfParams p{nx, ny, nz, 1.0, unknown_is_filled ? 1 : 0, 0};
  p.z_offset = z_offset;
  std::lock_guard<std::mutex> lock(ctx->mutex);
  VGT_TRY_HIP(vgt::LaunchClassRecordsFromOccupancy(occupancy_dev, static_cast<vgt::ClassRecord*>(records_dev), p,
                                                   static_cast<vgt::SlabLineSummary*>(summary_dev), ctx->stream),
              "pass 1");
  VGT_TRY_HIP(hipStreamSynchronize(ctx->stream), "synchronize");
  return VGT_HIP_OK;
}
#endif  // VGT_HIP_TESTING

/* ------------------------------ tracking grids ------------------------------ */

int vgt_hip_tracking_grids_create(vgt_hip_ctx* ctx, int64_t num_cells, int32_t num_grids,
                                  vgt_hip_grids** out_grids)
{
  if (!ctx || !out_grids) return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "null argument");
  *out_grids = nullptr;
  // zero-element buffers are an error, as in the reference (cuda_voxelization_helpers.cu:457-460)
  if (num_cells <= 0 || num_grids <= 0)
    return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "num_elements must be > 0");
  VGT_TRY_HIP(hipSetDevice(ctx->device), "set device");
  vgt_hip_grids* g = new (std::nothrow) vgt_hip_grids();
  if (!g) return Fail(VGT_HIP_ERR_RUNTIME, "out of host memory");
  g->ctx = ctx;
  g->device = ctx->device;
  g->num_cells = num_cells;
  g->num_grids = num_grids;
  const size_t bytes = static_cast<size_t>(num_cells) * num_grids * 2 * sizeof(int32_t);
  hipError_t err = PoolAllocate(ctx, &g->dev, bytes);
  if (err == hipSuccess)
  {
    std::lock_guard<std::mutex> lock(ctx->mutex);
    err = hipMemsetAsync(g->dev.data(), 0, bytes, ctx->stream);
  }
  if (err != hipSuccess)
  {
    delete g;
    return FailHip("Failed to allocate tracking grids", err);
  }
  AdoptChild(ctx);
  *out_grids = g;
  return VGT_HIP_OK;
}

void vgt_hip_tracking_grids_destroy(vgt_hip_grids* grids)
{
  if (!grids) return;
  vgt_hip_ctx* const ctx = grids->ctx;
  // (the buffer goes back to the pool before the handle's reference, which may be the context's last, is dropped)
  (void)hipSetDevice(grids->device);
  if (ctx->destroyed.load())
    (void)hipDeviceSynchronize();
  else
    (void)hipStreamSynchronize(ctx->stream);
  PoolRelease(ctx, &grids->dev);
  ReleaseChild(ctx, grids->device);
  delete grids;
}

int64_t vgt_hip_tracking_grids_num_cells(const vgt_hip_grids* grids)
{
  return grids ? grids->num_cells : 0;
}
int32_t vgt_hip_tracking_grids_num_grids(const vgt_hip_grids* grids)
{
  return grids ? grids->num_grids : 0;
}
int64_t vgt_hip_tracking_grids_offset(const vgt_hip_grids* grids, size_t grid_index)
{
  if (!grids || grid_index >= static_cast<size_t>(grids->num_grids)) return -1;
  return static_cast<int64_t>(grid_index) * grids->num_cells * 2;
}
void* vgt_hip_tracking_grids_dev_ptr(const vgt_hip_grids* grids, size_t grid_index)
{
  if (!grids || grid_index >= static_cast<size_t>(grids->num_grids)) return nullptr;
  return grids->dev.as<int32_t>() + static_cast<int64_t>(grid_index) * grids->num_cells * 2;
}

int vgt_hip_tracking_grids_clear(vgt_hip_ctx* ctx, vgt_hip_grids* grids)
{
  if (!ctx || !grids || grids->ctx != ctx)
    return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "invalid tracking grids");
  VGT_TRY_HIP(hipSetDevice(ctx->device), "set device");
  std::lock_guard<std::mutex> lock(ctx->mutex);
  const size_t bytes = static_cast<size_t>(grids->num_cells) * grids->num_grids * 2 * sizeof(int32_t);
  VGT_TRY_HIP(hipMemsetAsync(grids->dev.data(), 0, bytes, ctx->stream), "clear tracking grids");
  return VGT_HIP_OK;
}

/* --------------------------------- raycast ---------------------------------- */

int vgt_hip_raycast_points_f32_dev(vgt_hip_ctx* ctx, vgt_hip_grids* grids, size_t grid_index,
                                   const float* points_xyz_dev, int64_t num_points,
                                   float max_range, const float* grid_pointcloud_transform,
                                   float voxel_size, float inverse_voxel_size, float grid_x_size,
                                   float grid_y_size, float grid_z_size, int32_t num_x_voxels,
                                   int32_t num_y_voxels, int32_t num_z_voxels)
{
  const int rc = CheckRaycastArgs(ctx, grids, grid_index, points_xyz_dev, num_points,
                                  grid_pointcloud_transform, num_x_voxels, num_y_voxels,
                                  num_z_voxels);
  if (rc != VGT_HIP_OK) return rc;
  if (num_points == 0) return VGT_HIP_OK;
  VGT_TRY_HIP(hipSetDevice(ctx->device), "set device");
  vgt::RaycastGridF32 g;
  g.max_range = max_range;
  std::memcpy(g.xform, grid_pointcloud_transform, sizeof(g.xform));
  g.voxel_size = voxel_size;
  g.inverse_voxel_size = inverse_voxel_size;
  g.grid_size[0] = grid_x_size;
  g.grid_size[1] = grid_y_size;
  g.grid_size[2] = grid_z_size;
  g.counts[0] = num_x_voxels;
  g.counts[1] = num_y_voxels;
  g.counts[2] = num_z_voxels;
  int32_t* tracking = static_cast<int32_t*>(vgt_hip_tracking_grids_dev_ptr(grids, grid_index));
  std::lock_guard<std::mutex> lock(ctx->mutex);
  // stream order protects the scratch: the next call's kernels queue behind this one's
  const size_t scratch_bytes = vgt::RaycastScratchBytes(num_points);
  const int grown = GrowCache(ctx->stream, &ctx->ray_scratch, scratch_bytes, "drain before regrowing raycast scratch",
                              "allocate raycast scratch", scratch_bytes + scratch_bytes / 4);
  if (grown != VGT_HIP_OK) return grown;
  VGT_TRY_HIP(vgt::LaunchRaycastF32(points_xyz_dev, num_points, 3, g, tracking, ctx->raycast_threads,
                                    ctx->ray_scratch.data(), ctx->ray_scratch.bytes(), ctx->stream),
              "Failed to dispatch raycast kernel");
  return VGT_HIP_OK;
}

int vgt_hip_raycast_points_f32(vgt_hip_ctx* ctx, vgt_hip_grids* grids, size_t grid_index,
                               const float* points_xyz_host, int64_t num_points, float max_range,
                               const float* grid_pointcloud_transform, float voxel_size,
                               float inverse_voxel_size, float grid_x_size, float grid_y_size,
                               float grid_z_size, int32_t num_x_voxels, int32_t num_y_voxels,
                               int32_t num_z_voxels)
{
  const int rc = CheckRaycastArgs(ctx, grids, grid_index, points_xyz_host, num_points,
                                  grid_pointcloud_transform, num_x_voxels, num_y_voxels,
                                  num_z_voxels);
  if (rc != VGT_HIP_OK) return rc;
  if (num_points == 0) return VGT_HIP_OK;
  VGT_TRY_HIP(hipSetDevice(ctx->device), "set device");
  vgt::RaycastGridF32 g;
  g.max_range = max_range;
  std::memcpy(g.xform, grid_pointcloud_transform, sizeof(g.xform));
  g.voxel_size = voxel_size;
  g.inverse_voxel_size = inverse_voxel_size;
  g.grid_size[0] = grid_x_size;
  g.grid_size[1] = grid_y_size;
  g.grid_size[2] = grid_z_size;
  g.counts[0] = num_x_voxels;
  g.counts[1] = num_y_voxels;
  g.counts[2] = num_z_voxels;
  int32_t* tracking = static_cast<int32_t*>(vgt_hip_tracking_grids_dev_ptr(grids, grid_index));
  const size_t bytes = static_cast<size_t>(num_points) * 3 * sizeof(float);
  const int threads = ctx->raycast_threads;
  const size_t scratch_bytes = vgt::RaycastScratchBytes(num_points);
  return UploadAndRun(ctx, points_xyz_host, bytes, scratch_bytes,
                      [&](const void* points_dev, void* scratch, hipStream_t stream) {
                        return vgt::LaunchRaycastF32(static_cast<const float*>(points_dev), num_points, 3, g, tracking,
                                                     threads, scratch, scratch_bytes, stream);
                      });
}

int vgt_hip_raycast_pointcloud2_f32(vgt_hip_ctx* ctx, vgt_hip_grids* grids, size_t grid_index,
                                    const uint8_t* cloud_data_host, int64_t num_points, int64_t point_step,
                                    int64_t xyz_offset, float max_range,
                                    const float* grid_pointcloud_transform, float voxel_size,
                                    float inverse_voxel_size, float grid_x_size, float grid_y_size,
                                    float grid_z_size, int32_t num_x_voxels, int32_t num_y_voxels,
                                    int32_t num_z_voxels)
{
  const int rc = CheckRaycastArgs(ctx, grids, grid_index, cloud_data_host, num_points,
                                  grid_pointcloud_transform, num_x_voxels, num_y_voxels, num_z_voxels);
  if (rc != VGT_HIP_OK) return rc;
  // x, y, z are three consecutive FLOAT32 fields (pointcloud_voxelization_ros_interface.cpp:49-78);
  // the kernel reads them in place, which needs them 4-byte aligned inside the buffer
  if (xyz_offset < 0 || point_step < xyz_offset + 12)
    return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "PointCloud does not have sequential xyz fields");
  if (point_step % 4 != 0 || xyz_offset % 4 != 0)
    return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "point_step and the xyz offset must be multiples of 4");
  if (num_points == 0) return VGT_HIP_OK;
  VGT_TRY_HIP(hipSetDevice(ctx->device), "set device");
  vgt::RaycastGridF32 g;
  g.max_range = max_range;
  std::memcpy(g.xform, grid_pointcloud_transform, sizeof(g.xform));
  g.voxel_size = voxel_size;
  g.inverse_voxel_size = inverse_voxel_size;
  g.grid_size[0] = grid_x_size;
  g.grid_size[1] = grid_y_size;
  g.grid_size[2] = grid_z_size;
  g.counts[0] = num_x_voxels;
  g.counts[1] = num_y_voxels;
  g.counts[2] = num_z_voxels;
  int32_t* tracking = static_cast<int32_t*>(vgt_hip_tracking_grids_dev_ptr(grids, grid_index));
  const size_t bytes = static_cast<size_t>(num_points) * static_cast<size_t>(point_step);
  const int threads = ctx->raycast_threads;
  const size_t scratch_bytes = vgt::RaycastScratchBytes(num_points);
  return UploadAndRun(ctx, cloud_data_host, bytes, scratch_bytes,
                      [&](const void* cloud_dev, void* scratch, hipStream_t stream) {
                        const float* first =
                            reinterpret_cast<const float*>(static_cast<const uint8_t*>(cloud_dev) + xyz_offset);
                        return vgt::LaunchRaycastF32(first, num_points, point_step / 4, g, tracking, threads, scratch,
                                                     scratch_bytes, stream);
                      });
}

int vgt_hip_raycast_points_f64(vgt_hip_ctx* ctx, vgt_hip_grids* grids, size_t grid_index,
                               const double* points_xyz_host, int64_t num_points,
                               double max_range, const double* grid_pointcloud_transform,
                               double voxel_size, double inverse_voxel_size, double grid_x_size,
                               double grid_y_size, double grid_z_size, int32_t num_x_voxels,
                               int32_t num_y_voxels, int32_t num_z_voxels)
{
  const int rc = CheckRaycastArgs(ctx, grids, grid_index, points_xyz_host, num_points,
                                  grid_pointcloud_transform, num_x_voxels, num_y_voxels,
                                  num_z_voxels);
  if (rc != VGT_HIP_OK) return rc;
  if (num_points == 0) return VGT_HIP_OK;
  VGT_TRY_HIP(hipSetDevice(ctx->device), "set device");
  vgt::RaycastGridF64 g;
  g.max_range = max_range;
  std::memcpy(g.xform, grid_pointcloud_transform, sizeof(g.xform));
  g.voxel_size = voxel_size;
  g.inverse_voxel_size = inverse_voxel_size;
  g.grid_size[0] = grid_x_size;
  g.grid_size[1] = grid_y_size;
  g.grid_size[2] = grid_z_size;
  g.counts[0] = num_x_voxels;
  g.counts[1] = num_y_voxels;
  g.counts[2] = num_z_voxels;
  int32_t* tracking = static_cast<int32_t*>(vgt_hip_tracking_grids_dev_ptr(grids, grid_index));
  const size_t bytes = static_cast<size_t>(num_points) * 3 * sizeof(double);
  const int threads = ctx->raycast_threads;
  const size_t scratch_bytes = vgt::RaycastScratchBytes(num_points);
  return UploadAndRun(ctx, points_xyz_host, bytes, scratch_bytes,
                      [&](const void* points_dev, void* scratch, hipStream_t stream) {
                        return vgt::LaunchRaycastF64(static_cast<const double*>(points_dev), num_points, g, tracking,
                                                     threads, scratch, scratch_bytes, stream);
                      });
}

/* --------------------------------- filter ----------------------------------- */

int vgt_hip_filter_grid_create(vgt_hip_ctx* ctx, int64_t num_cells, const float* occupancy_host,
                               vgt_hip_filter** out_filter)
{
  if (!ctx || !out_filter) return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "null argument");
  *out_filter = nullptr;
  if (num_cells <= 0) return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "num_elements must be > 0");
  if (!occupancy_host) return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "to_copy cannot be nullptr");
  VGT_TRY_HIP(hipSetDevice(ctx->device), "set device");
  vgt_hip_filter* f = new (std::nothrow) vgt_hip_filter();
  if (!f) return Fail(VGT_HIP_ERR_RUNTIME, "out of host memory");
  f->ctx = ctx;
  f->device = ctx->device;
  f->num_cells = num_cells;
  const size_t bytes = static_cast<size_t>(num_cells) * sizeof(float);
  hipError_t err = PoolAllocate(ctx, &f->dev, bytes);
  if (err == hipSuccess)
  {
    // the caller's array is page-locked for the copy (a pageable 64 MiB copy is staged at a fifth of the link rate)
    const ScopedHostPin pin(occupancy_host, bytes);
    std::lock_guard<std::mutex> lock(ctx->mutex);
    err = hipMemcpyAsync(f->dev.data(), occupancy_host, bytes, hipMemcpyHostToDevice, ctx->stream);
    if (err == hipSuccess) err = hipStreamSynchronize(ctx->stream);
  }
  if (err != hipSuccess)
  {
    delete f;
    return FailHip("Failed to prepare filter grid", err);
  }
  AdoptChild(ctx);
  *out_filter = f;
  return VGT_HIP_OK;
}

namespace
{
// The filter kernel / a download is about to use the grid on the context's stream: order it behind a deferred upload.
static hipError_t OrderBehindUpload(vgt_hip_ctx* ctx, const vgt_hip_filter* filter)
{
  if (!filter->upload_pending) return hipSuccess;
  return hipStreamWaitEvent(ctx->stream, filter->uploaded, 0);
}
// The host has waited for work that was ordered behind the upload (or for the upload itself): the caller's array is free.
static void UploadHasFinished(vgt_hip_filter* filter)
{
  filter->upload_pending = false;
  delete static_cast<ScopedHostPin*>(filter->pin);
  filter->pin = nullptr;
}
}  // namespace

int vgt_hip_filter_grid_create_deferred(vgt_hip_ctx* ctx, int64_t num_cells, const float* occupancy_host,
                                        vgt_hip_filter** out_filter)
{
  if (!ctx || !out_filter) return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "null argument");
  *out_filter = nullptr;
  if (num_cells <= 0) return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "num_elements must be > 0");
  if (!occupancy_host) return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "to_copy cannot be nullptr");
  VGT_TRY_HIP(hipSetDevice(ctx->device), "set device");
  vgt_hip_filter* f = new (std::nothrow) vgt_hip_filter();
  if (!f) return Fail(VGT_HIP_ERR_RUNTIME, "out of host memory");
  f->ctx = ctx;
  f->device = ctx->device;
  f->num_cells = num_cells;
  const size_t bytes = static_cast<size_t>(num_cells) * sizeof(float);
  hipError_t err = PoolAllocate(ctx, &f->dev, bytes);
  if (err == hipSuccess) err = hipEventCreateWithFlags(&f->uploaded, hipEventDisableTiming);
  if (err == hipSuccess)
  {
    f->pin = new (std::nothrow) ScopedHostPin(occupancy_host, bytes);  // (nullptr: the copy runs from pageable memory)
    std::lock_guard<std::mutex> lock(ctx->mutex);
    if (!ctx->copy_in) err = hipStreamCreateWithFlags(&ctx->copy_in, hipStreamNonBlocking);
    // (a pooled buffer may still be read by work queued on the context's stream: the copy starts behind it)
    if (err == hipSuccess) err = hipEventRecord(f->uploaded, ctx->stream);
    if (err == hipSuccess) err = hipStreamWaitEvent(ctx->copy_in, f->uploaded, 0);
    if (err == hipSuccess)
      err = hipMemcpyAsync(f->dev.data(), occupancy_host, bytes, hipMemcpyHostToDevice, ctx->copy_in);
    if (err == hipSuccess) err = hipEventRecord(f->uploaded, ctx->copy_in);
    f->upload_pending = err == hipSuccess;
  }
  if (err != hipSuccess)
  {
    {
      // (a copy that was enqueued before the failure must not outlive the caller's array)
      std::lock_guard<std::mutex> lock(ctx->mutex);
      if (f->uploaded && ctx->copy_in) (void)hipStreamSynchronize(ctx->copy_in);
    }
    delete static_cast<ScopedHostPin*>(f->pin);
    if (f->uploaded) (void)hipEventDestroy(f->uploaded);
    delete f;
    return FailHip("Failed to prepare filter grid", err);
  }
  AdoptChild(ctx);
  *out_filter = f;
  return VGT_HIP_OK;
}

void vgt_hip_filter_grid_destroy(vgt_hip_filter* filter)
{
  if (!filter) return;
  vgt_hip_ctx* const ctx = filter->ctx;
  (void)hipSetDevice(filter->device);
  if (filter->upload_pending) (void)hipEventSynchronize(filter->uploaded);
  UploadHasFinished(filter);
  if (filter->uploaded) (void)hipEventDestroy(filter->uploaded);
  if (ctx->destroyed.load())
    (void)hipDeviceSynchronize();
  else
    (void)hipStreamSynchronize(ctx->stream);
  PoolRelease(ctx, &filter->dev);
  ReleaseChild(ctx, filter->device);
  delete filter;
}

int64_t vgt_hip_filter_grid_num_cells(const vgt_hip_filter* filter)
{
  return filter ? filter->num_cells : 0;
}
void* vgt_hip_filter_grid_dev_ptr(const vgt_hip_filter* filter)
{
  if (!filter) return nullptr;
  // A deferred upload is ordered behind nothing the caller's own streams know of: wait for it here, so that the
  // pointer can be used on any stream (the pin on the caller's array is released by retrieve / destroy as before).
  // (the flag is written under the context's mutex by filter / retrieve: read it the same way; a failed wait means the
  // grid's content is not known to be there -- no pointer then, the reason in vgt_hip_last_error(); the calling thread's
  // current device is left as it was)
  bool pending = false;
  {
    std::lock_guard<std::mutex> lock(filter->ctx->mutex);
    pending = filter->upload_pending;
  }
  if (pending)
  {
    int previous = -1;
    if (hipGetDevice(&previous) != hipSuccess) previous = -1;
    hipError_t err = hipSetDevice(filter->device);
    if (err == hipSuccess) err = hipEventSynchronize(filter->uploaded);
    if (previous >= 0 && previous != filter->device) (void)hipSetDevice(previous);
    if (err != hipSuccess)
    {
      (void)hipGetLastError();
      Fail(VGT_HIP_ERR_RUNTIME, std::string("waiting for the filter grid's upload: ") + hipGetErrorString(err));
      return nullptr;
    }
  }
  return filter->dev.data();
}

static int FilterImpl(vgt_hip_ctx* ctx, const vgt_hip_grids* grids, double percent_seen_free,
                      int32_t outlier_points_threshold, int32_t num_cameras_seen_free,
                      bool ratio_in_double, vgt_hip_filter* filter)
{
  if (!ctx || !grids || !filter) return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "null argument");
  if (grids->ctx != ctx || filter->ctx != ctx)
    return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "handles belong to another context");
  if (grids->num_cells != filter->num_cells)
    return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "tracking grids and filter grid differ in size");
  VGT_TRY_HIP(hipSetDevice(ctx->device), "set device");
  std::lock_guard<std::mutex> lock(ctx->mutex);
  VGT_TRY_HIP(OrderBehindUpload(ctx, filter), "order the filter behind the grid's upload");
  VGT_TRY_HIP(vgt::LaunchFilter(grids->dev.as<int32_t>(), grids->num_cells, grids->num_grids, percent_seen_free,
                                outlier_points_threshold, num_cameras_seen_free, ratio_in_double,
                                filter->dev.as<float>(), ctx->threads_per_block, ctx->stream),
              "Failed to dispatch filter kernel");
  return VGT_HIP_OK;
}

int vgt_hip_filter_tracking_grids(vgt_hip_ctx* ctx, const vgt_hip_grids* grids,
                                  float percent_seen_free, int32_t outlier_points_threshold,
                                  int32_t num_cameras_seen_free, vgt_hip_filter* filter)
{
  return FilterImpl(ctx, grids, static_cast<double>(percent_seen_free), outlier_points_threshold,
                    num_cameras_seen_free, false, filter);
}

int vgt_hip_filter_tracking_grids_f64(vgt_hip_ctx* ctx, const vgt_hip_grids* grids,
                                      double percent_seen_free, int32_t outlier_points_threshold,
                                      int32_t num_cameras_seen_free, vgt_hip_filter* filter)
{
  return FilterImpl(ctx, grids, percent_seen_free, outlier_points_threshold,
                    num_cameras_seen_free, true, filter);
}

int vgt_hip_retrieve_tracking_grid(vgt_hip_ctx* ctx, const vgt_hip_grids* grids, size_t grid_index,
                                   void* host_out)
{
  if (!ctx || !grids || !host_out || grids->ctx != ctx)
    return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "null argument");
  if (grid_index >= static_cast<size_t>(grids->num_grids))
    return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "tracking grid index out of range");
  VGT_TRY_HIP(hipSetDevice(ctx->device), "set device");
  std::lock_guard<std::mutex> lock(ctx->mutex);
  const size_t bytes = static_cast<size_t>(grids->num_cells) * 2 * sizeof(int32_t);
  VGT_TRY_HIP(hipMemcpyAsync(host_out, vgt_hip_tracking_grids_dev_ptr(grids, grid_index), bytes,
                             hipMemcpyDeviceToHost, ctx->stream),
              "Failed to memcpy the tracking grid back to the host");
  VGT_TRY_HIP(hipStreamSynchronize(ctx->stream), "retrieve tracking grid");
  return VGT_HIP_OK;
}

int vgt_hip_retrieve_filtered_grid(vgt_hip_ctx* ctx, const vgt_hip_filter* filter, void* host_out)
{
  if (!ctx || !filter || !host_out || filter->ctx != ctx)
    return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "null argument");
  VGT_TRY_HIP(hipSetDevice(ctx->device), "set device");
  const size_t bytes = static_cast<size_t>(filter->num_cells) * sizeof(float);
  const ScopedHostPin pin(host_out, bytes);
  std::lock_guard<std::mutex> lock(ctx->mutex);
  VGT_TRY_HIP(OrderBehindUpload(ctx, filter), "order the download behind the grid's upload");
  VGT_TRY_HIP(hipMemcpyAsync(host_out, filter->dev.data(), bytes, hipMemcpyDeviceToHost, ctx->stream),
              "Failed to memcpy the filter grid back to the host");
  VGT_TRY_HIP(hipStreamSynchronize(ctx->stream), "retrieve filtered grid");
  // (the handle is logically const for the caller; the finished upload's bookkeeping is not part of its value)
  if (filter->upload_pending) UploadHasFinished(const_cast<vgt_hip_filter*>(filter));
  return VGT_HIP_OK;
}

/* ----------------------------------- SDF ------------------------------------ */

size_t vgt_hip_sdf_workspace_bytes(int64_t nx, int64_t ny, int64_t nz)
{
  if (nx <= 0 || ny <= 0 || nz <= 0) return 0;
  return CarveWorkspace(nullptr, nx, ny, nz, 0).bytes;
}

size_t vgt_hip_sdf_workspace_bytes_for_variant(int64_t nx, int64_t ny, int64_t nz, int variant)
{
  if (nx <= 0 || ny <= 0 || nz <= 0 || variant < 0 || variant > 1) return 0;
  if (variant != 0 && !kHaveCrossCheck) return 0;  // the cross-check is not part of the product library
  return CarveWorkspace(nullptr, nx, ny, nz, variant).bytes;
}

int vgt_hip_sdf_from_occupancy_f32(vgt_hip_ctx* ctx, const float* occupancy_host, int64_t nx,
                                   int64_t ny, int64_t nz, double resolution,
                                   int unknown_is_filled, int add_virtual_border, float* sdf_host,
                                   float* out_min, float* out_max)
{
  const vgt::SdfParams p{nx, ny, nz, resolution, unknown_is_filled ? 1 : 0,
                         add_virtual_border ? 1 : 0};
  return SdfFromHost<float>(ctx, occupancy_host, p, sdf_host, out_min, out_max);
}

int vgt_hip_sdf_from_mask_u8(vgt_hip_ctx* ctx, const uint8_t* filled_mask_host, int64_t nx,
                             int64_t ny, int64_t nz, double resolution, int add_virtual_border,
                             float* sdf_host, float* out_min, float* out_max)
{
  const vgt::SdfParams p{nx, ny, nz, resolution, 0, add_virtual_border ? 1 : 0};
  return SdfFromHost<uint8_t>(ctx, filled_mask_host, p, sdf_host, out_min, out_max);
}

int vgt_hip_sdf_dev(vgt_hip_ctx* ctx, const float* occupancy_dev, int64_t nx, int64_t ny,
                    int64_t nz, double resolution, int unknown_is_filled, int add_virtual_border,
                    float* sdf_dev, void* workspace_dev, size_t workspace_bytes, float* minmax_dev)
{
  if (!ctx || !occupancy_dev || !sdf_dev)
    return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "null argument");
  const int rc = CheckSdfShape(nx, ny, nz, resolution);
  if (rc != VGT_HIP_OK) return rc;
  VGT_TRY_HIP(hipSetDevice(ctx->device), "set device");
  const vgt::SdfParams p{nx, ny, nz, resolution, unknown_is_filled ? 1 : 0,
                         add_virtual_border ? 1 : 0};
  std::lock_guard<std::mutex> lock(ctx->mutex);
  hipEvent_t* slot = TimingSlot(ctx);
  const int result = RunSdfPipeline<float>(ctx, occupancy_dev, p, sdf_dev, workspace_dev, workspace_bytes,
                                           minmax_dev, slot);
  if (slot && result == VGT_HIP_OK) ctx->timing_kind[static_cast<size_t>(ctx->timing_used++)] = 1;
  return result;
}

size_t vgt_hip_sdf_batch_workspace_bytes(int64_t batch, int64_t nx, int64_t ny, int64_t nz)
{
  if (batch <= 0 || nx <= 0 || ny <= 0 || nz <= 0) return 0;
  return CarveWorkspace(nullptr, nx, ny, nz, 0, batch).bytes;
}

int vgt_hip_sdf_batch_dev(vgt_hip_ctx* ctx, const float* occupancy_dev, int64_t batch, int64_t nx, int64_t ny,
                          int64_t nz, double resolution, int unknown_is_filled, int add_virtual_border,
                          float* sdf_dev, void* workspace_dev, size_t workspace_bytes, float* minmax_dev)
{
  if (!ctx || !occupancy_dev || !sdf_dev) return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "null argument");
  int rc = CheckSdfShape(nx, ny, nz, resolution);
  if (rc == VGT_HIP_OK) rc = CheckBatch(batch, nx, ny, nz);
  if (rc != VGT_HIP_OK) return rc;
  VGT_TRY_HIP(hipSetDevice(ctx->device), "set device");
  vgt::SdfParams p{nx, ny, nz, resolution, unknown_is_filled ? 1 : 0, add_virtual_border ? 1 : 0};
  p.batch = batch;
  std::lock_guard<std::mutex> lock(ctx->mutex);
  hipEvent_t* slot = TimingSlot(ctx);
  const int result = RunSdfPipeline<float>(ctx, occupancy_dev, p, sdf_dev, workspace_dev, workspace_bytes,
                                           minmax_dev, slot);
  if (slot && result == VGT_HIP_OK) ctx->timing_kind[static_cast<size_t>(ctx->timing_used++)] = 1;
  return result;
}

int vgt_hip_sdf_batch_from_occupancy_f32(vgt_hip_ctx* ctx, const float* const* occupancy_host, int64_t batch,
                                         int64_t nx, int64_t ny, int64_t nz, double resolution,
                                         int unknown_is_filled, int add_virtual_border, float* const* sdf_host,
                                         float* out_min, float* out_max)
{
  if (!ctx || !occupancy_host || !sdf_host) return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "null argument");
  int rc = CheckSdfShape(nx, ny, nz, resolution);
  if (rc != VGT_HIP_OK) return rc;
  if (batch <= 0) return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "batch must be positive");
  for (int64_t b = 0; b < batch; b++)
    if (!occupancy_host[b] || !sdf_host[b]) return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "null grid in the batch");
  VGT_TRY_HIP(hipSetDevice(ctx->device), "set device");
  const size_t n = static_cast<size_t>(nx * ny * nz);
  // Grids per launch: as many as the limits of a batch and a memory budget allow (the context keeps the buffers).
  const int64_t group = BatchGroup(batch, nx, ny, nz, size_t{2} << 30, n * 9);
  std::lock_guard<std::mutex> lock(ctx->mutex);
  const size_t ws_bytes = CarveWorkspace(nullptr, nx, ny, nz, ctx->variant, ctx->variant == 0 ? group : 1).bytes;
  VGT_TRY_HIP(ctx->sdf_in.Reserve(static_cast<size_t>(group) * n * sizeof(float)), "allocate SDF input");
  VGT_TRY_HIP(ctx->sdf_out.Reserve(static_cast<size_t>(group) * (n + 2) * sizeof(float)), "allocate SDF output");
  VGT_TRY_HIP(ctx->sdf_ws.Reserve(ws_bytes), "allocate SDF workspace");
  float* const in_dev = ctx->sdf_in.as<float>();
  float* const out_dev = ctx->sdf_out.as<float>();
  float* const mm_dev = out_dev + static_cast<size_t>(group) * n;
  std::vector<float> mm(static_cast<size_t>(group) * 2);
  hipStream_t s = ctx->stream;
  for (int64_t first = 0; first < batch; first += group)
  {
    const int64_t count = batch - first < group ? batch - first : group;
    // Inputs of 32 MiB and more are page-locked for the group's uploads (they hold data, their pages exist); smaller
    // ones -- for which locking and unlocking costs several times the copy -- cross through the context's ring.
    std::vector<std::unique_ptr<ScopedHostPin>> pins;
    if (n * sizeof(float) >= (size_t{32} << 20))
    {
      for (int64_t b = 0; b < count; b++) pins.emplace_back(new ScopedHostPin(occupancy_host[first + b], n * sizeof(float)));
      for (int64_t b = 0; b < count; b++)
        VGT_TRY_HIP(hipMemcpyAsync(in_dev + static_cast<size_t>(b) * n, occupancy_host[first + b], n * sizeof(float),
                                   hipMemcpyHostToDevice, s),
                    "copy occupancy to device");
    }
    else
    {
      std::vector<HostArrayCopy> uploads;
      for (int64_t b = 0; b < count; b++)
        uploads.push_back(HostArrayCopy{in_dev + static_cast<size_t>(b) * n, const_cast<float*>(occupancy_host[first + b])});
      const hipError_t moved = UploadFromHostArrays(ctx, uploads, n * sizeof(float), s);
      if (moved != hipSuccess) (void)hipStreamSynchronize(s);
      VGT_TRY_HIP(moved, "copy occupancy to device");
    }
    vgt::SdfParams p{nx, ny, nz, resolution, unknown_is_filled ? 1 : 0, add_virtual_border ? 1 : 0};
    if (ctx->variant == 0)
    {
      p.batch = count;
      rc = RunSdfPipeline<float>(ctx, in_dev, p, out_dev, ctx->sdf_ws.data(), ctx->sdf_ws.bytes(), mm_dev, nullptr);
      if (rc != VGT_HIP_OK) return rc;
    }
    else
    {
      // (the testing library with the cross-check selected: grid by grid)
      for (int64_t b = 0; b < count; b++)
      {
        rc = RunSdfPipeline<float>(ctx, in_dev + static_cast<size_t>(b) * n, p, out_dev + static_cast<size_t>(b) * n,
                                   ctx->sdf_ws.data(), ctx->sdf_ws.bytes(), mm_dev + 2 * b, nullptr);
        if (rc != VGT_HIP_OK) return rc;
      }
    }
    VGT_TRY_HIP(hipMemcpyAsync(mm.data(), mm_dev, static_cast<size_t>(count) * 2 * sizeof(float), hipMemcpyDeviceToHost, s),
                "copy extrema to host");
    {
      std::vector<HostArrayCopy> copies;
      for (int64_t b = 0; b < count; b++) copies.push_back(HostArrayCopy{out_dev + static_cast<size_t>(b) * n, sdf_host[first + b]});
      const hipError_t moved = DownloadToHostArrays(ctx, copies, n * sizeof(float), s);  // (synchronises the stream)
      if (moved != hipSuccess) (void)hipStreamSynchronize(s);
      VGT_TRY_HIP(moved, "copy SDF to host");
    }
    for (int64_t b = 0; b < count; b++)
    {
      if (out_min) out_min[first + b] = mm[static_cast<size_t>(2 * b)];
      if (out_max) out_max[first + b] = mm[static_cast<size_t>(2 * b + 1)];
    }
  }
  return VGT_HIP_OK;
}

int vgt_hip_sdf_dev_timed(vgt_hip_ctx* ctx, const float* occupancy_dev, int64_t nx, int64_t ny,
                          int64_t nz, double resolution, int unknown_is_filled,
                          int add_virtual_border, float* sdf_dev, void* workspace_dev,
                          size_t workspace_bytes, float* minmax_dev, float* kernel_ms)
{
  if (!ctx || !occupancy_dev || !sdf_dev || !kernel_ms)
    return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "null argument");
  const int rc = CheckSdfShape(nx, ny, nz, resolution);
  if (rc != VGT_HIP_OK) return rc;
  VGT_TRY_HIP(hipSetDevice(ctx->device), "set device");
  const vgt::SdfParams p{nx, ny, nz, resolution, unknown_is_filled ? 1 : 0,
                         add_virtual_border ? 1 : 0};
  hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
  int result = VGT_HIP_OK;
  for (int i = 0; i < 4 && result == VGT_HIP_OK; i++)
  {
    const hipError_t err = hipEventCreate(&ev[i]);
    if (err != hipSuccess) result = FailHip("create event", err);
  }
  if (result == VGT_HIP_OK)
  {
    std::lock_guard<std::mutex> lock(ctx->mutex);
    result = RunSdfPipeline<float>(ctx, occupancy_dev, p, sdf_dev, workspace_dev, workspace_bytes,
                                   minmax_dev, ev);
    const hipError_t err = hipStreamSynchronize(ctx->stream);
    if (result == VGT_HIP_OK && err != hipSuccess) result = FailHip("synchronize", err);
    for (int i = 0; i < 3 && result == VGT_HIP_OK; i++)
    {
      const hipError_t terr = hipEventElapsedTime(&kernel_ms[i], ev[i], ev[i + 1]);
      if (terr != hipSuccess) result = FailHip("event elapsed", terr);
    }
  }
  for (int i = 0; i < 4; i++)
    if (ev[i]) (void)hipEventDestroy(ev[i]);
  return result;
}

/* ------------------------------ multi-GPU Z slabs ----------------------------- */

/* ------------------- SDFs of the map types with tagged cells ------------------- */

namespace
{
static int CheckCells(const vgt_hip_ctx* ctx, const vgt_hip_cells* cells)
{
  if (!ctx || !cells) return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "null argument");
  if (cells->ctx != ctx) return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "cells belong to another context");
  return VGT_HIP_OK;
}

// mask (mode, objects) -> signed distance field in `sdf_dev`, extrema in ctx->minmax_out.
// Caller holds the context mutex.
static int RunCellsSdf(vgt_hip_ctx* ctx, vgt_hip_cells* c, int mode, int num_objects, const vgt::SdfParams& p,
                float* sdf_dev, float* minmax_dev = nullptr)  // (extrema: the context's two floats unless told otherwise)
{
  const int64_t n = c->nx * c->ny * c->nz;
  VGT_TRY_HIP(vgt::LaunchCellMask(c->records.as<void>(), n, c->cell_bytes, c->object_id_offset, mode,
                                  c->objects.as<uint32_t>(), num_objects, p.unknown_is_filled, c->mask.as<uint8_t>(),
                                  ctx->stream),
              "cell predicate");
  vgt::SdfParams mask_params = p;
  mask_params.unknown_is_filled = 0;
  // (the workspace was sized for the default pipeline: the cross-check, selected later, needs more)
  const size_t need = CarveWorkspace(nullptr, c->nx, c->ny, c->nz, ctx->variant).bytes;
  if (need > c->workspace.bytes())
  {
    VGT_TRY_HIP(hipStreamSynchronize(ctx->stream), "synchronize");
    VGT_TRY_HIP(c->workspace.Reserve(need), "allocate SDF workspace");
  }
  return RunSdfPipeline<uint8_t>(ctx, c->mask.as<uint8_t>(), mask_params, sdf_dev, c->workspace.data(),
                                 c->workspace.bytes(), minmax_dev ? minmax_dev : ctx->minmax_out.as<float>(), nullptr);
}

// A field of the context's stream into a host array (usually one the caller has just allocated) + the extrema.  The
// kernels that produce it are enqueued, not finished: preparing the array overlaps them.  Large arrays are faulted in
// by a few threads and page-locked for one DMA; medium ones cross through the context's page-locked ring
// (DownloadToHostArrays: locking fresh pages costs more than the copy); small ones take the runtime's pageable path.
static int CopySdfToHost(vgt_hip_ctx* ctx, const float* sdf_dev, int64_t n, float* sdf_host, float* out_min,
                  float* out_max)
{
  float mm[2] = {0.0f, 0.0f};
  const float* const minmax_dev = ctx->minmax_out.as<float>();
  const size_t bytes = static_cast<size_t>(n) * sizeof(float);
  hipError_t err = hipSuccess;
  if (bytes >= (size_t{32} << 20))
  {
    vgt::HostRangePopulator fresh(sdf_host, bytes);
    fresh.Wait();
    const ScopedHostPin pin(sdf_host, bytes);
    err = hipMemcpyAsync(sdf_host, sdf_dev, bytes, hipMemcpyDeviceToHost, ctx->stream);
    if (err == hipSuccess) err = hipMemcpyAsync(mm, minmax_dev, sizeof(mm), hipMemcpyDeviceToHost, ctx->stream);
    err = DrainKeepingFirst(ctx->stream, err);  // (before the array is unlocked, whatever happened)
  }
  else if (bytes >= (size_t{1} << 20))
  {
    err = hipMemcpyAsync(mm, minmax_dev, sizeof(mm), hipMemcpyDeviceToHost, ctx->stream);
    if (err == hipSuccess)
      err = DownloadToHostArrays(ctx, {HostArrayCopy{sdf_dev, sdf_host}}, bytes, ctx->stream);  // (synchronises)
    if (err != hipSuccess) (void)hipStreamSynchronize(ctx->stream);  // (`mm` is on this stack)
  }
  else
  {
    err = hipMemcpyAsync(sdf_host, sdf_dev, bytes, hipMemcpyDeviceToHost, ctx->stream);
    if (err == hipSuccess) err = hipMemcpyAsync(mm, minmax_dev, sizeof(mm), hipMemcpyDeviceToHost, ctx->stream);
    if (err == hipSuccess) err = hipStreamSynchronize(ctx->stream);
  }
  if (err != hipSuccess) return FailHip("copy SDF to host", err);
  if (out_min) *out_min = mm[0];
  if (out_max) *out_max = mm[1];
  return VGT_HIP_OK;
}
}  // namespace

int vgt_hip_cells_create(vgt_hip_ctx* ctx, const void* cells_host, int64_t nx, int64_t ny, int64_t nz,
                         int32_t cell_bytes, int32_t object_id_offset, vgt_hip_cells** out_cells)
{
  if (!ctx || !cells_host || !out_cells) return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "null argument");
  *out_cells = nullptr;
  const int rc = CheckSdfShape(nx, ny, nz, 1.0);
  if (rc != VGT_HIP_OK) return rc;
  if (cell_bytes < 4 || cell_bytes % 4 != 0 || cell_bytes > 64)
    return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "cell records must be 4..64 bytes, a multiple of 4");
  if (object_id_offset != -1 &&
      (object_id_offset < 4 || object_id_offset % 4 != 0 || object_id_offset + 4 > cell_bytes))
    return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "object id offset outside the cell record");
  VGT_TRY_HIP(hipSetDevice(ctx->device), "set device");
  std::unique_ptr<vgt_hip_cells> c(new (std::nothrow) vgt_hip_cells());
  if (!c) return Fail(VGT_HIP_ERR_RUNTIME, "out of host memory");
  c->ctx = ctx;
  c->device = ctx->device;
  c->nx = nx;
  c->ny = ny;
  c->nz = nz;
  c->cell_bytes = cell_bytes;
  c->object_id_offset = object_id_offset;
  const size_t n = static_cast<size_t>(nx * ny * nz);
  VGT_TRY_HIP(c->records.Allocate(n * static_cast<size_t>(cell_bytes)), "upload cell records");
  VGT_TRY_HIP(c->mask.Allocate(n), "upload cell records");
  VGT_TRY_HIP(c->sdf.Allocate(n * sizeof(float)), "upload cell records");
  VGT_TRY_HIP(c->workspace.Reserve(vgt_hip_sdf_workspace_bytes(nx, ny, nz)), "upload cell records");
  VGT_TRY_HIP(c->scalar.Allocate(2 * sizeof(uint32_t)), "upload cell records");
  {
    std::lock_guard<std::mutex> lock(ctx->mutex);
    VGT_TRY_HIP(hipMemcpyAsync(c->records.as<void>(), cells_host, n * static_cast<size_t>(cell_bytes),
                               hipMemcpyHostToDevice, ctx->stream),
                "upload cell records");
    VGT_TRY_HIP(hipStreamSynchronize(ctx->stream), "upload cell records");
  }
  AdoptChild(ctx);
  *out_cells = c.release();
  return VGT_HIP_OK;
}

void vgt_hip_cells_destroy(vgt_hip_cells* cells)
{
  if (!cells) return;
  ReleaseChild(cells->ctx, cells->device);
  delete cells;
}

int vgt_hip_cells_object_ids(vgt_hip_ctx* ctx, vgt_hip_cells* cells, uint32_t* ids_out, int64_t capacity,
                             int64_t* count)
{
  const int rc = CheckCells(ctx, cells);
  if (rc != VGT_HIP_OK) return rc;
  if (!count || capacity < 0 || (capacity > 0 && !ids_out))
    return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "invalid id buffer");
  *count = 0;
  if (cells->object_id_offset < 0) return VGT_HIP_OK;  // this map type has no object ids
  VGT_TRY_HIP(hipSetDevice(ctx->device), "set device");
  std::lock_guard<std::mutex> lock(ctx->mutex);
  const int64_t n = cells->nx * cells->ny * cells->nz;
  // One pass: every id goes into a device hash set, the set is compacted and sorted on the host (the reference
  // collects a std::set, tagged_object_occupancy_map.hpp:268-289).  Only a grid with more distinct ids than the
  // table can hold falls back to the one-id-per-launch scan.
  // Tagged maps usually hold a handful of ids: a 2^16-slot table (0.5 MiB) serves them; only when it overflows is the
  // table sized for the worst case (two slots per cell, up to 2^27 slots = 1 GiB).
  int full_log2 = 10;
  while (full_log2 < 27 && (int64_t{1} << full_log2) < 2 * n) full_log2++;
  const int attempts[2] = {std::min(16, full_log2), full_log2};
  for (int attempt = 0; attempt < 2; attempt++)
  {
    if (attempt == 1 && attempts[1] == attempts[0]) break;
    const int kTableLog2 = attempts[attempt];
    const size_t slots = size_t{1} << kTableLog2;
    vgt::DeviceTemp table_dev;  // (freed under the context's mutex, like the scan it serves)
    if (table_dev.Allocate((2 * slots + 64) * sizeof(uint32_t)) != hipSuccess)
    {
      (void)hipGetLastError();
      continue;
    }
    uint32_t* table = table_dev.as<uint32_t>();
    uint32_t* ids_dev = table + slots;
    uint32_t* count_overflow = ids_dev + slots;
    uint32_t header[2] = {0u, 1u};
    std::vector<uint32_t> ids;
    hipError_t err = hipMemsetAsync(table, 0, (2 * slots + 64) * sizeof(uint32_t), ctx->stream);
    if (err == hipSuccess)
      err = vgt::LaunchDistinctObjectIds(cells->records.as<void>(), n, cells->cell_bytes, cells->object_id_offset, table,
                                         kTableLog2, ids_dev, count_overflow, ctx->stream);
    if (err == hipSuccess)
      err = hipMemcpyAsync(header, count_overflow, sizeof(header), hipMemcpyDeviceToHost, ctx->stream);
    err = DrainKeepingFirst(ctx->stream, err);
    if (err == hipSuccess && header[1] == 0u && header[0] > 0u)
    {
      ids.resize(header[0]);
      err = hipMemcpy(ids.data(), ids_dev, ids.size() * sizeof(uint32_t), hipMemcpyDeviceToHost);
    }
    VGT_TRY_HIP(err, "object id scan");
    if (header[1] == 0u)
    {
      std::sort(ids.begin(), ids.end());
      *count = static_cast<int64_t>(ids.size());
      for (int64_t k = 0; k < *count && k < capacity; k++) ids_out[k] = ids[static_cast<size_t>(k)];
      return VGT_HIP_OK;
    }
  }
  uint32_t after = 0;  // ids > 0 only (tagged_object_occupancy_map.hpp:279-283)
  for (;;)
  {
    const uint32_t init[2] = {0xffffffffu, 0u};
    uint32_t* const scalar = cells->scalar.as<uint32_t>();
    VGT_TRY_HIP(hipMemcpyAsync(scalar, init, sizeof(init), hipMemcpyHostToDevice, ctx->stream), "reset id scan");
    VGT_TRY_HIP(vgt::LaunchNextObjectId(cells->records.as<void>(), n, cells->cell_bytes, cells->object_id_offset, after,
                                        scalar, ctx->stream),
                "object id scan");
    uint32_t next[2] = {0u, 0u};
    VGT_TRY_HIP(hipMemcpyAsync(next, scalar, sizeof(next), hipMemcpyDeviceToHost, ctx->stream),
                "read id scan");
    VGT_TRY_HIP(hipStreamSynchronize(ctx->stream), "id scan");
    if (!next[1]) break;
    if (*count < capacity) ids_out[*count] = next[0];
    (*count)++;
    after = next[0];
    if (after == 0xffffffffu) break;
  }
  return VGT_HIP_OK;
}

int vgt_hip_cells_sdf(vgt_hip_ctx* ctx, vgt_hip_cells* cells, const uint32_t* objects_to_use,
                      int64_t num_objects, double resolution, int unknown_is_filled, int add_virtual_border,
                      float* sdf_host, float* out_min, float* out_max)
{
  int rc = CheckCells(ctx, cells);
  if (rc != VGT_HIP_OK) return rc;
  if (!sdf_host || num_objects < 0 || (num_objects > 0 && !objects_to_use))
    return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "null argument");
  if (num_objects > 0 && cells->object_id_offset < 0)
    return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "this cell type carries no object id");
  rc = CheckSdfShape(cells->nx, cells->ny, cells->nz, resolution);
  if (rc != VGT_HIP_OK) return rc;
  VGT_TRY_HIP(hipSetDevice(ctx->device), "set device");
  // the reference looks the ids up in a std::set (tagged_object_occupancy_map.hpp:206-211)
  std::vector<uint32_t> objects(objects_to_use, objects_to_use + num_objects);
  std::sort(objects.begin(), objects.end());
  objects.erase(std::unique(objects.begin(), objects.end()), objects.end());
  std::lock_guard<std::mutex> lock(ctx->mutex);
  rc = GrowCache(ctx->stream, &cells->objects, objects.size() * sizeof(uint32_t), "drain before regrowing object list",
                 "allocate object list");
  if (rc != VGT_HIP_OK) return rc;
  if (!objects.empty())
  {
    VGT_TRY_HIP(hipMemcpyAsync(cells->objects.data(), objects.data(), objects.size() * sizeof(uint32_t),
                               hipMemcpyHostToDevice, ctx->stream),
                "upload object list");
    // `objects` is pageable host memory: the copy has been staged when the call returns
  }
  const vgt::SdfParams p{cells->nx, cells->ny, cells->nz, resolution, unknown_is_filled ? 1 : 0,
                         add_virtual_border ? 1 : 0};
  const size_t n = static_cast<size_t>(cells->nx * cells->ny * cells->nz);
  if (n * sizeof(float) <= (size_t{1} << 19) && EnsureStaging(ctx) == hipSuccess)
  {
    // a small field: the X pass writes it, and the extrema behind it, straight into the context's page-locked ring
    // (as SdfFromHost does for small maps: no download, one wait, one memcpy)
    float* const field = reinterpret_cast<float*>(static_cast<char*>(ctx->host_staging) + kStagingSlotBytes);
    rc = RunCellsSdf(ctx, cells, objects.empty() ? 0 : 1, static_cast<int>(objects.size()), p, field, field + n);
    const hipError_t err = hipStreamSynchronize(ctx->stream);
    if (rc == VGT_HIP_OK && err != hipSuccess) rc = FailHip("small tagged-map SDF extraction", err);
    if (rc != VGT_HIP_OK) return rc;
    std::memcpy(sdf_host, field, n * sizeof(float));
    if (out_min) *out_min = field[n];
    if (out_max) *out_max = field[n + 1];
    return VGT_HIP_OK;
  }
  rc = RunCellsSdf(ctx, cells, objects.empty() ? 0 : 1, static_cast<int>(objects.size()), p, cells->sdf.as<float>());
  if (rc != VGT_HIP_OK)
  {
    (void)hipStreamSynchronize(ctx->stream);
    return rc;
  }
  return CopySdfToHost(ctx, cells->sdf.as<float>(), cells->nx * cells->ny * cells->nz, sdf_host, out_min, out_max);
}

int vgt_hip_cells_object_sdfs(vgt_hip_ctx* ctx, vgt_hip_cells* cells, const uint32_t* object_ids,
                              int64_t num_objects, double resolution, int unknown_is_filled, int add_virtual_border,
                              float* const* sdf_host, float* out_min, float* out_max)
{
  int rc = CheckCells(ctx, cells);
  if (rc != VGT_HIP_OK) return rc;
  if (num_objects < 0 || (num_objects > 0 && (!object_ids || !sdf_host)))
    return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "null argument");
  if (num_objects > 0 && cells->object_id_offset < 0)
    return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "this cell type carries no object id");
  for (int64_t b = 0; b < num_objects; b++)
    if (!sdf_host[b]) return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "null field in the batch");
  rc = CheckSdfShape(cells->nx, cells->ny, cells->nz, resolution);
  if (rc != VGT_HIP_OK) return rc;
  if (num_objects == 0) return VGT_HIP_OK;
  VGT_TRY_HIP(hipSetDevice(ctx->device), "set device");
  const int64_t nx = cells->nx, ny = cells->ny, nz = cells->nz;
  const size_t n = static_cast<size_t>(nx * ny * nz);
  // Objects per launch: what the limits of a batch and a memory budget allow (9.25 bytes per voxel and object: mask,
  // intermediate field, field, records).
  const int64_t group = BatchGroup(num_objects, nx, ny, nz, size_t{4} << 30, n * 10);
  std::lock_guard<std::mutex> lock(ctx->mutex);
  if (ctx->variant != 0)
    return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "batches run on the default EDT pipeline only");
  hipStream_t s = ctx->stream;
  const size_t ws_bytes = CarveWorkspace(nullptr, nx, ny, nz, ctx->variant, group).bytes;
  const size_t sdf_bytes = static_cast<size_t>(group) * (n + 2) * sizeof(float);
  const size_t ids_bytes = static_cast<size_t>(group) * sizeof(uint32_t);
  if (cells->batch_masks.bytes() < static_cast<size_t>(group) * n || cells->batch_sdf.bytes() < sdf_bytes ||
      cells->batch_ws.bytes() < ws_bytes || cells->objects.bytes() < ids_bytes)
    VGT_TRY_HIP(hipStreamSynchronize(s), "drain before regrowing the batch buffers");
  VGT_TRY_HIP(cells->batch_masks.Reserve(static_cast<size_t>(group) * n), "allocate masks");
  VGT_TRY_HIP(cells->batch_sdf.Reserve(sdf_bytes), "allocate fields");
  VGT_TRY_HIP(cells->batch_ws.Reserve(ws_bytes), "allocate SDF workspace");
  VGT_TRY_HIP(cells->objects.Reserve(ids_bytes), "allocate object list");
  uint32_t* const ids_dev = cells->objects.as<uint32_t>();
  uint8_t* const masks_dev = cells->batch_masks.as<uint8_t>();
  float* const sdf_dev = cells->batch_sdf.as<float>();
  float* const mm_dev = sdf_dev + static_cast<size_t>(group) * n;
  std::vector<float> mm(static_cast<size_t>(group) * 2);
  for (int64_t first = 0; first < num_objects; first += group)
  {
    const int64_t count = num_objects - first < group ? num_objects - first : group;
    // (pageable source: staged when the call returns)
    VGT_TRY_HIP(hipMemcpyAsync(ids_dev, object_ids + first, static_cast<size_t>(count) * sizeof(uint32_t),
                               hipMemcpyHostToDevice, s),
                "upload object ids");
    VGT_TRY_HIP(vgt::LaunchCellObjectMasks(cells->records.as<void>(), static_cast<int64_t>(n), cells->cell_bytes,
                                           cells->object_id_offset, ids_dev, static_cast<int>(count),
                                           unknown_is_filled ? 1 : 0, masks_dev, s),
                "object masks");
    vgt::SdfParams p{nx, ny, nz, resolution, 0, add_virtual_border ? 1 : 0};
    p.batch = count;
    rc = RunSdfPipeline<uint8_t>(ctx, masks_dev, p, sdf_dev, cells->batch_ws.data(), cells->batch_ws.bytes(), mm_dev,
                                 nullptr);
    if (rc != VGT_HIP_OK)
    {
      (void)hipStreamSynchronize(s);
      return rc;
    }
    {
      // the fields go through the context's page-locked ring and on into the callers' arrays on several threads
      std::vector<HostArrayCopy> copies;
      for (int64_t b = 0; b < count; b++) copies.push_back(HostArrayCopy{sdf_dev + static_cast<size_t>(b) * n, sdf_host[first + b]});
      hipError_t err = hipMemcpyAsync(mm.data(), mm_dev, static_cast<size_t>(count) * 2 * sizeof(float), hipMemcpyDeviceToHost, s);
      const hipError_t moved = DownloadToHostArrays(ctx, copies, n * sizeof(float), s);  // (synchronises the stream)
      if (err == hipSuccess) err = moved;
      if (err != hipSuccess) (void)hipStreamSynchronize(s);
      VGT_TRY_HIP(err, "copy the objects' fields to the host");
    }
    for (int64_t b = 0; b < count; b++)
    {
      if (out_min) out_min[first + b] = mm[static_cast<size_t>(2 * b)];
      if (out_max) out_max[first + b] = mm[static_cast<size_t>(2 * b + 1)];
    }
  }
  return VGT_HIP_OK;
}

namespace
{
// ExtractFreeAndNamedObjectsSignedDistanceField into cells->sdf (extrema in ctx->minmax_out); cells->sdf_named exists.
// Caller holds the context mutex.
int RunFreeAndNamedSdf(vgt_hip_ctx* ctx, vgt_hip_cells* cells, const vgt::SdfParams& p)
{
  const int64_t n = cells->nx * cells->ny * cells->nz;
  float* const sdf = cells->sdf.as<float>();
  float* const sdf_named = cells->sdf_named.as<float>();
  int rc = RunCellsSdf(ctx, cells, 0, 0, p, sdf);                      // free-space field: every filled cell
  if (rc == VGT_HIP_OK) rc = RunCellsSdf(ctx, cells, 2, 0, p, sdf_named);  // cells of named objects only
  if (rc == VGT_HIP_OK)
  {
    uint32_t* enc = CarveWorkspace(cells->workspace.data(), cells->nx, cells->ny, cells->nz, ctx->variant).minmax_enc;
    hipError_t err = vgt::LaunchInitMinMax(enc, ctx->stream);
    if (err == hipSuccess) err = vgt::LaunchCombineFreeAndNamed(sdf, sdf_named, n, sdf, enc, ctx->stream);
    if (err == hipSuccess) err = vgt::LaunchDecodeMinMax(enc, ctx->minmax_out.as<float>(), ctx->stream);
    if (err != hipSuccess) rc = FailHip("combine fields", err);
  }
  return rc;
}
}  // namespace

int vgt_hip_cells_free_and_named_objects_sdf(vgt_hip_ctx* ctx, vgt_hip_cells* cells, double resolution,
                                             int unknown_is_filled, int add_virtual_border, float* sdf_host,
                                             float* out_min, float* out_max)
{
  int rc = CheckCells(ctx, cells);
  if (rc != VGT_HIP_OK) return rc;
  if (!sdf_host) return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "null argument");
  if (cells->object_id_offset < 0)
    return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "this cell type carries no object id");
  rc = CheckSdfShape(cells->nx, cells->ny, cells->nz, resolution);
  if (rc != VGT_HIP_OK) return rc;
  VGT_TRY_HIP(hipSetDevice(ctx->device), "set device");
  const int64_t n = cells->nx * cells->ny * cells->nz;
  std::lock_guard<std::mutex> lock(ctx->mutex);
  VGT_TRY_HIP(cells->sdf_named.Reserve(static_cast<size_t>(n) * sizeof(float)), "allocate second SDF");
  const vgt::SdfParams p{cells->nx, cells->ny, cells->nz, resolution, unknown_is_filled ? 1 : 0,
                         add_virtual_border ? 1 : 0};
  rc = RunFreeAndNamedSdf(ctx, cells, p);
  if (rc != VGT_HIP_OK)
  {
    (void)hipStreamSynchronize(ctx->stream);
    return rc;
  }
  return CopySdfToHost(ctx, cells->sdf.as<float>(), n, sdf_host, out_min, out_max);
}

/* ------------------------------ deferred timing ------------------------------ */

namespace
{
static void ReleaseTiming(vgt_hip_ctx* ctx)
{
  for (hipEvent_t e : ctx->timing_events)
    if (e) (void)hipEventDestroy(e);
  ctx->timing_events.clear();
  ctx->timing_kind.clear();
  ctx->timing_slots = 0;
  ctx->timing_used = 0;
}
}  // namespace

int vgt_hip_timing_start(vgt_hip_ctx* ctx, int32_t max_calls)
{
  if (!ctx || max_calls <= 0 || max_calls > 4096)
    return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "invalid timing capacity");
  VGT_TRY_HIP(hipSetDevice(ctx->device), "set device");
  std::lock_guard<std::mutex> lock(ctx->mutex);
  ReleaseTiming(ctx);
  ctx->timing_events.assign(static_cast<size_t>(max_calls) * 8, nullptr);
  ctx->timing_kind.assign(static_cast<size_t>(max_calls), 0);
  for (hipEvent_t& e : ctx->timing_events)
  {
    const hipError_t err = hipEventCreate(&e);
    if (err != hipSuccess)
    {
      ReleaseTiming(ctx);
      return FailHip("create event", err);
    }
  }
  ctx->timing_slots = max_calls;
  return VGT_HIP_OK;
}

int vgt_hip_timing_stop(vgt_hip_ctx* ctx, float* kernel_ms, int32_t* num_calls)
{
  if (!ctx || !kernel_ms || !num_calls) return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "null argument");
  VGT_TRY_HIP(hipSetDevice(ctx->device), "set device");
  std::lock_guard<std::mutex> lock(ctx->mutex);
  hipError_t err = hipStreamSynchronize(ctx->stream);
  *num_calls = ctx->timing_used;
  for (int i = 0; i < ctx->timing_used && err == hipSuccess; i++)
  {
    hipEvent_t* e = &ctx->timing_events[static_cast<size_t>(i) * 8];
    float* out = kernel_ms + 3 * i;
    float fix = 0.0f;
    if (ctx->timing_kind[static_cast<size_t>(i)] == 1)
    {
      err = hipEventElapsedTime(&out[0], e[0], e[1]);
      if (err == hipSuccess) err = hipEventElapsedTime(&out[1], e[1], e[2]);
      if (err == hipSuccess) err = hipEventElapsedTime(&out[2], e[2], e[3]);
    }
    else
    {
      err = hipEventElapsedTime(&out[0], e[0], e[1]);
      if (err == hipSuccess) err = hipEventElapsedTime(&fix, e[4], e[5]);
      if (err == hipSuccess) err = hipEventElapsedTime(&out[1], e[5], e[6]);
      if (err == hipSuccess) err = hipEventElapsedTime(&out[2], e[6], e[7]);
      out[0] += fix;  // the slab fix-up belongs to the Z pass
    }
  }
  ReleaseTiming(ctx);
  VGT_TRY_HIP(err, "read kernel timing");
  return VGT_HIP_OK;
}

/* ------------------------------- SDF consumers ------------------------------- */

int vgt_hip_sdf_coarse_gradient_dev(vgt_hip_ctx* ctx, const float* sdf_dev, int64_t nx, int64_t ny, int64_t nz,
                                    double resolution, int enable_edge_gradients, const double* rotation,
                                    double* gradient_dev, uint8_t* has_value_dev)
{
  if (!ctx || !sdf_dev || !gradient_dev) return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "null argument");
  const int rc = CheckSdfShape(nx, ny, nz, resolution);
  if (rc != VGT_HIP_OK) return rc;
  VGT_TRY_HIP(hipSetDevice(ctx->device), "set device");
  std::lock_guard<std::mutex> lock(ctx->mutex);
  VGT_TRY_HIP(vgt::LaunchCoarseGradient(sdf_dev, nx, ny, nz, resolution, enable_edge_gradients ? 1 : 0, rotation,
                                        gradient_dev, has_value_dev, ctx->stream),
              "coarse gradient");
  return VGT_HIP_OK;
}

int vgt_hip_sdf_coarse_gradient(vgt_hip_ctx* ctx, const float* sdf_host, int64_t nx, int64_t ny, int64_t nz,
                                double resolution, int enable_edge_gradients, const double* rotation,
                                double* gradient_host, uint8_t* has_value_host)
{
  if (!ctx || !sdf_host || !gradient_host) return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "null argument");
  const int rc = CheckSdfShape(nx, ny, nz, resolution);
  if (rc != VGT_HIP_OK) return rc;
  VGT_TRY_HIP(hipSetDevice(ctx->device), "set device");
  const size_t n = static_cast<size_t>(nx * ny * nz);
  vgt::HostStaging staging;
  const auto sdf = staging.In(sdf_host, n);
  const auto gradient = staging.Out(gradient_host, n * 3);
  const auto has = staging.Out(has_value_host, n);
  return staging.Run(*ctx, "coarse gradient", FailHip, [&](hipStream_t s) {
    return HipResult("coarse gradient",
                     vgt::LaunchCoarseGradient(sdf.dev(), nx, ny, nz, resolution, enable_edge_gradients ? 1 : 0, rotation,
                                               gradient.dev(), has.dev(), s));
  });
}

int vgt_hip_sdf_estimate_distance_dev(vgt_hip_ctx* ctx, const float* sdf_dev, int64_t nx, int64_t ny, int64_t nz,
                                      double resolution, const double* grid_from_world, const double* query_xyz_dev,
                                      int64_t num_queries, double* distance_dev, uint8_t* has_value_dev)
{
  if (!ctx || !sdf_dev || !distance_dev || num_queries < 0 || (num_queries > 0 && !query_xyz_dev))
    return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "null argument");
  const int rc = CheckSdfShape(nx, ny, nz, resolution);
  if (rc != VGT_HIP_OK) return rc;
  VGT_TRY_HIP(hipSetDevice(ctx->device), "set device");
  std::lock_guard<std::mutex> lock(ctx->mutex);
  VGT_TRY_HIP(vgt::LaunchEstimateDistance(sdf_dev, nx, ny, nz, resolution, grid_from_world, query_xyz_dev, num_queries,
                                          distance_dev, has_value_dev, ctx->stream),
              "estimate distance");
  return VGT_HIP_OK;
}

int vgt_hip_sdf_estimate_distance(vgt_hip_ctx* ctx, const float* sdf_host, int64_t nx, int64_t ny, int64_t nz,
                                  double resolution, const double* grid_from_world, const double* query_xyz_host,
                                  int64_t num_queries, double* distance_host, uint8_t* has_value_host)
{
  return SdfQueriesHost(ctx, sdf_host, nx, ny, nz, resolution, query_xyz_host, num_queries, 1, distance_host,
                        has_value_host, "estimate distance",
                        [&](const float* sdf_dev, const double* queries_dev, double* out_dev, uint8_t* has_dev,
                            uint32_t*, hipStream_t s) {
                          return vgt::LaunchEstimateDistance(sdf_dev, nx, ny, nz, resolution, grid_from_world,
                                                             queries_dev, num_queries, out_dev, has_dev, s);
                        });
}

int vgt_hip_sdf_fine_gradient(vgt_hip_ctx* ctx, const float* sdf_host, int64_t nx, int64_t ny, int64_t nz,
                              double resolution, const double* grid_from_world, const double* query_xyz_host,
                              int64_t num_queries, double nominal_window_size, double* gradient_host,
                              uint8_t* has_value_host)
{
  if (!std::isfinite(nominal_window_size) || nominal_window_size == 0.0)
    return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "the fine-gradient window must be finite and non-zero");
  return SdfQueriesHost(ctx, sdf_host, nx, ny, nz, resolution, query_xyz_host, num_queries, 3, gradient_host,
                        has_value_host, "fine gradient",
                        [&](const float* sdf_dev, const double* queries_dev, double* out_dev, uint8_t* has_dev,
                            uint32_t* flag_dev, hipStream_t s) {
                          return vgt::LaunchFineGradient(sdf_dev, nx, ny, nz, resolution, grid_from_world, queries_dev,
                                                         num_queries, nominal_window_size, out_dev, has_dev, flag_dev,
                                                         s);
                        });
}

int vgt_hip_sdf_project_out_of_collision_dev(vgt_hip_ctx* ctx, const float* sdf_dev, int64_t nx, int64_t ny, int64_t nz,
                                             double resolution, const double* grid_from_world, const double* rotation,
                                             const double* query_xyz_dev, int64_t num_queries, double minimum_distance,
                                             double stepsize_multiplier, int32_t max_iterations, double* position_dev,
                                             uint8_t* has_value_dev, uint8_t* status_dev, int32_t* iterations_dev)
{
  if (!ctx || !sdf_dev || !position_dev || num_queries < 0 || (num_queries > 0 && !query_xyz_dev))
    return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "null argument");
  const int rc = CheckProjectionArguments(nx, ny, nz, resolution, minimum_distance, stepsize_multiplier, max_iterations);
  if (rc != VGT_HIP_OK) return rc;
  VGT_TRY_HIP(hipSetDevice(ctx->device), "set device");
  std::lock_guard<std::mutex> lock(ctx->mutex);
  VGT_TRY_HIP(vgt::LaunchProjectOutOfCollision(sdf_dev, nx, ny, nz, resolution, grid_from_world, rotation, query_xyz_dev,
                                               num_queries, minimum_distance, stepsize_multiplier, max_iterations,
                                               position_dev, has_value_dev, status_dev, iterations_dev, ctx->stream),
              "project out of collision");
  return VGT_HIP_OK;
}

int vgt_hip_sdf_project_out_of_collision(vgt_hip_ctx* ctx, const float* sdf_host, int64_t nx, int64_t ny, int64_t nz,
                                         double resolution, const double* grid_from_world, const double* rotation,
                                         const double* query_xyz_host, int64_t num_queries, double minimum_distance,
                                         double stepsize_multiplier, int32_t max_iterations, double* position_host,
                                         uint8_t* has_value_host, uint8_t* status_host, int32_t* iterations_host)
{
  if (!ctx || !sdf_host || !position_host || num_queries < 0 || (num_queries > 0 && !query_xyz_host))
    return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "null argument");
  const int rc = CheckProjectionArguments(nx, ny, nz, resolution, minimum_distance, stepsize_multiplier, max_iterations);
  if (rc != VGT_HIP_OK) return rc;
  if (num_queries == 0) return VGT_HIP_OK;
  VGT_TRY_HIP(hipSetDevice(ctx->device), "set device");
  const char* what = "project out of collision";
  const size_t n = static_cast<size_t>(nx * ny * nz), q = static_cast<size_t>(num_queries);
  vgt::HostStaging staging;
  const auto sdf = staging.In(sdf_host, n);
  const auto queries = staging.In(query_xyz_host, q * 3);
  const auto position = staging.Out(position_host, q * 3);
  const auto has = staging.Out(has_value_host, q);
  const auto status = staging.Out(status_host, q);
  const auto iterations = staging.Out(iterations_host, q);
  return staging.Run(*ctx, what, FailHip, [&](hipStream_t s) {
    return HipResult(what, vgt::LaunchProjectOutOfCollision(
                               sdf.dev(), nx, ny, nz, resolution, grid_from_world, rotation, queries.dev(), num_queries,
                               minimum_distance, stepsize_multiplier, max_iterations, position.dev(), has.dev(),
                               status.dev(), iterations.dev(), s));
  });
}

int vgt_hip_cast_segments_dev(vgt_hip_ctx* ctx, const float* field_dev, int64_t nx, int64_t ny, int64_t nz,
                              double resolution, int32_t mode, int unknown_is_filled, double threshold, uint32_t flags,
                              const double* grid_from_world, const double* segments_dev, int64_t num_segments,
                              uint8_t* status_dev, int32_t* hit_index_dev, double* hit_fraction_dev,
                              int32_t* cells_examined_dev, float* min_value_dev, int32_t* min_index_dev)
{
  vgt::SegmentGrid grid;
  vgt::SegmentQuery query;
  const int rc = CheckSegmentArguments(ctx, field_dev, nx, ny, nz, resolution, mode, unknown_is_filled, threshold, flags,
                                       grid_from_world, segments_dev, num_segments, status_dev, min_value_dev,
                                       min_index_dev, &grid, &query);
  if (rc != VGT_HIP_OK) return rc;
  if (num_segments == 0 || nx * ny * nz == 0) return VGT_HIP_OK;
  VGT_TRY_HIP(hipSetDevice(ctx->device), "set device");
  std::lock_guard<std::mutex> lock(ctx->mutex);
  const vgt::SegmentOutputs out{status_dev, hit_index_dev, hit_fraction_dev, cells_examined_dev, min_value_dev,
                                min_index_dev};
  VGT_TRY_HIP(vgt::LaunchCastSegments(field_dev, grid, query, segments_dev, num_segments, out, ctx->stream),
              "cast segments");
  return VGT_HIP_OK;
}

int vgt_hip_cast_segments(vgt_hip_ctx* ctx, const float* field_host, int64_t nx, int64_t ny, int64_t nz,
                          double resolution, int32_t mode, int unknown_is_filled, double threshold, uint32_t flags,
                          const double* grid_from_world, const double* segments_host, int64_t num_segments,
                          uint8_t* status_host, int32_t* hit_index_host, double* hit_fraction_host,
                          int32_t* cells_examined_host, float* min_value_host, int32_t* min_index_host)
{
  vgt::SegmentGrid grid;
  vgt::SegmentQuery query;
  const int rc = CheckSegmentArguments(ctx, field_host, nx, ny, nz, resolution, mode, unknown_is_filled, threshold, flags,
                                       grid_from_world, segments_host, num_segments, status_host, min_value_host,
                                       min_index_host, &grid, &query);
  if (rc != VGT_HIP_OK) return rc;
  if (num_segments == 0 || nx * ny * nz == 0) return VGT_HIP_OK;
  VGT_TRY_HIP(hipSetDevice(ctx->device), "set device");
  const char* what = "cast segments";
  const size_t n = static_cast<size_t>(nx * ny * nz), q = static_cast<size_t>(num_segments);
  vgt::HostStaging staging;
  const auto field = staging.In(field_host, n);
  const auto segments = staging.In(segments_host, q * 6);
  const auto status = staging.Out(status_host, q);
  const auto hit_index = staging.Out(hit_index_host, q);
  const auto hit_fraction = staging.Out(hit_fraction_host, q);
  const auto cells_examined = staging.Out(cells_examined_host, q);
  const auto min_value = staging.Out(min_value_host, q);
  const auto min_index = staging.Out(min_index_host, q);
  return staging.Run(*ctx, what, FailHip, [&](hipStream_t s) {
    const vgt::SegmentOutputs out{status.dev(),         hit_index.dev(), hit_fraction.dev(),
                                  cells_examined.dev(), min_value.dev(), min_index.dev()};
    return HipResult(what, vgt::LaunchCastSegments(field.dev(), grid, query, segments.dev(), num_segments, out, s));
  });
}

int vgt_hip_check_spheres_dev(vgt_hip_ctx* ctx, const float* sdf_dev, int64_t nx, int64_t ny, int64_t nz,
                              double resolution, const double* grid_from_world, const double* rotation,
                              const double* sphere_xyzr_dev, const int32_t* sphere_link_dev, int64_t num_spheres,
                              const double* link_poses_dev, int64_t num_links, int64_t num_configurations,
                              double minimum_clearance, uint32_t flags, uint8_t* status_dev, double* min_clearance_dev,
                              int32_t* min_sphere_dev, int32_t* num_below_dev, int32_t* num_outside_dev,
                              double* min_gradient_dev, double* sphere_clearance_dev, double* sphere_gradient_dev)
{
  const CheckSpheresArguments a{sdf_dev, nx, ny, nz, resolution, grid_from_world, rotation, sphere_xyzr_dev,
                                sphere_link_dev, num_spheres, link_poses_dev, num_links, num_configurations,
                                minimum_clearance, flags,
                                {status_dev, min_clearance_dev, min_sphere_dev, num_below_dev, num_outside_dev,
                                 min_gradient_dev, sphere_clearance_dev, sphere_gradient_dev}};
  const int rc = a.Check(ctx);
  if (rc != VGT_HIP_OK) return rc;
  if (num_configurations == 0) return VGT_HIP_OK;
  VGT_TRY_HIP(hipSetDevice(ctx->device), "set device");
  std::lock_guard<std::mutex> lock(ctx->mutex);
  // (no spheres, or an empty grid: the kernel writes NO_VALUE and reads neither the field nor the model)
  VGT_TRY_HIP(a.Launch(sdf_dev, sphere_xyzr_dev, sphere_link_dev, link_poses_dev, a.out, ctx->stream), "check spheres");
  return VGT_HIP_OK;
}

int vgt_hip_check_spheres(vgt_hip_ctx* ctx, const float* sdf_host, int64_t nx, int64_t ny, int64_t nz, double resolution,
                          const double* grid_from_world, const double* rotation, const double* sphere_xyzr_host,
                          const int32_t* sphere_link_host, int64_t num_spheres, const double* link_poses_host,
                          int64_t num_links, int64_t num_configurations, double minimum_clearance, uint32_t flags,
                          uint8_t* status_host, double* min_clearance_host, int32_t* min_sphere_host,
                          int32_t* num_below_host, int32_t* num_outside_host, double* min_gradient_host,
                          double* sphere_clearance_host, double* sphere_gradient_host)
{
  const CheckSpheresArguments a{sdf_host, nx, ny, nz, resolution, grid_from_world, rotation, sphere_xyzr_host,
                                sphere_link_host, num_spheres, link_poses_host, num_links, num_configurations,
                                minimum_clearance, flags,
                                {status_host, min_clearance_host, min_sphere_host, num_below_host, num_outside_host,
                                 min_gradient_host, sphere_clearance_host, sphere_gradient_host}};
  int rc = a.Check(ctx);
  if (rc == VGT_HIP_OK) rc = a.CheckModel();
  if (rc != VGT_HIP_OK) return rc;
  if (num_configurations == 0) return VGT_HIP_OK;
  const size_t b = static_cast<size_t>(num_configurations), s = static_cast<size_t>(num_spheres);
  if (num_spheres == 0 || a.NumCells() == 0)
  {
    // nothing is comparable: the answer needs no device
    const double nan = std::numeric_limits<double>::quiet_NaN();
    for (size_t i = 0; i < b; i++)
    {
      status_host[i] = (num_spheres > 0 && (flags & VGT_HIP_SPHERES_OUTSIDE_IS_COLLISION)) ? VGT_HIP_SPHERES_COLLISION
                                                                                            : VGT_HIP_SPHERES_NO_VALUE;
      if (min_clearance_host) min_clearance_host[i] = nan;
      if (min_sphere_host) min_sphere_host[i] = -1;
      if (num_below_host) num_below_host[i] = 0;
      if (num_outside_host) num_outside_host[i] = static_cast<int32_t>(num_spheres);
      for (int k = 0; k < 3 && min_gradient_host; k++) min_gradient_host[3 * i + static_cast<size_t>(k)] = nan;
    }
    for (size_t i = 0; i < b * s && sphere_clearance_host; i++) sphere_clearance_host[i] = nan;
    for (size_t i = 0; i < b * s * 3 && sphere_gradient_host; i++) sphere_gradient_host[i] = nan;
    return VGT_HIP_OK;
  }
  VGT_TRY_HIP(hipSetDevice(ctx->device), "set device");
  const char* what = "check spheres";
  // (twelve arrays, and a staging holds eight: the inputs in one, the outputs in a second one inside its body)
  vgt::HostStaging inputs;
  const auto sdf = inputs.In(sdf_host, static_cast<size_t>(a.NumCells()));
  const auto xyzr = inputs.In(sphere_xyzr_host, s * 4);
  const auto link = inputs.In(sphere_link_host, s);
  const auto poses = inputs.In(link_poses_host, b * static_cast<size_t>(num_links) * 16);
  return inputs.Run(*ctx, what, FailHip, [&](hipStream_t stream) {
    vgt::HostStaging outputs;
    const auto status = outputs.Out(status_host, b);
    const auto min_clearance = outputs.Out(min_clearance_host, b);
    const auto min_sphere = outputs.Out(min_sphere_host, b);
    const auto num_below = outputs.Out(num_below_host, b);
    const auto num_outside = outputs.Out(num_outside_host, b);
    const auto min_gradient = outputs.Out(min_gradient_host, b * 3);
    const auto sphere_clearance = outputs.Out(sphere_clearance_host, b * s);
    const auto sphere_gradient = outputs.Out(sphere_gradient_host, b * s * 3);
    return outputs.RunLocked(stream, what, FailHip, [&](hipStream_t) {
      const vgt::BodyOutputs out{status.dev(),      min_clearance.dev(), min_sphere.dev(),       num_below.dev(),
                                 num_outside.dev(), min_gradient.dev(),  sphere_clearance.dev(), sphere_gradient.dev()};
      return HipResult(what, a.Launch(sdf.dev(), xyzr.dev(), link.dev(), poses.dev(), out, stream));
    });
  });
}

int vgt_hip_rasterize_spheres_dev(vgt_hip_ctx* ctx, int64_t nx, int64_t ny, int64_t nz, double resolution,
                                  const double* grid_from_world, const double* sphere_xyzr_dev,
                                  const int32_t* sphere_link_dev, int64_t num_spheres, const double* link_poses_dev,
                                  int64_t num_links, int64_t num_configurations, double padding,
                                  int64_t first_configuration_base, uint32_t flags, int32_t* first_configuration_dev)
{
  const RasterizeSpheresArguments a{nx, ny, nz, resolution, grid_from_world,
                                    {sphere_xyzr_dev, sphere_link_dev, num_spheres, link_poses_dev, num_links,
                                     num_configurations, padding},
                                    first_configuration_base, flags, first_configuration_dev};
  const int rc = a.Check(ctx);
  if (rc != VGT_HIP_OK) return rc;
  // an empty grid, or nothing to lower in an array that is kept: nothing to do
  if (a.NumCells() == 0 || (a.Keep() && (num_spheres == 0 || num_configurations == 0))) return VGT_HIP_OK;
  VGT_TRY_HIP(hipSetDevice(ctx->device), "set device");
  std::lock_guard<std::mutex> lock(ctx->mutex);
  VGT_TRY_HIP(a.Launch(sphere_xyzr_dev, sphere_link_dev, link_poses_dev, first_configuration_dev, ctx->stream),
              "rasterize spheres");
  return VGT_HIP_OK;
}

int vgt_hip_rasterize_spheres(vgt_hip_ctx* ctx, int64_t nx, int64_t ny, int64_t nz, double resolution,
                              const double* grid_from_world, const double* sphere_xyzr_host,
                              const int32_t* sphere_link_host, int64_t num_spheres, const double* link_poses_host,
                              int64_t num_links, int64_t num_configurations, double padding,
                              int64_t first_configuration_base, uint32_t flags, int32_t* first_configuration_host)
{
  const RasterizeSpheresArguments a{nx, ny, nz, resolution, grid_from_world,
                                    {sphere_xyzr_host, sphere_link_host, num_spheres, link_poses_host, num_links,
                                     num_configurations, padding},
                                    first_configuration_base, flags, first_configuration_host};
  int rc = a.Check(ctx);
  if (rc == VGT_HIP_OK) rc = a.body.CheckModel();
  if (rc != VGT_HIP_OK) return rc;
  const size_t cells = static_cast<size_t>(a.NumCells());
  if (cells == 0) return VGT_HIP_OK;
  if (num_spheres == 0 || num_configurations == 0)
  {
    // nothing covers anything: the answer needs no device
    for (size_t i = 0; i < cells && !a.Keep(); i++) first_configuration_host[i] = -1;
    return VGT_HIP_OK;
  }
  VGT_TRY_HIP(hipSetDevice(ctx->device), "set device");
  const char* what = "rasterize spheres";
  const size_t b = static_cast<size_t>(num_configurations), s = static_cast<size_t>(num_spheres);
  vgt::HostStaging staging;
  const auto xyzr = staging.In(sphere_xyzr_host, s * 4);
  const auto link = staging.In(sphere_link_host, s);
  const auto poses = staging.In(link_poses_host, b * static_cast<size_t>(num_links) * 16);
  const auto first = a.Keep() ? staging.InOut(first_configuration_host, cells) : staging.Out(first_configuration_host, cells);
  return staging.Run(*ctx, what, FailHip, [&](hipStream_t stream) {
    return HipResult(what, a.Launch(xyzr.dev(), link.dev(), poses.dev(), first.dev(), stream));
  });
}

int vgt_hip_spheres_cover_points_dev(vgt_hip_ctx* ctx, const float* points_xyz_dev, int64_t num_points,
                                     const double* world_from_points, const double* sphere_xyzr_dev,
                                     const int32_t* sphere_link_dev, int64_t num_spheres, const double* link_poses_dev,
                                     int64_t num_links, int64_t num_configurations, double padding, uint32_t flags,
                                     int32_t* first_configuration_dev, int32_t* first_sphere_dev,
                                     float* filtered_xyz_dev)
{
  const CoverPointsArguments a{points_xyz_dev, num_points, world_from_points,
                               {sphere_xyzr_dev, sphere_link_dev, num_spheres, link_poses_dev, num_links,
                                num_configurations, padding},
                               flags, first_configuration_dev, first_sphere_dev, filtered_xyz_dev};
  const int rc = a.Check(ctx);
  if (rc != VGT_HIP_OK) return rc;
  if (num_points == 0) return VGT_HIP_OK;
  VGT_TRY_HIP(hipSetDevice(ctx->device), "set device");
  std::lock_guard<std::mutex> lock(ctx->mutex);
  // (no spheres or no configurations: the kernel writes -1 and the plain copy and reads neither the model nor the poses)
  VGT_TRY_HIP(a.Launch(points_xyz_dev, sphere_xyzr_dev, sphere_link_dev, link_poses_dev, first_configuration_dev,
                       first_sphere_dev, filtered_xyz_dev, ctx->stream),
              "spheres cover points");
  return VGT_HIP_OK;
}

int vgt_hip_spheres_cover_points(vgt_hip_ctx* ctx, const float* points_xyz_host, int64_t num_points,
                                 const double* world_from_points, const double* sphere_xyzr_host,
                                 const int32_t* sphere_link_host, int64_t num_spheres, const double* link_poses_host,
                                 int64_t num_links, int64_t num_configurations, double padding, uint32_t flags,
                                 int32_t* first_configuration_host, int32_t* first_sphere_host, float* filtered_xyz_host)
{
  const CoverPointsArguments a{points_xyz_host, num_points, world_from_points,
                               {sphere_xyzr_host, sphere_link_host, num_spheres, link_poses_host, num_links,
                                num_configurations, padding},
                               flags, first_configuration_host, first_sphere_host, filtered_xyz_host};
  int rc = a.Check(ctx);
  if (rc == VGT_HIP_OK) rc = a.body.CheckModel();
  if (rc != VGT_HIP_OK) return rc;
  if (num_points == 0) return VGT_HIP_OK;
  const size_t n = static_cast<size_t>(num_points);
  if (num_spheres == 0 || num_configurations == 0)
  {
    // nothing covers anything: the answer needs no device
    for (size_t i = 0; i < n && first_configuration_host; i++) first_configuration_host[i] = -1;
    for (size_t i = 0; i < n && first_sphere_host; i++) first_sphere_host[i] = -1;
    if (filtered_xyz_host && filtered_xyz_host != points_xyz_host)
      std::memmove(filtered_xyz_host, points_xyz_host, n * 3 * sizeof(float));
    return VGT_HIP_OK;
  }
  VGT_TRY_HIP(hipSetDevice(ctx->device), "set device");
  const char* what = "spheres cover points";
  const size_t b = static_cast<size_t>(num_configurations), s = static_cast<size_t>(num_spheres);
  vgt::HostStaging staging;
  const auto points = staging.In(points_xyz_host, n * 3);
  const auto xyzr = staging.In(sphere_xyzr_host, s * 4);
  const auto link = staging.In(sphere_link_host, s);
  const auto poses = staging.In(link_poses_host, b * static_cast<size_t>(num_links) * 16);
  const auto first_configuration = staging.Out(first_configuration_host, n);
  const auto first_sphere = staging.Out(first_sphere_host, n);
  const auto filtered = staging.Out(filtered_xyz_host, n * 3);
  return staging.Run(*ctx, what, FailHip, [&](hipStream_t stream) {
    return HipResult(what, a.Launch(points.dev(), xyzr.dev(), link.dev(), poses.dev(), first_configuration.dev(),
                                    first_sphere.dev(), filtered.dev(), stream));
  });
}

/* ---------------------- point clouds aligned to an SDF ---------------------- */

size_t vgt_hip_align_points_workspace_bytes(int64_t num_points, int64_t num_poses)
{
  return vgt::AlignWorkspaceBytes(num_points, num_poses);
}

int vgt_hip_align_points_dev(vgt_hip_ctx* ctx, const float* sdf_dev, int64_t nx, int64_t ny, int64_t nz,
                             double resolution, const double* grid_from_world, const double* rotation,
                             const float* points_xyz_dev, int64_t num_points, const double* poses_dev,
                             int64_t num_poses, const double* pivot, int32_t max_iterations, int32_t min_points,
                             double damping, double max_residual, double target_distance,
                             double translation_tolerance, double rotation_tolerance, double* poses_out_dev,
                             uint8_t* status_dev, int32_t* num_used_dev, int32_t* num_outside_dev,
                             int32_t* num_rejected_dev, double* sum_squared_dev, int32_t* evaluations_dev,
                             double* normal_equations_dev, double* last_step_dev, void* workspace_dev,
                             size_t workspace_bytes)
{
  const AlignPointsArguments a{sdf_dev, nx, ny, nz, resolution, grid_from_world, rotation, points_xyz_dev, num_points,
                               poses_dev, num_poses, pivot, max_iterations, min_points, damping, max_residual,
                               target_distance, translation_tolerance, rotation_tolerance,
                               {poses_out_dev, status_dev, num_used_dev, num_outside_dev, num_rejected_dev,
                                sum_squared_dev, evaluations_dev, normal_equations_dev, last_step_dev}};
  const int rc = a.Check(ctx);
  if (rc != VGT_HIP_OK) return rc;
  if (!workspace_dev) return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "null argument");
  if (workspace_bytes < vgt::AlignWorkspaceBytes(num_points, num_poses))
    return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "cloud-alignment workspace too small");
  VGT_TRY_HIP(hipSetDevice(ctx->device), "set device");
  std::lock_guard<std::mutex> lock(ctx->mutex);
  VGT_TRY_HIP(a.Launch(sdf_dev, points_xyz_dev, poses_dev, a.out, workspace_dev, ctx->stream), "align points");
  return VGT_HIP_OK;
}

int vgt_hip_align_points(vgt_hip_ctx* ctx, const float* sdf_host, int64_t nx, int64_t ny, int64_t nz, double resolution,
                         const double* grid_from_world, const double* rotation, const float* points_xyz_host,
                         int64_t num_points, const double* poses_host, int64_t num_poses, const double* pivot,
                         int32_t max_iterations, int32_t min_points, double damping, double max_residual,
                         double target_distance, double translation_tolerance, double rotation_tolerance,
                         double* poses_out_host, uint8_t* status_host, int32_t* num_used_host, int32_t* num_outside_host,
                         int32_t* num_rejected_host, double* sum_squared_host, int32_t* evaluations_host,
                         double* normal_equations_host, double* last_step_host)
{
  const AlignPointsArguments a{sdf_host, nx, ny, nz, resolution, grid_from_world, rotation, points_xyz_host, num_points,
                               poses_host, num_poses, pivot, max_iterations, min_points, damping, max_residual,
                               target_distance, translation_tolerance, rotation_tolerance,
                               {poses_out_host, status_host, num_used_host, num_outside_host, num_rejected_host,
                                sum_squared_host, evaluations_host, normal_equations_host, last_step_host}};
  const int rc = a.Check(ctx);
  if (rc != VGT_HIP_OK) return rc;
  VGT_TRY_HIP(hipSetDevice(ctx->device), "set device");
  const char* what = "align points";
  const size_t n = static_cast<size_t>(num_points), b = static_cast<size_t>(num_poses);
  // (thirteen arrays, and a staging holds eight: the inputs, the workspace and the poses in one, the other outputs in a
  // second one inside its body)
  vgt::HostStaging inputs;
  const auto sdf = inputs.In(sdf_host, static_cast<size_t>(a.NumCells()));
  const auto points = inputs.In(points_xyz_host, n * 3);
  const auto poses = inputs.In(poses_host, b * 16);
  const auto poses_out = inputs.Out(poses_out_host, b * 16);
  const auto workspace = inputs.Scratch<void>(vgt::AlignWorkspaceBytes(num_points, num_poses));
  return inputs.Run(*ctx, what, FailHip, [&](hipStream_t stream) {
    vgt::HostStaging outputs;
    const auto status = outputs.Out(status_host, b);
    const auto num_used = outputs.Out(num_used_host, b);
    const auto num_outside = outputs.Out(num_outside_host, b);
    const auto num_rejected = outputs.Out(num_rejected_host, b);
    const auto sum_squared = outputs.Out(sum_squared_host, b);
    const auto evaluations = outputs.Out(evaluations_host, b);
    const auto normal_equations = outputs.Out(normal_equations_host, b * 27);
    const auto last_step = outputs.Out(last_step_host, b * 6);
    return outputs.RunLocked(stream, what, FailHip, [&](hipStream_t) {
      const vgt::AlignOutputs out{poses_out.dev(),   status.dev(),      num_used.dev(),
                                  num_outside.dev(), num_rejected.dev(), sum_squared.dev(),
                                  evaluations.dev(), normal_equations.dev(), last_step.dev()};
      return HipResult(what, a.Launch(sdf.dev(), points.dev(), poses.dev(), out, workspace.dev(), stream));
    });
  });
}

/* ---------------------- nearest cell of the other class ---------------------- */

size_t vgt_hip_nearest_workspace_bytes(int64_t nx, int64_t ny, int64_t nz)
{
  if (!NearestShapeWithinLimits(nx, ny, nz)) return 0;
  return vgt::CarveNearestWorkspace(nx, ny, nz).bytes;
}

int vgt_hip_nearest_dev(vgt_hip_ctx* ctx, const float* occupancy_dev, int64_t nx, int64_t ny, int64_t nz,
                        int unknown_is_filled, int32_t* nearest_dev, int32_t* d2_dev_or_null, void* workspace_dev,
                        size_t workspace_bytes)
{
  if (!ctx || !occupancy_dev || !nearest_dev || !workspace_dev) return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "null argument");
  const int rc = CheckNearestShape(nx, ny, nz);
  if (rc != VGT_HIP_OK) return rc;
  if (workspace_bytes < vgt::CarveNearestWorkspace(nx, ny, nz).bytes)
    return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "nearest-cell workspace too small");
  VGT_TRY_HIP(hipSetDevice(ctx->device), "set device");
  std::lock_guard<std::mutex> lock(ctx->mutex);
  VGT_TRY_HIP(vgt::LaunchNearest<float>(occupancy_dev, MakeNearestGrid(nx, ny, nz, unknown_is_filled), nearest_dev,
                                        d2_dev_or_null, workspace_dev, ctx->stream),
              "nearest cells");
  return VGT_HIP_OK;
}

int vgt_hip_nearest_from_occupancy_f32(vgt_hip_ctx* ctx, const float* occupancy_host, int64_t nx, int64_t ny, int64_t nz,
                                       int unknown_is_filled, int32_t* nearest_host, int32_t* d2_host_or_null)
{
  return NearestFromHost<float>(ctx, occupancy_host, nx, ny, nz, unknown_is_filled, nearest_host, d2_host_or_null);
}

int vgt_hip_nearest_from_mask_u8(vgt_hip_ctx* ctx, const uint8_t* filled_mask_host, int64_t nx, int64_t ny, int64_t nz,
                                 int32_t* nearest_host, int32_t* d2_host_or_null)
{
  return NearestFromHost<uint8_t>(ctx, filled_mask_host, nx, ny, nz, 0, nearest_host, d2_host_or_null);
}

int vgt_hip_cells_nearest(vgt_hip_ctx* ctx, vgt_hip_cells* cells, const uint32_t* objects_to_use, int64_t num_objects,
                          int unknown_is_filled, int32_t* nearest_host, int32_t* d2_host_or_null,
                          uint32_t* object_host_or_null)
{
  int rc = CheckCells(ctx, cells);
  if (rc != VGT_HIP_OK) return rc;
  if (!nearest_host || num_objects < 0 || (num_objects > 0 && !objects_to_use))
    return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "null argument");
  if ((num_objects > 0 || object_host_or_null) && cells->object_id_offset < 0)
    return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "this cell type carries no object id");
  rc = CheckNearestShape(cells->nx, cells->ny, cells->nz);
  if (rc != VGT_HIP_OK) return rc;
  VGT_TRY_HIP(hipSetDevice(ctx->device), "set device");
  const char* what = "nearest cells of a tagged map";
  // (sorted and distinct, as vgt_hip_cells_sdf hands the list to the same predicate kernel)
  std::vector<uint32_t> objects(objects_to_use, objects_to_use + num_objects);
  std::sort(objects.begin(), objects.end());
  objects.erase(std::unique(objects.begin(), objects.end()), objects.end());
  const int64_t cells_total = cells->nx * cells->ny * cells->nz;
  const size_t n = static_cast<size_t>(cells_total);
  vgt::HostStaging staging;
  const auto nearest = staging.Out(nearest_host, n);
  const auto d2 = staging.Out(d2_host_or_null, n);
  const auto object = staging.Out(object_host_or_null, n);
  const auto workspace = staging.Scratch(vgt::CarveNearestWorkspace(cells->nx, cells->ny, cells->nz).bytes);
  return staging.Run(*ctx, what, FailHip, [&](hipStream_t s) -> int {
    const int grown = GrowCache(s, &cells->objects, objects.size() * sizeof(uint32_t),
                                "drain before regrowing object list", "allocate object list");
    if (grown != VGT_HIP_OK) return grown;
    if (!objects.empty())  // (pageable source: staged when the call returns)
      VGT_TRY_HIP(hipMemcpyAsync(cells->objects.data(), objects.data(), objects.size() * sizeof(uint32_t),
                                 hipMemcpyHostToDevice, s),
                  what);
    VGT_TRY_HIP(vgt::LaunchCellMask(cells->records.as<void>(), cells_total, cells->cell_bytes, cells->object_id_offset,
                                    objects.empty() ? 0 : 1, cells->objects.as<uint32_t>(),
                                    static_cast<int>(objects.size()), unknown_is_filled ? 1 : 0,
                                    cells->mask.as<uint8_t>(), s),
                what);
    VGT_TRY_HIP(vgt::LaunchNearest<uint8_t>(cells->mask.as<uint8_t>(), MakeNearestGrid(cells->nx, cells->ny, cells->nz, 0),
                                            nearest.dev(), d2.dev(), workspace.dev(), s),
                what);
    if (!object_host_or_null) return VGT_HIP_OK;
    return HipResult(what, vgt::LaunchNearestObjectId(cells->records.as<void>(), cells_total, cells->cell_bytes,
                                                      cells->object_id_offset, cells->mask.as<uint8_t>(),
                                                      nearest.dev(), object.dev(), s));
  });
}

int vgt_hip_sdf_local_extrema_map_dev(vgt_hip_ctx* ctx, const float* sdf_dev, int64_t nx, int64_t ny, int64_t nz,
                                      double resolution, const double* rotation, double* extrema_dev)
{
  if (!ctx || !sdf_dev || !extrema_dev) return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "null argument");
  const int rc = CheckSdfShape(nx, ny, nz, resolution);
  if (rc != VGT_HIP_OK) return rc;
  if (nx * ny * nz >= 0x7fffffffLL)
    return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "the local extrema map supports grids below 2^31 cells");
  VGT_TRY_HIP(hipSetDevice(ctx->device), "set device");
  vgt::DeviceTemp scratch;
  VGT_TRY_HIP(scratch.Allocate(vgt::LocalExtremaScratchBytes(nx * ny * nz)), "allocate extrema scratch");
  std::lock_guard<std::mutex> lock(ctx->mutex);
  const hipError_t err = vgt::LaunchLocalExtremaMap(sdf_dev, nx, ny, nz, resolution, rotation, extrema_dev,
                                                    scratch.as<void>(), ctx->stream);
  VGT_TRY_HIP(DrainKeepingFirst(ctx->stream, err), "local extrema map");  // (the scratch goes with the call)
  return VGT_HIP_OK;
}

int vgt_hip_sdf_local_extrema_map(vgt_hip_ctx* ctx, const float* sdf_host, int64_t nx, int64_t ny, int64_t nz,
                                  double resolution, const double* rotation, double* extrema_host)
{
  if (!ctx || !sdf_host || !extrema_host) return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "null argument");
  const int rc = CheckSdfShape(nx, ny, nz, resolution);
  if (rc != VGT_HIP_OK) return rc;
  if (nx * ny * nz >= 0x7fffffffLL)
    return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "the local extrema map supports grids below 2^31 cells");
  VGT_TRY_HIP(hipSetDevice(ctx->device), "set device");
  const size_t n = static_cast<size_t>(nx * ny * nz);
  vgt::HostStaging staging;
  const auto sdf = staging.In(sdf_host, n);
  const auto extrema = staging.Out(extrema_host, n * 3);
  const auto scratch = staging.Scratch(vgt::LocalExtremaScratchBytes(nx * ny * nz));
  return staging.Run(*ctx, "local extrema map", FailHip, [&](hipStream_t s) {
    return HipResult("local extrema map", vgt::LaunchLocalExtremaMap(sdf.dev(), nx, ny, nz, resolution, rotation,
                                                                     extrema.dev(), scratch.dev(), s));
  });
}

/* ------------------- connected components and spatial segments ------------------- */

namespace
{
int CheckComponentGrid(int64_t nx, int64_t ny, int64_t nz)
{
  if (nx <= 0 || ny <= 0 || nz <= 0) return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "grid extents must be positive");
  constexpr int64_t kLimit = 0x7fffffffLL;
  if (nx >= kLimit || ny >= kLimit || nz >= kLimit || nx * ny >= kLimit || nx * ny * nz >= kLimit)
    return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "component labelling supports grids below 2^31 cells");
  return VGT_HIP_OK;
}

int CheckThreshold(double connected_threshold)
{
  if (!(connected_threshold >= 0.0))
    return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "the connected threshold must be a number >= 0");
  return VGT_HIP_OK;
}

int CheckSegmentCells(const vgt_hip_ctx* ctx, const vgt_hip_cells* cells)
{
  const int rc = CheckCells(ctx, cells);
  if (rc != VGT_HIP_OK) return rc;
  if (cells->object_id_offset < 0)
    return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "this cell type carries no object id: it has no spatial segments");
  return CheckComponentGrid(cells->nx, cells->ny, cells->nz);
}

// Labels the grid on the context's stream into labels_dev and waits for the number of components.
// Caller holds the context mutex and has set the device.
int RunLabelling(vgt_hip_ctx* ctx, const void* cells_dev, int cell_bytes, int object_id_offset, int mode,
                 const double* extrema_dev, double connected_threshold, int64_t nx, int64_t ny, int64_t nz,
                 uint32_t* labels_dev, uint32_t* num_components)
{
  const int64_t n = nx * ny * nz;
  const size_t need = vgt::ComponentScratchBytes(n);
  const int grown = GrowCache(ctx->stream, &ctx->component_ws, need, "drain before regrowing the labelling scratch",
                              "allocate labelling scratch");
  if (grown != VGT_HIP_OK) return grown;
  void* const scratch = ctx->component_ws.data();
  const hipError_t err = vgt::LaunchLabelComponents(cells_dev, cell_bytes, object_id_offset, mode, extrema_dev,
                                                    connected_threshold, nx, ny, nz, labels_dev, scratch, ctx->stream);
  uint32_t count = 0;
  VGT_TRY_HIP(ReadBack(ctx->stream, err, &count, vgt::ComponentCountPtr(scratch, n)), "label components");
  *num_components = count;
  return VGT_HIP_OK;
}

}  // namespace

int vgt_hip_connected_components_dev(vgt_hip_ctx* ctx, const float* occupancy_dev, int64_t nx, int64_t ny, int64_t nz,
                                     uint32_t* labels_dev, uint32_t* num_components)
{
  const int rc = CheckComponentGrid(nx, ny, nz);
  if (rc != VGT_HIP_OK) return rc;
  if (!ctx || !occupancy_dev || !labels_dev || !num_components)
    return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "null argument");
  VGT_TRY_HIP(hipSetDevice(ctx->device), "set device");
  std::lock_guard<std::mutex> lock(ctx->mutex);
  return RunLabelling(ctx, occupancy_dev, 4, -1, vgt::kComponentClasses, nullptr, 0.0, nx, ny, nz, labels_dev,
                      num_components);
}

int vgt_hip_connected_components(vgt_hip_ctx* ctx, const float* occupancy_host, int64_t nx, int64_t ny, int64_t nz,
                                 uint32_t* labels_host, uint32_t* num_components)
{
  const int rc = CheckComponentGrid(nx, ny, nz);
  if (rc != VGT_HIP_OK) return rc;
  if (!ctx || !occupancy_host || !labels_host || !num_components)
    return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "null argument");
  VGT_TRY_HIP(hipSetDevice(ctx->device), "set device");
  const size_t n = static_cast<size_t>(nx * ny * nz);
  vgt::HostStaging staging;
  const auto occupancy = staging.In(occupancy_host, n);
  const auto labels = staging.Out(labels_host, n);
  return staging.Run(*ctx, "connected components", FailHip, [&](hipStream_t) {
    return RunLabelling(ctx, occupancy.dev(), 4, -1, vgt::kComponentClasses, nullptr, 0.0, nx, ny, nz, labels.dev(),
                        num_components);
  });
}

/* --------------------------------- enclosed space --------------------------------- */

namespace
{
// Everything that can be said about the arguments of the two entry points before any HIP call.
int CheckFillArguments(const vgt_hip_ctx* ctx, const void* cells, int cell_bytes, int64_t nx, int64_t ny, int64_t nz)
{
  if (!ctx || !cells) return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "null argument");
  if (cell_bytes != 4 && cell_bytes != 8)
    return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "cell_bytes must be 4 (OccupancyCell) or 8 (OccupancyComponentCell)");
  return CheckComponentGrid(nx, ny, nz);
}

// Enqueues the fill on the context's stream; with `num_filled` it waits for the count.  Caller holds the context mutex
// and has set the device.
int RunFillEnclosed(vgt_hip_ctx* ctx, void* cells_dev, int cell_bytes, int64_t nx, int64_t ny, int64_t nz,
                    int unknown_is_filled, int64_t* num_filled)
{
  const size_t need = vgt::FillScratchBytes(nx * ny * nz);
  const int grown = GrowCache(ctx->stream, &ctx->component_ws, need, "drain before regrowing the labelling scratch",
                              "allocate labelling scratch");
  if (grown != VGT_HIP_OK) return grown;
  void* const scratch = ctx->component_ws.data();
  const hipError_t err = vgt::LaunchFillEnclosed(cells_dev, cell_bytes, unknown_is_filled, nx, ny, nz, scratch, ctx->stream);
  if (!num_filled)
  {
    VGT_TRY_HIP(err, "fill enclosed space");
    return VGT_HIP_OK;
  }
  unsigned long long count = 0;
  VGT_TRY_HIP(ReadBack(ctx->stream, err, &count, vgt::FillCountPtr(scratch)), "fill enclosed space");
  *num_filled = static_cast<int64_t>(count);
  return VGT_HIP_OK;
}
}  // namespace

int vgt_hip_fill_enclosed_dev(vgt_hip_ctx* ctx, void* cells_dev, int cell_bytes, int64_t nx, int64_t ny, int64_t nz,
                              int unknown_is_filled, int64_t* num_filled)
{
  const int rc = CheckFillArguments(ctx, cells_dev, cell_bytes, nx, ny, nz);
  if (rc != VGT_HIP_OK) return rc;
  VGT_TRY_HIP(hipSetDevice(ctx->device), "set device");
  std::lock_guard<std::mutex> lock(ctx->mutex);
  return RunFillEnclosed(ctx, cells_dev, cell_bytes, nx, ny, nz, unknown_is_filled, num_filled);
}

int vgt_hip_fill_enclosed(vgt_hip_ctx* ctx, void* cells_host, int cell_bytes, int64_t nx, int64_t ny, int64_t nz,
                          int unknown_is_filled, int64_t* num_filled)
{
  const int rc = CheckFillArguments(ctx, cells_host, cell_bytes, nx, ny, nz);
  if (rc != VGT_HIP_OK) return rc;
  VGT_TRY_HIP(hipSetDevice(ctx->device), "set device");
  const size_t map_bytes = static_cast<size_t>(nx * ny * nz) * static_cast<size_t>(cell_bytes);
  vgt::HostStaging staging;
  const auto map = staging.InOut(static_cast<char*>(cells_host), map_bytes);
  int64_t count = 0;
  const int result = staging.Run(*ctx, "fill enclosed space", FailHip, [&](hipStream_t) {
    return RunFillEnclosed(ctx, map.dev(), cell_bytes, nx, ny, nz, unknown_is_filled, &count);
  });
  if (result == VGT_HIP_OK && num_filled) *num_filled = count;
  return result;
}

int vgt_hip_cells_connected_components(vgt_hip_ctx* ctx, vgt_hip_cells* cells, int connect_across_objects,
                                       uint32_t* labels_host, uint32_t* num_components)
{
  int rc = CheckCells(ctx, cells);
  if (rc != VGT_HIP_OK) return rc;
  if (!labels_host || !num_components) return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "null argument");
  rc = CheckComponentGrid(cells->nx, cells->ny, cells->nz);
  if (rc != VGT_HIP_OK) return rc;
  VGT_TRY_HIP(hipSetDevice(ctx->device), "set device");
  const bool by_object = cells->object_id_offset >= 0 && !connect_across_objects;
  vgt::HostStaging staging;
  const auto labels = staging.Out(labels_host, static_cast<size_t>(cells->nx * cells->ny * cells->nz));
  return staging.Run(*ctx, "connected components of a tagged map", FailHip, [&](hipStream_t) {
    return RunLabelling(ctx, cells->records.as<void>(), cells->cell_bytes, cells->object_id_offset,
                        by_object ? vgt::kComponentClassesAndIds : vgt::kComponentClasses, nullptr, 0.0, cells->nx,
                        cells->ny, cells->nz, labels.dev(), num_components);
  });
}

int vgt_hip_cells_spatial_segments_dev(vgt_hip_ctx* ctx, vgt_hip_cells* cells, const double* extrema_dev,
                                       double connected_threshold, uint32_t* labels_dev, uint32_t* num_segments)
{
  int rc = CheckThreshold(connected_threshold);
  if (rc != VGT_HIP_OK) return rc;
  rc = CheckSegmentCells(ctx, cells);
  if (rc != VGT_HIP_OK) return rc;
  if (!extrema_dev || !labels_dev || !num_segments) return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "null argument");
  VGT_TRY_HIP(hipSetDevice(ctx->device), "set device");
  std::lock_guard<std::mutex> lock(ctx->mutex);
  return RunLabelling(ctx, cells->records.as<void>(), cells->cell_bytes, cells->object_id_offset, vgt::kComponentSegments,
                      extrema_dev, connected_threshold, cells->nx, cells->ny, cells->nz, labels_dev, num_segments);
}

int vgt_hip_cells_spatial_segments(vgt_hip_ctx* ctx, vgt_hip_cells* cells, const double* extrema_host,
                                   double connected_threshold, uint32_t* labels_host, uint32_t* num_segments)
{
  int rc = CheckThreshold(connected_threshold);
  if (rc != VGT_HIP_OK) return rc;
  rc = CheckSegmentCells(ctx, cells);
  if (rc != VGT_HIP_OK) return rc;
  if (!extrema_host || !labels_host || !num_segments) return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "null argument");
  VGT_TRY_HIP(hipSetDevice(ctx->device), "set device");
  const size_t n = static_cast<size_t>(cells->nx * cells->ny * cells->nz);
  vgt::HostStaging staging;
  const auto extrema = staging.In(extrema_host, n * 3);
  const auto labels = staging.Out(labels_host, n);
  return staging.Run(*ctx, "spatial segments", FailHip, [&](hipStream_t) {
    return RunLabelling(ctx, cells->records.as<void>(), cells->cell_bytes, cells->object_id_offset,
                        vgt::kComponentSegments, extrema.dev(), connected_threshold, cells->nx, cells->ny, cells->nz,
                        labels.dev(), num_segments);
  });
}

int vgt_hip_cells_update_spatial_segments(vgt_hip_ctx* ctx, vgt_hip_cells* cells, double connected_threshold,
                                          double resolution, int unknown_is_filled, int add_virtual_border,
                                          const double* rotation, uint32_t* labels_host, uint32_t* num_segments)
{
  int rc = CheckThreshold(connected_threshold);
  if (rc != VGT_HIP_OK) return rc;
  rc = CheckSegmentCells(ctx, cells);
  if (rc != VGT_HIP_OK) return rc;
  if (!labels_host || !num_segments) return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "null argument");
  rc = CheckSdfShape(cells->nx, cells->ny, cells->nz, resolution);
  if (rc != VGT_HIP_OK) return rc;
  VGT_TRY_HIP(hipSetDevice(ctx->device), "set device");
  const int64_t nx = cells->nx, ny = cells->ny, nz = cells->nz, n = nx * ny * nz;
  vgt::HostStaging staging;
  const auto extrema = staging.Scratch<double>(static_cast<size_t>(n) * 3 * sizeof(double));
  const auto extrema_scratch = staging.Scratch(vgt::LocalExtremaScratchBytes(n));
  const auto labels = staging.Out(labels_host, static_cast<size_t>(n));
  // S/tagged_object_occupancy_component_map.cpp:786-790: the field of every filled cell with a virtual border, the
  // free-and-named-objects field without; its extrema map; the segments.  Field and map stay on the device.
  return staging.Run(*ctx, "update spatial segments", FailHip, [&](hipStream_t s) {
    const vgt::SdfParams p{nx, ny, nz, resolution, unknown_is_filled ? 1 : 0, add_virtual_border ? 1 : 0};
    if (!add_virtual_border)
      VGT_TRY_HIP(cells->sdf_named.Reserve(static_cast<size_t>(n) * sizeof(float)), "update spatial segments");
    const int sdf_rc = add_virtual_border ? RunCellsSdf(ctx, cells, 0, 0, p, cells->sdf.as<float>())
                                          : RunFreeAndNamedSdf(ctx, cells, p);
    if (sdf_rc != VGT_HIP_OK) return sdf_rc;
    VGT_TRY_HIP(vgt::LaunchLocalExtremaMap(cells->sdf.as<float>(), nx, ny, nz, resolution, rotation, extrema.dev(),
                                           extrema_scratch.dev(), s),
                "update spatial segments");
    return RunLabelling(ctx, cells->records.as<void>(), cells->cell_bytes, cells->object_id_offset,
                        vgt::kComponentSegments, extrema.dev(), connected_threshold, nx, ny, nz, labels.dev(),
                        num_segments);
  });
}

namespace
{
int CheckSurfaceMaskArguments(const vgt_hip_ctx* ctx, const void* occupancy, const void* labels, int64_t nx, int64_t ny,
                              int64_t nz, int component_types, const void* mask)
{
  const int rc = CheckComponentGrid(nx, ny, nz);
  if (rc != VGT_HIP_OK) return rc;
  if (component_types < 1 || component_types > 7)
    return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "component types must be a combination of 1 (filled), 2 (empty), 4 (unknown)");
  if (!ctx || !occupancy || !labels || !mask) return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "null argument");
  return VGT_HIP_OK;
}
}  // namespace

int vgt_hip_component_surface_mask_dev(vgt_hip_ctx* ctx, const float* occupancy_dev, const uint32_t* labels_dev,
                                       int64_t nx, int64_t ny, int64_t nz, int component_types, uint8_t* mask_dev)
{
  const int rc = CheckSurfaceMaskArguments(ctx, occupancy_dev, labels_dev, nx, ny, nz, component_types, mask_dev);
  if (rc != VGT_HIP_OK) return rc;
  VGT_TRY_HIP(hipSetDevice(ctx->device), "set device");
  std::lock_guard<std::mutex> lock(ctx->mutex);
  VGT_TRY_HIP(vgt::LaunchComponentSurfaceMask(occupancy_dev, labels_dev, nx, ny, nz, component_types, mask_dev,
                                              ctx->stream),
              "component surface mask");
  return VGT_HIP_OK;
}

int vgt_hip_component_surface_mask(vgt_hip_ctx* ctx, const float* occupancy_host, const uint32_t* labels_host,
                                   int64_t nx, int64_t ny, int64_t nz, int component_types, uint8_t* mask_host)
{
  const int rc = CheckSurfaceMaskArguments(ctx, occupancy_host, labels_host, nx, ny, nz, component_types, mask_host);
  if (rc != VGT_HIP_OK) return rc;
  VGT_TRY_HIP(hipSetDevice(ctx->device), "set device");
  const size_t n = static_cast<size_t>(nx * ny * nz);
  vgt::HostStaging staging;
  const auto occupancy = staging.In(occupancy_host, n);
  const auto labels = staging.In(labels_host, n);
  const auto mask = staging.Out(mask_host, n);
  return staging.Run(*ctx, "component surface mask", FailHip, [&](hipStream_t s) {
    return HipResult("component surface mask",
                     vgt::LaunchComponentSurfaceMask(occupancy.dev(), labels.dev(), nx, ny, nz, component_types,
                                                     mask.dev(), s));
  });
}

/* ------------------------- selected cells as compact ordered lists ------------------------- */

namespace
{
// Everything that can be said about a selection before any HIP call (the context is not looked into).
int CheckSelectArguments(const vgt_hip_ctx* ctx, const void* values, bool has_labels, int64_t nx, int64_t ny, int64_t nz,
                         int rule, int class_mask, float threshold, const void* indices_out, const void* labels_out,
                         int64_t capacity, const int64_t* count)
{
  if (!ctx || !values || !count) return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "null argument");
  const int rc = CheckComponentGrid(nx, ny, nz);
  if (rc != VGT_HIP_OK) return rc;
  if (rule != VGT_HIP_SELECT_ALL && rule != VGT_HIP_SELECT_SURFACE_26 && rule != VGT_HIP_SELECT_COMPONENT_SURFACE)
    return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "unknown selection rule " + std::to_string(rule));
  if (class_mask < 1 || class_mask > 15)
    return Fail(VGT_HIP_ERR_INVALID_ARGUMENT,
                "the class mask must be a combination of 1 (above), 2 (below), 4 (equal), 8 (unordered)");
  if (rule == VGT_HIP_SELECT_SURFACE_26 && threshold != 0.5f)
    return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "the 26-neighbour surface rule is defined for the threshold 0.5 only");
  if (threshold != threshold) return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "the threshold must be a number");
  if (rule == VGT_HIP_SELECT_COMPONENT_SURFACE && !has_labels)
    return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "the component surface rule needs labels");
  if (labels_out && !has_labels) return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "a label list needs labels");
  if (capacity < 0 || (capacity > 0 && !indices_out))
    return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "invalid index buffer (capacity without a buffer, or a negative one)");
  return VGT_HIP_OK;
}

// Marks and counts on the context's stream and waits for the count (*count); with room for it, the lists go to the
// DEVICE buffers of `out` (out.capacity as the caller gave it; nothing is written when the count exceeds it) and the
// stream is drained.  Caller holds the context mutex and has set the device.
int RunSelect(vgt_hip_ctx* ctx, const vgt::SelectGrid& grid, const vgt::SelectOutput& out, int64_t* count)
{
  const int64_t n = static_cast<int64_t>(grid.nx) * grid.ny * grid.nz;
  const size_t need = vgt::SelectScratchBytes(n);
  const int grown = GrowCache(ctx->stream, &ctx->select_ws, need, "drain before regrowing the selection scratch",
                              "allocate selection scratch");
  if (grown != VGT_HIP_OK) return grown;
  void* const scratch = ctx->select_ws.data();
  hipError_t err = vgt::LaunchSelectMark(grid, scratch, ctx->stream);
  uint32_t selected = 0;
  VGT_TRY_HIP(ReadBack(ctx->stream, err, &selected, vgt::SelectCountPtr(scratch, n)), "select cells");
  *count = static_cast<int64_t>(selected);
  if (!out.indices_dev) return VGT_HIP_OK;  // count only
  if (*count > out.capacity)
    return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "the selection holds " + std::to_string(*count) +
                                                  " cells, the output buffers " + std::to_string(out.capacity));
  if (*count == 0) return VGT_HIP_OK;
  err = vgt::LaunchSelectEmit(grid, out, scratch, ctx->stream);
  VGT_TRY_HIP(DrainKeepingFirst(ctx->stream, err), "select cells");
  return VGT_HIP_OK;
}

// RunSelect with lists in HOST memory: counts, then emits into device buffers of exactly the count and downloads them.
// payload_source_dev / payload_stride: where payload_host's uint32 come from.  Caller holds the context mutex.
int RunSelectToHost(vgt_hip_ctx* ctx, const vgt::SelectGrid& grid, const void* payload_source_dev, int payload_stride,
                    int32_t* indices_host, float* values_host, uint32_t* payload_host, int64_t capacity, int64_t* count)
{
  vgt::SelectOutput none{};
  int rc = RunSelect(ctx, grid, none, count);
  if (rc != VGT_HIP_OK || !indices_host) return rc;
  if (*count > capacity)
    return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "the selection holds " + std::to_string(*count) +
                                                  " cells, the output buffers " + std::to_string(capacity));
  if (*count == 0) return VGT_HIP_OK;
  const size_t selected = static_cast<size_t>(*count);
  vgt::HostStaging staging;
  const auto indices = staging.Out(indices_host, selected);
  const auto values = staging.Out(values_host, selected);
  const auto payload = staging.Out(payload_host, selected);
  return staging.RunLocked(ctx->stream, "select cells", FailHip, [&](hipStream_t s) {
    vgt::SelectOutput out{};
    out.indices_dev = indices.dev();
    out.values_dev = values.dev();
    out.payload_dev = payload.dev();
    out.payload_source_dev = payload_source_dev;
    out.payload_stride = payload_stride;
    out.capacity = *count;
    // (the scratch still holds the marks of the count above: same grid, same stream, nothing enqueued in between)
    return HipResult("select cells", vgt::LaunchSelectEmit(grid, out, ctx->select_ws.data(), s));
  });
}

vgt::SelectGrid MakeSelectGrid(const void* cells_dev, int cell_bytes, const void* labels_dev, int label_stride, int64_t nx,
                               int64_t ny, int64_t nz, int rule, int class_mask, float threshold)
{
  vgt::SelectGrid g;
  g.cells_dev = cells_dev;
  g.cell_bytes = cell_bytes;
  g.labels_dev = labels_dev;
  g.label_stride = label_stride;
  g.nx = static_cast<int>(nx);
  g.ny = static_cast<int>(ny);
  g.nz = static_cast<int>(nz);
  g.rule = rule;
  g.class_mask = class_mask;
  g.threshold = threshold;
  return g;
}
}  // namespace

int vgt_hip_select_cells_dev(vgt_hip_ctx* ctx, const float* values_dev, const uint32_t* labels_dev, int64_t nx,
                             int64_t ny, int64_t nz, int rule, int class_mask, float threshold, int32_t* indices_out,
                             float* values_out, uint32_t* labels_out, int64_t capacity, int64_t* count)
{
  const int rc = CheckSelectArguments(ctx, values_dev, labels_dev != nullptr, nx, ny, nz, rule, class_mask, threshold,
                                      indices_out, labels_out, capacity, count);
  if (rc != VGT_HIP_OK) return rc;
  VGT_TRY_HIP(hipSetDevice(ctx->device), "set device");
  const vgt::SelectGrid grid = MakeSelectGrid(values_dev, 4, labels_dev, 4, nx, ny, nz, rule, class_mask, threshold);
  vgt::SelectOutput out{};
  out.indices_dev = indices_out;
  out.values_dev = values_out;
  out.payload_dev = labels_out;
  out.payload_source_dev = labels_dev;
  out.payload_stride = 4;
  out.capacity = capacity;
  std::lock_guard<std::mutex> lock(ctx->mutex);
  return RunSelect(ctx, grid, out, count);
}

int vgt_hip_select_cells(vgt_hip_ctx* ctx, const float* values_host, const uint32_t* labels_host, int64_t nx, int64_t ny,
                         int64_t nz, int rule, int class_mask, float threshold, int32_t* indices_out, float* values_out,
                         uint32_t* labels_out, int64_t capacity, int64_t* count)
{
  const int rc = CheckSelectArguments(ctx, values_host, labels_host != nullptr, nx, ny, nz, rule, class_mask, threshold,
                                      indices_out, labels_out, capacity, count);
  if (rc != VGT_HIP_OK) return rc;
  VGT_TRY_HIP(hipSetDevice(ctx->device), "set device");
  const size_t n = static_cast<size_t>(nx * ny * nz);
  // (labels that neither the rule nor a list needs stay on the host)
  const bool use_labels = labels_host && (rule == VGT_HIP_SELECT_COMPONENT_SURFACE || labels_out);
  vgt::HostStaging staging;
  const auto values = staging.In(values_host, n);
  const auto labels = staging.In(use_labels ? labels_host : nullptr, n);
  return staging.Run(*ctx, "select cells", FailHip, [&](hipStream_t) {
    const vgt::SelectGrid grid =
        MakeSelectGrid(values.dev(), 4, labels.dev(), 4, nx, ny, nz, rule, class_mask, threshold);
    return RunSelectToHost(ctx, grid, labels.dev(), 4, indices_out, values_out, labels_out, capacity, count);
  });
}

int vgt_hip_cells_select(vgt_hip_ctx* ctx, vgt_hip_cells* cells, const uint32_t* labels_dev_or_null, int rule,
                         int class_mask, int32_t* indices_host, float* occupancy_host, uint32_t* payload_host,
                         int payload_member, int64_t capacity, int64_t* count)
{
  int rc = CheckCells(ctx, cells);
  if (rc != VGT_HIP_OK) return rc;
  // where the layout keeps its members (include/vgt_hip.h)
  const int object_id_at = cells->object_id_offset;
  const int component_at = cells->cell_bytes == 16 ? 8 : (cells->cell_bytes == 8 && object_id_at < 0 ? 4 : -1);
  const int segment_at = cells->cell_bytes == 16 ? 12 : -1;
  int payload_at = -1;
  switch (payload_member)
  {
    case VGT_HIP_CELL_MEMBER_NONE:
      if (payload_host) return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "a payload buffer without a payload member");
      break;
    case VGT_HIP_CELL_MEMBER_OBJECT_ID:
      payload_at = object_id_at;
      break;
    case VGT_HIP_CELL_MEMBER_COMPONENT:
      payload_at = component_at;
      break;
    case VGT_HIP_CELL_MEMBER_SPATIAL_SEGMENT:
      payload_at = segment_at;
      break;
    default:
      return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "unknown payload member " + std::to_string(payload_member));
  }
  if (payload_member != VGT_HIP_CELL_MEMBER_NONE && payload_at < 0)
    return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "this cell layout does not have the payload member asked for");
  const bool own_labels = !labels_dev_or_null && component_at >= 0;
  rc = CheckSelectArguments(ctx, cells, labels_dev_or_null || own_labels, cells->nx, cells->ny, cells->nz, rule,
                            class_mask, 0.5f, indices_host, nullptr, capacity, count);
  if (rc != VGT_HIP_OK) return rc;
  VGT_TRY_HIP(hipSetDevice(ctx->device), "set device");
  const char* const records = cells->records.as<char>();
  const vgt::SelectGrid grid =
      MakeSelectGrid(records, cells->cell_bytes, own_labels ? static_cast<const void*>(records + component_at) : labels_dev_or_null,
                     own_labels ? cells->cell_bytes : 4, cells->nx, cells->ny, cells->nz, rule, class_mask, 0.5f);
  std::lock_guard<std::mutex> lock(ctx->mutex);
  return RunSelectToHost(ctx, grid, payload_at >= 0 ? records + payload_at : nullptr, cells->cell_bytes, indices_host,
                         occupancy_host, payload_at >= 0 ? payload_host : nullptr, capacity, count);
}

/* ------------------------- the iso-surface as an indexed triangle mesh ------------------------- */

namespace
{
// Where a caller wants the mesh, in host or in device memory.
struct SurfaceBuffers
{
  double* vertices;
  int32_t* vertex_cells;
  int64_t vertex_capacity;
  int32_t* triangles;
  int64_t triangle_capacity;
  int64_t* num_vertices;
  int64_t* num_triangles;
};

// Everything that can be said about an extraction before any HIP call (the context is not looked into).
int CheckSurfaceArguments(const vgt_hip_ctx* ctx, const void* values, int64_t nx, int64_t ny, int64_t nz, float iso,
                          double resolution, const SurfaceBuffers& b)
{
  if (!ctx || !values || !b.num_vertices || !b.num_triangles) return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "null argument");
  const int rc = CheckComponentGrid(nx, ny, nz);
  if (rc != VGT_HIP_OK) return rc;
  if (!(resolution > 0.0) || !std::isfinite(resolution))
    return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "resolution must be finite and greater than zero");
  if (!std::isfinite(iso)) return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "the iso level must be finite");
  if (b.triangles && !b.vertices)
    return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "a triangle buffer needs a vertex buffer: the triangles index the vertices");
  if (b.vertex_cells && !b.vertices) return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "a vertex cell buffer needs a vertex buffer");
  if (b.vertex_capacity < 0 || (b.vertex_capacity > 0 && !b.vertices))
    return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "invalid vertex buffer (capacity without a buffer, or a negative one)");
  if (b.triangle_capacity < 0 || (b.triangle_capacity > 0 && !b.triangles))
    return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "invalid triangle buffer (capacity without a buffer, or a negative one)");
  return VGT_HIP_OK;
}

vgt::SurfaceGrid MakeSurfaceGrid(const void* values_dev, int value_stride, int64_t nx, int64_t ny, int64_t nz, float iso,
                                 int inside_above, double resolution, const double* world_from_grid)
{
  vgt::SurfaceGrid g{};
  g.values_dev = values_dev;
  g.value_stride = value_stride;
  g.nx = static_cast<int>(nx);
  g.ny = static_cast<int>(ny);
  g.nz = static_cast<int>(nz);
  g.iso = iso;
  g.inside_above = inside_above ? 1 : 0;
  g.resolution = resolution;
  g.has_transform = world_from_grid ? 1 : 0;
  if (world_from_grid) std::memcpy(g.world_from_grid, world_from_grid, sizeof(g.world_from_grid));
  return g;
}

// A grid with an extent of 1 has no cubes: an empty mesh, nothing launched.
bool SurfaceHasNoCubes(int64_t nx, int64_t ny, int64_t nz, const SurfaceBuffers& b)
{
  if (nx > 1 && ny > 1 && nz > 1) return false;
  *b.num_vertices = 0;
  *b.num_triangles = 0;
  return true;
}

// Marks and counts on the context's stream, waits for the two counts and stores them; then compares them with the
// capacities.  *emit: there is something to write and room for it.  Caller holds the context mutex and has set the device.
int CountSurface(vgt_hip_ctx* ctx, const vgt::SurfaceGrid& grid, const SurfaceBuffers& b, bool* emit)
{
  *emit = false;
  const int64_t n = static_cast<int64_t>(grid.nx) * grid.ny * grid.nz;
  const int grown = GrowCache(ctx->stream, &ctx->surface_ws, vgt::SurfaceScratchBytes(n),
                              "drain before regrowing the surface scratch", "allocate surface scratch");
  if (grown != VGT_HIP_OK) return grown;
  void* const scratch = ctx->surface_ws.data();
  const hipError_t err = vgt::LaunchSurfaceMark(grid, scratch, ctx->stream);
  vgt::SurfaceCounts counts{};
  VGT_TRY_HIP(ReadBack(ctx->stream, err, &counts, vgt::SurfaceCountsPtr(scratch, n)), "extract surface");
  // (3 int32 per triangle, 2 triangles per quad: 3 * num_triangles stays below 2^31)
  if (counts.quads * 6ull >= 0x80000000ull)
    return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "the surface holds " + std::to_string(counts.quads * 2ull) +
                                                  " triangles: 3 * num_triangles must stay below 2^31");
  *b.num_vertices = static_cast<int64_t>(counts.vertices);
  *b.num_triangles = static_cast<int64_t>(counts.quads) * 2;
  if (!b.vertices) return VGT_HIP_OK;  // count only
  if (*b.num_vertices > b.vertex_capacity)
    return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "the surface holds " + std::to_string(*b.num_vertices) +
                                                  " vertices, the vertex buffers " + std::to_string(b.vertex_capacity));
  if (b.triangles && *b.num_triangles > b.triangle_capacity)
    return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "the surface holds " + std::to_string(*b.num_triangles) +
                                                  " triangles, the triangle buffer " + std::to_string(b.triangle_capacity));
  *emit = *b.num_vertices > 0;
  return VGT_HIP_OK;
}

// The mesh into DEVICE buffers, from the marks of the CountSurface just before (same grid, same stream, nothing enqueued
// in between).
hipError_t EmitSurface(vgt_hip_ctx* ctx, const vgt::SurfaceGrid& grid, double* vertices_dev, int32_t* vertex_cells_dev,
                       int32_t* triangles_dev, int64_t num_triangles, hipStream_t s)
{
  const vgt::SurfaceOutput out{vertices_dev, vertex_cells_dev, num_triangles > 0 ? triangles_dev : nullptr};
  return vgt::LaunchSurfaceEmit(grid, out, ctx->surface_ws.data(), s);
}

// Counts, then emits into device buffers of exactly the counts and downloads them.  Caller holds the context mutex.
int RunSurfaceToHost(vgt_hip_ctx* ctx, const vgt::SurfaceGrid& grid, const SurfaceBuffers& b)
{
  bool emit = false;
  const int rc = CountSurface(ctx, grid, b, &emit);
  if (rc != VGT_HIP_OK || !emit) return rc;
  const size_t num_vertices = static_cast<size_t>(*b.num_vertices), num_triangles = static_cast<size_t>(*b.num_triangles);
  vgt::HostStaging staging;
  const auto vertices = staging.Out(b.vertices, num_vertices * 3);
  const auto vertex_cells = staging.Out(b.vertex_cells, num_vertices);
  const auto triangles = staging.Out(num_triangles ? b.triangles : nullptr, num_triangles * 3);
  return staging.RunLocked(ctx->stream, "extract surface", FailHip, [&](hipStream_t s) {
    return HipResult("extract surface", EmitSurface(ctx, grid, vertices.dev(), vertex_cells.dev(), triangles.dev(),
                                                    *b.num_triangles, s));
  });
}
}  // namespace

int vgt_hip_extract_surface_dev(vgt_hip_ctx* ctx, const float* values_dev, int64_t nx, int64_t ny, int64_t nz, float iso,
                                int inside_above, double resolution, const double* world_from_grid,
                                double* vertices_xyz_dev, int32_t* vertex_cells_dev, int64_t vertex_capacity,
                                int32_t* triangles_dev, int64_t triangle_capacity, int64_t* num_vertices,
                                int64_t* num_triangles)
{
  const SurfaceBuffers b{vertices_xyz_dev, vertex_cells_dev, vertex_capacity, triangles_dev,
                         triangle_capacity, num_vertices,    num_triangles};
  const int rc = CheckSurfaceArguments(ctx, values_dev, nx, ny, nz, iso, resolution, b);
  if (rc != VGT_HIP_OK) return rc;
  if (SurfaceHasNoCubes(nx, ny, nz, b)) return VGT_HIP_OK;
  VGT_TRY_HIP(hipSetDevice(ctx->device), "set device");
  const vgt::SurfaceGrid grid = MakeSurfaceGrid(values_dev, 4, nx, ny, nz, iso, inside_above, resolution, world_from_grid);
  std::lock_guard<std::mutex> lock(ctx->mutex);
  bool emit = false;
  const int counted = CountSurface(ctx, grid, b, &emit);
  if (counted != VGT_HIP_OK || !emit) return counted;
  const hipError_t err =
      EmitSurface(ctx, grid, vertices_xyz_dev, vertex_cells_dev, triangles_dev, *num_triangles, ctx->stream);
  VGT_TRY_HIP(DrainKeepingFirst(ctx->stream, err), "extract surface");
  return VGT_HIP_OK;
}

int vgt_hip_extract_surface(vgt_hip_ctx* ctx, const float* values_host, int64_t nx, int64_t ny, int64_t nz, float iso,
                            int inside_above, double resolution, const double* world_from_grid, double* vertices_xyz_out,
                            int32_t* vertex_cells_out, int64_t vertex_capacity, int32_t* triangles_out,
                            int64_t triangle_capacity, int64_t* num_vertices, int64_t* num_triangles)
{
  const SurfaceBuffers b{vertices_xyz_out, vertex_cells_out, vertex_capacity, triangles_out,
                         triangle_capacity, num_vertices,    num_triangles};
  const int rc = CheckSurfaceArguments(ctx, values_host, nx, ny, nz, iso, resolution, b);
  if (rc != VGT_HIP_OK) return rc;
  if (SurfaceHasNoCubes(nx, ny, nz, b)) return VGT_HIP_OK;
  VGT_TRY_HIP(hipSetDevice(ctx->device), "set device");
  vgt::HostStaging staging;
  const auto values = staging.In(values_host, static_cast<size_t>(nx * ny * nz));
  return staging.Run(*ctx, "extract surface", FailHip, [&](hipStream_t) {
    return RunSurfaceToHost(
        ctx, MakeSurfaceGrid(values.dev(), 4, nx, ny, nz, iso, inside_above, resolution, world_from_grid), b);
  });
}

int vgt_hip_cells_extract_surface(vgt_hip_ctx* ctx, vgt_hip_cells* cells, double resolution,
                                  const double* world_from_grid, double* vertices_xyz_out, int32_t* vertex_cells_out,
                                  int64_t vertex_capacity, int32_t* triangles_out, int64_t triangle_capacity,
                                  int64_t* num_vertices, int64_t* num_triangles)
{
  int rc = CheckCells(ctx, cells);
  if (rc != VGT_HIP_OK) return rc;
  const SurfaceBuffers b{vertices_xyz_out, vertex_cells_out, vertex_capacity, triangles_out,
                         triangle_capacity, num_vertices,    num_triangles};
  rc = CheckSurfaceArguments(ctx, cells, cells->nx, cells->ny, cells->nz, 0.5f, resolution, b);
  if (rc != VGT_HIP_OK) return rc;
  if (SurfaceHasNoCubes(cells->nx, cells->ny, cells->nz, b)) return VGT_HIP_OK;
  VGT_TRY_HIP(hipSetDevice(ctx->device), "set device");
  // (the float occupancy is the first member of every cell layout)
  const vgt::SurfaceGrid grid = MakeSurfaceGrid(cells->records.as<void>(), cells->cell_bytes, cells->nx, cells->ny,
                                                cells->nz, 0.5f, 1, resolution, world_from_grid);
  std::lock_guard<std::mutex> lock(ctx->mutex);
  return RunSurfaceToHost(ctx, grid, b);
}

/* ------------------------- cost-to-go through free space, path tracing ------------------------- */

namespace
{
bool TravelShapeWithinLimits(int64_t nx, int64_t ny, int64_t nz)
{
  constexpr int64_t kLimit = 0x7fffffffLL;
  if (nx < 0 || ny < 0 || nz < 0) return false;
  if (nx == 0 || ny == 0 || nz == 0) return true;
  return nx <= kLimit && ny <= kLimit && nz <= kLimit && nx * ny <= kLimit && nx * ny * nz <= kLimit;
}

// Everything that can be said about a cost-to-go call before any HIP call (the context is not looked into).  mode: null
// for cell records, which have no field mode.
int CheckTravelArguments(const vgt_hip_ctx* ctx, const void* field, int64_t nx, int64_t ny, int64_t nz,
                         const int32_t* mode, double threshold, const uint32_t* weights, uint32_t flags,
                         const int32_t* sources, int64_t num_sources, uint32_t cost_limit, const uint32_t* cost,
                         vgt::TravelGrid* grid)
{
  if (!ctx || !field || !weights || !cost) return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "null argument");
  if (num_sources < 0) return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "the number of sources must not be negative");
  if (num_sources > 0 && !sources) return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "null argument");
  if (nx < 0 || ny < 0 || nz < 0) return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "grid extents must not be negative");
  if (!TravelShapeWithinLimits(nx, ny, nz))
    return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "travel costs support grids below 2^31 cells");
  if (mode && *mode != VGT_HIP_TRAVEL_OCCUPANCY && *mode != VGT_HIP_TRAVEL_SDF_ABOVE)
    return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "unknown travel-cost mode");
  if (flags & ~VGT_HIP_TRAVEL_NO_CORNER_CUTTING) return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "unknown travel-cost flag");
  if (mode && *mode == VGT_HIP_TRAVEL_SDF_ABOVE && std::isnan(threshold))
    return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "the SDF threshold must be a number");
  if (weights[0] == 0u) return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "weights[0] (the axis moves) must be greater than zero");
  if (weights[0] > 65535u || weights[1] > 65535u || weights[2] > 65535u)
    return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "a move weight must be at most 65535");
  if (cost_limit == VGT_HIP_TRAVEL_UNREACHED)
    return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "the cost limit must be at most 0xfffffffe (which means no limit)");
  *grid = vgt::TravelGrid{static_cast<int>(nx), static_cast<int>(ny), static_cast<int>(nz),
                          {weights[0], weights[1], weights[2]}, flags, cost_limit};
  return VGT_HIP_OK;
}

int TravelSourceOf(int32_t mode)
{
  return mode == VGT_HIP_TRAVEL_OCCUPANCY ? vgt::kTravelFromOccupancy : vgt::kTravelFromSdf;
}

// Seeds, runs the rounds until no tile is active (one word read back per round), then `toward` and the count.  Every
// buffer is on the device; the stream is idle when this returns.  Caller holds the context mutex and has set the device.
int RunTravelCost(hipStream_t s, const void* field_dev, int source, int unknown_is_filled, double threshold,
                  const vgt::TravelGrid& grid, const int32_t* sources_dev, const uint32_t* source_costs_dev,
                  int64_t num_sources, uint32_t* cost_dev, int32_t* toward_dev, int64_t* num_reached,
                  void* workspace_dev)
{
  const char* what = "travel cost";
  const vgt::TravelWorkspace w = vgt::CarveTravelWorkspace(grid.nx, grid.ny, grid.nz);
  auto* const status_dev = reinterpret_cast<vgt::TravelStatus*>(static_cast<char*>(workspace_dev) + w.status_offset);
  hipError_t err = vgt::LaunchTravelSeed(field_dev, source, unknown_is_filled, threshold, grid, sources_dev,
                                         source_costs_dev, num_sources, cost_dev, workspace_dev, s);
  // (see vgt_hip.h, method: after round k every cell with a least-cost path of fewer than k tile changes is final, and a
  // path visits a cell once, so it changes tile fewer times than the grid has cells)
  const int64_t most_rounds = static_cast<int64_t>(grid.nx) * grid.ny * grid.nz + 2;
  int64_t round = 0;
  for (bool active = num_sources > 0; active && err == hipSuccess; round++)
  {
    if (round == most_rounds)
    {
      (void)hipStreamSynchronize(s);
      return Fail(VGT_HIP_ERR_RUNTIME, "[travel cost] tiles are still active after cells + 2 rounds");
    }
    err = vgt::LaunchTravelRound(grid, cost_dev, workspace_dev, round, s);
    uint32_t next_active = 0;
    err = ReadBack(s, err, &next_active, &status_dev->active[(round + 1) & 1]);
    active = next_active != 0u;
  }
  if (err == hipSuccess && (toward_dev || num_reached))
    err = vgt::LaunchTravelToward(grid, sources_dev, source_costs_dev, num_sources, cost_dev, toward_dev, workspace_dev, s);
  const uint32_t rounds = static_cast<uint32_t>(round);
  if (err == hipSuccess)
    err = hipMemcpyAsync(&status_dev->rounds, &rounds, sizeof(rounds), hipMemcpyHostToDevice, s);
  unsigned long long reached = 0;
  VGT_TRY_HIP(ReadBack(s, err, &reached, &status_dev->reached), what);
  if (num_reached) *num_reached = static_cast<int64_t>(reached);
  return VGT_HIP_OK;
}

int CheckTraceArguments(const vgt_hip_ctx* ctx, const int32_t* toward, int64_t num_cells, const int32_t* starts,
                        int64_t num_starts, int32_t max_cells, const int32_t* paths, const int32_t* lengths,
                        const uint8_t* status)
{
  if (!ctx || !toward || !paths || !lengths || !status) return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "null argument");
  if (num_starts < 0) return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "the number of starts must not be negative");
  if (num_starts > 0 && !starts) return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "null argument");
  if (num_cells < 0 || num_cells >= 0x80000000LL)
    return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "path tracing supports grids below 2^31 cells");
  if (max_cells < 1) return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "max_cells must be at least 1");
  return VGT_HIP_OK;
}
}  // namespace

size_t vgt_hip_travel_cost_workspace_bytes(int64_t nx, int64_t ny, int64_t nz)
{
  if (!TravelShapeWithinLimits(nx, ny, nz) || nx * ny * nz == 0) return 0;
  return vgt::CarveTravelWorkspace(nx, ny, nz).bytes;
}

int vgt_hip_travel_cost_dev(vgt_hip_ctx* ctx, const float* field_dev, int64_t nx, int64_t ny, int64_t nz, int32_t mode,
                            int unknown_is_filled, double threshold, const uint32_t* weights, uint32_t flags,
                            const int32_t* sources_dev, const uint32_t* source_costs_dev, int64_t num_sources,
                            uint32_t cost_limit, uint32_t* cost_dev, int32_t* toward_dev, int64_t* num_reached,
                            void* workspace_dev, size_t workspace_bytes)
{
  vgt::TravelGrid grid;
  const int rc = CheckTravelArguments(ctx, field_dev, nx, ny, nz, &mode, threshold, weights, flags,
                                      sources_dev, num_sources, cost_limit, cost_dev, &grid);
  if (rc != VGT_HIP_OK) return rc;
  if (nx * ny * nz == 0)
  {
    if (num_reached) *num_reached = 0;
    return VGT_HIP_OK;
  }
  if (!workspace_dev) return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "null argument");
  if (workspace_bytes < vgt::CarveTravelWorkspace(nx, ny, nz).bytes)
    return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "travel-cost workspace too small");
  VGT_TRY_HIP(hipSetDevice(ctx->device), "set device");
  std::lock_guard<std::mutex> lock(ctx->mutex);
  return RunTravelCost(ctx->stream, field_dev, TravelSourceOf(mode), unknown_is_filled ? 1 : 0, threshold, grid,
                       sources_dev, source_costs_dev, num_sources, cost_dev, toward_dev, num_reached, workspace_dev);
}

int vgt_hip_travel_cost(vgt_hip_ctx* ctx, const float* field_host, int64_t nx, int64_t ny, int64_t nz, int32_t mode,
                        int unknown_is_filled, double threshold, const uint32_t* weights, uint32_t flags,
                        const int32_t* sources_host, const uint32_t* source_costs_host, int64_t num_sources,
                        uint32_t cost_limit, uint32_t* cost_host, int32_t* toward_host, int64_t* num_reached)
{
  vgt::TravelGrid grid;
  const int rc = CheckTravelArguments(ctx, field_host, nx, ny, nz, &mode, threshold, weights, flags,
                                      sources_host, num_sources, cost_limit, cost_host, &grid);
  if (rc != VGT_HIP_OK) return rc;
  if (nx * ny * nz == 0)
  {
    if (num_reached) *num_reached = 0;
    return VGT_HIP_OK;
  }
  VGT_TRY_HIP(hipSetDevice(ctx->device), "set device");
  const size_t n = static_cast<size_t>(nx * ny * nz), q = static_cast<size_t>(num_sources);
  vgt::HostStaging staging;
  const auto field = staging.In(field_host, n);
  const auto sources = staging.In(sources_host, q);
  const auto source_costs = staging.In(source_costs_host, q);
  const auto cost = staging.Out(cost_host, n);
  const auto toward = staging.Out(toward_host, n);
  const auto workspace = staging.Scratch(vgt::CarveTravelWorkspace(nx, ny, nz).bytes);
  int64_t reached = 0;
  const int result = staging.Run(*ctx, "travel cost", FailHip, [&](hipStream_t s) {
    return RunTravelCost(s, field.dev(), TravelSourceOf(mode), unknown_is_filled ? 1 : 0, threshold, grid, sources.dev(),
                         source_costs.dev(), num_sources, cost.dev(), toward.dev(), &reached, workspace.dev());
  });
  if (result == VGT_HIP_OK && num_reached) *num_reached = reached;
  return result;
}

int vgt_hip_cells_travel_cost(vgt_hip_ctx* ctx, vgt_hip_cells* cells, const uint32_t* objects_to_use,
                              int64_t num_objects, int unknown_is_filled, const uint32_t* weights, uint32_t flags,
                              const int32_t* sources_host, const uint32_t* source_costs_host, int64_t num_sources,
                              uint32_t cost_limit, uint32_t* cost_host, int32_t* toward_host, int64_t* num_reached)
{
  int rc = CheckCells(ctx, cells);
  if (rc != VGT_HIP_OK) return rc;
  if (num_objects < 0 || (num_objects > 0 && !objects_to_use)) return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "null argument");
  if (num_objects > 0 && cells->object_id_offset < 0)
    return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "this cell type carries no object id");
  vgt::TravelGrid grid;
  rc = CheckTravelArguments(ctx, cells, cells->nx, cells->ny, cells->nz, nullptr, 0.0, weights, flags, sources_host,
                            num_sources, cost_limit, cost_host, &grid);
  if (rc != VGT_HIP_OK) return rc;
  const int64_t cells_total = cells->nx * cells->ny * cells->nz;
  if (cells_total == 0)
  {
    if (num_reached) *num_reached = 0;
    return VGT_HIP_OK;
  }
  VGT_TRY_HIP(hipSetDevice(ctx->device), "set device");
  const char* what = "travel cost of a tagged map";
  // (sorted and distinct, as vgt_hip_cells_sdf hands the list to the same predicate kernel)
  std::vector<uint32_t> objects(objects_to_use, objects_to_use + num_objects);
  std::sort(objects.begin(), objects.end());
  objects.erase(std::unique(objects.begin(), objects.end()), objects.end());
  const size_t n = static_cast<size_t>(cells_total), q = static_cast<size_t>(num_sources);
  vgt::HostStaging staging;
  const auto sources = staging.In(sources_host, q);
  const auto source_costs = staging.In(source_costs_host, q);
  const auto cost = staging.Out(cost_host, n);
  const auto toward = staging.Out(toward_host, n);
  const auto workspace = staging.Scratch(vgt::CarveTravelWorkspace(cells->nx, cells->ny, cells->nz).bytes);
  int64_t reached = 0;
  const int result = staging.Run(*ctx, what, FailHip, [&](hipStream_t s) -> int {
    const int grown = GrowCache(s, &cells->objects, objects.size() * sizeof(uint32_t),
                                "drain before regrowing object list", "allocate object list");
    if (grown != VGT_HIP_OK) return grown;
    if (!objects.empty())  // (pageable source: staged when the call returns)
      VGT_TRY_HIP(hipMemcpyAsync(cells->objects.data(), objects.data(), objects.size() * sizeof(uint32_t),
                                 hipMemcpyHostToDevice, s),
                  what);
    VGT_TRY_HIP(vgt::LaunchCellMask(cells->records.as<void>(), cells_total, cells->cell_bytes, cells->object_id_offset,
                                    objects.empty() ? 0 : 1, cells->objects.as<uint32_t>(),
                                    static_cast<int>(objects.size()), unknown_is_filled ? 1 : 0,
                                    cells->mask.as<uint8_t>(), s),
                what);
    return RunTravelCost(s, cells->mask.as<uint8_t>(), vgt::kTravelFromMask, 0, 0.0, grid, sources.dev(),
                         source_costs.dev(), num_sources, cost.dev(), toward.dev(), &reached, workspace.dev());
  });
  if (result == VGT_HIP_OK && num_reached) *num_reached = reached;
  return result;
}

int vgt_hip_trace_paths_dev(vgt_hip_ctx* ctx, const int32_t* toward_dev, int64_t num_cells, const int32_t* starts_dev,
                            int64_t num_starts, int32_t max_cells, int32_t* paths_dev, int32_t* lengths_dev,
                            uint8_t* status_dev)
{
  const int rc = CheckTraceArguments(ctx, toward_dev, num_cells, starts_dev, num_starts, max_cells, paths_dev,
                                     lengths_dev, status_dev);
  if (rc != VGT_HIP_OK || num_starts == 0) return rc;
  VGT_TRY_HIP(hipSetDevice(ctx->device), "set device");
  std::lock_guard<std::mutex> lock(ctx->mutex);
  VGT_TRY_HIP(vgt::LaunchTracePaths(toward_dev, num_cells, starts_dev, num_starts, max_cells, paths_dev, lengths_dev,
                                    status_dev, ctx->stream),
              "trace paths");
  return VGT_HIP_OK;
}

int vgt_hip_trace_paths(vgt_hip_ctx* ctx, const int32_t* toward_host, int64_t num_cells, const int32_t* starts_host,
                        int64_t num_starts, int32_t max_cells, int32_t* paths_host, int32_t* lengths_host,
                        uint8_t* status_host)
{
  const int rc = CheckTraceArguments(ctx, toward_host, num_cells, starts_host, num_starts, max_cells, paths_host,
                                     lengths_host, status_host);
  if (rc != VGT_HIP_OK || num_starts == 0) return rc;
  VGT_TRY_HIP(hipSetDevice(ctx->device), "set device");
  const size_t q = static_cast<size_t>(num_starts);
  vgt::HostStaging staging;
  const auto toward = staging.In(toward_host, static_cast<size_t>(num_cells));
  const auto starts = staging.In(starts_host, q);
  // (up and down: the slots beyond a path's length come back as the caller gave them)
  const auto paths = staging.InOut(paths_host, q * static_cast<size_t>(max_cells));
  const auto lengths = staging.Out(lengths_host, q);
  const auto status = staging.Out(status_host, q);
  return staging.Run(*ctx, "trace paths", FailHip, [&](hipStream_t s) {
    return HipResult("trace paths", vgt::LaunchTracePaths(toward.dev(), num_cells, starts.dev(), num_starts, max_cells,
                                                          paths.dev(), lengths.dev(), status.dev(), s));
  });
}

/* ------------------------- holes and voids per component ------------------------- */

static_assert(sizeof(vgt_hip_component_topology_t) == 32 &&
                  sizeof(vgt::ComponentTopologyEntry) == sizeof(vgt_hip_component_topology_t),
              "the device table is the ABI's table");

namespace
{
// Everything that can be said about the arguments of the three entry points before any HIP call.
int CheckTopologyGrid(int64_t nx, int64_t ny, int64_t nz, int component_types)
{
  const int rc = CheckComponentGrid(nx, ny, nz);
  if (rc != VGT_HIP_OK) return rc;
  // (each extent is below 2^31 - 1 and their product too: no overflow in 64 bits)
  if ((nx + 1) * (ny + 1) >= 0x7fffffffLL || vgt::TopologyVertices(nx, ny, nz) >= 0x7fffffffLL)
    return Fail(VGT_HIP_ERR_INVALID_ARGUMENT,
                "component topology needs the vertex lattice (nx + 1)(ny + 1)(nz + 1) below 2^31 vertices");
  if (component_types < 1 || component_types > 7)
    return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "component types must be a combination of 1 (filled), 2 (empty), 4 (unknown)");
  return VGT_HIP_OK;
}

// The table of a labelled grid into out_host (num_components + 1 entries).  Caller holds the context mutex and has set
// the device.
int RunTopology(vgt_hip_ctx* ctx, const vgt::TopologyGrid& grid, vgt_hip_component_topology_t* out_host)
{
  const size_t table_bytes = (static_cast<size_t>(grid.num_components) + 1) * sizeof(vgt::ComponentTopologyEntry);
  vgt::DeviceTemp vertex_scratch, node_scratch, table_dev;
  unsigned long long num_nodes = 0;
  VGT_TRY_HIP(vertex_scratch.Allocate(vgt::TopologyVertexScratchBytes(grid.nx, grid.ny, grid.nz)), "component topology");
  VGT_TRY_HIP(table_dev.Allocate(table_bytes), "component topology");
  void* const vertices = vertex_scratch.as<void>();
  hipError_t err = vgt::LaunchTopologyCountNodes(grid, vertices, ctx->stream);
  VGT_TRY_HIP(ReadBack(ctx->stream, err, &num_nodes, vgt::TopologyNodeCountPtr(vertices, grid.nx, grid.ny, grid.nz)),
              "component topology");
  if (num_nodes >= 0x7fffffffULL)
    return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "component topology supports fewer than 2^31 surface nodes");
  if (num_nodes > 0)
    VGT_TRY_HIP(node_scratch.Allocate(vgt::TopologyNodeScratchBytes(static_cast<int64_t>(num_nodes))),
                "component topology");
  err = vgt::LaunchTopologyFromNodes(grid, vertices, static_cast<int64_t>(num_nodes), node_scratch.as<void>(),
                                     table_dev.as<vgt::ComponentTopologyEntry>(), ctx->stream);
  if (err == hipSuccess)
    err = hipMemcpyAsync(out_host, table_dev.as<void>(), table_bytes, hipMemcpyDeviceToHost, ctx->stream);
  VGT_TRY_HIP(DrainKeepingFirst(ctx->stream, err), "component topology");  // (the buffers go with the call)
  return VGT_HIP_OK;
}

// Labels the cells into a temporary device grid, then the table (and the labels, when asked for) to the host: one unit
// on the context.  Exactly one of the two sources is given: `occupancy_host`, which is uploaded (then records_dev is
// null and cell_bytes 4), or a handle's `records_dev` (then occupancy_host is null).
int LabelAndTopology(vgt_hip_ctx* ctx, const float* occupancy_host, const void* records_dev, int cell_bytes,
                     int object_id_offset, int mode, int64_t nx, int64_t ny, int64_t nz, int component_types,
                     uint32_t* labels_host, uint32_t* num_components, vgt_hip_component_topology_t* out_host,
                     uint64_t out_capacity)
{
  const size_t n = static_cast<size_t>(nx * ny * nz);
  vgt::HostStaging staging;
  const auto occupancy = staging.In(occupancy_host, n);
  const auto labels = labels_host ? staging.Out(labels_host, n) : staging.Scratch<uint32_t>(n * sizeof(uint32_t));
  return staging.Run(*ctx, "component topology", FailHip, [&](hipStream_t) {
    const void* const cells_dev = occupancy_host ? occupancy.dev() : records_dev;
    uint32_t count = 0;
    const int rc = RunLabelling(ctx, cells_dev, cell_bytes, object_id_offset, mode, nullptr, 0.0, nx, ny, nz,
                                labels.dev(), &count);
    if (rc != VGT_HIP_OK) return rc;
    *num_components = count;
    if (out_capacity < static_cast<uint64_t>(count) + 1)
      return Fail(VGT_HIP_ERR_INVALID_ARGUMENT,
                  "the topology table needs num_components + 1 = " + std::to_string(static_cast<uint64_t>(count) + 1) +
                      " entries, out_capacity is " + std::to_string(out_capacity));
    return RunTopology(ctx, vgt::TopologyGrid{cells_dev, cell_bytes, labels.dev(), nx, ny, nz, component_types, count},
                       out_host);
  });
}
}  // namespace

int vgt_hip_component_topology_dev(vgt_hip_ctx* ctx, const float* occupancy_dev, const uint32_t* labels_dev,
                                   int64_t nx, int64_t ny, int64_t nz, int component_types, uint32_t num_components,
                                   vgt_hip_component_topology_t* out_host)
{
  const int rc = CheckTopologyGrid(nx, ny, nz, component_types);
  if (rc != VGT_HIP_OK) return rc;
  if (static_cast<int64_t>(num_components) > nx * ny * nz)
    return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "a grid cannot hold more components than cells");
  if (!ctx || !occupancy_dev || !labels_dev || !out_host) return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "null argument");
  VGT_TRY_HIP(hipSetDevice(ctx->device), "set device");
  std::lock_guard<std::mutex> lock(ctx->mutex);
  return RunTopology(ctx, vgt::TopologyGrid{occupancy_dev, 4, labels_dev, nx, ny, nz, component_types, num_components},
                     out_host);
}

int vgt_hip_component_topology(vgt_hip_ctx* ctx, const float* occupancy_host, int64_t nx, int64_t ny, int64_t nz,
                               int component_types, uint32_t* labels_host, uint32_t* num_components,
                               vgt_hip_component_topology_t* out_host, uint64_t out_capacity)
{
  const int rc = CheckTopologyGrid(nx, ny, nz, component_types);
  if (rc != VGT_HIP_OK) return rc;
  if (!ctx || !occupancy_host || !num_components || !out_host)
    return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "null argument");
  VGT_TRY_HIP(hipSetDevice(ctx->device), "set device");
  return LabelAndTopology(ctx, occupancy_host, nullptr, 4, -1, vgt::kComponentClasses, nx, ny, nz, component_types,
                          labels_host, num_components, out_host, out_capacity);
}

int vgt_hip_cells_component_topology(vgt_hip_ctx* ctx, vgt_hip_cells* cells, int connect_across_objects,
                                     int component_types, uint32_t* labels_host, uint32_t* num_components,
                                     vgt_hip_component_topology_t* out_host, uint64_t out_capacity)
{
  if (component_types < 1 || component_types > 7)
    return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "component types must be a combination of 1 (filled), 2 (empty), 4 (unknown)");
  int rc = CheckCells(ctx, cells);
  if (rc != VGT_HIP_OK) return rc;
  if (!num_components || !out_host) return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "null argument");
  rc = CheckTopologyGrid(cells->nx, cells->ny, cells->nz, component_types);
  if (rc != VGT_HIP_OK) return rc;
  VGT_TRY_HIP(hipSetDevice(ctx->device), "set device");
  const bool by_object = cells->object_id_offset >= 0 && !connect_across_objects;
  return LabelAndTopology(ctx, nullptr, cells->records.as<void>(), cells->cell_bytes, cells->object_id_offset,
                          by_object ? vgt::kComponentClassesAndIds : vgt::kComponentClasses, cells->nx, cells->ny,
                          cells->nz, component_types, labels_host, num_components, out_host, out_capacity);
}

/* ------------------------------ mesh rasterizer ------------------------------ */

namespace
{
constexpr int64_t kMeshMaxCells = int64_t{1} << 40;
constexpr int64_t kMeshMaxTriangles = 0x7fffffffLL;

// Everything that can be said about the arguments of the two entry points before any HIP call.
int CheckMeshArguments(const vgt_hip_ctx* ctx, const void* vertices, int64_t num_vertices, const void* triangles,
                       int64_t num_triangles, const void* cells, int cell_bytes, int64_t nx, int64_t ny, int64_t nz,
                       double resolution, const double* world_from_grid, const double* grid_from_world, int rule)
{
  if (!ctx || !vertices || !triangles || !cells) return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "null argument");
  if (num_vertices < 0 || num_triangles < 0)
    return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "the numbers of vertices and triangles must not be negative");
  if (num_triangles > kMeshMaxTriangles) return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "at most 2^31 - 1 triangles per call");
  if (nx <= 0 || ny <= 0 || nz <= 0) return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "grid extents must be positive");
  if (nx > kMeshMaxCells || ny > kMeshMaxCells / nx || nz > kMeshMaxCells / (nx * ny))
    return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "the mesh rasterizer supports grids of at most 2^40 cells");
  if (!(resolution > 0.0) || !std::isfinite(resolution))
    return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "resolution must be finite and greater than zero");
  if (cell_bytes != 4 && cell_bytes != 8)
    return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "cell_bytes must be 4 (OccupancyCell) or 8 (OccupancyComponentCell)");
  if (rule != VGT_HIP_MESH_RULE_REFERENCE && rule != VGT_HIP_MESH_RULE_NEAREST)
    return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "rule must be 0 (reference) or 1 (nearest)");
  if ((world_from_grid == nullptr) != (grid_from_world == nullptr))
    return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "give both transforms (world_from_grid and grid_from_world) or neither");
  return VGT_HIP_OK;
}

vgt::MeshGrid MakeMeshGrid(int cell_bytes, int64_t nx, int64_t ny, int64_t nz, double resolution,
                           const double* world_from_grid, const double* grid_from_world, int enforce_contains, int rule)
{
  vgt::MeshGrid grid{};
  grid.nx = nx;
  grid.ny = ny;
  grid.nz = nz;
  grid.resolution = resolution;
  // S/mesh_rasterizer.cpp:117-119, in that form
  const double min_check_radius = resolution * 0.5;
  const double max_check_radius = min_check_radius * std::sqrt(3.0);
  grid.max_check_radius_squared = std::pow(max_check_radius, 2.0);
  grid.has_transform = world_from_grid ? 1 : 0;
  if (world_from_grid)
  {
    std::memcpy(grid.world_from_grid, world_from_grid, sizeof(grid.world_from_grid));
    std::memcpy(grid.grid_from_world, grid_from_world, sizeof(grid.grid_from_world));
  }
  grid.enforce = enforce_contains ? 1 : 0;
  grid.rule = rule;
  grid.cell_bytes = cell_bytes;
  return grid;
}

// Set-up, the checks between the two steps, the bricks.  Caller holds the context mutex and has set the device.  Waits
// for the set-up's findings; under `enforce` also for the bricks' (otherwise the bricks are left enqueued).
int RunMeshRasterize(vgt_hip_ctx* ctx, const double* vertices_dev, int64_t num_vertices, const int32_t* triangles_dev,
                     int64_t num_triangles, void* cells_dev, const vgt::MeshGrid& grid)
{
  const size_t need = vgt::MeshScratchBytes(num_triangles);
  const int grown = GrowCache(ctx->stream, &ctx->mesh_ws, need, "drain before regrowing the mesh scratch",
                              "allocate mesh scratch");
  if (grown != VGT_HIP_OK) return grown;
  void* const scratch = ctx->mesh_ws.data();
  vgt::MeshTotals totals{};
  vgt::MeshStatus status{};
  hipError_t err = vgt::LaunchMeshSetup(vertices_dev, num_vertices, triangles_dev, num_triangles, grid, scratch, ctx->stream);
  if (err == hipSuccess)
    err = hipMemcpyAsync(&totals, vgt::MeshTotalsPtr(scratch, num_triangles), sizeof(totals), hipMemcpyDeviceToHost,
                         ctx->stream);
  VGT_TRY_HIP(ReadBack(ctx->stream, err, &status, vgt::MeshStatusPtr(scratch, num_triangles)), "mesh set-up");
  if (status.bits & vgt::kMeshBadIndex)
    return Fail(VGT_HIP_ERR_INVALID_ARGUMENT,
                "triangle " + std::to_string(status.first[0]) + " has a vertex index out of range");
  if (status.bits & vgt::kMeshNonFinite)
    return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "triangle " + std::to_string(status.first[1]) + " has a non-finite vertex");
  if (status.bits & vgt::kMeshDegenerate)
    return Fail(VGT_HIP_ERR_INVALID_ARGUMENT,
                "triangle " + std::to_string(status.first[2]) + " is degenerate (its normal has zero length)");
  if (totals.cells > vgt::kMeshMaxCandidateCells)
    return Fail(VGT_HIP_ERR_INVALID_ARGUMENT,
                "the triangles' index ranges hold more than 2^36 candidate cells: refused (is the mesh inside the map?)");
  VGT_TRY_HIP(vgt::LaunchMeshBricks(grid, num_triangles, totals.bricks, scratch, cells_dev, ctx->stream), "mesh bricks");
  if (!grid.enforce) return VGT_HIP_OK;
  VGT_TRY_HIP(ReadBack(ctx->stream, hipSuccess, &status, vgt::MeshStatusPtr(scratch, num_triangles)), "mesh bricks");
  if (status.bits & vgt::kMeshNotContained)
    return Fail(VGT_HIP_ERR_RUNTIME,
                "Triangle is not contained by occupancy map (triangle " + std::to_string(status.first[3]) + ")");
  return VGT_HIP_OK;
}
}  // namespace

int vgt_hip_rasterize_mesh_dev(vgt_hip_ctx* ctx, const double* vertices_xyz_dev, int64_t num_vertices,
                               const int32_t* triangles_dev, int64_t num_triangles, void* cells_dev, int cell_bytes,
                               int64_t nx, int64_t ny, int64_t nz, double resolution, const double* world_from_grid,
                               const double* grid_from_world, int enforce_contains, int rule)
{
  const int rc = CheckMeshArguments(ctx, vertices_xyz_dev, num_vertices, triangles_dev, num_triangles, cells_dev,
                                    cell_bytes, nx, ny, nz, resolution, world_from_grid, grid_from_world, rule);
  if (rc != VGT_HIP_OK) return rc;
  if (num_triangles == 0) return VGT_HIP_OK;
  VGT_TRY_HIP(hipSetDevice(ctx->device), "set device");
  const vgt::MeshGrid grid =
      MakeMeshGrid(cell_bytes, nx, ny, nz, resolution, world_from_grid, grid_from_world, enforce_contains, rule);
  std::lock_guard<std::mutex> lock(ctx->mutex);
  return RunMeshRasterize(ctx, vertices_xyz_dev, num_vertices, triangles_dev, num_triangles, cells_dev, grid);
}

int vgt_hip_rasterize_mesh(vgt_hip_ctx* ctx, const double* vertices_xyz_host, int64_t num_vertices,
                           const int32_t* triangles_host, int64_t num_triangles, void* cells_host, int cell_bytes,
                           int64_t nx, int64_t ny, int64_t nz, double resolution, const double* world_from_grid,
                           const double* grid_from_world, int enforce_contains, int rule)
{
  const int rc = CheckMeshArguments(ctx, vertices_xyz_host, num_vertices, triangles_host, num_triangles, cells_host,
                                    cell_bytes, nx, ny, nz, resolution, world_from_grid, grid_from_world, rule);
  if (rc != VGT_HIP_OK) return rc;
  if (num_triangles == 0) return VGT_HIP_OK;
  VGT_TRY_HIP(hipSetDevice(ctx->device), "set device");
  const vgt::MeshGrid grid =
      MakeMeshGrid(cell_bytes, nx, ny, nz, resolution, world_from_grid, grid_from_world, enforce_contains, rule);
  vgt::HostStaging staging;
  const auto vertices = staging.In(vertices_xyz_host, static_cast<size_t>(num_vertices) * 3);
  const auto triangles = staging.In(triangles_host, static_cast<size_t>(num_triangles) * 3);
  const auto map = staging.InOut(static_cast<char*>(cells_host), static_cast<size_t>(nx * ny * nz) * cell_bytes);
  return staging.Run(*ctx, "rasterize mesh", FailHip, [&](hipStream_t) {
    return RunMeshRasterize(ctx, vertices.dev(), num_vertices, triangles.dev(), num_triangles, map.dev(), grid);
  });
}

int vgt_hip_mesh_grid_for(const double* vertices_xyz_host, int64_t num_vertices, double resolution, int64_t* nx,
                          int64_t* ny, int64_t* nz, double* origin_xyz)
{
  if (!vertices_xyz_host || !nx || !ny || !nz || !origin_xyz) return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "null argument");
  if (num_vertices <= 0) return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "a mesh needs at least one vertex");
  if (!(resolution > 0.0) || !std::isfinite(resolution))
    return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "resolution must be finite and greater than zero");
  // S/mesh_rasterizer.cpp:243-269
  double lower[3], upper[3];
  for (int a = 0; a < 3; a++)
  {
    lower[a] = std::numeric_limits<double>::infinity();
    upper[a] = -std::numeric_limits<double>::infinity();
  }
  for (int64_t i = 0; i < num_vertices; i++)
    for (int a = 0; a < 3; a++)
    {
      const double v = vertices_xyz_host[3 * i + a];
      if (!std::isfinite(v)) return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "vertex " + std::to_string(i) + " is not finite");
      lower[a] = v < lower[a] ? v : lower[a];
      upper[a] = v > upper[a] ? v : upper[a];
    }
  const double buffer_size = resolution * 2.0;
  int64_t counts[3];
  for (int a = 0; a < 3; a++)
  {
    const double object_size = upper[a] - lower[a];
    const double grid_dimension = object_size + buffer_size;
    const double cells = std::ceil(grid_dimension / resolution);  // VoxelGridSizes::FromGridSizes
    if (!(cells >= 1.0 && cells <= 2147483647.0))
      return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "the mesh needs more than 2^31 - 1 cells along an axis at this resolution");
    counts[a] = static_cast<int64_t>(cells);
  }
  *nx = counts[0];
  *ny = counts[1];
  *nz = counts[2];
  for (int a = 0; a < 3; a++) origin_xyz[a] = lower[a] - resolution;
  return VGT_HIP_OK;
}

/* --------------------------------- multi-GPU --------------------------------- */

size_t vgt_hip_sdf_slab_summary_bytes(int64_t nx, int64_t ny)
{
  if (nx <= 0 || ny <= 0) return 0;
  return static_cast<size_t>(nx) * static_cast<size_t>(ny) * sizeof(vgt::SlabLineSummary);
}

namespace
{
// Times `count` consecutive kernel groups with events when kernel_ms is requested.
struct StageTimer
{
  hipEvent_t ev[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
  int n = 0;
  bool enabled = false;
  int Init(bool on, int stages)
  {
    enabled = on;
    if (!on) return VGT_HIP_OK;
    for (int i = 0; i <= stages; i++)
    {
      const hipError_t err = hipEventCreate(&ev[i]);
      if (err != hipSuccess) return FailHip("create event", err);
      n = i + 1;
    }
    return VGT_HIP_OK;
  }
  hipError_t Mark(int i, hipStream_t s) { return enabled ? hipEventRecord(ev[i], s) : hipSuccess; }
  int Finish(hipStream_t s, float* out, int stages)
  {
    if (!enabled) return VGT_HIP_OK;
    hipError_t err = hipStreamSynchronize(s);
    for (int i = 0; i < stages && err == hipSuccess; i++)
      err = hipEventElapsedTime(&out[i], ev[i], ev[i + 1]);
    return err == hipSuccess ? VGT_HIP_OK : FailHip("stage timing", err);
  }
  ~StageTimer()
  {
    for (int i = 0; i < n; i++)
      if (ev[i]) (void)hipEventDestroy(ev[i]);
  }
};
}  // namespace

int vgt_hip_sdf_slab_begin_dev(vgt_hip_ctx* ctx, const float* occupancy_dev, int64_t nx, int64_t ny,
                               int64_t nz_local, int64_t z_offset, int unknown_is_filled,
                               void* workspace_dev, size_t workspace_bytes, void* summary_dev,
                               float* kernel_ms)
{
  if (!ctx || !occupancy_dev || !workspace_dev || !summary_dev)
    return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "null argument");
  const int rc = CheckSdfShape(nx, ny, nz_local, 1.0);
  if (rc != VGT_HIP_OK) return rc;
  if (z_offset < 0 || z_offset + nz_local > vgt::kMaxExtent)
    return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "slab lies outside the supported Z extent");
  VGT_TRY_HIP(hipSetDevice(ctx->device), "set device");
  vgt::SdfParams p{nx, ny, nz_local, 1.0, unknown_is_filled ? 1 : 0, 0};
  p.z_offset = z_offset;
  const SdfWorkspace ws = CarveWorkspace(workspace_dev, nx, ny, nz_local, ctx->variant);
  if (workspace_bytes < ws.bytes) return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "SDF workspace too small");
  StageTimer timer;
  const int trc = timer.Init(kernel_ms != nullptr, 1);
  if (trc != VGT_HIP_OK) return trc;
  std::lock_guard<std::mutex> lock(ctx->mutex);
  hipEvent_t* slot = kernel_ms ? nullptr : TimingSlot(ctx);
  VGT_TRY_HIP(timer.Mark(0, ctx->stream), "event record");
  if (slot) VGT_TRY_HIP(hipEventRecord(slot[0], ctx->stream), "event record");
  VGT_TRY_HIP(LaunchPassOne<float>(occupancy_dev, ws, p, 0, static_cast<vgt::SlabLineSummary*>(summary_dev), ctx->stream),
              "pass 1");
  if (slot) VGT_TRY_HIP(hipEventRecord(slot[1], ctx->stream), "event record");
  VGT_TRY_HIP(timer.Mark(1, ctx->stream), "event record");
  return timer.Finish(ctx->stream, kernel_ms, 1);
}

int vgt_hip_sdf_slab_range(int64_t nz_global, int32_t world, int32_t rank, int64_t* z_offset, int64_t* nz_local)
{
  if (!z_offset || !nz_local) return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "null argument");
  if (nz_global <= 0 || world <= 0 || world > nz_global || rank < 0 || rank >= world)
    return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "invalid slab partition");
  vgt::SlabRange(nz_global, world, rank, z_offset, nz_local);
  return VGT_HIP_OK;
}

size_t vgt_hip_sdf_slab_carries_bytes(int64_t nx, int64_t ny)
{
  if (nx <= 0 || ny <= 0) return 0;
  return static_cast<size_t>(nx) * static_cast<size_t>(ny) * sizeof(vgt::SlabLineCarry);
}

int vgt_hip_sdf_slab_carries_dev(vgt_hip_ctx* ctx, const void* gathered_summaries_dev, int32_t world,
                                 int32_t rank, int64_t nx, int64_t ny, int64_t nz_global, void* carries_dev)
{
  if (!ctx || !gathered_summaries_dev || !carries_dev)
    return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "null argument");
  if (world <= 0 || rank < 0 || rank >= world || nx <= 0 || ny <= 0 || nz_global < world ||
      nz_global > vgt::kMaxExtent)
    return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "invalid slab partition");
  VGT_TRY_HIP(hipSetDevice(ctx->device), "set device");
  std::lock_guard<std::mutex> lock(ctx->mutex);
  VGT_TRY_HIP(vgt::LaunchSlabCarries(static_cast<const vgt::SlabLineSummary*>(gathered_summaries_dev), world, rank,
                                     nx * ny, nz_global, static_cast<vgt::SlabLineCarry*>(carries_dev), ctx->stream),
              "slab carries");
  // the carries hold for the slab that vgt_hip_sdf_slab_range gives this rank, and for no other
  vgt_hip_ctx::SlabNote note{0, 0, nz_global};
  vgt::SlabRange(nz_global, world, rank, &note.z_offset, &note.nz_local);
  if (ctx->slab_notes.size() > 64) ctx->slab_notes.clear();
  ctx->slab_notes[carries_dev] = note;
  return VGT_HIP_OK;
}

int vgt_hip_sdf_slab_finish_dev(vgt_hip_ctx* ctx, int64_t nx, int64_t ny, int64_t nz_local,
                                int64_t z_offset, int64_t nz_global, double resolution,
                                int add_virtual_border, const void* carries_dev, float* sdf_dev,
                                void* workspace_dev, size_t workspace_bytes, float* minmax_dev,
                                float* kernel_ms)
{
  if (!ctx || !carries_dev || !sdf_dev || !workspace_dev)
    return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "null argument");
  const int rc = CheckSdfShape(nx, ny, nz_local, resolution);
  if (rc != VGT_HIP_OK) return rc;
  if (z_offset < 0 || nz_global < z_offset + nz_local || nz_global > vgt::kMaxExtent)
    return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "slab lies outside the global Z extent");
  VGT_TRY_HIP(hipSetDevice(ctx->device), "set device");
  vgt::SdfParams p{nx, ny, nz_local, resolution, 0, add_virtual_border ? 1 : 0};
  p.z_offset = z_offset;
  p.nz_global = nz_global;
  const SdfWorkspace ws = CarveWorkspace(workspace_dev, nx, ny, nz_local, ctx->variant);
  if (workspace_bytes < ws.bytes) return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "SDF workspace too small");
  StageTimer timer;
  const int trc = timer.Init(kernel_ms != nullptr, 3);
  if (trc != VGT_HIP_OK) return trc;
  std::lock_guard<std::mutex> lock(ctx->mutex);
  {
    const auto note = ctx->slab_notes.find(carries_dev);
    if (note != ctx->slab_notes.end())
    {
      const bool other = note->second.z_offset != z_offset || note->second.nz_local != nz_local ||
                         note->second.nz_global != nz_global;
      // (consumed either way: a later buffer at the same address -- a caching allocator's reuse -- starts without a note)
      ctx->slab_notes.erase(note);
      if (other)
        return Fail(VGT_HIP_ERR_INVALID_ARGUMENT,
                    "the carries were computed for another slab: slabs must be the ranges of vgt_hip_sdf_slab_range");
    }
  }
  hipStream_t s = ctx->stream;
  hipEvent_t* slot = kernel_ms ? nullptr : TimingSlot(ctx);
  VGT_TRY_HIP(vgt::LaunchInitMinMax(ws.minmax_enc, s), "init min/max");
  VGT_TRY_HIP(timer.Mark(0, s), "event record");
  if (slot) VGT_TRY_HIP(hipEventRecord(slot[4], s), "event record");
  VGT_TRY_HIP(LaunchSlabFixup(ws, static_cast<const vgt::SlabLineCarry*>(carries_dev), p, s), "slab fix-up");
  VGT_TRY_HIP(timer.Mark(1, s), "event record");
  if (slot) VGT_TRY_HIP(hipEventRecord(slot[5], s), "event record");
  VGT_TRY_HIP(LaunchPassTwo(ws, p, 0, s), "Y pass");
  VGT_TRY_HIP(timer.Mark(2, s), "event record");
  if (slot) VGT_TRY_HIP(hipEventRecord(slot[6], s), "event record");
  VGT_TRY_HIP(LaunchPassThree(ws, p, sdf_dev, s), "X pass");
  VGT_TRY_HIP(timer.Mark(3, s), "event record");
  if (slot)
  {
    VGT_TRY_HIP(hipEventRecord(slot[7], s), "event record");
    ctx->timing_kind[static_cast<size_t>(ctx->timing_used++)] = 2;
  }
  if (minmax_dev) VGT_TRY_HIP(vgt::LaunchDecodeMinMax(ws.minmax_enc, minmax_dev, s), "min/max");
  return timer.Finish(s, kernel_ms, 3);
}

/* ------------------- forward kinematics and the clearance gradient in joint space ------------------- */

namespace
{
constexpr int64_t kTwoTo31 = int64_t{1} << 31;

// The checks of the two forward-kinematics entry points; *done: nothing is left to do (B == 0).
int CheckForwardKinematics(const vgt_hip_ctx* ctx, const vgt_hip_kinematics* tree, const double* joint_values,
                           int64_t num_configurations, const double* link_poses, bool* done)
{
  *done = false;
  if (!ctx || !tree || !link_poses) return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "null argument");
  if (num_configurations < 0) return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "negative number of configurations");
  if (num_configurations >= kTwoTo31)
    return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "forward kinematics supports fewer than 2^31 configurations");
  if (num_configurations == 0)
  {
    *done = true;  // (before the tree is looked at)
    return VGT_HIP_OK;
  }
  if (tree->ctx != ctx) return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "the kinematic tree belongs to another context");
  if (tree->num_joints > 0 && !joint_values) return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "null argument");
  if (num_configurations * tree->num_links >= kTwoTo31)
    return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "forward kinematics supports fewer than 2^31 (configuration, link) pairs");
  return VGT_HIP_OK;
}

// Enqueues one forward kinematics on `stream`; the context's mutex is held (the tree's limits buffer is one per tree).
hipError_t EnqueueForwardKinematics(const vgt_hip_kinematics* tree, const double* joint_values_dev,
                                    int64_t num_configurations, const double* world_from_base,
                                    const double* joint_limits, double* link_poses_dev, uint8_t* status_dev,
                                    hipStream_t stream)
{
  const bool limited = joint_limits && tree->num_joints > 0;
  if (limited)
  {
    // (pageable host memory: the runtime has taken its copy when the call returns)
    const hipError_t err = hipMemcpyAsync(tree->limits.as<double>(), joint_limits,
                                          static_cast<size_t>(tree->num_joints) * 2 * sizeof(double),
                                          hipMemcpyHostToDevice, stream);
    if (err != hipSuccess) return err;
  }
  return vgt::LaunchForwardKinematics(tree->links.as<vgt::KinematicLink>(), tree->num_links, tree->num_joints,
                                      tree->lds_links, joint_values_dev, num_configurations, world_from_base,
                                      limited ? tree->limits.as<double>() : nullptr, link_poses_dev, status_dev,
                                      g_kinematics_workgroups.load(), stream);
}

struct JointGradientArguments
{
  const vgt_hip_kinematics* tree;
  const double* link_poses;
  int64_t num_configurations;
  const double* sphere_xyzr;
  const int32_t* sphere_link;
  int64_t num_spheres;
  const int32_t* min_sphere;
  const double* min_gradient;
  const double* sphere_weight;
  const double* sphere_gradient;
  double* joint_gradient;

  bool Worst() const { return min_sphere != nullptr; }
  // *done: nothing is left to do (B == 0 or J == 0).
  int Check(const vgt_hip_ctx* ctx, bool* done) const
  {
    *done = false;
    if (!ctx || !tree) return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "null argument");
    const bool worst = min_sphere && min_gradient, summed = sphere_weight && sphere_gradient;
    const bool any_worst = min_sphere || min_gradient, any_summed = sphere_weight || sphere_gradient;
    if (worst == summed || any_worst != worst || any_summed != summed)
      return Fail(VGT_HIP_ERR_INVALID_ARGUMENT,
                  "exactly one pair of (min_sphere, min_gradient) and (sphere_weight, sphere_gradient) must be given");
    if (num_configurations < 0 || num_spheres < 0) return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "negative count");
    if (num_configurations >= kTwoTo31 || num_spheres >= kTwoTo31)
      return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "the joint gradient supports fewer than 2^31 configurations and spheres");
    if (num_configurations == 0)
    {
      *done = true;  // (before the tree is looked at)
      return VGT_HIP_OK;
    }
    if (tree->ctx != ctx) return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "the kinematic tree belongs to another context");
    if (tree->num_joints == 0)
    {
      *done = true;
      return VGT_HIP_OK;
    }
    if (!link_poses || !joint_gradient || (num_spheres > 0 && (!sphere_xyzr || !sphere_link)))
      return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "null argument");
    if (num_configurations * tree->num_links >= kTwoTo31 || num_configurations * tree->num_joints >= kTwoTo31 ||
        num_configurations * num_spheres >= kTwoTo31)
      return Fail(VGT_HIP_ERR_INVALID_ARGUMENT,
                  "the joint gradient supports fewer than 2^31 (configuration, link), (configuration, joint) and "
                  "(configuration, sphere) pairs");
    return VGT_HIP_OK;
  }
  hipError_t Launch(const double* poses_dev, const double* xyzr_dev, const int32_t* link_dev, const int32_t* min_sphere_dev,
                    const double* min_gradient_dev, const double* weight_dev, const double* gradient_dev,
                    double* joint_gradient_dev, hipStream_t stream) const
  {
    return vgt::LaunchClearanceJointGradient(tree->links.as<vgt::KinematicLink>(), tree->num_links, tree->num_joints,
                                             poses_dev, num_configurations, xyzr_dev, link_dev, num_spheres,
                                             min_sphere_dev, min_gradient_dev, weight_dev, gradient_dev,
                                             joint_gradient_dev, g_kinematics_workgroups.load(), stream);
  }
};
}  // namespace

int vgt_hip_kinematics_create(vgt_hip_ctx* ctx, int64_t num_links, int64_t num_joints, const int32_t* parent,
                              const int32_t* joint_type, const int32_t* joint_index, const double* axis,
                              const double* origin, vgt_hip_kinematics** out_tree)
{
  if (out_tree) *out_tree = nullptr;
  if (!ctx || !parent || !joint_type || !joint_index || !axis || !origin || !out_tree)
    return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "null argument");
  if (num_links <= 0) return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "a kinematic tree needs at least one link");
  if (num_links >= kTwoTo31) return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "a kinematic tree has fewer than 2^31 links");
  if (num_joints < 0) return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "negative number of joints");
  for (int64_t i = 0; i < num_links; i++)
  {
    const std::string name = "link " + std::to_string(i) + ": ";
    if (parent[i] < -1 || parent[i] >= i)
      return Fail(VGT_HIP_ERR_INVALID_ARGUMENT,
                  name + "parent " + std::to_string(parent[i]) + " is not below " + std::to_string(i));
    if (joint_type[i] != VGT_HIP_JOINT_FIXED && joint_type[i] != VGT_HIP_JOINT_REVOLUTE &&
        joint_type[i] != VGT_HIP_JOINT_PRISMATIC)
      return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, name + "joint type " + std::to_string(joint_type[i]) + " is unknown");
    if (joint_type[i] != VGT_HIP_JOINT_FIXED && (joint_index[i] < 0 || joint_index[i] >= num_joints))
      return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, name + "joint index " + std::to_string(joint_index[i]) +
                                                    " is not in [0, " + std::to_string(num_joints) + ")");
  }
  std::vector<vgt::KinematicLink> links;
  try
  {
    links.resize(static_cast<size_t>(num_links));
  }
  catch (const std::bad_alloc&)
  {
    return Fail(VGT_HIP_ERR_RUNTIME, "out of host memory");
  }
  for (int64_t i = 0; i < num_links; i++)
  {
    vgt::KinematicLink& link = links[static_cast<size_t>(i)];
    link.parent = parent[i];
    link.joint_type = joint_type[i];
    link.joint_index = joint_type[i] == VGT_HIP_JOINT_FIXED ? 0 : joint_index[i];
    link.reserved = 0;
    for (int k = 0; k < 3; k++) link.axis[k] = axis[3 * i + k];
    for (int c = 0; c < 4; c++)
      for (int r = 0; r < 3; r++) link.origin[3 * c + r] = origin[16 * i + 4 * c + r];
  }
  VGT_TRY_HIP(hipSetDevice(ctx->device), "set device");
  vgt_hip_kinematics* tree = new (std::nothrow) vgt_hip_kinematics();
  if (!tree) return Fail(VGT_HIP_ERR_RUNTIME, "out of host memory");
  tree->ctx = ctx;
  tree->device = ctx->device;
  tree->num_links = num_links;
  tree->num_joints = num_joints;
  tree->lds_links = vgt::AssignKinematicsLdsSlots(links.data(), num_links);
  const size_t bytes = links.size() * sizeof(vgt::KinematicLink);
  hipError_t err = tree->links.Allocate(bytes);
  if (err == hipSuccess) err = tree->limits.Allocate(static_cast<size_t>(num_joints > 0 ? num_joints : 1) * 2 * sizeof(double));
  if (err == hipSuccess) err = tree->chain.Allocate(static_cast<size_t>(num_links) * sizeof(int32_t));
  if (err == hipSuccess)
  {
    std::lock_guard<std::mutex> lock(ctx->mutex);
    err = hipMemcpyAsync(tree->links.as<void>(), links.data(), bytes, hipMemcpyHostToDevice, ctx->stream);
    err = DrainKeepingFirst(ctx->stream, err);  // (`links` goes with this scope)
  }
  if (err != hipSuccess)
  {
    delete tree;
    return FailHip("Failed to upload the kinematic tree", err);
  }
  tree->host_links = std::move(links);
  AdoptChild(ctx);
  *out_tree = tree;
  return VGT_HIP_OK;
}

void vgt_hip_kinematics_destroy(vgt_hip_kinematics* tree)
{
  if (!tree) return;
  vgt_hip_ctx* const ctx = tree->ctx;
  const int device = tree->device;
  // (ReleaseChild waits for the work that may still read the tree; the buffers go after it, the context's record -- the
  // handle's reference may be its last -- is not touched again)
  ReleaseChild(ctx, device);
  delete tree;
}

int64_t vgt_hip_kinematics_num_links(const vgt_hip_kinematics* tree) { return tree ? tree->num_links : 0; }
int64_t vgt_hip_kinematics_num_joints(const vgt_hip_kinematics* tree) { return tree ? tree->num_joints : 0; }
int32_t vgt_hip_kinematics_lds_links(void) { return vgt::kKinematicsLdsLinks; }

int vgt_hip_forward_kinematics_dev(vgt_hip_ctx* ctx, const vgt_hip_kinematics* tree, const double* joint_values_dev,
                                   int64_t num_configurations, const double* world_from_base,
                                   const double* joint_limits, double* link_poses_dev, uint8_t* status_dev)
{
  bool done = false;
  const int rc = CheckForwardKinematics(ctx, tree, joint_values_dev, num_configurations, link_poses_dev, &done);
  if (rc != VGT_HIP_OK || done) return rc;
  VGT_TRY_HIP(hipSetDevice(ctx->device), "set device");
  std::lock_guard<std::mutex> lock(ctx->mutex);
  VGT_TRY_HIP(EnqueueForwardKinematics(tree, joint_values_dev, num_configurations, world_from_base, joint_limits,
                                       link_poses_dev, status_dev, ctx->stream),
              "forward kinematics");
  return VGT_HIP_OK;
}

int vgt_hip_forward_kinematics(vgt_hip_ctx* ctx, const vgt_hip_kinematics* tree, const double* joint_values_host,
                               int64_t num_configurations, const double* world_from_base, const double* joint_limits,
                               double* link_poses_host, uint8_t* status_host)
{
  bool done = false;
  const int rc = CheckForwardKinematics(ctx, tree, joint_values_host, num_configurations, link_poses_host, &done);
  if (rc != VGT_HIP_OK || done) return rc;
  VGT_TRY_HIP(hipSetDevice(ctx->device), "set device");
  const char* what = "forward kinematics";
  const size_t b = static_cast<size_t>(num_configurations);
  vgt::HostStaging staging;
  // (a tree without joints: one double stands in, so that the kernel has an address it never reads)
  const double none = 0.0;
  const auto values = tree->num_joints > 0 ? staging.In(joint_values_host, b * static_cast<size_t>(tree->num_joints))
                                           : staging.In(&none, 1);
  const auto poses = staging.Out(link_poses_host, b * static_cast<size_t>(tree->num_links) * 16);
  const auto status = staging.Out(status_host, b);
  return staging.Run(*ctx, what, FailHip, [&](hipStream_t s) {
    return HipResult(what, EnqueueForwardKinematics(tree, values.dev(), num_configurations, world_from_base,
                                                    joint_limits, poses.dev(), status.dev(), s));
  });
}

int vgt_hip_clearance_joint_gradient_dev(vgt_hip_ctx* ctx, const vgt_hip_kinematics* tree, const double* link_poses_dev,
                                         int64_t num_configurations, const double* sphere_xyzr_dev,
                                         const int32_t* sphere_link_dev, int64_t num_spheres,
                                         const int32_t* min_sphere_dev, const double* min_gradient_dev,
                                         const double* sphere_weight_dev, const double* sphere_gradient_dev,
                                         double* joint_gradient_dev)
{
  const JointGradientArguments a{tree, link_poses_dev, num_configurations, sphere_xyzr_dev, sphere_link_dev, num_spheres,
                                 min_sphere_dev, min_gradient_dev, sphere_weight_dev, sphere_gradient_dev,
                                 joint_gradient_dev};
  bool done = false;
  const int rc = a.Check(ctx, &done);
  if (rc != VGT_HIP_OK || done) return rc;
  VGT_TRY_HIP(hipSetDevice(ctx->device), "set device");
  std::lock_guard<std::mutex> lock(ctx->mutex);
  VGT_TRY_HIP(a.Launch(link_poses_dev, sphere_xyzr_dev, sphere_link_dev, min_sphere_dev, min_gradient_dev,
                       sphere_weight_dev, sphere_gradient_dev, joint_gradient_dev, ctx->stream),
              "clearance joint gradient");
  return VGT_HIP_OK;
}

int vgt_hip_clearance_joint_gradient(vgt_hip_ctx* ctx, const vgt_hip_kinematics* tree, const double* link_poses_host,
                                     int64_t num_configurations, const double* sphere_xyzr_host,
                                     const int32_t* sphere_link_host, int64_t num_spheres, const int32_t* min_sphere_host,
                                     const double* min_gradient_host, const double* sphere_weight_host,
                                     const double* sphere_gradient_host, double* joint_gradient_host)
{
  const JointGradientArguments a{tree, link_poses_host, num_configurations, sphere_xyzr_host, sphere_link_host,
                                 num_spheres, min_sphere_host, min_gradient_host, sphere_weight_host,
                                 sphere_gradient_host, joint_gradient_host};
  bool done = false;
  const int rc = a.Check(ctx, &done);
  if (rc != VGT_HIP_OK || done) return rc;
  VGT_TRY_HIP(hipSetDevice(ctx->device), "set device");
  const char* what = "clearance joint gradient";
  const size_t b = static_cast<size_t>(num_configurations), s = static_cast<size_t>(num_spheres);
  vgt::HostStaging staging;
  const auto poses = staging.In(link_poses_host, b * static_cast<size_t>(tree->num_links) * 16);
  const auto xyzr = staging.In(sphere_xyzr_host, s * 4);
  const auto link = staging.In(sphere_link_host, s);
  const auto min_sphere = staging.In(min_sphere_host, b);
  const auto min_gradient = staging.In(min_gradient_host, b * 3);
  const auto weight = staging.In(sphere_weight_host, b * s);
  const auto gradient = staging.In(sphere_gradient_host, b * s * 3);
  const auto out = staging.Out(joint_gradient_host, b * static_cast<size_t>(tree->num_joints));
  return staging.Run(*ctx, what, FailHip, [&](hipStream_t stream) {
    return HipResult(what, a.Launch(poses.dev(), xyzr.dev(), link.dev(), min_sphere.dev(), min_gradient.dev(),
                                    weight.dev(), gradient.dev(), out.dev(), stream));
  });
}

/* ------------------- inverse kinematics: tip poses to joint values ------------------- */

namespace
{
// What the two inverse-kinematics entry points share: the arguments, the checks both make before any device work (which
// find the chain) and the enqueue.
struct SolveIkArguments
{
  const vgt_hip_kinematics* tree;
  int32_t tip_link;
  const double* targets;
  int64_t num_targets, seeds_per_target;
  const double* seeds;
  const double* world_from_base;
  const double* joint_limits;
  const double* task_weights;
  int32_t max_iterations;
  double damping, max_step, position_tolerance, rotation_tolerance;
  const uint8_t* status;

  std::vector<int32_t> chain;  // the links from the base to the tip (Check)
  int moving = 0;              // how many of them are not fixed

  int64_t NumProblems() const { return num_targets * seeds_per_target; }

  int Check(const vgt_hip_ctx* ctx)
  {
    if (!ctx || !tree || !targets || !status) return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "null argument");
    if (num_targets <= 0 || seeds_per_target <= 0)
      return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "inverse kinematics needs at least one target and one seed per target");
    if (num_targets >= kTwoTo31 || seeds_per_target >= kTwoTo31 || NumProblems() >= kTwoTo31)
      return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "inverse kinematics supports fewer than 2^31 problems");
    if (tree->ctx != ctx) return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "the kinematic tree belongs to another context");
    if (tree->num_joints > 0 && !seeds) return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "null argument");
    if (tip_link < 0 || tip_link >= tree->num_links)
      return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "tip link " + std::to_string(tip_link) + " is not in [0, " +
                                                    std::to_string(tree->num_links) + ")");
    if (max_iterations < 0 || max_iterations > 10000)
      return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "max_iterations must lie in [0, 10000]");
    if (!(damping >= 0.0) || !std::isfinite(damping))
      return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "the damping must be finite and not negative");
    if (!(max_step > 0.0)) return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "max_step must be positive (+infinity is allowed)");
    if (!(position_tolerance >= 0.0) || !(rotation_tolerance >= 0.0))
      return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "a tolerance must not be negative");
    for (int k = 0; task_weights && k < 6; k++)
      if (!(task_weights[k] >= 0.0) || !std::isfinite(task_weights[k]))
        return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "a task weight must be finite and not negative");
    const std::vector<vgt::KinematicLink>& links = tree->host_links;
    std::vector<int32_t> reader;  // per column the moving chain link that reads it, -1: none
    try
    {
      for (int32_t i = tip_link; i >= 0; i = links[static_cast<size_t>(i)].parent) chain.push_back(i);
      reader.assign(static_cast<size_t>(tree->num_joints), -1);
    }
    catch (const std::bad_alloc&)
    {
      return Fail(VGT_HIP_ERR_RUNTIME, "out of host memory");
    }
    std::reverse(chain.begin(), chain.end());
    int64_t count = 0;
    for (const int32_t i : chain)
    {
      const vgt::KinematicLink& link = links[static_cast<size_t>(i)];
      if (link.joint_type == vgt::kJointFixed) continue;
      int32_t& first = reader[static_cast<size_t>(link.joint_index)];
      if (first >= 0)
        return Fail(VGT_HIP_ERR_INVALID_ARGUMENT,
                    "links " + std::to_string(first) + " and " + std::to_string(i) + " on the chain to link " +
                        std::to_string(tip_link) + " both read column " + std::to_string(link.joint_index) +
                        ": inverse kinematics does not take a mimic joint on the chain");
      first = i;
      count++;
    }
    if (count > vgt::kIkMaxChainJoints)
      return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "the chain to link " + std::to_string(tip_link) + " has " +
                                                    std::to_string(count) + " moving links; inverse kinematics takes at most " +
                                                    std::to_string(vgt::kIkMaxChainJoints));
    moving = static_cast<int>(count);
    return VGT_HIP_OK;
  }

  // Enqueues the call on `stream`; the context's mutex is held (the tree's chain and limits buffers are one per tree).
  hipError_t Enqueue(const double* targets_dev, const double* seeds_dev, const vgt::IkOutputs& out, hipStream_t stream) const
  {
    // (pageable host memory: the runtime has taken its copies when the calls return)
    hipError_t err = hipMemcpyAsync(tree->chain.as<int32_t>(), chain.data(), chain.size() * sizeof(int32_t),
                                    hipMemcpyHostToDevice, stream);
    const bool limited = joint_limits && tree->num_joints > 0;
    if (err == hipSuccess && limited)
      err = hipMemcpyAsync(tree->limits.as<double>(), joint_limits,
                           static_cast<size_t>(tree->num_joints) * 2 * sizeof(double), hipMemcpyHostToDevice, stream);
    if (err != hipSuccess) return err;
    vgt::IkOptions options{max_iterations, damping, max_step, position_tolerance, rotation_tolerance, {1, 1, 1, 1, 1, 1}};
    for (int k = 0; task_weights && k < 6; k++) options.weights[k] = task_weights[k];
    return vgt::LaunchSolveIk(tree->links.as<vgt::KinematicLink>(), tree->num_joints, tree->chain.as<int32_t>(),
                              static_cast<int>(chain.size()), moving, targets_dev, seeds_per_target, seeds_dev,
                              NumProblems(), world_from_base, limited ? tree->limits.as<double>() : nullptr, options, out,
                              g_kinematics_workgroups.load(), stream);
  }
};
}  // namespace

int32_t vgt_hip_ik_max_chain_joints(void) { return vgt::kIkMaxChainJoints; }

size_t vgt_hip_solve_ik_workspace_bytes(int64_t num_joints, int64_t num_problems)
{
  if (num_joints < 0 || num_joints >= kTwoTo31 || num_problems <= 0 || num_problems >= kTwoTo31) return 0;
  return static_cast<size_t>(num_joints) * static_cast<size_t>(num_problems) * sizeof(double);
}

int vgt_hip_solve_ik_dev(vgt_hip_ctx* ctx, const vgt_hip_kinematics* tree, int32_t tip_link, const double* targets_dev,
                         int64_t num_targets, int64_t seeds_per_target, const double* seeds_dev,
                         const double* world_from_base, const double* joint_limits, const double* task_weights,
                         int32_t max_iterations, double damping, double max_step, double position_tolerance,
                         double rotation_tolerance, double* joints_out_dev, uint8_t* status_dev, int32_t* iterations_dev,
                         double* error_dev, double* tip_pose_dev, uint8_t* fk_status_dev, void* workspace_dev,
                         size_t workspace_bytes)
{
  SolveIkArguments a{tree, tip_link, targets_dev, num_targets, seeds_per_target, seeds_dev, world_from_base, joint_limits,
                     task_weights, max_iterations, damping, max_step, position_tolerance, rotation_tolerance, status_dev,
                     {}, 0};
  const int rc = a.Check(ctx);
  if (rc != VGT_HIP_OK) return rc;
  double* rows = joints_out_dev;
  if (!rows && tree->num_joints > 0)
  {
    if (!workspace_dev) return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "without joints_out the call needs its workspace");
    if (workspace_bytes < vgt_hip_solve_ik_workspace_bytes(tree->num_joints, a.NumProblems()))
      return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "the workspace is smaller than vgt_hip_solve_ik_workspace_bytes says");
    rows = static_cast<double*>(workspace_dev);
  }
  VGT_TRY_HIP(hipSetDevice(ctx->device), "set device");
  std::lock_guard<std::mutex> lock(ctx->mutex);
  VGT_TRY_HIP(a.Enqueue(targets_dev, seeds_dev, {rows, status_dev, iterations_dev, error_dev, tip_pose_dev, fk_status_dev},
                        ctx->stream),
              "solve ik");
  return VGT_HIP_OK;
}

int vgt_hip_solve_ik(vgt_hip_ctx* ctx, const vgt_hip_kinematics* tree, int32_t tip_link, const double* targets_host,
                     int64_t num_targets, int64_t seeds_per_target, const double* seeds_host,
                     const double* world_from_base, const double* joint_limits, const double* task_weights,
                     int32_t max_iterations, double damping, double max_step, double position_tolerance,
                     double rotation_tolerance, double* joints_out_host, uint8_t* status_host, int32_t* iterations_host,
                     double* error_host, double* tip_pose_host, uint8_t* fk_status_host)
{
  SolveIkArguments a{tree, tip_link, targets_host, num_targets, seeds_per_target, seeds_host, world_from_base,
                     joint_limits, task_weights, max_iterations, damping, max_step, position_tolerance,
                     rotation_tolerance, status_host, {}, 0};
  const int rc = a.Check(ctx);
  if (rc != VGT_HIP_OK) return rc;
  VGT_TRY_HIP(hipSetDevice(ctx->device), "set device");
  const char* what = "solve ik";
  const size_t b = static_cast<size_t>(a.NumProblems()), joints = static_cast<size_t>(tree->num_joints);
  vgt::HostStaging staging;
  // (a tree without joints: one double stands in, so that the kernel has an address it never reads)
  const double none = 0.0;
  const auto targets = staging.In(targets_host, static_cast<size_t>(num_targets) * 16);
  const auto seeds = joints > 0 ? staging.In(seeds_host, b * joints) : staging.In(&none, 1);
  // the working rows: the caller's output, or scratch when the caller does without it
  const auto rows = joints_out_host ? staging.Out(joints_out_host, b * joints)
                                    : staging.Scratch<double>((b * joints > 0 ? b * joints : 1) * sizeof(double));
  const auto status = staging.Out(status_host, b);
  const auto iterations = staging.Out(iterations_host, b);
  const auto error = staging.Out(error_host, b * 6);
  const auto tip_pose = staging.Out(tip_pose_host, b * 16);
  const auto fk_status = staging.Out(fk_status_host, b);
  return staging.Run(*ctx, what, FailHip, [&](hipStream_t s) {
    return HipResult(what, a.Enqueue(targets.dev(), seeds.dev(),
                                     {rows.dev(), status.dev(), iterations.dev(), error.dev(), tip_pose.dev(),
                                      fk_status.dev()},
                                     s));
  });
}

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
                                      uint8_t* fk_status_host, double* joint_gradient_host)
{
  if (!ctx || !tree || !status_host) return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "null argument");
  if (num_configurations < 0) return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "negative number of configurations");
  if (num_configurations >= kTwoTo31)
    return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "forward kinematics supports fewer than 2^31 configurations");
  if (num_configurations == 0) return VGT_HIP_OK;  // (before the tree is looked at)
  bool done = false;
  // (the poses stay on the device: the tree itself stands in where the checks ask for a pointer that is not null)
  const double* const stand_in = reinterpret_cast<const double*>(tree);
  int rc = CheckForwardKinematics(ctx, tree, joint_values_host, num_configurations, stand_in, &done);
  if (rc != VGT_HIP_OK) return rc;
  const CheckSpheresArguments a{sdf_host, nx, ny, nz, resolution, grid_from_world, rotation, sphere_xyzr_host,
                                sphere_link_host, num_spheres, stand_in, tree->num_links, num_configurations,
                                minimum_clearance, flags,
                                {status_host, min_clearance_host, min_sphere_host, num_below_host, num_outside_host,
                                 min_gradient_host, sphere_clearance_host, sphere_gradient_host}};
  rc = a.Check(ctx);
  if (rc == VGT_HIP_OK) rc = a.CheckModel();
  if (rc != VGT_HIP_OK) return rc;
  const bool with_gradient = joint_gradient_host && tree->num_joints > 0;
  if (with_gradient && num_configurations * tree->num_joints >= kTwoTo31)
    return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "the joint gradient supports fewer than 2^31 (configuration, joint) pairs");
  VGT_TRY_HIP(hipSetDevice(ctx->device), "set device");
  const char* what = "check spheres from joints";
  const size_t b = static_cast<size_t>(num_configurations), s = static_cast<size_t>(num_spheres);
  const size_t joints = static_cast<size_t>(tree->num_joints);
  const double none = 0.0;
  // (ten outputs and seven inputs, and a staging holds eight arrays: three of them, the later ones inside the first one's body)
  vgt::HostStaging inputs;
  const auto sdf = inputs.In(sdf_host, static_cast<size_t>(a.NumCells()));
  const auto xyzr = inputs.In(sphere_xyzr_host, s * 4);
  const auto link = inputs.In(sphere_link_host, s);
  const auto values = joints > 0 ? inputs.In(joint_values_host, b * joints) : inputs.In(&none, 1);
  const auto poses = inputs.Scratch<double>(b * static_cast<size_t>(tree->num_links) * 16 * sizeof(double));
  // what the gradient reads, when the caller does not want it back
  vgt::HostStaging::Handle<int32_t> own_min_sphere;
  vgt::HostStaging::Handle<double> own_min_gradient;
  if (with_gradient && !min_sphere_host) own_min_sphere = inputs.Scratch<int32_t>(b * sizeof(int32_t));
  if (with_gradient && !min_gradient_host) own_min_gradient = inputs.Scratch<double>(b * 3 * sizeof(double));
  return inputs.Run(*ctx, what, FailHip, [&](hipStream_t stream) {
    vgt::HostStaging checks;
    const auto status = checks.Out(status_host, b);
    const auto min_clearance = checks.Out(min_clearance_host, b);
    const auto min_sphere = checks.Out(min_sphere_host, b);
    const auto num_below = checks.Out(num_below_host, b);
    const auto num_outside = checks.Out(num_outside_host, b);
    const auto min_gradient = checks.Out(min_gradient_host, b * 3);
    const auto sphere_clearance = checks.Out(sphere_clearance_host, b * s);
    const auto sphere_gradient = checks.Out(sphere_gradient_host, b * s * 3);
    return checks.RunLocked(stream, what, FailHip, [&](hipStream_t) {
      vgt::HostStaging kinematics;
      const auto fk_status = kinematics.Out(fk_status_host, b);
      const auto joint_gradient = kinematics.Out(with_gradient ? joint_gradient_host : nullptr, b * joints);
      return kinematics.RunLocked(stream, what, FailHip, [&](hipStream_t) {
        hipError_t err = EnqueueForwardKinematics(tree, values.dev(), num_configurations, world_from_base, joint_limits,
                                                  poses.dev(), fk_status.dev(), stream);
        int32_t* const worst = min_sphere_host ? min_sphere.dev() : own_min_sphere.dev();
        double* const worst_gradient = min_gradient_host ? min_gradient.dev() : own_min_gradient.dev();
        const vgt::BodyOutputs out{status.dev(),      min_clearance.dev(), worst,                  num_below.dev(),
                                   num_outside.dev(), worst_gradient,      sphere_clearance.dev(), sphere_gradient.dev()};
        if (err == hipSuccess) err = a.Launch(sdf.dev(), xyzr.dev(), link.dev(), poses.dev(), out, stream);
        if (err == hipSuccess && with_gradient)
          err = vgt::LaunchClearanceJointGradient(tree->links.as<vgt::KinematicLink>(), tree->num_links,
                                                  tree->num_joints, poses.dev(), num_configurations, xyzr.dev(),
                                                  link.dev(), num_spheres, worst, worst_gradient, nullptr, nullptr,
                                                  joint_gradient.dev(), g_kinematics_workgroups.load(), stream);
        return HipResult(what, err);
      });
    });
  });
}

/* ------------------- motions between joint configurations checked against an SDF ------------------- */

namespace
{
// What the two motion entry points share: the arguments and the checks both make before any device work.
struct CheckMotionsArguments
{
  const float* sdf;
  int64_t nx, ny, nz;
  double resolution;
  const double *grid_from_world, *rotation;
  const double* sphere_xyzr;
  const int32_t* sphere_link;
  int64_t num_spheres;
  const vgt_hip_kinematics* tree;
  const double *joint_from, *joint_to;
  const int32_t* num_steps;
  int32_t uniform_steps;
  int64_t num_motions;
  const double *world_from_base, *joint_limits;
  double minimum_clearance;
  uint32_t flags;
  vgt::MotionOutputs out;

  int64_t NumCells() const { return nx * ny * nz; }
  // *done: nothing is left to do (E == 0).
  int Check(const vgt_hip_ctx* ctx, bool* done) const
  {
    *done = false;
    if (!ctx || !sdf || !tree || !out.status || (num_spheres > 0 && (!sphere_xyzr || !sphere_link)))
      return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "null argument");
    if (num_spheres < 0 || num_motions < 0)
      return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "the numbers of spheres and motions must not be negative");
    if (!num_steps && uniform_steps < 0)
      return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "uniform_steps " + std::to_string(uniform_steps) + " is negative");
    if (nx < 0 || ny < 0 || nz < 0) return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "grid extents must not be negative");
    if (!(resolution > 0.0) || !std::isfinite(resolution))
      return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "Grid must have uniform, positive resolution");
    // (extent by extent: the product of three int64 extents can overflow)
    const int64_t most = 0x7fffffffLL;
    if (nx > most || ny > most || nz > most || (nx > 0 && ny > 0 && nz > 0 && (nx * ny > most || nx * ny * nz > most)))
      return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "motion checks support grids below 2^31 cells");
    if (std::isnan(minimum_clearance)) return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "minimum_clearance must not be NaN");
    if (flags & ~(VGT_HIP_SPHERES_OUTSIDE_IS_COLLISION | VGT_HIP_MOTION_STOP_AT_COLLISION))
      return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "unknown motion check flag");
    if (num_spheres > most || num_motions > most)
      return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "motion checks support fewer than 2^31 spheres and motions");
    *done = num_motions == 0;  // (before the tree is looked at)
    return VGT_HIP_OK;
  }
  // What needs the tree (after E == 0, which succeeds before the tree is looked at).
  int CheckTree(const vgt_hip_ctx* ctx) const
  {
    if (tree->ctx != ctx) return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "the kinematic tree belongs to another context");
    if (vgt::MotionTileSamples(tree->num_links) == 0)
      return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "motion checks take trees of at most " + std::to_string(vgt::kMotionMaxLinks) +
                                                    " links, this one has " + std::to_string(tree->num_links));
    if (tree->num_joints > 0 && (!joint_from || !joint_to)) return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "null argument");
    if (num_motions * tree->num_joints >= kTwoTo31)
      return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "motion checks support fewer than 2^31 (motion, joint) pairs");
    return VGT_HIP_OK;
  }
  // The host form's own checks: it can look at the step counts and the model (the links once the tree is known).
  int CheckHostArrays() const
  {
    for (int64_t e = 0; num_steps && e < num_motions; e++)
      if (num_steps[e] < 0)
        return Fail(VGT_HIP_ERR_INVALID_ARGUMENT,
                    "motion " + std::to_string(e) + ": num_steps " + std::to_string(num_steps[e]));
    for (int64_t s = 0; s < num_spheres; s++)
      if (!(sphere_xyzr[4 * s + 3] >= 0.0))
        return Fail(VGT_HIP_ERR_INVALID_ARGUMENT,
                    "sphere " + std::to_string(s) + ": the radius must not be negative or NaN");
    return VGT_HIP_OK;
  }
  int CheckHostLinks() const
  {
    for (int64_t s = 0; s < num_spheres; s++)
      if (sphere_link[s] < 0 || sphere_link[s] >= tree->num_links)
        return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "sphere " + std::to_string(s) + ": link " +
                                                      std::to_string(sphere_link[s]) + " is not in [0, num_links)");
    return VGT_HIP_OK;
  }
  // Enqueues the check on `stream`; the context's mutex is held (the tree's limits buffer is one per tree).
  hipError_t Enqueue(const float* sdf_dev, const double* xyzr_dev, const int32_t* link_dev, const double* from_dev,
                     const double* to_dev, const int32_t* steps_dev, const vgt::MotionOutputs& out_dev,
                     hipStream_t stream) const
  {
    const bool limited = joint_limits && tree->num_joints > 0;
    if (limited)
    {
      // (pageable host memory: the runtime has taken its copy when the call returns)
      const hipError_t err = hipMemcpyAsync(tree->limits.as<double>(), joint_limits,
                                            static_cast<size_t>(tree->num_joints) * 2 * sizeof(double),
                                            hipMemcpyHostToDevice, stream);
      if (err != hipSuccess) return err;
    }
    return vgt::LaunchCheckMotions(sdf_dev, nx, ny, nz, resolution, grid_from_world, rotation, xyzr_dev, link_dev,
                                   num_spheres, tree->links.as<vgt::KinematicLink>(), tree->num_links, tree->num_joints,
                                   from_dev, to_dev, steps_dev, uniform_steps, num_motions, world_from_base,
                                   limited ? tree->limits.as<double>() : nullptr, minimum_clearance,
                                   (flags & VGT_HIP_SPHERES_OUTSIDE_IS_COLLISION) ? 1 : 0,
                                   (flags & VGT_HIP_MOTION_STOP_AT_COLLISION) ? 1 : 0, out_dev,
                                   g_motion_workgroups.load(), stream);
  }

};
}  // namespace

int32_t vgt_hip_motion_tile_samples(int64_t num_links) { return vgt::MotionTileSamples(num_links); }

int vgt_hip_check_motions_dev(vgt_hip_ctx* ctx, const float* sdf_dev, int64_t nx, int64_t ny, int64_t nz,
                              double resolution, const double* grid_from_world, const double* rotation,
                              const double* sphere_xyzr_dev, const int32_t* sphere_link_dev, int64_t num_spheres,
                              const vgt_hip_kinematics* tree, const double* joint_from_dev, const double* joint_to_dev,
                              const int32_t* num_steps_dev, int32_t uniform_steps, int64_t num_motions,
                              const double* world_from_base, const double* joint_limits, double minimum_clearance,
                              uint32_t flags, uint8_t* status_dev, int32_t* first_collision_dev,
                              double* min_clearance_dev, int32_t* min_sample_dev, int32_t* min_sphere_dev,
                              double* min_gradient_dev, uint8_t* fk_status_dev)
{
  const CheckMotionsArguments a{sdf_dev, nx, ny, nz, resolution, grid_from_world, rotation, sphere_xyzr_dev,
                                sphere_link_dev, num_spheres, tree, joint_from_dev, joint_to_dev, num_steps_dev,
                                uniform_steps, num_motions, world_from_base, joint_limits, minimum_clearance, flags,
                                {status_dev, first_collision_dev, min_clearance_dev, min_sample_dev, min_sphere_dev,
                                 min_gradient_dev, fk_status_dev}};
  bool done = false;
  int rc = a.Check(ctx, &done);
  if (rc != VGT_HIP_OK || done) return rc;
  rc = a.CheckTree(ctx);
  if (rc != VGT_HIP_OK) return rc;
  VGT_TRY_HIP(hipSetDevice(ctx->device), "set device");
  std::lock_guard<std::mutex> lock(ctx->mutex);
  VGT_TRY_HIP(a.Enqueue(sdf_dev, sphere_xyzr_dev, sphere_link_dev, joint_from_dev, joint_to_dev, num_steps_dev, a.out,
                        ctx->stream),
              "check motions");
  return VGT_HIP_OK;
}

int vgt_hip_check_motions(vgt_hip_ctx* ctx, const float* sdf_host, int64_t nx, int64_t ny, int64_t nz, double resolution,
                          const double* grid_from_world, const double* rotation, const double* sphere_xyzr_host,
                          const int32_t* sphere_link_host, int64_t num_spheres, const vgt_hip_kinematics* tree,
                          const double* joint_from_host, const double* joint_to_host, const int32_t* num_steps_host,
                          int32_t uniform_steps, int64_t num_motions, const double* world_from_base,
                          const double* joint_limits, double minimum_clearance, uint32_t flags, uint8_t* status_host,
                          int32_t* first_collision_host, double* min_clearance_host, int32_t* min_sample_host,
                          int32_t* min_sphere_host, double* min_gradient_host, uint8_t* fk_status_host)
{
  const CheckMotionsArguments a{sdf_host, nx, ny, nz, resolution, grid_from_world, rotation, sphere_xyzr_host,
                                sphere_link_host, num_spheres, tree, joint_from_host, joint_to_host, num_steps_host,
                                uniform_steps, num_motions, world_from_base, joint_limits, minimum_clearance, flags,
                                {status_host, first_collision_host, min_clearance_host, min_sample_host, min_sphere_host,
                                 min_gradient_host, fk_status_host}};
  bool done = false;
  int rc = a.Check(ctx, &done);
  if (rc != VGT_HIP_OK || done) return rc;
  rc = a.CheckHostArrays();
  if (rc == VGT_HIP_OK) rc = a.CheckTree(ctx);
  if (rc == VGT_HIP_OK) rc = a.CheckHostLinks();
  if (rc != VGT_HIP_OK) return rc;
  VGT_TRY_HIP(hipSetDevice(ctx->device), "set device");
  const char* what = "check motions";
  const size_t e = static_cast<size_t>(num_motions), s = static_cast<size_t>(num_spheres);
  const size_t joints = static_cast<size_t>(tree->num_joints);
  // (a tree without joints: one double stands in, so that the kernel has an address it never reads)
  const double none = 0.0;
  // (seven outputs and six inputs, and a staging holds eight arrays: two of them, the second inside the first one's body)
  vgt::HostStaging inputs;
  const auto sdf = inputs.In(sdf_host, static_cast<size_t>(a.NumCells()));
  const auto xyzr = inputs.In(sphere_xyzr_host, s * 4);
  const auto link = inputs.In(sphere_link_host, s);
  const auto from = joints > 0 ? inputs.In(joint_from_host, e * joints) : inputs.In(&none, 1);
  const auto to = joints > 0 ? inputs.In(joint_to_host, e * joints) : inputs.In(&none, 1);
  const auto steps = inputs.In(num_steps_host, e);
  return inputs.Run(*ctx, what, FailHip, [&](hipStream_t stream) {
    vgt::HostStaging outputs;
    const auto status = outputs.Out(status_host, e);
    const auto first_collision = outputs.Out(first_collision_host, e);
    const auto min_clearance = outputs.Out(min_clearance_host, e);
    const auto min_sample = outputs.Out(min_sample_host, e);
    const auto min_sphere = outputs.Out(min_sphere_host, e);
    const auto min_gradient = outputs.Out(min_gradient_host, e * 3);
    const auto fk_status = outputs.Out(fk_status_host, e);
    return outputs.RunLocked(stream, what, FailHip, [&](hipStream_t) {
      const vgt::MotionOutputs out{status.dev(),     first_collision.dev(), min_clearance.dev(), min_sample.dev(),
                                   min_sphere.dev(), min_gradient.dev(),    fk_status.dev()};
      return HipResult(what, a.Enqueue(sdf.dev(), xyzr.dev(), link.dev(), from.dev(), to.dev(), steps.dev(), out, stream));
    });
  });
}

/* ------------------- the obstacle cost of configurations given as joint values, and its joint gradient ------------------- */

namespace
{
// What the two cost entry points share: the arguments and the checks both make before any device work.
struct ClearanceCostArguments
{
  const float* sdf;
  int64_t nx, ny, nz;
  double resolution;
  const double *grid_from_world, *rotation;
  const double* sphere_xyzr;
  const int32_t* sphere_link;
  int64_t num_spheres;
  const vgt_hip_kinematics* tree;
  const double* joint_values;
  int64_t num_configurations;
  const double *world_from_base, *joint_limits;
  double margin;
  uint32_t flags;
  vgt::CostOutputs out;

  int64_t NumCells() const { return nx * ny * nz; }
  // *done: nothing is left to do (B == 0).
  int Check(const vgt_hip_ctx* ctx, bool* done) const
  {
    *done = false;
    if (!ctx || !sdf || !tree || !out.cost || (num_spheres > 0 && (!sphere_xyzr || !sphere_link)))
      return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "null argument");
    if (num_spheres < 0 || num_configurations < 0)
      return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "the numbers of spheres and configurations must not be negative");
    if (nx < 0 || ny < 0 || nz < 0) return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "grid extents must not be negative");
    if (!(resolution > 0.0) || !std::isfinite(resolution))
      return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "Grid must have uniform, positive resolution");
    // (extent by extent: the product of three int64 extents can overflow)
    const int64_t most = 0x7fffffffLL;
    if (nx > most || ny > most || nz > most || (nx > 0 && ny > 0 && nz > 0 && (nx * ny > most || nx * ny * nz > most)))
      return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "clearance costs support grids below 2^31 cells");
    if (!(margin > 0.0) || !std::isfinite(margin))
      return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "margin must be positive and finite");
    if (flags != 0) return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "unknown clearance cost flag");
    if (num_spheres > most || num_configurations > most || num_spheres * num_configurations > most)
      return Fail(VGT_HIP_ERR_INVALID_ARGUMENT,
                  "clearance costs support fewer than 2^31 spheres, configurations and (configuration, sphere) pairs");
    *done = num_configurations == 0;  // (before the tree is looked at)
    return VGT_HIP_OK;
  }
  // What needs the tree (after B == 0, which succeeds before the tree is looked at).
  int CheckTree(const vgt_hip_ctx* ctx) const
  {
    if (tree->ctx != ctx) return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "the kinematic tree belongs to another context");
    if (vgt::CostTileSamples(tree->num_links) == 0)
      return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "clearance costs take trees of at most " +
                                                    std::to_string(vgt::kCostMaxLinks) + " links, this one has " +
                                                    std::to_string(tree->num_links));
    if (tree->num_joints > 0 && !joint_values) return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "null argument");
    if (num_configurations * tree->num_joints >= kTwoTo31)
      return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "clearance costs support fewer than 2^31 (configuration, joint) pairs");
    if (num_configurations * tree->num_links >= kTwoTo31)
      return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "clearance costs support fewer than 2^31 (configuration, link) pairs");
    return VGT_HIP_OK;
  }
  // The host form's own checks: it can look at the model (the links once the tree is known).
  int CheckHostArrays() const
  {
    for (int64_t s = 0; s < num_spheres; s++)
      if (!(sphere_xyzr[4 * s + 3] >= 0.0))
        return Fail(VGT_HIP_ERR_INVALID_ARGUMENT,
                    "sphere " + std::to_string(s) + ": the radius must not be negative or NaN");
    return VGT_HIP_OK;
  }
  int CheckHostLinks() const
  {
    for (int64_t s = 0; s < num_spheres; s++)
      if (sphere_link[s] < 0 || sphere_link[s] >= tree->num_links)
        return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "sphere " + std::to_string(s) + ": link " +
                                                      std::to_string(sphere_link[s]) + " is not in [0, num_links)");
    return VGT_HIP_OK;
  }
  // Enqueues the call on `stream`; the context's mutex is held (the tree's limits buffer is one per tree).
  hipError_t Enqueue(const float* sdf_dev, const double* xyzr_dev, const int32_t* link_dev, const double* joints_dev,
                     const vgt::CostOutputs& out_dev, hipStream_t stream) const
  {
    const bool limited = joint_limits && tree->num_joints > 0;
    if (limited)
    {
      // (pageable host memory: the runtime has taken its copy when the call returns)
      const hipError_t err = hipMemcpyAsync(tree->limits.as<double>(), joint_limits,
                                            static_cast<size_t>(tree->num_joints) * 2 * sizeof(double),
                                            hipMemcpyHostToDevice, stream);
      if (err != hipSuccess) return err;
    }
    return vgt::LaunchClearanceCost(sdf_dev, nx, ny, nz, resolution, grid_from_world, rotation, xyzr_dev, link_dev,
                                    num_spheres, tree->links.as<vgt::KinematicLink>(), tree->num_links, tree->num_joints,
                                    joints_dev, num_configurations, world_from_base,
                                    limited ? tree->limits.as<double>() : nullptr, margin, out_dev,
                                    g_cost_workgroups.load(), stream);
  }
};
}  // namespace

int32_t vgt_hip_cost_tile_samples(int64_t num_links) { return vgt::CostTileSamples(num_links); }

int vgt_hip_clearance_cost_dev(vgt_hip_ctx* ctx, const float* sdf_dev, int64_t nx, int64_t ny, int64_t nz,
                               double resolution, const double* grid_from_world, const double* rotation,
                               const double* sphere_xyzr_dev, const int32_t* sphere_link_dev, int64_t num_spheres,
                               const vgt_hip_kinematics* tree, const double* joint_values_dev,
                               int64_t num_configurations, const double* world_from_base, const double* joint_limits,
                               double margin, uint32_t flags, double* cost_dev, double* joint_gradient_dev,
                               int32_t* num_active_dev, int32_t* num_outside_dev, int32_t* num_without_gradient_dev,
                               uint8_t* fk_status_dev)
{
  const ClearanceCostArguments a{sdf_dev, nx, ny, nz, resolution, grid_from_world, rotation, sphere_xyzr_dev,
                                 sphere_link_dev, num_spheres, tree, joint_values_dev, num_configurations,
                                 world_from_base, joint_limits, margin, flags,
                                 {cost_dev, joint_gradient_dev, num_active_dev, num_outside_dev,
                                  num_without_gradient_dev, fk_status_dev}};
  bool done = false;
  int rc = a.Check(ctx, &done);
  if (rc != VGT_HIP_OK || done) return rc;
  rc = a.CheckTree(ctx);
  if (rc != VGT_HIP_OK) return rc;
  VGT_TRY_HIP(hipSetDevice(ctx->device), "set device");
  std::lock_guard<std::mutex> lock(ctx->mutex);
  VGT_TRY_HIP(a.Enqueue(sdf_dev, sphere_xyzr_dev, sphere_link_dev, joint_values_dev, a.out, ctx->stream),
              "clearance cost");
  return VGT_HIP_OK;
}

int vgt_hip_clearance_cost(vgt_hip_ctx* ctx, const float* sdf_host, int64_t nx, int64_t ny, int64_t nz, double resolution,
                           const double* grid_from_world, const double* rotation, const double* sphere_xyzr_host,
                           const int32_t* sphere_link_host, int64_t num_spheres, const vgt_hip_kinematics* tree,
                           const double* joint_values_host, int64_t num_configurations, const double* world_from_base,
                           const double* joint_limits, double margin, uint32_t flags, double* cost_host,
                           double* joint_gradient_host, int32_t* num_active_host, int32_t* num_outside_host,
                           int32_t* num_without_gradient_host, uint8_t* fk_status_host)
{
  const ClearanceCostArguments a{sdf_host, nx, ny, nz, resolution, grid_from_world, rotation, sphere_xyzr_host,
                                 sphere_link_host, num_spheres, tree, joint_values_host, num_configurations,
                                 world_from_base, joint_limits, margin, flags,
                                 {cost_host, joint_gradient_host, num_active_host, num_outside_host,
                                  num_without_gradient_host, fk_status_host}};
  bool done = false;
  int rc = a.Check(ctx, &done);
  if (rc != VGT_HIP_OK || done) return rc;
  rc = a.CheckHostArrays();
  if (rc == VGT_HIP_OK) rc = a.CheckTree(ctx);
  if (rc == VGT_HIP_OK) rc = a.CheckHostLinks();
  if (rc != VGT_HIP_OK) return rc;
  VGT_TRY_HIP(hipSetDevice(ctx->device), "set device");
  const char* what = "clearance cost";
  const size_t b = static_cast<size_t>(num_configurations), s = static_cast<size_t>(num_spheres);
  const size_t joints = static_cast<size_t>(tree->num_joints);
  // (a tree without joints: one double stands in, so that the kernel has an address it never reads)
  const double none = 0.0;
  // (six outputs and four inputs, and a staging holds eight arrays: two of them, the second inside the first one's body)
  vgt::HostStaging inputs;
  const auto sdf = inputs.In(sdf_host, static_cast<size_t>(a.NumCells()));
  const auto xyzr = inputs.In(sphere_xyzr_host, s * 4);
  const auto link = inputs.In(sphere_link_host, s);
  const auto values = joints > 0 ? inputs.In(joint_values_host, b * joints) : inputs.In(&none, 1);
  return inputs.Run(*ctx, what, FailHip, [&](hipStream_t stream) {
    vgt::HostStaging outputs;
    const auto cost = outputs.Out(cost_host, b);
    const auto joint_gradient = outputs.Out(joint_gradient_host, b * joints);
    const auto num_active = outputs.Out(num_active_host, b);
    const auto num_outside = outputs.Out(num_outside_host, b);
    const auto num_without_gradient = outputs.Out(num_without_gradient_host, b);
    const auto fk_status = outputs.Out(fk_status_host, b);
    return outputs.RunLocked(stream, what, FailHip, [&](hipStream_t) {
      const vgt::CostOutputs out{cost.dev(),        joint_gradient.dev(),       num_active.dev(),
                                 num_outside.dev(), num_without_gradient.dev(), fk_status.dev()};
      return HipResult(what, a.Enqueue(sdf.dev(), xyzr.dev(), link.dev(), values.dev(), out, stream));
    });
  });
}

/* ------------------------- self-collision of a sphere model, batched over configurations ------------------------- */

namespace
{
// What the four self-collision entry points share: the arguments and the checks they make before any device work.
struct SelfCollisionArguments
{
  const double* sphere_xyzr;
  const int32_t* sphere_link;
  int64_t num_spheres;
  const int32_t* pairs;
  int64_t num_pairs;
  const vgt_hip_kinematics* tree;  // the poses form: only for the gradient
  const double* joint_values;      // the joint-value form
  const double* link_poses;        // the poses form
  bool from_joints;
  int64_t num_configurations, num_links;  // (the joint-value form: num_links is the tree's, filled in by Check)
  const double *world_from_base, *joint_limits;
  double minimum_clearance;
  uint32_t flags;
  vgt::SelfCollisionOutputs out;

  int64_t NumJoints() const { return tree ? tree->num_joints : 0; }
  // *done: nothing is left to do (B == 0).
  int Check(const vgt_hip_ctx* ctx, bool* done)
  {
    *done = false;
    if (!ctx || !out.status || (from_joints && !tree) || (num_spheres > 0 && (!sphere_xyzr || !sphere_link)) ||
        (num_spheres > 0 && num_pairs > 0 && !pairs))
      return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "null argument");
    if (num_spheres < 0 || num_pairs < 0 || num_configurations < 0 || (!from_joints && num_links < 0))
      return Fail(VGT_HIP_ERR_INVALID_ARGUMENT,
                  "the numbers of spheres, pairs, configurations and links must not be negative");
    if (std::isnan(minimum_clearance)) return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "minimum_clearance must not be NaN");
    if ((flags & ~VGT_HIP_SELF_NO_VALUE_IS_COLLISION) != 0)
      return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "unknown self-collision flag");
    if (out.joint_gradient && !tree)
      return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "the joint gradient needs the kinematic tree");
    const int64_t most = 0x7fffffffLL;
    if (num_spheres > most || num_pairs > most || num_configurations > most)
      return Fail(VGT_HIP_ERR_INVALID_ARGUMENT,
                  "self-collision checks support fewer than 2^31 spheres, pairs and configurations");
    if (out.pair_clearance && num_configurations * num_pairs > most)
      return Fail(VGT_HIP_ERR_INVALID_ARGUMENT,
                  "self-collision checks support fewer than 2^31 (configuration, pair) clearances");
    *done = num_configurations == 0;  // (before the tree is looked at)
    return VGT_HIP_OK;
  }
  // What needs the tree or the number of links (after B == 0, which succeeds before either is looked at).
  int CheckTree(const vgt_hip_ctx* ctx)
  {
    if (tree && tree->ctx != ctx)
      return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "the kinematic tree belongs to another context");
    if (from_joints)
      num_links = tree->num_links;
    else if (tree && tree->num_links != num_links)
      return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "the kinematic tree has " + std::to_string(tree->num_links) +
                                                    " links, the poses have " + std::to_string(num_links));
    if (vgt::SelfCollisionTileSamples(num_links, num_spheres) == 0)
      return Fail(VGT_HIP_ERR_INVALID_ARGUMENT,
                  "self-collision checks take at least one link and 96 bytes per link + 32 per sphere + 256 within " +
                      std::to_string(vgt::kSelfLdsLimit) + ", this model has " + std::to_string(num_links) +
                      " links and " + std::to_string(num_spheres) + " spheres");
    if (from_joints ? (tree->num_joints > 0 && !joint_values) : !link_poses)
      return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "null argument");
    if (num_configurations * NumJoints() >= kTwoTo31)
      return Fail(VGT_HIP_ERR_INVALID_ARGUMENT,
                  "self-collision checks support fewer than 2^31 (configuration, joint) pairs");
    if (num_configurations * num_links >= kTwoTo31)
      return Fail(VGT_HIP_ERR_INVALID_ARGUMENT,
                  "self-collision checks support fewer than 2^31 (configuration, link) pairs");
    return VGT_HIP_OK;
  }
  // The host forms' own checks: they can look at the model and the pairs (the links once their number is known).
  int CheckHostArrays() const
  {
    for (int64_t s = 0; s < num_spheres; s++)
      if (!(sphere_xyzr[4 * s + 3] >= 0.0))
        return Fail(VGT_HIP_ERR_INVALID_ARGUMENT,
                    "sphere " + std::to_string(s) + ": the radius must not be negative or NaN");
    for (int64_t p = 0; num_spheres > 0 && p < num_pairs; p++)
    {
      const int64_t a = pairs[2 * p], b = pairs[2 * p + 1];
      for (const int64_t sphere : {a, b})
        if (sphere < 0 || sphere >= num_spheres)
          return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "pair " + std::to_string(p) + ": sphere " + std::to_string(sphere) +
                                                        " is outside [0, " + std::to_string(num_spheres) + ")");
      if (a >= b)
        return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "pair " + std::to_string(p) + ": (" + std::to_string(a) + ", " +
                                                      std::to_string(b) + ") is not ascending");
    }
    return VGT_HIP_OK;
  }
  int CheckHostLinks() const
  {
    for (int64_t s = 0; s < num_spheres; s++)
      if (sphere_link[s] < 0 || sphere_link[s] >= num_links)
        return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "sphere " + std::to_string(s) + ": link " +
                                                      std::to_string(sphere_link[s]) + " is not in [0, num_links)");
    return VGT_HIP_OK;
  }
  // Enqueues the call on `stream`; the context's mutex is held (the tree's limits buffer is one per tree).
  hipError_t Enqueue(const double* xyzr_dev, const int32_t* link_dev, const int32_t* pairs_dev, const double* source_dev,
                     const vgt::SelfCollisionOutputs& out_dev, hipStream_t stream) const
  {
    const bool limited = from_joints && joint_limits && tree->num_joints > 0;
    if (limited)
    {
      // (pageable host memory: the runtime has taken its copy when the call returns)
      const hipError_t err = hipMemcpyAsync(tree->limits.as<double>(), joint_limits,
                                            static_cast<size_t>(tree->num_joints) * 2 * sizeof(double),
                                            hipMemcpyHostToDevice, stream);
      if (err != hipSuccess) return err;
    }
    return vgt::LaunchSelfCollision(xyzr_dev, link_dev, num_spheres, pairs_dev, num_pairs,
                                    tree ? tree->links.as<vgt::KinematicLink>() : nullptr, num_links, NumJoints(),
                                    from_joints ? source_dev : nullptr, from_joints ? nullptr : source_dev,
                                    num_configurations, world_from_base, limited ? tree->limits.as<double>() : nullptr,
                                    minimum_clearance, (flags & VGT_HIP_SELF_NO_VALUE_IS_COLLISION) ? 1 : 0, out_dev,
                                    g_self_collision_workgroups.load(), stream);
  }
  int RunOnDevice(vgt_hip_ctx* ctx)
  {
    bool done = false;
    int rc = Check(ctx, &done);
    if (rc != VGT_HIP_OK || done) return rc;
    rc = CheckTree(ctx);
    if (rc != VGT_HIP_OK) return rc;
    VGT_TRY_HIP(hipSetDevice(ctx->device), "set device");
    // (a tree without joints: an address the kernel never reads stands in, so that the launcher can tell the forms)
    static const double none = 0.0;
    const double* const source = from_joints ? (joint_values ? joint_values : &none) : link_poses;
    std::lock_guard<std::mutex> lock(ctx->mutex);
    VGT_TRY_HIP(Enqueue(sphere_xyzr, sphere_link, pairs, source, out, ctx->stream), "self-collision check");
    return VGT_HIP_OK;
  }
  int RunFromHost(vgt_hip_ctx* ctx)
  {
    bool done = false;
    int rc = Check(ctx, &done);
    if (rc != VGT_HIP_OK || done) return rc;
    rc = CheckHostArrays();
    if (rc == VGT_HIP_OK) rc = CheckTree(ctx);
    if (rc == VGT_HIP_OK) rc = CheckHostLinks();
    if (rc != VGT_HIP_OK) return rc;
    VGT_TRY_HIP(hipSetDevice(ctx->device), "set device");
    const char* what = "self-collision check";
    const size_t b = static_cast<size_t>(num_configurations), s = static_cast<size_t>(num_spheres);
    const size_t p = static_cast<size_t>(num_pairs), joints = static_cast<size_t>(NumJoints());
    // (a tree without joints: one double stands in, so that the kernel has an address it never reads)
    const double none = 0.0;
    // (nine outputs and four inputs, and a staging holds eight arrays: two of them, the second inside the first one's
    // body; the per-pair output goes with the inputs)
    vgt::HostStaging inputs;
    const auto xyzr = inputs.In(sphere_xyzr, s * 4);
    const auto link = inputs.In(sphere_link, s);
    const auto list = inputs.In(pairs, p * 2);
    const auto source = !from_joints ? inputs.In(link_poses, b * static_cast<size_t>(num_links) * 16)
                        : joints > 0 ? inputs.In(joint_values, b * joints)
                                     : inputs.In(&none, 1);
    const auto pair_clearance = inputs.Out(out.pair_clearance, num_spheres > 0 ? b * p : 0);
    return inputs.Run(*ctx, what, FailHip, [&](hipStream_t stream) {
      vgt::HostStaging outputs;
      const auto status = outputs.Out(out.status, b);
      const auto num_below = outputs.Out(out.num_below, b);
      const auto num_without_value = outputs.Out(out.num_without_value, b);
      const auto min_clearance = outputs.Out(out.min_clearance, b);
      const auto min_pair = outputs.Out(out.min_pair, b);
      const auto min_direction = outputs.Out(out.min_direction, b * 3);
      const auto joint_gradient = outputs.Out(out.joint_gradient, b * joints);
      const auto fk_status = outputs.Out(out.fk_status, b);
      return outputs.RunLocked(stream, what, FailHip, [&](hipStream_t) {
        const vgt::SelfCollisionOutputs out_dev{status.dev(),        num_below.dev(),     num_without_value.dev(),
                                                min_clearance.dev(), min_pair.dev(),      min_direction.dev(),
                                                joint_gradient.dev(), fk_status.dev(),    pair_clearance.dev()};
        return HipResult(what, Enqueue(xyzr.dev(), link.dev(), list.dev(), source.dev(), out_dev, stream));
      });
    });
  }
};
}  // namespace

/* ------------------- motions checked against an SDF and against the robot itself in one call ------------------- */

namespace
{
// What the two entry points share: the arguments and the checks both make before any device work.
struct CheckMotionsWithSelfArguments
{
  const float* sdf;  // nullptr: no environment part
  int64_t nx, ny, nz;
  double resolution;
  const double *grid_from_world, *rotation;
  const double* sphere_xyzr;
  const int32_t* sphere_link;
  int64_t num_spheres;
  const int32_t* pairs;
  int64_t num_pairs;  // 0: no self part
  const vgt_hip_kinematics* tree;
  const double *joint_from, *joint_to;
  const int32_t* num_steps;
  int32_t uniform_steps;
  int64_t num_motions;
  const double *world_from_base, *joint_limits;
  double minimum_clearance, self_minimum_clearance;
  uint32_t flags;
  vgt::MotionSelfOutputs out;

  int64_t NumCells() const { return sdf ? nx * ny * nz : 0; }
  // *done: nothing is left to do (E == 0).
  int Check(const vgt_hip_ctx* ctx, bool* done) const
  {
    *done = false;
    if (!ctx || !tree || !out.status || (num_spheres > 0 && (!sphere_xyzr || !sphere_link)) ||
        (num_spheres > 0 && num_pairs > 0 && !pairs))
      return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "null argument");
    if (num_spheres < 0 || num_pairs < 0 || num_motions < 0)
      return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "the numbers of spheres, pairs and motions must not be negative");
    if (!sdf && num_pairs == 0)
      return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "neither a field nor a pair: there is nothing to check the motions against");
    if (!num_steps && uniform_steps < 0)
      return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "uniform_steps " + std::to_string(uniform_steps) + " is negative");
    const int64_t most = 0x7fffffffLL;
    if (sdf)
    {
      if (nx < 0 || ny < 0 || nz < 0) return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "grid extents must not be negative");
      if (!(resolution > 0.0) || !std::isfinite(resolution))
        return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "Grid must have uniform, positive resolution");
      // (extent by extent: the product of three int64 extents can overflow)
      if (nx > most || ny > most || nz > most || (nx > 0 && ny > 0 && nz > 0 && (nx * ny > most || nx * ny * nz > most)))
        return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "motion checks support grids below 2^31 cells");
      if (std::isnan(minimum_clearance)) return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "minimum_clearance must not be NaN");
    }
    if (num_pairs > 0 && std::isnan(self_minimum_clearance))
      return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "self_minimum_clearance must not be NaN");
    if (flags & ~(VGT_HIP_SPHERES_OUTSIDE_IS_COLLISION | VGT_HIP_MOTION_STOP_AT_COLLISION |
                  VGT_HIP_MOTION_SELF_NO_VALUE_IS_COLLISION))
      return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "unknown motion check flag");
    if (num_spheres > most || num_pairs > most || num_motions > most)
      return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "motion checks support fewer than 2^31 spheres, pairs and motions");
    *done = num_motions == 0;  // (before the tree is looked at)
    return VGT_HIP_OK;
  }
  // What needs the tree (after E == 0, which succeeds before the tree is looked at).
  int CheckTree(const vgt_hip_ctx* ctx) const
  {
    if (tree->ctx != ctx) return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "the kinematic tree belongs to another context");
    if (vgt::MotionSelfTileSamples(tree->num_links, num_spheres) == 0)
      return Fail(VGT_HIP_ERR_INVALID_ARGUMENT,
                  "motion checks with the self part take at least one link and 96 bytes per link + 32 per sphere + " +
                      std::to_string(vgt::kMotionSelfRecordBytes) + " within " +
                      std::to_string(vgt::kMotionSelfLdsLimit) + ", this model has " + std::to_string(tree->num_links) +
                      " links and " + std::to_string(num_spheres) + " spheres");
    if (tree->num_joints > 0 && (!joint_from || !joint_to)) return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "null argument");
    if (num_motions * tree->num_joints >= kTwoTo31)
      return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "motion checks support fewer than 2^31 (motion, joint) pairs");
    return VGT_HIP_OK;
  }
  // The host form's own checks: it can look at the step counts, the model and the pairs (the links once the tree is
  // known).
  int CheckHostArrays() const
  {
    for (int64_t e = 0; num_steps && e < num_motions; e++)
      if (num_steps[e] < 0)
        return Fail(VGT_HIP_ERR_INVALID_ARGUMENT,
                    "motion " + std::to_string(e) + ": num_steps " + std::to_string(num_steps[e]));
    for (int64_t s = 0; s < num_spheres; s++)
      if (!(sphere_xyzr[4 * s + 3] >= 0.0))
        return Fail(VGT_HIP_ERR_INVALID_ARGUMENT,
                    "sphere " + std::to_string(s) + ": the radius must not be negative or NaN");
    for (int64_t p = 0; num_spheres > 0 && p < num_pairs; p++)
    {
      const int64_t a = pairs[2 * p], b = pairs[2 * p + 1];
      for (const int64_t sphere : {a, b})
        if (sphere < 0 || sphere >= num_spheres)
          return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "pair " + std::to_string(p) + ": sphere " + std::to_string(sphere) +
                                                        " is outside [0, " + std::to_string(num_spheres) + ")");
      if (a >= b)
        return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "pair " + std::to_string(p) + ": (" + std::to_string(a) + ", " +
                                                      std::to_string(b) + ") is not ascending");
    }
    return VGT_HIP_OK;
  }
  int CheckHostLinks() const
  {
    for (int64_t s = 0; s < num_spheres; s++)
      if (sphere_link[s] < 0 || sphere_link[s] >= tree->num_links)
        return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "sphere " + std::to_string(s) + ": link " +
                                                      std::to_string(sphere_link[s]) + " is not in [0, num_links)");
    return VGT_HIP_OK;
  }
  // Enqueues the check on `stream`; the context's mutex is held (the tree's limits buffer is one per tree).
  hipError_t Enqueue(const float* sdf_dev, const double* xyzr_dev, const int32_t* link_dev, const int32_t* pairs_dev,
                     const double* from_dev, const double* to_dev, const int32_t* steps_dev,
                     const vgt::MotionSelfOutputs& out_dev, hipStream_t stream) const
  {
    const bool limited = joint_limits && tree->num_joints > 0;
    if (limited)
    {
      // (pageable host memory: the runtime has taken its copy when the call returns)
      const hipError_t err = hipMemcpyAsync(tree->limits.as<double>(), joint_limits,
                                            static_cast<size_t>(tree->num_joints) * 2 * sizeof(double),
                                            hipMemcpyHostToDevice, stream);
      if (err != hipSuccess) return err;
    }
    return vgt::LaunchCheckMotionsWithSelf(
        sdf_dev, nx, ny, nz, resolution, grid_from_world, rotation, xyzr_dev, link_dev, num_spheres, pairs_dev, num_pairs,
        tree->links.as<vgt::KinematicLink>(), tree->num_links, tree->num_joints, from_dev, to_dev, steps_dev,
        uniform_steps, num_motions, world_from_base, limited ? tree->limits.as<double>() : nullptr, minimum_clearance,
        self_minimum_clearance, (flags & VGT_HIP_SPHERES_OUTSIDE_IS_COLLISION) ? 1 : 0,
        (flags & VGT_HIP_MOTION_SELF_NO_VALUE_IS_COLLISION) ? 1 : 0, (flags & VGT_HIP_MOTION_STOP_AT_COLLISION) ? 1 : 0,
        out_dev, g_motion_self_workgroups.load(), stream);
  }
};
}  // namespace

int32_t vgt_hip_motion_self_tile_samples(int64_t num_links, int64_t num_spheres)
{
  return vgt::MotionSelfTileSamples(num_links, num_spheres);
}

int vgt_hip_check_motions_with_self_dev(
    vgt_hip_ctx* ctx, const float* sdf_dev, int64_t nx, int64_t ny, int64_t nz, double resolution,
    const double* grid_from_world, const double* rotation, const double* sphere_xyzr_dev, const int32_t* sphere_link_dev,
    int64_t num_spheres, const int32_t* pairs_dev, int64_t num_pairs, const vgt_hip_kinematics* tree,
    const double* joint_from_dev, const double* joint_to_dev, const int32_t* num_steps_dev, int32_t uniform_steps,
    int64_t num_motions, const double* world_from_base, const double* joint_limits, double minimum_clearance,
    double self_minimum_clearance, uint32_t flags, uint8_t* status_dev, int32_t* first_collision_dev,
    uint8_t* collision_cause_dev, double* min_clearance_dev, int32_t* min_sample_dev, int32_t* min_sphere_dev,
    double* min_gradient_dev, double* self_min_clearance_dev, int32_t* self_min_sample_dev, int32_t* self_min_pair_dev,
    uint8_t* fk_status_dev)
{
  const CheckMotionsWithSelfArguments a{
      sdf_dev, nx, ny, nz, resolution, grid_from_world, rotation, sphere_xyzr_dev, sphere_link_dev, num_spheres, pairs_dev,
      num_pairs, tree, joint_from_dev, joint_to_dev, num_steps_dev, uniform_steps, num_motions, world_from_base,
      joint_limits, minimum_clearance, self_minimum_clearance, flags,
      {status_dev, first_collision_dev, collision_cause_dev, min_clearance_dev, min_sample_dev, min_sphere_dev,
       min_gradient_dev, self_min_clearance_dev, self_min_sample_dev, self_min_pair_dev, fk_status_dev}};
  bool done = false;
  int rc = a.Check(ctx, &done);
  if (rc != VGT_HIP_OK || done) return rc;
  rc = a.CheckTree(ctx);
  if (rc != VGT_HIP_OK) return rc;
  VGT_TRY_HIP(hipSetDevice(ctx->device), "set device");
  std::lock_guard<std::mutex> lock(ctx->mutex);
  VGT_TRY_HIP(a.Enqueue(sdf_dev, sphere_xyzr_dev, sphere_link_dev, pairs_dev, joint_from_dev, joint_to_dev, num_steps_dev,
                        a.out, ctx->stream),
              "check motions with self");
  return VGT_HIP_OK;
}

int vgt_hip_check_motions_with_self(
    vgt_hip_ctx* ctx, const float* sdf_host, int64_t nx, int64_t ny, int64_t nz, double resolution,
    const double* grid_from_world, const double* rotation, const double* sphere_xyzr_host,
    const int32_t* sphere_link_host, int64_t num_spheres, const int32_t* pairs_host, int64_t num_pairs,
    const vgt_hip_kinematics* tree, const double* joint_from_host, const double* joint_to_host,
    const int32_t* num_steps_host, int32_t uniform_steps, int64_t num_motions, const double* world_from_base,
    const double* joint_limits, double minimum_clearance, double self_minimum_clearance, uint32_t flags,
    uint8_t* status_host, int32_t* first_collision_host, uint8_t* collision_cause_host, double* min_clearance_host,
    int32_t* min_sample_host, int32_t* min_sphere_host, double* min_gradient_host, double* self_min_clearance_host,
    int32_t* self_min_sample_host, int32_t* self_min_pair_host, uint8_t* fk_status_host)
{
  const CheckMotionsWithSelfArguments a{
      sdf_host, nx, ny, nz, resolution, grid_from_world, rotation, sphere_xyzr_host, sphere_link_host, num_spheres,
      pairs_host, num_pairs, tree, joint_from_host, joint_to_host, num_steps_host, uniform_steps, num_motions,
      world_from_base, joint_limits, minimum_clearance, self_minimum_clearance, flags,
      {status_host, first_collision_host, collision_cause_host, min_clearance_host, min_sample_host, min_sphere_host,
       min_gradient_host, self_min_clearance_host, self_min_sample_host, self_min_pair_host, fk_status_host}};
  bool done = false;
  int rc = a.Check(ctx, &done);
  if (rc != VGT_HIP_OK || done) return rc;
  rc = a.CheckHostArrays();
  if (rc == VGT_HIP_OK) rc = a.CheckTree(ctx);
  if (rc == VGT_HIP_OK) rc = a.CheckHostLinks();
  if (rc != VGT_HIP_OK) return rc;
  VGT_TRY_HIP(hipSetDevice(ctx->device), "set device");
  const char* what = "check motions with self";
  const size_t e = static_cast<size_t>(num_motions), s = static_cast<size_t>(num_spheres);
  const size_t joints = static_cast<size_t>(tree->num_joints);
  // (a tree without joints: one double stands in, so that the kernel has an address it never reads)
  const double none = 0.0;
  // (eleven outputs and seven inputs, and a staging holds eight arrays: three of them, each inside the one before's body)
  vgt::HostStaging inputs;
  const auto sdf = inputs.In(sdf_host, static_cast<size_t>(a.NumCells()));
  const auto xyzr = inputs.In(sphere_xyzr_host, s * 4);
  const auto link = inputs.In(sphere_link_host, s);
  const auto list = inputs.In(num_spheres > 0 ? pairs_host : nullptr, static_cast<size_t>(num_pairs) * 2);
  const auto from = joints > 0 ? inputs.In(joint_from_host, e * joints) : inputs.In(&none, 1);
  const auto to = joints > 0 ? inputs.In(joint_to_host, e * joints) : inputs.In(&none, 1);
  const auto steps = inputs.In(num_steps_host, e);
  return inputs.Run(*ctx, what, FailHip, [&](hipStream_t stream) {
    vgt::HostStaging outputs;
    const auto status = outputs.Out(status_host, e);
    const auto first_collision = outputs.Out(first_collision_host, e);
    const auto collision_cause = outputs.Out(collision_cause_host, e);
    const auto min_clearance = outputs.Out(min_clearance_host, e);
    const auto min_sample = outputs.Out(min_sample_host, e);
    const auto min_sphere = outputs.Out(min_sphere_host, e);
    const auto min_gradient = outputs.Out(min_gradient_host, e * 3);
    const auto fk_status = outputs.Out(fk_status_host, e);
    return outputs.RunLocked(stream, what, FailHip, [&](hipStream_t) {
      vgt::HostStaging self_outputs;
      const auto self_min_clearance = self_outputs.Out(self_min_clearance_host, e);
      const auto self_min_sample = self_outputs.Out(self_min_sample_host, e);
      const auto self_min_pair = self_outputs.Out(self_min_pair_host, e);
      return self_outputs.RunLocked(stream, what, FailHip, [&](hipStream_t) {
        const vgt::MotionSelfOutputs out{status.dev(),          first_collision.dev(),    collision_cause.dev(),
                                         min_clearance.dev(),   min_sample.dev(),         min_sphere.dev(),
                                         min_gradient.dev(),    self_min_clearance.dev(), self_min_sample.dev(),
                                         self_min_pair.dev(),   fk_status.dev()};
        return HipResult(what, a.Enqueue(sdf.dev(), xyzr.dev(), link.dev(), list.dev(), from.dev(), to.dev(), steps.dev(),
                                         out, stream));
      });
    });
  });
}

int32_t vgt_hip_self_collision_tile_samples(int64_t num_links, int64_t num_spheres)
{
  return vgt::SelfCollisionTileSamples(num_links, num_spheres);
}

int vgt_hip_check_self_collision_dev(vgt_hip_ctx* ctx, const double* sphere_xyzr_dev, const int32_t* sphere_link_dev,
                                     int64_t num_spheres, const int32_t* pairs_dev, int64_t num_pairs,
                                     const vgt_hip_kinematics* tree, const double* joint_values_dev,
                                     int64_t num_configurations, const double* world_from_base,
                                     const double* joint_limits, double minimum_clearance, uint32_t flags,
                                     uint8_t* status_dev, int32_t* num_below_dev, int32_t* num_without_value_dev,
                                     double* min_clearance_dev, int32_t* min_pair_dev, double* min_direction_dev,
                                     double* joint_gradient_dev, uint8_t* fk_status_dev, double* pair_clearance_dev)
{
  SelfCollisionArguments a{sphere_xyzr_dev, sphere_link_dev, num_spheres, pairs_dev, num_pairs, tree, joint_values_dev,
                           nullptr, true, num_configurations, 0, world_from_base, joint_limits, minimum_clearance, flags,
                           {status_dev, num_below_dev, num_without_value_dev, min_clearance_dev, min_pair_dev,
                            min_direction_dev, joint_gradient_dev, fk_status_dev, pair_clearance_dev}};
  return a.RunOnDevice(ctx);
}

int vgt_hip_check_self_collision(vgt_hip_ctx* ctx, const double* sphere_xyzr_host, const int32_t* sphere_link_host,
                                 int64_t num_spheres, const int32_t* pairs_host, int64_t num_pairs,
                                 const vgt_hip_kinematics* tree, const double* joint_values_host,
                                 int64_t num_configurations, const double* world_from_base, const double* joint_limits,
                                 double minimum_clearance, uint32_t flags, uint8_t* status_host, int32_t* num_below_host,
                                 int32_t* num_without_value_host, double* min_clearance_host, int32_t* min_pair_host,
                                 double* min_direction_host, double* joint_gradient_host, uint8_t* fk_status_host,
                                 double* pair_clearance_host)
{
  SelfCollisionArguments a{sphere_xyzr_host, sphere_link_host, num_spheres, pairs_host, num_pairs, tree,
                           joint_values_host, nullptr, true, num_configurations, 0, world_from_base, joint_limits,
                           minimum_clearance, flags,
                           {status_host, num_below_host, num_without_value_host, min_clearance_host, min_pair_host,
                            min_direction_host, joint_gradient_host, fk_status_host, pair_clearance_host}};
  return a.RunFromHost(ctx);
}

int vgt_hip_check_self_collision_poses_dev(vgt_hip_ctx* ctx, const double* sphere_xyzr_dev,
                                           const int32_t* sphere_link_dev, int64_t num_spheres, const int32_t* pairs_dev,
                                           int64_t num_pairs, const double* link_poses_dev, int64_t num_configurations,
                                           int64_t num_links, const vgt_hip_kinematics* tree, double minimum_clearance,
                                           uint32_t flags, uint8_t* status_dev, int32_t* num_below_dev,
                                           int32_t* num_without_value_dev, double* min_clearance_dev,
                                           int32_t* min_pair_dev, double* min_direction_dev, double* joint_gradient_dev,
                                           double* pair_clearance_dev)
{
  SelfCollisionArguments a{sphere_xyzr_dev, sphere_link_dev, num_spheres, pairs_dev, num_pairs, tree, nullptr,
                           link_poses_dev, false, num_configurations, num_links, nullptr, nullptr, minimum_clearance,
                           flags,
                           {status_dev, num_below_dev, num_without_value_dev, min_clearance_dev, min_pair_dev,
                            min_direction_dev, joint_gradient_dev, nullptr, pair_clearance_dev}};
  return a.RunOnDevice(ctx);
}

int vgt_hip_check_self_collision_poses(vgt_hip_ctx* ctx, const double* sphere_xyzr_host, const int32_t* sphere_link_host,
                                       int64_t num_spheres, const int32_t* pairs_host, int64_t num_pairs,
                                       const double* link_poses_host, int64_t num_configurations, int64_t num_links,
                                       const vgt_hip_kinematics* tree, double minimum_clearance, uint32_t flags,
                                       uint8_t* status_host, int32_t* num_below_host, int32_t* num_without_value_host,
                                       double* min_clearance_host, int32_t* min_pair_host, double* min_direction_host,
                                       double* joint_gradient_host, double* pair_clearance_host)
{
  SelfCollisionArguments a{sphere_xyzr_host, sphere_link_host, num_spheres, pairs_host, num_pairs, tree, nullptr,
                           link_poses_host, false, num_configurations, num_links, nullptr, nullptr, minimum_clearance,
                           flags,
                           {status_host, num_below_host, num_without_value_host, min_clearance_host, min_pair_host,
                            min_direction_host, joint_gradient_host, nullptr, pair_clearance_host}};
  return a.RunFromHost(ctx);
}

int vgt_hip_self_collision_pairs(const int32_t* sphere_link, int64_t num_spheres, const int32_t* parent,
                                 int64_t num_links, const int32_t* ignored_link_pairs, int64_t num_ignored,
                                 uint32_t flags, int32_t* pairs_out, int64_t capacity, int64_t* count)
{
  if (!count || (num_spheres > 0 && !sphere_link) || (num_ignored > 0 && !ignored_link_pairs) ||
      (capacity > 0 && !pairs_out))
    return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "null argument");
  if (num_spheres < 0 || num_links < 0 || num_ignored < 0 || capacity < 0)
    return Fail(VGT_HIP_ERR_INVALID_ARGUMENT,
                "the numbers of spheres, links and ignored pairs and the capacity must not be negative");
  if ((flags & ~VGT_HIP_SELF_PAIRS_SKIP_ADJACENT) != 0)
    return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "unknown self-collision pair flag");
  if (num_spheres > 0x7fffffffLL)
    return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "self-collision pairs support fewer than 2^31 spheres");
  for (int64_t s = 0; s < num_spheres; s++)
    if (sphere_link[s] < 0 || sphere_link[s] >= num_links)
      return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "sphere " + std::to_string(s) + ": link " +
                                                    std::to_string(sphere_link[s]) + " is not in [0, num_links)");
  for (int64_t i = 0; parent && i < num_links; i++)
    if (parent[i] < -1 || parent[i] >= num_links)
      return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "link " + std::to_string(i) + ": parent " + std::to_string(parent[i]) +
                                                    " is not in [-1, num_links)");
  // the ignored pairs as sorted keys low * L + high
  std::vector<int64_t> ignored;
  ignored.reserve(static_cast<size_t>(num_ignored));
  for (int64_t i = 0; i < num_ignored; i++)
  {
    const int64_t first = ignored_link_pairs[2 * i], second = ignored_link_pairs[2 * i + 1];
    for (const int64_t link : {first, second})
      if (link < 0 || link >= num_links)
        return Fail(VGT_HIP_ERR_INVALID_ARGUMENT, "ignored pair " + std::to_string(i) + ": link " +
                                                      std::to_string(link) + " is not in [0, num_links)");
    ignored.push_back(std::min(first, second) * num_links + std::max(first, second));
  }
  std::sort(ignored.begin(), ignored.end());
  const bool skip_adjacent = (flags & VGT_HIP_SELF_PAIRS_SKIP_ADJACENT) != 0 && parent != nullptr;
  int64_t found = 0;
  for (int64_t a = 0; a < num_spheres; a++)
    for (int64_t b = a + 1; b < num_spheres; b++)
    {
      const int64_t la = sphere_link[a], lb = sphere_link[b];
      if (la == lb) continue;
      if (skip_adjacent && (parent[la] == lb || parent[lb] == la)) continue;
      if (!ignored.empty() &&
          std::binary_search(ignored.begin(), ignored.end(), std::min(la, lb) * num_links + std::max(la, lb)))
        continue;
      if (found < capacity)
      {
        pairs_out[2 * found] = static_cast<int32_t>(a);
        pairs_out[2 * found + 1] = static_cast<int32_t>(b);
      }
      found++;
    }
  *count = found;
  return VGT_HIP_OK;
}

}  // extern "C"
