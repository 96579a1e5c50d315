// The cross-check EDT of libvgt_hip_testing.so (edt_crosscheck_kernels.hip): an implementation of the signed distance
// transform that shares no pass with the product's, selected per context with vgt_hip_set_edt_variant(ctx, 1) and
// compared against the product's by the parity tests.  Included by its own source and by vgt_hip_capi.hip only; the
// product library links none of it.
//
// Intermediate encodings:
//  pass 1 (Z scan)  -> int16: +d for a free voxel, -d for a filled voxel, d = distance in voxels along Z to the nearest
//                      voxel of the OTHER class, |value| == kInf16 when the line holds no such voxel.
//  pass 2 (Y pass)  -> int32: +-(squared distance in the YZ plane), two's complement, magnitude kInf32 when none.
//  pass 3 (X pass)  -> float SDF.
// The line passes are a pruned outward search per voxel straight from HBM; they take whole grids only (no batches, no
// ranges of an axis).  Exact, like the product's.
#pragma once

#include "vgt_internal.hpp"

namespace vgt
{
// Bytes of the pass-1 field (the workspace holds it where the product's class records would be).
inline size_t CrossCheckFieldBytes(int64_t voxels) { return static_cast<size_t>(voxels) * sizeof(int16_t); }

// All asynchronous on `stream`.
// Pass 1: occupancy (float) or mask (u8) -> int16.  `summary` (optional, multi-GPU) receives one SlabLineSummary per
// (x, y) line.
hipError_t LaunchCrossCheckScanZFromOccupancy(const float* occupancy, int16_t* out16, const SdfParams& p,
                                              SlabLineSummary* summary, hipStream_t stream);
hipError_t LaunchCrossCheckScanZFromMask(const uint8_t* mask, int16_t* out16, const SdfParams& p,
                                         SlabLineSummary* summary, hipStream_t stream);
// Multi-GPU: folds the carries of the other slabs into the slab-local pass-1 distances, in place.
hipError_t LaunchCrossCheckSlabFixup(int16_t* io16, const SlabLineCarry* carries, const SdfParams& p,
                                     hipStream_t stream);
// Y pass: int16 -> int32.
hipError_t LaunchCrossCheckPassY(const int16_t* in16, int32_t* out32, const SdfParams& p, hipStream_t stream);
// X pass + finalize: int32 -> float SDF, min/max folded into minmax_enc (as LaunchPassXFinalize).
hipError_t LaunchCrossCheckPassXFinalize(const int32_t* in32, float* sdf, uint32_t* minmax_enc, const SdfParams& p,
                                         hipStream_t stream);
// Diagnostic (vgt_hip_debug_finalize_check): compares the fast final conversion with the exact one over `count`
// squared distances from `first`; result_dev[0] = number of differing values, result_dev[1] = first differing d2 (or ~0).
hipError_t LaunchFinalizeCheck(int64_t first, int64_t count, double resolution, unsigned long long* result_dev,
                               hipStream_t stream);
}  // namespace vgt
