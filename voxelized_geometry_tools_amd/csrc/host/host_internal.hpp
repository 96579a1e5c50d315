// Private to the sources of the C++ host layer (csrc/host/hip_*.cc): not installed, not among the library's dynamic symbols.
#pragma once

#include <stdexcept>
#include <string>

#include "../../../include/vgt_hip.h"

namespace vgt_hip
{
namespace detail
{
// The process's one context of a device, shared by every free-standing entry point of the layer (SDF extraction and its
// consumers, the tagged maps, components, topology, the mesh rasterizer).  Created on first use and kept for the life of
// the process (deliberately never destroyed: static destruction order against the HIP runtime is not defined).  The
// context caches its device buffers, so a caller that calls repeatedly pays for context creation and hipMalloc once
// (ReleaseCachedDeviceMemory() returns them); the C ABI serialises concurrent calls on one context.  A device that
// cannot be opened: std::runtime_error("HIP SDF backend is not available: ...").
__attribute__((visibility("hidden"))) vgt_hip_ctx* SharedSdfContext(int device);

// A C ABI error code as the reference's exception: std::invalid_argument for VGT_HIP_ERR_INVALID_ARGUMENT, else
// std::runtime_error.
[[noreturn]] __attribute__((visibility("hidden"))) inline void ThrowForCode(int rc, const std::string& msg)
{
  if (rc == VGT_HIP_ERR_INVALID_ARGUMENT) throw std::invalid_argument(msg);
  throw std::runtime_error(msg);
}
}  // namespace detail
}  // namespace vgt_hip
