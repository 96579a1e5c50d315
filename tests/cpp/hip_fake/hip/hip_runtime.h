// A fake of the few HIP runtime calls that csrc/device_memory.hpp and csrc/host_staging.hpp use, for
// tests/cpp/test_host_staging.cc: device memory is host memory, copies happen at once (so a sanitizer sees an overrun
// of a carved array), every call is logged, and the n-th call of a kind can be told to fail.  Not the sweep
// emulation's hip_shim: that one stands in for device code, this one for the host API.
#pragma once

#include <cstddef>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <vector>

enum hipError_t
{
  hipSuccess = 0,
  hipErrorInvalidValue = 1,
  hipErrorOutOfMemory = 2,
  hipErrorLaunchFailure = 719,
  hipErrorUnknown = 999
};
enum hipMemcpyKind
{
  hipMemcpyHostToDevice = 1,
  hipMemcpyDeviceToHost = 2
};
typedef struct ihipStream_t* hipStream_t;

namespace hip_fake
{
enum Kind
{
  kMalloc,
  kFree,
  kUpload,    // hipMemcpyAsync, host to device
  kDownload,  // hipMemcpyAsync, device to host
  kMemset,
  kSynchronize,
  kGetLastError,
  kKinds
};
struct Call
{
  Kind kind;
  const void* dst;
  const void* src;
  size_t bytes;
  hipStream_t stream;
};
struct State
{
  std::vector<Call> log;
  int seen[kKinds] = {};
  int fail_nth[kKinds] = {};  // 1-based; 0: never
  hipError_t fail_with[kKinds] = {};
  int live_allocations = 0;
  std::mutex* watched = nullptr;  // hipFree notes whether this mutex could be taken
  int frees_with_mutex_free = 0, frees_with_mutex_held = 0;
};
inline State& state()
{
  static State s;
  return s;
}
inline void Reset(std::mutex* watched)
{
  state() = State();
  state().watched = watched;
}
inline void FailNth(Kind kind, int nth, hipError_t err) { state().fail_nth[kind] = nth, state().fail_with[kind] = err; }
inline int Count(Kind kind) { return state().seen[kind]; }
// Logs the call; what it returns is the call's result (a call that fails does nothing else).
inline hipError_t Enter(Kind kind, const void* dst, const void* src, size_t bytes, hipStream_t stream)
{
  State& s = state();
  s.log.push_back(Call{kind, dst, src, bytes, stream});
  return ++s.seen[kind] == s.fail_nth[kind] ? s.fail_with[kind] : hipSuccess;
}
}  // namespace hip_fake

inline hipError_t hipMalloc(void** ptr, size_t bytes)
{
  *ptr = nullptr;
  const hipError_t err = hip_fake::Enter(hip_fake::kMalloc, nullptr, nullptr, bytes, nullptr);
  if (err != hipSuccess) return err;
  if (posix_memalign(ptr, 256, bytes) != 0) return hipErrorOutOfMemory;
  hip_fake::state().log.back().dst = *ptr;
  hip_fake::state().live_allocations++;
  return hipSuccess;
}
inline hipError_t hipFree(void* ptr)
{
  hip_fake::State& s = hip_fake::state();
  if (s.watched)
  {
    const bool mutex_free = s.watched->try_lock();
    if (mutex_free) s.watched->unlock();
    (mutex_free ? s.frees_with_mutex_free : s.frees_with_mutex_held)++;
  }
  const hipError_t err = hip_fake::Enter(hip_fake::kFree, ptr, nullptr, 0, nullptr);
  if (err != hipSuccess) return err;
  std::free(ptr);
  s.live_allocations--;
  return hipSuccess;
}
inline hipError_t hipMemcpyAsync(void* dst, const void* src, size_t bytes, hipMemcpyKind kind, hipStream_t stream)
{
  const hipError_t err =
      hip_fake::Enter(kind == hipMemcpyHostToDevice ? hip_fake::kUpload : hip_fake::kDownload, dst, src, bytes, stream);
  if (err == hipSuccess) std::memcpy(dst, src, bytes);
  return err;
}
inline hipError_t hipMemsetAsync(void* dst, int value, size_t bytes, hipStream_t stream)
{
  const hipError_t err = hip_fake::Enter(hip_fake::kMemset, dst, nullptr, bytes, stream);
  if (err == hipSuccess) std::memset(dst, value, bytes);
  return err;
}
inline hipError_t hipStreamSynchronize(hipStream_t stream)
{
  return hip_fake::Enter(hip_fake::kSynchronize, nullptr, nullptr, 0, stream);
}
inline hipError_t hipGetLastError() { return hip_fake::Enter(hip_fake::kGetLastError, nullptr, nullptr, 0, nullptr); }
