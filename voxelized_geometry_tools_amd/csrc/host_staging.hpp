// The device side of one host-pointer call of the C ABI: the call declares its arrays, then Run() allocates them as ONE
// block carved at 256-byte boundaries, takes the context's mutex once, uploads, runs the body, downloads and waits for
// the stream.  The rules on failure are the same for every caller: an upload that fails keeps the body from running; a
// body that fails keeps everything from being downloaded (host outputs stay as the caller gave them) and its code comes
// back unchanged; the first HIP error is the one reported; whatever was enqueued is waited for, once, before Run()
// returns.  The object is a local of whoever calls Run(), so the block is freed after Run() has dropped the mutex; the
// block of a RunLocked() call goes with the scope of the function that made it, usually under the lock already held.
// Knows nothing of the ABI: the context is any type with `mutex` and `stream`, and `fail(what, hipError_t)` makes the
// return code.  tests/cpp/test_host_staging.cc runs every path, the failing ones too, against a fake runtime on the CPU.
#pragma once

#include <hip/hip_runtime.h>

#include "device_memory.hpp"

#include <cstddef>
#include <mutex>

namespace vgt
{
class HostStaging
{
  struct Slot
  {
    void* dev = nullptr;
    const void* upload_from = nullptr;
    void* download_to = nullptr;
    size_t bytes = 0, offset = 0;
  };

public:
  // The device address is there once Run() has allocated, i.e. inside the body; null for an output nobody asked for.
  template <class T>
  class Handle
  {
  public:
    T* dev() const { return slot_ ? static_cast<T*>(slot_->dev) : nullptr; }

  private:
    friend class HostStaging;
    const Slot* slot_ = nullptr;
  };

  HostStaging() = default;
  HostStaging(const HostStaging&) = delete;
  HostStaging& operator=(const HostStaging&) = delete;

  // An upload, a download, both.  A null `host` is an array the call does without: nothing is reserved and its device
  // address is null.  An array of no elements has a valid address and is not copied.
  template <class T>
  Handle<T> In(const T* host, size_t count) { return host ? Add<T>(host, nullptr, count * sizeof(T)) : Handle<T>(); }
  template <class T>
  Handle<T> Out(T* host, size_t count) { return host ? Add<T>(nullptr, host, count * sizeof(T)) : Handle<T>(); }
  template <class T>
  Handle<T> InOut(T* host, size_t count) { return host ? Add<T>(host, host, count * sizeof(T)) : Handle<T>(); }
  // No host side.
  template <class T = void>
  Handle<T> Scratch(size_t bytes) { return Add<T>(nullptr, nullptr, bytes); }

  template <class Ctx, class Fail, class Body>
  int Run(Ctx& ctx, const char* what, Fail fail, Body body)
  {
    const hipError_t err = Allocate();
    if (err != hipSuccess) return fail(what, err);
    std::lock_guard<std::mutex> lock(ctx.mutex);
    return Staged(ctx.stream, what, fail, body);
  }
  // For a caller that holds the context's mutex already (and frees the block under it, unless it outlives the lock).
  template <class Fail, class Body>
  int RunLocked(hipStream_t stream, const char* what, Fail fail, Body body)
  {
    const hipError_t err = Allocate();
    return err != hipSuccess ? fail(what, err) : Staged(stream, what, fail, body);
  }

private:
  static constexpr int kMaxSlots = 8;
  static constexpr size_t kAlign = 256;

  template <class T>
  Handle<T> Add(const void* upload_from, void* download_to, size_t bytes)
  {
    Handle<T> handle;
    if (used_ == kMaxSlots) return overflow_ = true, handle;
    slots_[used_] = Slot{nullptr, upload_from, download_to, bytes, 0};
    handle.slot_ = &slots_[used_++];
    return handle;
  }

  hipError_t Allocate()
  {
    if (overflow_) return hipErrorInvalidValue;
    size_t total = 0;
    for (int i = 0; i < used_; i++)
    {
      slots_[i].offset = (total + kAlign - 1) / kAlign * kAlign;
      total = slots_[i].offset + (slots_[i].bytes ? slots_[i].bytes : 1);
    }
    if (total == 0) return hipSuccess;
    const hipError_t err = block_.Allocate(total);
    for (int i = 0; i < used_ && err == hipSuccess; i++) slots_[i].dev = block_.as<char>() + slots_[i].offset;
    return err;
  }

  template <class Fail, class Body>
  int Staged(hipStream_t s, const char* what, Fail fail, Body body)
  {
    hipError_t err = hipSuccess;
    for (int i = 0; i < used_ && err == hipSuccess; i++)
      if (slots_[i].upload_from && slots_[i].bytes)
        err = hipMemcpyAsync(slots_[i].dev, slots_[i].upload_from, slots_[i].bytes, hipMemcpyHostToDevice, s);
    const int rc = err == hipSuccess ? body(s) : 0;
    for (int i = 0; i < used_ && err == hipSuccess && rc == 0; i++)
      if (slots_[i].download_to && slots_[i].bytes)
        err = hipMemcpyAsync(slots_[i].download_to, slots_[i].dev, slots_[i].bytes, hipMemcpyDeviceToHost, s);
    const hipError_t sync = hipStreamSynchronize(s);  // whatever happened: the block is about to go
    if (err == hipSuccess) err = sync;
    if (rc != 0) return rc;
    return err == hipSuccess ? 0 : fail(what, err);
  }

  DeviceTemp block_;
  Slot slots_[kMaxSlots];
  int used_ = 0;
  bool overflow_ = false;
};
}  // namespace vgt
