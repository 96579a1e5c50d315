// Owners of device memory for the host code of the C ABI (vgt_hip_capi.hip, vgt_hipx_multi.hip).  Both are move-only and
// free what they hold when they go; neither synchronises anything: whoever lets one go, or regrows it, has made sure
// that no enqueued work still uses the memory.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <utility>

namespace vgt
{
// One hipMalloc that lives as long as its scope: the fixed buffers of a handle, the temporaries of vgt_hipx_multi.hip,
// and the one block of a host-pointer entry point (host_staging.hpp, which frees it after the context's mutex is dropped).
class DeviceTemp
{
public:
  DeviceTemp() = default;
  DeviceTemp(DeviceTemp&& other) noexcept : ptr_(std::exchange(other.ptr_, nullptr)) {}
  DeviceTemp& operator=(DeviceTemp&& other) noexcept
  {
    if (this != &other)
    {
      Release();
      ptr_ = std::exchange(other.ptr_, nullptr);
    }
    return *this;
  }
  ~DeviceTemp() { Release(); }

  hipError_t Allocate(size_t bytes)
  {
    Release();
    const hipError_t err = hipMalloc(&ptr_, bytes);
    if (err != hipSuccess) ptr_ = nullptr;
    return err;
  }
  void Release()
  {
    if (ptr_) (void)hipFree(ptr_);
    ptr_ = nullptr;
  }
  template <class T>
  T* as() const
  {
    return static_cast<T*>(ptr_);
  }
  explicit operator bool() const { return ptr_ != nullptr; }

private:
  void* ptr_ = nullptr;
};

// A buffer that is kept across calls and only ever grows: pointer and capacity travel together.
class DeviceCache
{
public:
  DeviceCache() = default;
  DeviceCache(DeviceCache&& other) noexcept
      : ptr_(std::exchange(other.ptr_, nullptr)), bytes_(std::exchange(other.bytes_, 0))
  {
  }
  DeviceCache& operator=(DeviceCache&& other) noexcept
  {
    if (this != &other)
    {
      (void)Release();
      ptr_ = std::exchange(other.ptr_, nullptr);
      bytes_ = std::exchange(other.bytes_, 0);
    }
    return *this;
  }
  ~DeviceCache() { (void)Release(); }

  // Keeps an allocation that is large enough; otherwise frees it and allocates exactly `need`.  Empty after a failure.
  hipError_t Reserve(size_t need)
  {
    if (ptr_ && bytes_ >= need) return hipSuccess;
    (void)Release();
    const hipError_t err = hipMalloc(&ptr_, need);
    if (err == hipSuccess)
      bytes_ = need;
    else
      ptr_ = nullptr;
    return err;
  }
  hipError_t Release()
  {
    const hipError_t err = ptr_ ? hipFree(ptr_) : hipSuccess;
    ptr_ = nullptr;
    bytes_ = 0;
    return err;
  }
  void* data() const { return ptr_; }
  size_t bytes() const { return bytes_; }
  template <class T>
  T* as() const
  {
    return static_cast<T*>(ptr_);
  }

private:
  void* ptr_ = nullptr;
  size_t bytes_ = 0;
};
}  // namespace vgt
