// Host-side HIP resource layer of the native core: the one HIP_CHECK and the
// one owner each for device memory, streams, events and the current device.
// hipcore.hip and the files it includes (hbm_memtest.hip, cu_check.hip,
// valu_check.hip, gemm_check.hip, and burnin_host.h for HIP_CHECK) create and release these
// resources here and nowhere else, so a throwing HIP_CHECK
// between an allocation and its release leaks nothing, and every entry point
// hands the calling thread back on the device it came in on.
//
// Host only: nothing here is device code, and nothing depends on torch.
#pragma once
#include <hip/hip_runtime.h>

#include <stdexcept>
#include <string>
#include <utility>

#define HIP_CHECK(expr)                                                        \
  do {                                                                         \
    hipError_t _e = (expr);                                                    \
    if (_e != hipSuccess) {                                                    \
      throw std::runtime_error(std::string(#expr) + " failed: " +              \
                               hipGetErrorString(_e));                         \
    }                                                                          \
  } while (0)

namespace hip_host {

// Makes `device` current for the enclosing scope and restores the caller's
// device on exit: torch keeps its own notion of the current device, and a
// probe that left another one set would move the caller's next allocation.
class DeviceScope {
 public:
  explicit DeviceScope(int device) {
    HIP_CHECK(hipGetDevice(&prev_));
    HIP_CHECK(hipSetDevice(device));
  }
  DeviceScope(const DeviceScope&) = delete;
  DeviceScope& operator=(const DeviceScope&) = delete;
  ~DeviceScope() { (void)hipSetDevice(prev_); }

 private:
  int prev_ = -1;
};

// Owns `count` elements of device memory on `device`; movable, so a
// std::vector of them works. Allocates and frees with its own device current
// and leaves the caller's device as it was.
template <typename T>
struct DeviceBuf {
  T* ptr = nullptr;
  int device = -1;
  DeviceBuf(int device, size_t count) : device(device) {
    DeviceScope scope(device);
    HIP_CHECK(hipMalloc(&ptr, count * sizeof(T)));
  }
  DeviceBuf(DeviceBuf&& o) noexcept
      : ptr(std::exchange(o.ptr, nullptr)), device(o.device) {}
  DeviceBuf& operator=(DeviceBuf&& o) noexcept {
    std::swap(ptr, o.ptr);
    std::swap(device, o.device);
    return *this;
  }
  ~DeviceBuf() {
    if (!ptr) return;
    int prev = -1;  // a destructor must not throw: no DeviceScope here
    (void)hipGetDevice(&prev);
    (void)hipSetDevice(device);
    (void)hipFree(ptr);
    if (prev >= 0) (void)hipSetDevice(prev);
  }
};

// A stream on the device that is current at construction.
struct Stream {
  hipStream_t s = nullptr;
  Stream() { HIP_CHECK(hipStreamCreate(&s)); }
  Stream(const Stream&) = delete;
  Stream& operator=(const Stream&) = delete;
  ~Stream() { (void)hipStreamDestroy(s); }
  void synchronize() const { HIP_CHECK(hipStreamSynchronize(s)); }
};

// An event on the device that is current at construction.
struct Event {
  hipEvent_t e = nullptr;
  Event() { HIP_CHECK(hipEventCreate(&e)); }
  Event(const Event&) = delete;
  Event& operator=(const Event&) = delete;
  ~Event() { (void)hipEventDestroy(e); }
  void record(const Stream& stream) const { HIP_CHECK(hipEventRecord(e, stream.s)); }
  void synchronize() const { HIP_CHECK(hipEventSynchronize(e)); }
  // Both events must have completed.
  static float elapsed_ms(const Event& from, const Event& to) {
    float ms = 0.f;
    HIP_CHECK(hipEventElapsedTime(&ms, from.e, to.e));
    return ms;
  }
};

}  // namespace hip_host
