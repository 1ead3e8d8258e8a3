// dcrx_hip.h — how libdcrx's host code reports a HIP error and owns what it takes from the HIP runtime: device and pinned
// memory, streams, events.  Private to the translation units that already include hip_runtime.h; nothing here is device code.
// An owner frees what it holds when it goes out of scope or is assigned over, so an error path cannot leave a buffer behind
// and a struct of owners is released by assigning it a fresh one.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <string>
#include <utility>

#include "../../include/dcrx.h"

namespace dcrx {

int set_err(int code, const char *msg);      // dcrx_api.cpp: the thread's dcrx_last_error()

// the code and message of a failed HIP call (the runtime's own record of it is cleared: it has been reported here)
inline int hip_fail(hipError_t e, const char *what) {
  const std::string m = std::string(what) + ": " + hipGetErrorString(e);
  (void)hipGetLastError();
  return set_err((e == hipErrorNoDevice || e == hipErrorInvalidDevice) ? DCRX_E_NOGPU : DCRX_E_HIP, m.c_str());
}

#define HIP_TRY(call)                                         \
  do {                                                        \
    hipError_t e_ = (call);                                   \
    if (e_ != hipSuccess) return ::dcrx::hip_fail(e_, #call); \
  } while (0)

// What the four owners share: one handle of type H (null: nothing held) that Release gives back; it moves, it is not copied.
template <class H, auto Release> class HipOwner {
 public:
  HipOwner() = default;
  HipOwner(HipOwner &&o) noexcept : h_(std::exchange(o.h_, H{})) {}
  HipOwner &operator=(HipOwner &&o) noexcept {
    if (this != &o) { reset(); h_ = std::exchange(o.h_, H{}); }
    return *this;
  }
  ~HipOwner() { reset(); }
  void reset() { if (h_) (void)Release(h_); h_ = H{}; }
  operator H() const { return h_; }      // what the HIP calls and the kernels take
  H get() const { return h_; }           // ... where a template has to deduce the type

 protected:
  int took(hipError_t e, const char *what) {      // the call that was to fill h_
    if (e == hipSuccess) return DCRX_OK;
    h_ = H{};
    return hip_fail(e, what);
  }
  H h_{};
};

// `count` elements of T in device memory (the current device's), or in pinned host memory; what was held before is freed first
template <class T> struct DevBuf : HipOwner<T *, hipFree> {
  int alloc(size_t count) { this->reset(); return this->took(hipMalloc(reinterpret_cast<void **>(&this->h_), count * sizeof(T)), "hipMalloc"); }
};
template <class T> struct PinnedBuf : HipOwner<T *, hipHostFree> {
  int alloc(size_t count) { this->reset(); return this->took(hipHostMalloc(reinterpret_cast<void **>(&this->h_), count * sizeof(T), hipHostMallocDefault), "hipHostMalloc"); }
};
// a non-blocking stream (it orders against no other stream, the null stream included)
struct Stream : HipOwner<hipStream_t, hipStreamDestroy> {
  int create() { reset(); return took(hipStreamCreateWithFlags(&h_, hipStreamNonBlocking), "hipStreamCreateWithFlags"); }
};
// an event that can be timed (hipEventElapsedTime), or one that only orders streams (cheaper to record)
struct Event : HipOwner<hipEvent_t, hipEventDestroy> {
  int create(bool timing) { reset(); return took(timing ? hipEventCreate(&h_) : hipEventCreateWithFlags(&h_, hipEventDisableTiming), "hipEventCreate"); }
};

// Makes `device` the current one for a scope and puts the caller's back at its end: what belongs to a device is released
// with that device current.  A negative device, or a runtime that cannot name the current one, leaves everything as it is.
class DeviceGuard {
 public:
  explicit DeviceGuard(int device) {
    if (device < 0 || hipGetDevice(&prev_) != hipSuccess) { prev_ = -1; return; }
    if (prev_ == device || hipSetDevice(device) != hipSuccess) prev_ = -1;
  }
  ~DeviceGuard() { if (prev_ >= 0) (void)hipSetDevice(prev_); }
  DeviceGuard(const DeviceGuard &) = delete;
  DeviceGuard &operator=(const DeviceGuard &) = delete;

 private:
  int prev_ = -1;      // the device to go back to (-1: nothing was switched)
};

}  // namespace dcrx
