// pfb_pdw_scratch.hpp -- host plumbing every driver of pfb_pdw.hip shares: the error text, the per-device scratch arenas
// and pinned block, the call context (PdwCall) and the two run-time -> compile-time dispatches.  No kernels, and
// nothing of the reference scripts: this is what their MATLAB workspace is here.
#pragma once

#include <hip/hip_runtime.h>
#include <mutex>
#include <optional>
#include <string>
#include <type_traits>

#include "pfb_common.h"  // abi_guard, launch_transpose_slab (pfb_kernels.hip)
#include "pfb_host.h"    // resolve_device, DeviceGuard

namespace {
thread_local std::string g_pdw_detail;
thread_local int g_pdw_path = 0;

// leaves the function with the error's code; a driver's PdwCall synchronises the stream on the way out
#define PDW_TRY(expr)                                                                  \
  do {                                                                                 \
    const hipError_t e__ = (expr);                                                     \
    if (e__ != hipSuccess) {                                                           \
      g_pdw_detail = std::string(#expr) + ": " + hipGetErrorString(e__);               \
      (void)hipGetLastError();                                                         \
      return (e__ == hipErrorOutOfMemory) ? PFB_ERR_NO_MEMORY : PFB_ERR_HIP;           \
    }                                                                                  \
  } while (0)

// Device scratch is kept between calls (grow-only, one pair of arenas per device): a call needs some
// twenty buffers, and allocating and freeing them cost more than the kernels of a short extraction.
// Arena 0 holds everything sized by (F, M); arena 1 the edge lists and PDWs, sized by the pulse count.
constexpr int kMaxDevices = 64;
struct Arena {
  char* p = nullptr;
  size_t cap = 0, used = 0;
};
std::mutex g_ws_mutex;
Arena g_ws[kMaxDevices][2];

// small pinned host block per device: the words that cross the bus in the middle of an extraction (edge totals, flags,
// medians down; column bases up) move by DMA instead of through the runtime's pageable-copy staging
struct HostPin {
  char* p = nullptr;
  size_t cap = 0;
};
HostPin g_pin[kMaxDevices];
hipError_t pin_reserve(HostPin& h, size_t bytes) {
  if (bytes <= h.cap) return hipSuccess;
  if (h.p) (void)hipHostFree(h.p);
  h.p = nullptr;
  h.cap = 0;
  const hipError_t e = hipHostMalloc((void**)&h.p, bytes, hipHostMallocDefault);
  if (e == hipSuccess) h.cap = bytes;
  return e;
}

hipError_t arena_reserve(Arena& a, size_t bytes) {
  a.used = 0;
  if (bytes <= a.cap) return hipSuccess;
  (void)hipFree(a.p);
  a.p = nullptr;
  a.cap = 0;
  bytes += bytes / 8;
  const hipError_t e = hipMalloc((void**)&a.p, bytes);
  if (e == hipSuccess) a.cap = bytes;
  return e;
}
constexpr size_t kAlign = 256;
size_t padded(size_t bytes) { return (bytes + kAlign - 1) / kAlign * kAlign; }
template <class T>
T* take(Arena& a, size_t count) {  // an arena without memory only measures: nullptr, and `used` advances
  T* r = a.p ? reinterpret_cast<T*>(a.p + a.used) : nullptr;
  a.used += padded(count * sizeof(T));
  return r;
}
// An arena's layout is written once, as a callable that takes every buffer of the call: it runs on a measuring arena,
// the real one is reserved for exactly what that handed out, and it runs again there.
template <class Layout>
hipError_t arena_layout(Arena& a, Layout&& layout) {
  Arena measure{};
  layout(measure);
  const hipError_t e = arena_reserve(a, measure.used);
  if (e == hipSuccess) layout(a);
  return e;
}

// One call of an entry point, made at the top of its driver once the arguments are checked: the device (the call runs
// on it, the caller's comes back afterwards), the lock (one extraction per process at a time shares the scratch), the
// arenas and the stream.  rc != PFB_OK: the device was refused and the driver returns rc.  Every other way out of the
// driver, early or not, passes the destructor's stream sync.
struct PdwCall {
  int dev = 0;
  const int rc;
  std::optional<pfb::DeviceGuard> guard;
  std::unique_lock<std::mutex> lock;
  Arena &ws, &ws2;
  const hipStream_t st;
  PdwCall(int32_t device_id, void* hip_stream)
      : rc(resolve(device_id, &dev)), ws(g_ws[dev][0]), ws2(g_ws[dev][1]), st(static_cast<hipStream_t>(hip_stream)) {
    if (rc != PFB_OK) return;
    guard.emplace(dev);
    lock = std::unique_lock<std::mutex>(g_ws_mutex);
  }
  ~PdwCall() { if (rc == PFB_OK) (void)hipStreamSynchronize(st); }
  static int resolve(int32_t device_id, int* dev) {
    int rc = pfb::resolve_device(device_id, dev);
    if (rc == PFB_OK && *dev >= kMaxDevices) rc = PFB_ERR_BAD_ARG;
    if (rc != PFB_OK) *dev = 0;
    return rc;
  }
};

// a run-time bool as std::true_type / std::false_type, a sample format as std::integral_constant<int, PFB_FMT_*>:
// fn is a generic lambda that names its kernel or function template with decltype(tag)::value
template <class Fn>
void with_bool(bool b, Fn&& fn) { if (b) fn(std::true_type{}); else fn(std::false_type{}); }
template <class Fn>
int with_format(uint32_t sample_format, Fn&& fn) {
  switch (sample_format) {
    case PFB_FMT_INT8_IQ: return fn(std::integral_constant<int, PFB_FMT_INT8_IQ>{});
    case PFB_FMT_INT16_IQ: return fn(std::integral_constant<int, PFB_FMT_INT16_IQ>{});
    default: return fn(std::integral_constant<int, PFB_FMT_CF32>{});
  }
}
}  // namespace
