// pfb_list.hpp -- what the three list units share, and nobody else includes: pfb_deint.hip, pfb_assoc.hip and
// pfb_cluster.hip each take a list of up to 2^20 small integer records, in host or device memory, work in one grow-only
// scratch block carved into arrays (Carver, pfb_host.h), hand a small Control block back to the host and report the
// kernels they ran joined with `+`.
//   block_scan        exclusive scan of one value per lane over a workgroup of kThreads
//   list_scan         one workgroup: the counts of up to 1024 workgroups become the counts before each
// A unit keeps its own kernels (count and scatter among them: they read its flags and clear its accumulators), its
// Settings and checks, the one function that carves its scratch, every entry point and the sequence of its launches.
// Everything here is internal to the including unit: the three are separate code objects with host stubs of their own.
#pragma once

#include <hip/hip_runtime.h>

#include <string>

#include "pfb_common.h"
#include "pfb_host.h"

namespace {

using namespace pfb;
using u64 = unsigned long long;

constexpr int kThreads = 256;  // lanes of every workgroup of a list unit

// exclusive scan of one value per lane over the workgroup; *total: the sum
__device__ __forceinline__ uint32_t block_scan(uint32_t v, uint32_t* total) {
  __shared__ uint32_t wave_total[kThreads / 64];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  uint32_t inc = v;
  for (int d = 1; d < 64; d <<= 1) {
    const uint32_t o = __shfl_up(inc, d, 64);
    if (lane >= d) inc += o;
  }
  __syncthreads();  // wave_total of a call before is read
  if (lane == 63) wave_total[wv] = inc;
  __syncthreads();
  uint32_t before = 0, all = 0;
  for (int k = 0; k < kThreads / 64; ++k) {
    if (k < wv) before += wave_total[k];
    all += wave_total[k];
  }
  *total = all;
  return before + inc - v;
}

// one workgroup: counts[0 .. blocks) become the counts before each, blocks <= 1024; kTotal: the sum goes to *total_out
// (a template parameter, not a null test: without the store the kernel is the deinterleaver's as it was, byte for byte)
template <bool kTotal>
__global__ void __launch_bounds__(kThreads) list_scan(uint32_t* counts, uint32_t blocks, uint32_t* total_out) {
  uint32_t v[4], sum = 0;
  for (uint32_t k = 0; k < 4; ++k) {
    const uint32_t i = threadIdx.x * 4 + k;
    v[k] = i < blocks ? counts[i] : 0;
    sum += v[k];
  }
  uint32_t total;
  uint32_t at = block_scan(sum, &total);
  for (uint32_t k = 0; k < 4; ++k) {
    const uint32_t i = threadIdx.x * 4 + k;
    if (i < blocks) counts[i] = at;
    at += v[k];
  }
  if (kTotal && threadIdx.x == 0) *total_out = total;
}

// ---------------------------------------------------------------------------------
// host: the state of a handle and of a call

enum { kTierAuto = 0, kTierLds = 1, kTierGlobal = 2 };

struct ListHandle {
  int device = 0;
  hipStream_t stream = nullptr;
  hipEvent_t ev_switch = nullptr;
  char* d_scratch = nullptr;
  size_t cap = 0;  // records the scratch is carved for
  std::string last_kernel;

  // grow-only: a scratch of `bytes` for lists of `want` records; what it held is not kept
  int ensure(size_t want, size_t bytes) {
    if (want <= cap) return PFB_OK;
    (void)hipFree(d_scratch);
    d_scratch = nullptr;
    cap = 0;
    HIP_TRY(hipMalloc(reinterpret_cast<void**>(&d_scratch), bytes));
    cap = want;
    return PFB_OK;
  }
  void release() {
    DeviceGuard g(device);
    (void)hipFree(d_scratch);
    if (ev_switch) (void)hipEventDestroy(ev_switch);
  }
};

struct ListCall {
  std::string kernels;  // what the call launched, each name once
  void ran(const char* name) {
    if (kernels.find(name) != std::string::npos) return;
    if (!kernels.empty()) kernels += "+";
    kernels += name;
  }
};

bool misaligned(const void* p, uintptr_t to) { return reinterpret_cast<uintptr_t>(p) % to != 0; }

// what every call that takes a list checks before the device is touched; a device list is aligned to `align` bytes
int check_list(const ListHandle* h, const void* list, uint64_t n, uint64_t max_n, uint32_t mem, uintptr_t align) {
  if (!h || mem > PFB_MEM_DEVICE || n > max_n || (n > 0 && !list)) return PFB_ERR_BAD_ARG;
  if (mem == PFB_MEM_DEVICE && misaligned(list, align)) return PFB_ERR_BAD_ARG;
  return PFB_OK;
}

// a result from the scratch to the caller's memory of kind `mem`, on the stream
int copy_out(hipStream_t stream, void* dst, const void* d_src, size_t bytes, uint32_t mem) {
  if (!bytes) return PFB_OK;
  HIP_TRY(hipMemcpyAsync(dst, d_src, bytes, mem == PFB_MEM_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, stream));
  return PFB_OK;
}

// a control block to the host: returns once it is there
template <class T>
int fetch(hipStream_t stream, const T* d_src, T* out) {
  HIP_TRY(hipMemcpyAsync(out, d_src, sizeof(T), hipMemcpyDeviceToHost, stream));
  HIP_TRY(hipStreamSynchronize(stream));
  return PFB_OK;
}

static_assert(PFB_ERR_INTERNAL < 0 && PFB_ERR_HIP < 0 && PFB_ERR_NO_MEMORY < 0, "a status is told from a count by its sign");

// Rounds until one hooks nothing: queue_round(r) queues round r, whose kernels set d_hooked[r] where they hooked.
// Returns the rounds made, one at least, or a status, which is negative: PFB_ERR_INTERNAL when `limit` rounds all hooked.
template <class F>
int hook_until_still(hipStream_t stream, const uint32_t* d_hooked, int limit, F queue_round) {
  for (int r = 0;; ++r) {
    if (r == limit) return PFB_ERR_INTERNAL;
    const int rc = queue_round((uint32_t)r);
    if (rc != PFB_OK) return rc;
    uint32_t hooked = 0;
    HIP_TRY(hipMemcpyAsync(&hooked, d_hooked + r, sizeof(hooked), hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    if (!hooked) return r + 1;
  }
}

// the bodies of pfb_*_destroy, _set_stream, _sync, _get_device and _get_stats
template <class H>
int destroy_list(H* h) {
  if (!h) return PFB_ERR_BAD_ARG;
  h->release();
  delete h;
  return PFB_OK;
}

int set_list_stream(ListHandle* h, void* hip_stream) {
  if (!h) return PFB_ERR_BAD_ARG;
  return switch_stream(h->device, &h->stream, &h->ev_switch, static_cast<hipStream_t>(hip_stream));
}

int sync_list(ListHandle* h) {
  if (!h) return PFB_ERR_BAD_ARG;
  DeviceGuard g(h->device);
  HIP_TRY(hipStreamSynchronize(h->stream));
  return PFB_OK;
}

int list_device(const ListHandle* h, int* device_id) {
  if (!h || !device_id) return PFB_ERR_BAD_ARG;
  *device_id = h->device;
  return PFB_OK;
}

template <class H, class S>
int list_stats(const H* h, S* stats_out) {
  if (!h || !stats_out) return PFB_ERR_BAD_ARG;
  *stats_out = h->stats;
  return PFB_OK;
}

}  // namespace
