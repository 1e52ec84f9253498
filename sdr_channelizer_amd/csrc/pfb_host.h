// pfb_host.h -- host-only plumbing of every unit that has a host side (pfb_api.cpp, pfb_stft_api.cpp, pfb_event.cpp and
// the .hip units with entry points of their own; defined in pfb_host.cpp): HIP error mapping, device selection, stream
// switch, twiddle upload, the carving of a scratch block, the staged host-pointer pipeline and the .iq record reader.
// What only the matched filter and its bank share is in pfb_ols_host.h, the two map detectors in pfb_rdmap.hpp, the
// three list units (deinterleaver, associator, clusterer) in pfb_list.hpp.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <functional>
#include <string>

#include "pfb_channelizer.h"

namespace pfb {

extern thread_local std::string g_detail;  // what pfb_last_error_detail() returns

// map a failed HIP call to a PFB_ERR_* status, keep its text in g_detail and clear the sticky error
int hip_fail(hipError_t e, const char* what);

#define HIP_TRY(expr)                                       \
  do {                                                      \
    const hipError_t e__ = (expr);                          \
    if (e__ != hipSuccess) return pfb::hip_fail(e__, #expr); \
  } while (0)

struct DeviceGuard {  // run on the handle's device, restore the caller's afterwards
  int prev = -1;
  bool switched = false;
  explicit DeviceGuard(int dev) {
    if (hipGetDevice(&prev) == hipSuccess && prev != dev) switched = (hipSetDevice(dev) == hipSuccess);
  }
  ~DeviceGuard() {
    if (switched) (void)hipSetDevice(prev);
  }
};

// A device_id argument: -1 (any negative) is the device current now.  PFB_ERR_NO_DEVICE without a HIP device,
// PFB_ERR_BAD_ARG for an ordinal past the last device.
int resolve_device(int requested, int* dev);

// What pfb_dwell_analyze and pfb_dwell_from_iq_file check of their config before the device is touched (pfb_event.cpp);
// from_file: sample format, bit width, fs and mem come from the record, not from the config.
int dwell_check_config(const pfb_dwell_config* cfg, bool from_file);

// pfb_*_set_stream: what the old stream still has queued for the handle comes first on the new one
int switch_stream(int device, hipStream_t* stream, hipEvent_t* ev_switch, hipStream_t next);

// a grow-only device buffer: at least `want` bytes at *p, *have of them now; what it held is not kept
int grow(void** p, size_t* have, size_t want);

// workgroups for `items` at `per_block` each: one at least, `cap` at most (the kernels stride)
unsigned grid_for(uint64_t items, unsigned per_block, unsigned cap);

constexpr size_t round_up(size_t v, size_t to) { return (v + to - 1) / to * to; }

// A scratch block cut into typed arrays of whole 256-byte pieces, in the order they are asked for.  Without a base it
// only measures: every array is null then, and bytes() is what the block must hold.
struct Carver {
  char* base = nullptr;
  size_t at = 0;
  template <class T>
  T* array(size_t count) {
    const size_t here = at;
    at += round_up(count * sizeof(T), 256);
    return base ? reinterpret_cast<T*>(base + here) : nullptr;
  }
  size_t bytes() const { return at; }
};

// tw[m] = e^{+j 2 pi m / n}, m = 0..n-1 (from float64), into a new device array
hipError_t upload_twiddles(uint32_t n, float2** d_tw);

// Device staging of a handle's host-pointer calls: two buffer sets, so that chunk i+1 crosses PCIe inbound while
// chunk i is transformed and chunk i-1 goes out, and the two copy streams with their events.  Grow-only.
struct HostStage {
  void* d_in[2] = {nullptr, nullptr};
  void* d_out[2] = {nullptr, nullptr};
  size_t in_bytes = 0, out_bytes = 0;
  hipStream_t s_in = nullptr, s_out = nullptr;
  hipEvent_t ev_in[2] = {nullptr, nullptr}, ev_k[2] = {nullptr, nullptr}, ev_out[2] = {nullptr, nullptr};
  int ensure(size_t in, size_t out);  // both sets of at least these sizes (0: leave that side alone)
  void release();                     // on the owning handle's device
};

struct StageSteps {  // how a handle turns one staged chunk into frames
  uint64_t chunk;        // samples per staging step
  uint64_t max_frames;   // the most frames one step can complete
  size_t in_bps;         // bytes per input sample
  size_t frame_bytes;    // bytes per output frame
  std::function<uint64_t(uint64_t m)> frames_for;  // frames the next m samples complete (the handle's state now)
  // queue the transform of m device samples and the state update on the handle's stream; f frames land at d_out,
  // frame-major rows, or channel-major at row out_row0 of columns out_ld frames long
  std::function<int(const void* d_in, uint64_t m, void* d_out, uint64_t f, int64_t out_ld, int64_t out_row0)> enqueue;
};

// Where the frames of a staged call go: rows [row0, row0 + frames) of `ptr`, frame-major (ld = 0) or channel-major
// (a cols x ld matrix, one column per channel).  device: `ptr` is device memory that the kernels fill in place.
struct StageOut {
  void* ptr;
  bool device = false;
  uint64_t ld = 0;
  uint64_t row0 = 0;
  int cols = 0;
};

// Transform n host samples through `st`: copy-in on st.s_in, the kernels on `stream`, copy-out on st.s_out (page-locked
// caller buffers keep both PCIe directions busy at once).  Returns once the output is in place (device output: once the
// input has left the host buffer) -- or, on failure, once nothing touches the caller's buffers any more.
int stage_host(HostStage& st, hipStream_t stream, const StageSteps& steps, const void* in, uint64_t n,
               const StageOut& out);

// What pfb_waterfall.hip reads of a channelizer or STFT handle whose output it reduces (pfb_wf_from_*_iq_file):
// defined next to each handle, pfb_api.cpp and pfb_stft_api.cpp.
struct OutputDesc {
  int device = 0;
  hipStream_t stream = nullptr;
  int fmt = 0, bit_width = 0, bps = 0;  // of the input samples
  uint32_t width = 0;                   // output values per frame: M, nfft
  uint32_t element = 0;                 // PFB_WF_* of one output value
  uint32_t layout = 0;                  // PFB_WF_ROWS / PFB_WF_COLUMNS
  bool reducible = true;                // false: the output is not a power (PFB_STFT_DB)
  uint64_t carry_max = 0;               // the most samples the handle carries from call to call
};
OutputDesc describe_output(const pfb_handle* h);
OutputDesc describe_output(const pfb_stft_handle* h);

struct Record {  // an open .iq record whose header has been parsed and checked
  int fd = -1;
  pfb_iq_info info{};  // zeroed: callers copy it out even when the record could not be opened
  Record() = default;
  Record(const Record&) = delete;  // owns the descriptor
  Record& operator=(const Record&) = delete;
  ~Record();
  // payload length against the file size; format and bit width against the caller's (fmt < 0: any record)
  int open(const char* path, int fmt = -1, int bit_width = -1);
  // Walk the payload in chunks through two page-locked buffers: reader threads fill the next one while consume() works
  // on samples [first, first + m) and must be done with `buf` when it returns.  A short read is PFB_ERR_BAD_FORMAT.
  int read(uint64_t chunk, const std::function<int(const char* buf, uint64_t first, uint64_t m)>& consume);
};

}  // namespace pfb
