// pfb_api.cpp -- host side of the channelizer's C ABI in include/pfb_channelizer.h.
//
// Owns: the handle (taps, twiddles, history, counters, options), the choice between the shape's fused plan and the
// generic kernel, the launch itself (launch_frames: one kernel, or slabs + transpose; how a fused plan is launched is
// decided in pfb_launch_policy.h), the host-pointer and .iq paths (over the staged pipeline and the record reader of
// pfb_host.h), time sharding, the state blob and the copy yardsticks of pfb_channelizer_dev.h.  All arithmetic is in
// the kernels (pfb_kernels*.hip); there is deliberately no CPU implementation here.  The STFT's ABI is in
// pfb_stft_api.cpp.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <new>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "pfb_common.h"
#include "pfb_channelizer_dev.h"
#include "pfb_fast_cfg.hpp"  // launch_blocks: the one launch of a kernel entry
#include "pfb_host.h"
#include "pfb_launch_policy.h"

using pfb::DeviceGuard;
using pfb::g_detail;
using pfb::hip_fail;

namespace {

constexpr uint32_t kStateMagic = 0x50464231u;  // "PFB1"
constexpr int kExpSeparateHistory = 2;  // PFB_OPT_EXPERIMENT bit 1: the history update always as a launch of its own

struct StateHeader {
  uint32_t magic, M, P, D, fmt, hist_samples, phase, reserved;
  uint64_t frame_index;
};

}  // namespace

struct pfb_handle {
  int M = 0, P = 0, D = 0, off = 0;
  int fmt = 0, bit_width = 0, layout = 0;
  unsigned flags = 0;
  int device = 0;
  int num_cus = 256;       // compute units of the device (slab sizing)
  int bps = 0;             // bytes per input sample
  int out_elem = 8;        // bytes per output element: complex64, or float32 with PFB_FLAG_MAGNITUDE
  int hist_samples = 0;    // M*P + D
  float* d_taps = nullptr;   // M*P, scaled by 2^-(bit_width-1)
  float2* d_tw = nullptr;    // M
  float* d_taps_lane = nullptr;   // fast kernels: per-column tap table
  float2* d_tw_lane = nullptr;    // fast kernels: inter-pass twiddle rows
  void* d_hist[2] = {nullptr, nullptr};
  int cur = 0;               // which history buffer is current
  uint32_t phase = 0;        // samples carried since the last frame boundary (0..D-1)
  uint64_t frame_index = 0;  // global index of the next frame
  hipStream_t stream = nullptr;
  const pfb::FastKernelInfo* fast = nullptr;
  pfb_fast_plan_desc plan{};  // fast's row of the table as pfb_fast_plan_info gives it: what the launch policy reads
  // options
  int opt_kernel = 0;
  int opt_frames_per_block = 0;
  int64_t opt_host_chunk = 0;
  int opt_nontemporal = 0;
  int opt_xcd_remap = -1;  // -1: per schedule (on for 0..3, off for the wave-pair schedule)
  int opt_experiment = 0;
  int opt_variant = 0;
  int opt_schedule = -1;  // -1: the instantiation's measured default
  int opt_grid = 0;
  int opt_tile_waves = 8;
  int64_t opt_slab_frames = 0;  // channel-major by slabs: frames per slab (0 = ~32 MiB of output)
  void* d_slab = nullptr;       // frame-major scratch of the slab path
  size_t slab_bytes = 0;
  void* d_matrix = nullptr;     // pfb_pdw_from_iq_file: the record's channel matrix (grow-only)
  size_t matrix_bytes = 0;
  const char* last_kernel = "";
  pfb_launch_report last_launch{};  // what launch_frames handed to the kernel last time (pfb_last_launch)
  pfb::KernelEntry last_entry{};    // the kernel that launch ran (pfb_last_entry)
  pfb::HostStage stage;  // host-pointer calls (stage.d_in[0] is also pfb_prime's scratch)
  // PFB_OPT_PROFILE: event pairs around each channelizer kernel launch
  int opt_profile = 0;
  std::vector<std::pair<hipEvent_t, hipEvent_t>> ev_pool;  // reusable pairs
  size_t ev_used = 0;
  // time sharding (pfb_shard_attach): this handle owns segment shard_rank of shard_world
  int shard_rank = 0, shard_world = 1;
  bool shard_ring = false;
  pfb_halo_exchange_fn shard_exchange = nullptr;
  void* shard_user = nullptr;
  void* d_halo = nullptr;            // hist_samples raw samples; the predecessor's tail lands in its last halo_samples
  hipStream_t s_halo = nullptr;      // side stream of the exchange
  hipEvent_t ev_seg = nullptr, ev_halo = nullptr;
  hipEvent_t ev_switch = nullptr;    // pfb_set_stream: orders the old stream's work in front of the new stream's
};

pfb::OutputDesc pfb::describe_output(const pfb_handle* h) {
  pfb::OutputDesc d;
  d.device = h->device;
  d.stream = h->stream;
  d.fmt = h->fmt;
  d.bit_width = h->bit_width;
  d.bps = h->bps;
  d.width = (uint32_t)h->M;
  d.element = !(h->flags & PFB_FLAG_MAGNITUDE) ? PFB_WF_COMPLEX : ((h->flags & PFB_FLAG_POWER) ? PFB_WF_POWER : PFB_WF_MAGNITUDE);
  d.layout = h->layout == PFB_LAYOUT_CHANNEL_MAJOR ? PFB_WF_COLUMNS : PFB_WF_ROWS;
  d.carry_max = (uint64_t)h->D - 1;
  return d;
}

namespace {

void free_handle(pfb_handle* h) {
  if (!h) return;
  DeviceGuard g(h->device);
  (void)hipFree(h->d_taps);
  (void)hipFree(h->d_tw);
  (void)hipFree(h->d_taps_lane);
  (void)hipFree(h->d_tw_lane);
  (void)hipFree(h->d_hist[0]);
  (void)hipFree(h->d_hist[1]);
  (void)hipFree(h->d_slab);
  (void)hipFree(h->d_matrix);
  (void)hipFree(h->d_halo);
  h->stage.release();
  if (h->s_halo) (void)hipStreamDestroy(h->s_halo);
  if (h->ev_seg) (void)hipEventDestroy(h->ev_seg);
  if (h->ev_halo) (void)hipEventDestroy(h->ev_halo);
  if (h->ev_switch) (void)hipEventDestroy(h->ev_switch);
  for (auto& pr : h->ev_pool) { (void)hipEventDestroy(pr.first); (void)hipEventDestroy(pr.second); }
  delete h;
}

uint64_t frames_for(const pfb_handle* h, uint64_t n) { return (h->phase + n) / (uint64_t)h->D; }

// PFB_OPT_PROFILE: take the next event pair of the pool (a new one when all are in use) and record its first event on
// the stream.  *second is the event to record behind the launch, null when not profiling or 4096 pairs are taken.
int begin_profile(pfb_handle* h, hipEvent_t* second) {
  *second = nullptr;
  if (!h->opt_profile || h->ev_used >= 4096) return PFB_OK;
  if (h->ev_used == h->ev_pool.size()) {
    hipEvent_t a = nullptr, b = nullptr;
    HIP_TRY(hipEventCreate(&a));
    if (hipEventCreate(&b) != hipSuccess) { (void)hipEventDestroy(a); return hip_fail(hipGetLastError(), "hipEventCreate"); }
    h->ev_pool.emplace_back(a, b);
  }
  HIP_TRY(hipEventRecord(h->ev_pool[h->ev_used].first, h->stream));
  *second = h->ev_pool[h->ev_used].second;
  ++h->ev_used;  // only a pair whose first event was recorded counts as used
  return PFB_OK;
}

// What the launch policy decided goes into a fused call's KernelParams here, for launch_frames and pfb_plan_entry alike.
void apply_policy(pfb::KernelParams& p, const pfb_launch_report& rep) {
  p.schedule = rep.schedule;
  p.frames_per_block = rep.frames_per_block;
  p.xcd_remap = rep.xcd_remap;
}

// Every fused launch: resolve p to its kernel entry (the plan's select, a pure function), launch that entry, and keep it
// next to last_launch -- the report is what was asked of the kernel, the entry is what ran.
int launch_fused(pfb_handle* h, const pfb::KernelParams& p) {
  const pfb::KernelEntry e = h->fast->select(p);
  HIP_TRY(pfb::launch_blocks(e, p, h->stream));
  h->last_entry = e;
  return PFB_OK;
}

// Channel-major by slabs of sf frames: the frame-major kernel fills the handle's scratch slab (grown here), the
// transpose kernel moves it into place.  p is the whole call's launch; its output fields say where the matrix is.
int launch_by_slabs(pfb_handle* h, const pfb::KernelParams& p, long long sf) {
  const size_t need = (size_t)sf * h->M * h->out_elem;
  if (need > h->slab_bytes) {
    HIP_TRY(hipStreamSynchronize(h->stream));
    (void)hipFree(h->d_slab);
    h->d_slab = nullptr; h->slab_bytes = 0;
    HIP_TRY(hipMalloc(&h->d_slab, need));
    h->slab_bytes = need;
  }
  for (long long f0 = 0; f0 < p.frames; f0 += sf) {
    pfb::KernelParams q = p;
    q.layout = PFB_LAYOUT_FRAME_MAJOR;
    q.out = static_cast<float2*>(h->d_slab);
    q.frames = std::min<long long>(sf, p.frames - f0);
    q.frame0 = p.frame0 + f0;
    q.in = static_cast<const char*>(p.in) + (size_t)f0 * h->D * h->bps;
    q.n_in = p.n_in - f0 * h->D;
    if (f0 > 0)  // "history" of a later slab = the input samples in front of it
      q.hist = static_cast<const char*>(q.in) - (size_t)h->hist_samples * h->bps;
    const int rc = launch_fused(h, q);
    if (rc != PFB_OK) return rc;
    HIP_TRY(pfb::launch_transpose_slab(h->d_slab, q.frames, h->M, p.out, p.out_ld, p.out_frame0 + f0, h->out_elem, h->stream));
  }
  return PFB_OK;
}

// Launch the channelizer kernel(s) for local frames [f_begin, f_end) of a device buffer of n samples.  `hist` holds
// the hist_samples raw samples in front of d_iq[0]; it is only read when f_begin == 0 (a later range starts at
// least hist_samples into the buffer, so its "history" is the buffer itself).  Output row f lands where a call
// over the whole buffer would put it.  No state change, no host sync.  hist_out (enqueue only, f_begin == 0 and
// n >= hist_samples): where the launch itself leaves the next call's history when it is a single kernel -- *carried says
// whether it did; by slabs it does not.
int launch_frames(pfb_handle* h, const void* d_iq, uint64_t n, const void* hist, void* d_out, uint64_t f_begin,
                  uint64_t f_end, int64_t out_ld, int64_t out_frame0, void* hist_out = nullptr, bool* carried = nullptr) {
  if (carried) *carried = false;
  if (f_end <= f_begin) return PFB_OK;
  if (f_begin > 0) {
    if (f_begin * (uint64_t)h->D < (uint64_t)h->hist_samples) return PFB_ERR_BAD_ARG;
    const size_t skip = (size_t)f_begin * h->D * h->bps;
    hist = static_cast<const char*>(d_iq) + skip - (size_t)h->hist_samples * h->bps;
    d_iq = static_cast<const char*>(d_iq) + skip;
    n -= f_begin * (uint64_t)h->D;
    if (h->layout == PFB_LAYOUT_FRAME_MAJOR) d_out = static_cast<char*>(d_out) + (size_t)f_begin * h->M * h->out_elem;
    else out_frame0 += (int64_t)f_begin;
  }
  const uint64_t frames = f_end - f_begin;
  pfb::KernelParams p{};
  p.in = d_iq;
  p.hist = hist;
  p.out = static_cast<float2*>(d_out);
  p.taps = h->d_taps;
  p.tw = h->d_tw;
  p.taps_lane = h->d_taps_lane;
  p.tw_lane = h->d_tw_lane;
  p.n_in = (long long)n;
  p.frames = (long long)frames;
  p.frame0 = (long long)(h->frame_index + f_begin);
  p.out_ld = out_ld;
  p.out_frame0 = out_frame0;
  p.base = (h->off - (int)h->phase) - (h->D - 1);
  p.hist_samples = h->hist_samples;
  p.M = h->M; p.P = h->P; p.D = h->D;
  p.fmt = h->fmt;
  p.layout = h->layout;
  p.flags = h->flags;
  p.nontemporal = h->opt_nontemporal;
  p.xcd_remap = h->opt_xcd_remap < 0 ? 1 : h->opt_xcd_remap;
  p.experiment = h->opt_experiment;
  p.grid_override = h->opt_grid;
  p.tile_waves = h->opt_tile_waves;
  const bool want_fast = h->fast && h->opt_kernel != 1;
  if (h->opt_kernel == 2 && !want_fast) return PFB_ERR_UNSUPPORTED;
  hipEvent_t ev_second = nullptr;
  const int prc = begin_profile(h, &ev_second);
  if (prc != PFB_OK) return prc;
  if (want_fast) {
    const pfb::LaunchRequest rq{h->opt_schedule, h->opt_frames_per_block, h->opt_xcd_remap, h->opt_slab_frames,
                                h->layout == PFB_LAYOUT_CHANNEL_MAJOR, (h->flags & PFB_FLAG_MAGNITUDE) != 0, h->num_cus};
    const pfb_launch_report rep = pfb::plan_launch(h->plan, rq, frames);
    apply_policy(p, rep);
    const int cpt = h->fast->cols_per_thread;
    const int bmod = ((p.base % cpt) + cpt) % cpt;
    p.vec_ok = (bmod == 0) && (reinterpret_cast<uintptr_t>(d_iq) % (uintptr_t)(h->bps * cpt) == 0);
    if (rep.by_slabs) {
      const int rc = launch_by_slabs(h, p, (long long)rep.slab_frames);
      if (rc != PFB_OK) return rc;
    } else {
      p.hist_out = hist_out;
      const int rc = launch_fused(h, p);
      if (rc != PFB_OK) return rc;
      if (carried) *carried = hist_out != nullptr;
    }
    h->last_kernel = h->fast->name;
    h->last_launch = rep;
  } else {
    p.hist_out = hist_out;
    HIP_TRY(pfb::launch_generic(p, h->stream, &h->last_entry));
    if (carried) *carried = hist_out != nullptr;
    h->last_kernel = "pfb_generic";
    h->last_launch = pfb_launch_report{};
    h->last_launch.frames = frames;
  }
  if (ev_second) HIP_TRY(hipEventRecord(ev_second, h->stream));
  return PFB_OK;
}

void advance_counters(pfb_handle* h, uint64_t n, uint64_t frames) {
  h->phase = (uint32_t)((h->phase + n) % (uint64_t)h->D);
  h->frame_index += frames;
}

// carry the last hist_samples raw samples of [history | d_iq] and advance the counters
int advance_state(pfb_handle* h, const void* d_iq, uint64_t n, uint64_t frames) {
  if (n > 0) {
    HIP_TRY(pfb::launch_update_history(h->d_hist[h->cur], d_iq, (long long)n, h->d_hist[h->cur ^ 1],
                                       h->hist_samples, h->bps, h->stream));
    h->cur ^= 1;
  }
  advance_counters(h, n, frames);
  return PFB_OK;
}

// enqueue kernel + history update for device-resident buffers; no host sync.  A call that is at least one history long
// and produces frames in a single kernel carries its history inside that launch (carry_history, pfb_fast_cfg.hpp): one
// launch per call.  Shorter calls (old history is mixed in), calls without a frame, the slab route and
// kExpSeparateHistory take pfb_update_history_kernel behind the channelizer kernel.
int enqueue(pfb_handle* h, const void* d_iq, uint64_t n, void* d_out, uint64_t frames, int64_t out_ld,
            int64_t out_frame0) {
  const bool fuse = frames > 0 && n >= (uint64_t)h->hist_samples && !(h->opt_experiment & kExpSeparateHistory);
  bool carried = false;
  const int rc = launch_frames(h, d_iq, n, h->d_hist[h->cur], d_out, 0, frames, out_ld, out_frame0,
                               fuse ? h->d_hist[h->cur ^ 1] : nullptr, &carried);
  if (rc != PFB_OK) return rc;
  if (!carried) return advance_state(h, d_iq, n, frames);
  h->cur ^= 1;
  advance_counters(h, n, frames);
  return PFB_OK;
}

// The host path stages through h->stage in chunks of whole frames, so a chunk boundary never falls inside a frame's
// decimation step: PFB_OPT_HOST_CHUNK_SAMPLES, or 2^24 samples.  `out` as in pfb::stage_host: pfb_process fills rows
// [0, frames) of a frame-major buffer or of an M x frames matrix; the .iq front end walks row0 through a record.
int process_host(pfb_handle* h, const void* iq, uint64_t n, const pfb::StageOut& out, uint64_t chunk = 0) {
  if (chunk == 0) chunk = h->opt_host_chunk > 0 ? (uint64_t)h->opt_host_chunk : (uint64_t)1 << 24;
  chunk = ((chunk + h->D - 1) / h->D) * h->D;
  const pfb::StageSteps steps{
      chunk, chunk / h->D + 1, (size_t)h->bps, (size_t)h->M * h->out_elem,
      [h](uint64_t m) { return frames_for(h, m); },
      [h](const void* d_in, uint64_t m, void* d_out, uint64_t f, int64_t out_ld, int64_t out_row0) {
        return enqueue(h, d_in, m, d_out, f, out_ld, out_row0);
      }};
  return pfb::stage_host(h->stage, h->stream, steps, iq, n, out);
}

// Allocate the per-lane tables of fused plan f and fill them from the handle's taps and twiddles (the null stream is
// drained when this returns).  On an error nothing stays allocated and both pointers are null.
hipError_t make_lane_tables(const pfb_handle* h, const pfb::FastKernelInfo* f, float** taps_lane, float2** tw_lane) {
  *taps_lane = nullptr;
  *tw_lane = nullptr;
  hipError_t e = hipMalloc((void**)taps_lane, (size_t)f->taps_lane_floats * sizeof(float));
  if (e == hipSuccess) e = hipMalloc((void**)tw_lane, (size_t)f->tw_lane_elems * sizeof(float2));
  if (e == hipSuccess) e = f->init_tables(h->d_taps, h->d_tw, *taps_lane, *tw_lane, nullptr);
  if (e == hipSuccess) e = hipStreamSynchronize(nullptr);
  if (e != hipSuccess) {
    (void)hipFree(*taps_lane);
    (void)hipFree(*tw_lane);
    *taps_lane = nullptr;
    *tw_lane = nullptr;
  }
  return e;
}

// rows [row0, ...) of the handle's output layout: frame-major rows, or an M x ld channel-major matrix
pfb::StageOut layout_out(const pfb_handle* h, void* out, bool device, uint64_t ld, uint64_t row0) {
  return h->layout == PFB_LAYOUT_FRAME_MAJOR ? pfb::StageOut{out, device, 0, row0, 0}
                                             : pfb::StageOut{out, device, ld, row0, h->M};
}

// The timing loop of the two copy yardsticks: scratch of in_bytes (set to 1s) and out_bytes on the current device, one
// warm-up launch, then `iters` launches of launch(in, out) between an event pair.  *bytes_per_sec = the bytes one
// launch moves, times iters, over the elapsed time.
template <class Launch>
int time_copy(const char* what, size_t in_bytes, size_t out_bytes, double bytes_per_launch, int iters, Launch launch,
              double* bytes_per_sec) {
  void *in = nullptr, *out = nullptr;
  hipEvent_t e0 = nullptr, e1 = nullptr;
  int rc = PFB_OK;
  float ms = 0.f;
  hipError_t e = hipMalloc(&in, in_bytes);
  if (e == hipSuccess) e = hipMalloc(&out, out_bytes);
  if (e == hipSuccess) e = hipMemset(in, 1, in_bytes);
  if (e == hipSuccess) e = hipEventCreate(&e0);
  if (e == hipSuccess) e = hipEventCreate(&e1);
  if (e == hipSuccess) e = launch(in, out);  // warm-up
  if (e == hipSuccess) e = hipEventRecord(e0, nullptr);
  for (int i = 0; i < iters && e == hipSuccess; ++i) e = launch(in, out);
  if (e == hipSuccess) e = hipEventRecord(e1, nullptr);
  if (e == hipSuccess) e = hipEventSynchronize(e1);
  if (e == hipSuccess) e = hipEventElapsedTime(&ms, e0, e1);
  if (e != hipSuccess) rc = hip_fail(e, what);
  else *bytes_per_sec = bytes_per_launch * iters / ((double)ms * 1e-3);
  if (e0) (void)hipEventDestroy(e0);
  if (e1) (void)hipEventDestroy(e1);
  (void)hipFree(in);
  (void)hipFree(out);
  return rc;
}

}  // namespace

extern "C" {

int pfb_abi_version(void) { return PFB_ABI_VERSION; }

const char* pfb_last_error_detail(void) { return g_detail.c_str(); }

const char* pfb_strerror(int status) {
  switch (status) {
    case PFB_OK: return "ok";
    case PFB_ERR_BAD_ARG: return "bad argument";
    case PFB_ERR_BAD_FORMAT: return "bad sample or record format";
    case PFB_ERR_UNSUPPORTED: return "unsupported configuration";
    case PFB_ERR_NO_DEVICE: return "no HIP device";
    case PFB_ERR_HIP: return "HIP runtime error";
    case PFB_ERR_NO_MEMORY: return "out of memory";
    case PFB_ERR_CAPACITY: return "output buffer too small";
    case PFB_ERR_INTERNAL: return "internal error (C++ exception stopped at the ABI)";
    case PFB_ERR_COMM: return "halo exchange callback failed";
    default: return "unknown status";
  }
}

int pfb_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) {
    (void)hipGetLastError();
    return 0;
  }
  return n;
}

int pfb_center_frequencies(uint32_t M, double fs, double* out) {
  if (!out || M == 0) return PFB_ERR_BAD_ARG;
  for (uint32_t k = 0; k < M; ++k) {
    const int64_t kk = (k < (M + 1) / 2) ? (int64_t)k : (int64_t)k - (int64_t)M;
    out[k] = (double)kk * fs / (double)M;
  }
  return PFB_OK;
}

int pfb_center_frequencies_ordered(uint32_t M, double fs, uint32_t order, double* out) {
  if (!out || M == 0 || order > PFB_FREQ_ORDER_CENTERED) return PFB_ERR_BAD_ARG;
  if (order == PFB_FREQ_ORDER_FFT) return pfb_center_frequencies(M, fs, out);
  for (uint32_t c = 0; c < M; ++c)  // column c of fftshift(out,2) is FFT column (c + ceil(M/2)) mod M
    out[c] = ((double)c - (double)(M / 2)) * fs / (double)M;
  return PFB_OK;
}

int pfb_selftest_exception_guard(int kind) {
  return pfb::abi_guard([&]() -> int {
    if (kind == 0) throw std::bad_alloc();
    if (kind == 1) throw std::runtime_error("pfb_selftest_exception_guard");
    if (kind == 2) throw 42;
    return PFB_OK;
  });
}

static double bessel_i0(double x) {
  double sum = 1.0, term = 1.0;
  const double q = x * x / 4.0;
  for (int k = 1; k < 200; ++k) {
    term *= q / ((double)k * (double)k);
    sum += term;
    if (term < 1e-17 * sum) break;
  }
  return sum;
}

int pfb_design_prototype(uint32_t M, uint32_t P, double atten_db, float* taps) {
  if (!taps || M == 0 || P == 0) return PFB_ERR_BAD_ARG;
  const double pi = 3.14159265358979323846;
  const int L = (int)(M * P);
  double beta = 0.0;
  if (atten_db > 50.0) beta = 0.1102 * (atten_db - 8.7);
  else if (atten_db >= 21.0) beta = 0.5842 * std::pow(atten_db - 21.0, 0.4) + 0.07886 * (atten_db - 21.0);
  const double i0b = bessel_i0(beta);
  for (int n = 0; n < L; ++n) {
    const double t = ((double)n - (double)L / 2.0) / (double)M;
    const double s = (t == 0.0) ? 1.0 : std::sin(pi * t) / (pi * t);
    const double r = 2.0 * (double)n / (double)L - 1.0;
    const double w = bessel_i0(beta * std::sqrt(std::fmax(0.0, 1.0 - r * r))) / i0b;
    taps[n] = (float)(s / (double)M * w);
  }
  return PFB_OK;
}

int pfb_create(const pfb_config* cfg, pfb_handle** out) {
  return pfb::abi_guard([&]() -> int {
  if (!cfg || !out) return PFB_ERR_BAD_ARG;
  *out = nullptr;
  if (cfg->struct_size != sizeof(pfb_config) || !cfg->taps) return PFB_ERR_BAD_ARG;
  const uint32_t M = cfg->num_channels, P_given = cfg->taps_per_channel;
  const uint32_t D = cfg->decimation ? cfg->decimation : M;
  if (M < 2 || P_given < 1 || D < 1 || D > M) return PFB_ERR_BAD_ARG;
  if (M > 4096 || P_given > 64) return PFB_ERR_UNSUPPORTED;
  // A prototype with fewer taps per channel than a fused shape has is the same filter with zero taps appended
  // (h[n] = 0 for n >= M * P adds exact zeros to every branch sum), so it runs on that shape's kernel -- which is
  // memory-bound anyway -- instead of falling to the generic one.  From here on the handle simply has P taps per
  // channel (history, state blob and halo sizes follow).
  uint32_t P = P_given;
  if (cfg->sample_format <= PFB_FMT_CF32 && !pfb::find_fast_kernel((int)M, (int)P, (int)D, (int)cfg->sample_format)) {
    for (uint32_t p2 = P_given + 1; p2 <= 16; ++p2)
      if (pfb::find_fast_kernel((int)M, (int)p2, (int)D, (int)cfg->sample_format)) { P = p2; break; }
  }
  if (cfg->sample_format > PFB_FMT_CF32) return PFB_ERR_BAD_FORMAT;
  if (cfg->output_layout > PFB_LAYOUT_CHANNEL_MAJOR) return PFB_ERR_BAD_ARG;
  if ((cfg->flags & PFB_FLAG_POWER) && !(cfg->flags & PFB_FLAG_MAGNITUDE)) return PFB_ERR_BAD_ARG;
  int bw = (int)cfg->bit_width;
  if (cfg->sample_format == PFB_FMT_INT8_IQ && (bw < 1 || bw > 8)) return PFB_ERR_BAD_FORMAT;
  if (cfg->sample_format == PFB_FMT_INT16_IQ && (bw < 1 || bw > 16)) return PFB_ERR_BAD_FORMAT;
  if (cfg->sample_format == PFB_FMT_CF32) bw = 1;  // scale 1
  const int off = cfg->input_offset < 0 ? (int)D - 1 : cfg->input_offset;
  if (off >= (int)D) return PFB_ERR_BAD_ARG;

  int dev = 0;
  const int drc = pfb::resolve_device(cfg->device_id, &dev);
  if (drc != PFB_OK) return drc;

  pfb_handle* h = new (std::nothrow) pfb_handle();
  if (!h) return PFB_ERR_NO_MEMORY;
  h->M = (int)M; h->P = (int)P; h->D = (int)D; h->off = off;
  h->fmt = (int)cfg->sample_format; h->bit_width = bw; h->layout = (int)cfg->output_layout;
  h->flags = cfg->flags;
  h->out_elem = (cfg->flags & PFB_FLAG_MAGNITUDE) ? 4 : 8;
  h->device = dev;
  h->bps = pfb::bytes_per_sample(h->fmt);
  h->hist_samples = (int)(M * P + D);
  // (a channel-major handle takes the shape's default plan too: plans without a channel-major instantiation of
  // their own go through frame-major slabs, see pfb_launch_policy.h)
  int row = -1;
  h->fast = pfb::find_fast_kernel(h->M, h->P, h->D, h->fmt, 0, false, &row);
  if (h->fast) (void)pfb_fast_plan_info(row, &h->plan);

  DeviceGuard g(dev);
  {
    int cus = 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && cus > 0) h->num_cus = cus;
    else (void)hipGetLastError();
  }
  const size_t L = (size_t)M * P, L_given = (size_t)M * P_given;
  std::vector<float> taps(L, 0.0f);
  const float scale = std::ldexp(1.0f, -(bw - 1));  // power of two: h*scale is exact
  for (size_t i = 0; i < L_given; ++i) taps[i] = cfg->taps[i] * scale;
  const size_t hist_bytes = (size_t)h->hist_samples * h->bps;
  hipError_t e = hipMalloc((void**)&h->d_taps, L * sizeof(float));
  if (e == hipSuccess) e = pfb::upload_twiddles(M, &h->d_tw);
  if (e == hipSuccess) e = hipMalloc(&h->d_hist[0], hist_bytes);
  if (e == hipSuccess) e = hipMalloc(&h->d_hist[1], hist_bytes);
  if (e == hipSuccess) e = hipMemcpy(h->d_taps, taps.data(), L * sizeof(float), hipMemcpyHostToDevice);
  if (e == hipSuccess && h->fast) e = make_lane_tables(h, h->fast, &h->d_taps_lane, &h->d_tw_lane);
  if (e == hipSuccess) e = hipMemset(h->d_hist[0], 0, hist_bytes);
  if (e == hipSuccess) e = hipMemset(h->d_hist[1], 0, hist_bytes);
  if (e != hipSuccess) {
    const int rc = hip_fail(e, "pfb_create allocation");
    free_handle(h);
    return rc;
  }
  *out = h;
  return PFB_OK;
  });
}

int pfb_destroy(pfb_handle* h) {
  return pfb::abi_guard([&]() -> int {
  if (!h) return PFB_ERR_BAD_ARG;
  free_handle(h);
  return PFB_OK;
  });
}

int pfb_reset(pfb_handle* h) {
  return pfb::abi_guard([&]() -> int {
  if (!h) return PFB_ERR_BAD_ARG;
  DeviceGuard g(h->device);
  const size_t hist_bytes = (size_t)h->hist_samples * h->bps;
  HIP_TRY(hipMemsetAsync(h->d_hist[h->cur], 0, hist_bytes, h->stream));
  h->phase = 0;
  h->frame_index = 0;
  return PFB_OK;
  });
}

int pfb_set_stream(pfb_handle* h, void* hip_stream) {
  return pfb::abi_guard([&]() -> int {
  if (!h) return PFB_ERR_BAD_ARG;
  return pfb::switch_stream(h->device, &h->stream, &h->ev_switch, static_cast<hipStream_t>(hip_stream));
  });
}

int pfb_frames_for(const pfb_handle* h, uint64_t n, uint64_t* frames_out) {
  if (!h || !frames_out) return PFB_ERR_BAD_ARG;
  *frames_out = frames_for(h, n);
  return PFB_OK;
}

int pfb_process_async(pfb_handle* h, const void* d_iq, uint64_t n, void* d_out, uint64_t cap,
                      uint64_t* frames_out) {
  return pfb::abi_guard([&]() -> int {
  if (!h || (n > 0 && !d_iq)) return PFB_ERR_BAD_ARG;
  const uint64_t f = frames_for(h, n);
  if (frames_out) *frames_out = f;
  if (f > cap) return PFB_ERR_CAPACITY;
  if (f > 0 && !d_out) return PFB_ERR_BAD_ARG;
  DeviceGuard g(h->device);
  return enqueue(h, d_iq, n, d_out, f, (int64_t)f, 0);
  });
}

int pfb_sync(pfb_handle* h) {
  return pfb::abi_guard([&]() -> int {
  if (!h) return PFB_ERR_BAD_ARG;
  DeviceGuard g(h->device);
  HIP_TRY(hipStreamSynchronize(h->stream));
  return PFB_OK;
  });
}

int pfb_process(pfb_handle* h, const void* iq, uint64_t n, void* out, uint64_t cap, uint64_t* frames_out,
                uint32_t mem) {
  return pfb::abi_guard([&]() -> int {
  if (!h || (n > 0 && !iq) || mem > PFB_MEM_DEVICE) return PFB_ERR_BAD_ARG;
  const uint64_t f = frames_for(h, n);
  if (frames_out) *frames_out = f;
  if (f > cap) return PFB_ERR_CAPACITY;
  if (f > 0 && !out) return PFB_ERR_BAD_ARG;
  DeviceGuard g(h->device);
  if (mem == PFB_MEM_DEVICE) {
    const int rc = enqueue(h, iq, n, out, f, (int64_t)f, 0);
    if (rc != PFB_OK) return rc;
    HIP_TRY(hipStreamSynchronize(h->stream));
    return PFB_OK;
  }
  return process_host(h, iq, n, layout_out(h, out, false, f, 0));
  });
}

namespace {

// Stream the record's payload through the channelizer: the record reader's two page-locked chunk buffers, one filled
// from the file while the other crosses PCIe and is transformed by the staged host path, which overlaps its own
// copy-in / transform / copy-out underneath.  device_out: `out` is device memory and nothing comes back.
int stream_record(pfb_handle* h, pfb::Record& rec, void* out, uint64_t need, bool device_out, uint64_t* frames_out) {
  const uint64_t chunk = (((uint64_t)1 << 24) / h->D) * h->D;  // whole frames, 64 MB of int16 I/Q
  // four staging steps per chunk, so that the copy-in / transform / copy-out pipeline of the host path has stages
  // to overlap inside each call (measured: 3.3 -> 3.7 GS/s; larger file chunks lose more at the ends than they gain)
  const uint64_t steps = h->opt_host_chunk > 0 ? (uint64_t)h->opt_host_chunk : (uint64_t)1 << 22;
  uint64_t frames_done = 0;
  const int rc = rec.read(chunk, [&](const char* buf, uint64_t, uint64_t m) {
    const uint64_t fr = frames_for(h, m);
    DeviceGuard g(h->device);
    // channel-major: one M x `need` matrix for the whole record, this chunk fills rows frames_done...
    const int r = process_host(h, buf, m, layout_out(h, out, device_out, need, frames_done), steps);
    frames_done += fr;
    return r;
  });
  if (frames_out) *frames_out = frames_done;
  return rc;
}

}  // namespace

int pfb_process_iq_file(pfb_handle* h, const char* path, void* out, uint64_t cap, uint64_t* frames_out,
                        pfb_iq_info* info_out) {
  return pfb::abi_guard([&]() -> int {
  if (!h || !path) return PFB_ERR_BAD_ARG;
  pfb::Record rec;
  const int rc = rec.open(path, h->fmt, h->bit_width);
  if (info_out) *info_out = rec.info;
  if (rc != PFB_OK) return rc;
  const uint64_t need = frames_for(h, rec.info.packet.numSamples);
  if (frames_out) *frames_out = need;
  if (need > cap) return PFB_ERR_CAPACITY;
  if (need > 0 && !out) return PFB_ERR_BAD_ARG;
  return stream_record(h, rec, out, need, false, frames_out);
  });
}

int pfb_pdw_from_iq_file(pfb_handle* h, const char* path, double snr_threshold_db, uint32_t pdw_flags, pfb_pdw* out,
                         uint64_t capacity, uint64_t* count, double* noise_floor_out, pfb_iq_info* info_out) {
  return pfb::abi_guard([&]() -> int {
  if (!h || !path || !count || (capacity > 0 && !out)) return PFB_ERR_BAD_ARG;
  // the PDW stage reads a frame-major complex matrix (mag = abs(iq), phase = angle(iq), :67-68)
  if (h->layout != PFB_LAYOUT_FRAME_MAJOR || (h->flags & PFB_FLAG_MAGNITUDE)) return PFB_ERR_UNSUPPORTED;
  pfb::Record rec;
  int rc = rec.open(path, h->fmt, h->bit_width);
  if (info_out) *info_out = rec.info;
  if (rc != PFB_OK) return rc;
  const pfb_iq_info& info = rec.info;
  const uint64_t need = frames_for(h, info.packet.numSamples);
  const size_t bytes = (size_t)std::max<uint64_t>(need, 1) * h->M * sizeof(float2);
  {
    DeviceGuard g(h->device);
    if (bytes > h->matrix_bytes) {
      if (hipStreamSynchronize(h->stream) != hipSuccess) return PFB_ERR_HIP;
      (void)hipFree(h->d_matrix);
      h->d_matrix = nullptr; h->matrix_bytes = 0;
      if (hipMalloc(&h->d_matrix, bytes) != hipSuccess) { (void)hipGetLastError(); return PFB_ERR_NO_MEMORY; }
      h->matrix_bytes = bytes;
    }
  }
  uint64_t frames = 0;
  rc = stream_record(h, rec, h->d_matrix, need, true, &frames);
  if (rc != PFB_OK) return rc;
  if (frames == 0) {  // a record shorter than one frame holds no pulse
    *count = 0;
    return PFB_OK;
  }
  // the kernels are queued on the handle's stream; the extraction runs behind them on the same stream
  return pfb_pdw_extract(h->d_matrix, frames, (uint32_t)h->M, (uint32_t)h->D, (double)info.packet.sampleRateSps,
                         (double)info.packet.frequencyHz, info.packet.sampleStartTime, snr_threshold_db, pdw_flags, out,
                         capacity, count, noise_floor_out, PFB_MEM_DEVICE, h->device, h->stream);
  });
}

namespace {

// The payload of an open record into a new device buffer, on a new stream: 64 MB chunks through the record reader's
// page-locked buffers.  The caller destroys *st and frees *d_iq whatever comes back.
int record_to_device(pfb::Record& rec, void** d_iq, hipStream_t* st, const char* what) {
  const uint64_t n = rec.info.packet.numSamples;
  const size_t bps = rec.info.bytes_per_sample;
  if (hipMalloc(d_iq, n * bps) != hipSuccess || hipStreamCreate(st) != hipSuccess) {
    (void)hipGetLastError();
    return PFB_ERR_NO_MEMORY;
  }
  return rec.read(((uint64_t)64 << 20) / bps, [&](const char* buf, uint64_t first, uint64_t m) {
    const hipError_t e = hipMemcpyAsync(static_cast<char*>(*d_iq) + first * bps, buf, m * bps, hipMemcpyHostToDevice, *st);
    const hipError_t e2 = hipStreamSynchronize(*st);
    return (e != hipSuccess || e2 != hipSuccess) ? hip_fail(e != hipSuccess ? e : e2, what) : (int)PFB_OK;
  });
}

}  // namespace

int pfb_pdw_raw_from_iq_file(const char* path, double snr_threshold_db, double trailing_threshold_db, pfb_pdw* out,
                             uint64_t capacity, uint64_t* count, double* noise_floor_out, pfb_iq_info* info_out,
                             int32_t device_id) {
  return pfb::abi_guard([&]() -> int {
  if (!path || !count || (capacity > 0 && !out)) return PFB_ERR_BAD_ARG;
  int dev = 0;
  int rc = pfb::resolve_device(device_id, &dev);
  if (rc != PFB_OK) return rc;
  pfb::Record rec;
  rc = rec.open(path);
  if (info_out) *info_out = rec.info;
  if (rc != PFB_OK) return rc;
  const pfb_iq_info& info = rec.info;
  DeviceGuard g(dev);
  const uint64_t n = info.packet.numSamples;
  if (n == 0) return PFB_ERR_BAD_ARG;
  // the record goes to the device; the extraction then runs on the device-resident stream
  void* d_iq = nullptr;
  hipStream_t st = nullptr;
  rc = record_to_device(rec, &d_iq, &st, "pfb_pdw_raw_from_iq_file");
  if (rc == PFB_OK)
    rc = pfb_pdw_extract_raw(d_iq, n, info.sample_format, info.packet.bitWidth, (double)info.packet.sampleRateSps,
                             (double)info.packet.frequencyHz, info.packet.sampleStartTime, snr_threshold_db,
                             trailing_threshold_db, out, capacity, count, noise_floor_out, PFB_MEM_DEVICE, dev, st);
  if (st) (void)hipStreamDestroy(st);
  (void)hipFree(d_iq);
  return rc;
  });
}

int pfb_dwell_from_iq_file(const char* path, const pfb_dwell_config* cfg, pfb_pdw* out, uint64_t capacity, uint64_t* count,
                           pfb_dwell_stats* stats, pfb_iq_info* info_out) {
  return pfb::abi_guard([&]() -> int {
  if (!path || !count || !stats || (capacity > 0 && !out)) return PFB_ERR_BAD_ARG;
  int rc = pfb::dwell_check_config(cfg, true);
  if (rc != PFB_OK) return rc;
  int dev = 0;
  rc = pfb::resolve_device(cfg->device_id, &dev);
  if (rc != PFB_OK) return rc;
  pfb::Record rec;
  rc = rec.open(path);
  if (info_out) *info_out = rec.info;
  if (rc != PFB_OK) return rc;
  const pfb_iq_info& info = rec.info;
  DeviceGuard g(dev);
  const uint64_t n = info.packet.numSamples;
  if (n < 2) return PFB_ERR_BAD_ARG;
  // the payload goes to the device as in pfb_pdw_raw_from_iq_file; the record's header overrides the config
  pfb_dwell_config c = *cfg;
  c.sample_format = info.sample_format;
  c.bit_width = info.packet.bitWidth;
  c.fs = (double)info.packet.sampleRateSps;
  c.fc = (double)info.packet.frequencyHz;
  c.sample_start_time = info.packet.sampleStartTime;
  c.mem = PFB_MEM_DEVICE;
  c.device_id = dev;
  void* d_iq = nullptr;
  hipStream_t st = nullptr;
  rc = record_to_device(rec, &d_iq, &st, "pfb_dwell_from_iq_file");
  if (rc == PFB_OK) rc = pfb_dwell_analyze(&c, d_iq, n, out, capacity, count, stats, st);
  if (st) (void)hipStreamDestroy(st);
  (void)hipFree(d_iq);
  return rc;
  });
}

uint64_t pfb_history_samples(const pfb_handle* h) { return h ? (uint64_t)h->hist_samples : 0; }

int pfb_prime(pfb_handle* h, const void* iq, uint64_t n, uint32_t mem) {
  return pfb::abi_guard([&]() -> int {
  if (!h || (n > 0 && !iq) || mem > PFB_MEM_DEVICE) return PFB_ERR_BAD_ARG;
  if (n == 0) return PFB_OK;
  DeviceGuard g(h->device);
  const uint64_t f = frames_for(h, n);
  // only the trailing hist_samples matter
  const uint64_t keep = std::min<uint64_t>(n, (uint64_t)h->hist_samples);
  const char* tail = static_cast<const char*>(iq) + (n - keep) * h->bps;
  const void* d_tail = tail;
  if (mem == PFB_MEM_HOST) {
    const int rc = h->stage.ensure((size_t)keep * h->bps, 0);
    if (rc != PFB_OK) return rc;
    HIP_TRY(hipMemcpyAsync(h->stage.d_in[0], tail, (size_t)keep * h->bps, hipMemcpyHostToDevice, h->stream));
    d_tail = h->stage.d_in[0];
  }
  HIP_TRY(pfb::launch_update_history(h->d_hist[h->cur], d_tail, (long long)keep, h->d_hist[h->cur ^ 1],
                                     h->hist_samples, h->bps, h->stream));
  h->cur ^= 1;
  h->phase = (uint32_t)((h->phase + n) % (uint64_t)h->D);
  h->frame_index += f;
  if (mem == PFB_MEM_HOST) HIP_TRY(hipStreamSynchronize(h->stream));
  return PFB_OK;
  });
}

uint64_t pfb_halo_samples(const pfb_handle* h) { return h ? (uint64_t)(h->M * h->P - 1 - h->off) : 0; }

uint64_t pfb_shard_head_frames(const pfb_handle* h) {
  return h ? (uint64_t)((h->hist_samples + h->D - 1) / h->D) : 0;
}

void* pfb_halo_recv_buffer(pfb_handle* h) {
  if (!h || !h->d_halo) return nullptr;
  return static_cast<char*>(h->d_halo) + ((size_t)h->hist_samples - (size_t)pfb_halo_samples(h)) * h->bps;
}

int pfb_shard_attach(pfb_handle* h, const pfb_shard_config* cfg) {
  return pfb::abi_guard([&]() -> int {
  if (!h || !cfg || cfg->struct_size != sizeof(pfb_shard_config)) return PFB_ERR_BAD_ARG;
  if (cfg->world < 1 || cfg->rank < 0 || cfg->rank >= cfg->world) return PFB_ERR_BAD_ARG;
  if (cfg->world > 1 && !cfg->exchange) return PFB_ERR_BAD_ARG;
  DeviceGuard g(h->device);
  if (!h->d_halo) {
    // sized like the history so the kernels index it the same way; only its last pfb_halo_samples() are ever read
    const size_t bytes = (size_t)h->hist_samples * h->bps;
    HIP_TRY(hipMalloc(&h->d_halo, bytes));
    HIP_TRY(hipMemset(h->d_halo, 0, bytes));
    HIP_TRY(hipStreamCreateWithFlags(&h->s_halo, hipStreamNonBlocking));
    HIP_TRY(hipEventCreateWithFlags(&h->ev_seg, hipEventDisableTiming));
    HIP_TRY(hipEventCreateWithFlags(&h->ev_halo, hipEventDisableTiming));
  }
  h->shard_rank = cfg->rank;
  h->shard_world = cfg->world;
  h->shard_ring = cfg->ring != 0;
  h->shard_exchange = cfg->exchange;
  h->shard_user = cfg->user;
  return PFB_OK;
  });
}

int pfb_process_shard_async(pfb_handle* h, const void* d_seg, uint64_t n, void* d_out, uint64_t cap, uint64_t* frames_out) {
  return pfb::abi_guard([&]() -> int {
  if (!h || !d_seg) return PFB_ERR_BAD_ARG;
  // a shard is cut on frame boundaries: whole frames in, no carried tail before or after
  if (h->phase != 0 || n % (uint64_t)h->D != 0) return PFB_ERR_BAD_ARG;
  const uint64_t F = n / (uint64_t)h->D, head = pfb_shard_head_frames(h);
  if (frames_out) *frames_out = F;
  // a segment shorter than its head frames has no interior: everything waits for the halo; it must still hold the tail
  // the next shard needs (and the history the handle keeps)
  if (F == 0 || n < (uint64_t)h->hist_samples) return PFB_ERR_BAD_ARG;
  if (F > cap) return PFB_ERR_CAPACITY;
  if (!d_out) return PFB_ERR_BAD_ARG;
  DeviceGuard g(h->device);
  const int world = h->shard_world, rank = h->shard_rank;
  const bool receiving = world > 1 && (h->shard_ring || rank > 0);
  const bool sending = world > 1 && (h->shard_ring || rank + 1 < world);
  const size_t halo_bytes = (size_t)pfb_halo_samples(h) * h->bps;
  if (sending || receiving) {
    // side stream: the exchange starts once everything queued so far on the handle's stream (the caller's writes of
    // the segment, the previous call's head frames that still read the landing zone) has finished
    HIP_TRY(hipEventRecord(h->ev_seg, h->stream));
    HIP_TRY(hipStreamWaitEvent(h->s_halo, h->ev_seg, 0));
    // What I pass on: the tail of THIS segment -- except the last rank of a ring, whose successor (rank 0) works on the
    // NEXT call's first segment: it gets the tail of my PREVIOUS segment, i.e. my carried state (zeros after a reset, so
    // the very first segment of the stream starts from zero state like a fresh dsp.Channelizer).  A matched transport
    // pairs rank 0's receive in call i with my send in call i; sending the current tail there would hand rank 0 samples
    // from its own future.
    const bool pass_state = h->shard_ring && rank == world - 1;
    const char* tail = pass_state
                           ? static_cast<const char*>(h->d_hist[h->cur]) + ((size_t)h->hist_samples * h->bps - halo_bytes)
                           : static_cast<const char*>(d_seg) + (size_t)n * h->bps - halo_bytes;
    const int crc = h->shard_exchange(h->shard_user, sending ? tail : nullptr, receiving ? pfb_halo_recv_buffer(h) : nullptr,
                                      halo_bytes, sending ? (rank + 1) % world : -1,
                                      receiving ? (rank + world - 1) % world : -1, h->s_halo);
    if (crc != 0) {
      char buf[96];
      std::snprintf(buf, sizeof(buf), "halo exchange callback returned %d", crc);
      g_detail = buf;
      return PFB_ERR_COMM;
    }
    HIP_TRY(hipEventRecord(h->ev_halo, h->s_halo));
  }
  // main stream: every frame whose window lies inside the segment starts now ...
  const uint64_t nhead = head < F ? head : F;
  int rc = launch_frames(h, d_seg, n, nullptr, d_out, nhead, F, (int64_t)F, 0);
  if (rc != PFB_OK) return rc;
  // ... the head frames once the halo has landed (a wait on the GPU, not on the host); a shard that receives
  // nothing continues from the handle's own state.  Waiting for the event also puts the SEND in front of
  // whatever the caller queues next on this stream, so pfb_sync() covers both transfers.
  if (sending || receiving) HIP_TRY(hipStreamWaitEvent(h->stream, h->ev_halo, 0));
  rc = launch_frames(h, d_seg, n, receiving ? h->d_halo : h->d_hist[h->cur], d_out, 0, nhead, (int64_t)F, 0);
  if (rc != PFB_OK) return rc;
  return advance_state(h, d_seg, n, F);
  });
}

int pfb_get_state(pfb_handle* h, void* buf, size_t* bytes) {
  return pfb::abi_guard([&]() -> int {
  if (!h || !bytes) return PFB_ERR_BAD_ARG;
  const size_t hist_bytes = (size_t)h->hist_samples * h->bps;
  const size_t need = sizeof(StateHeader) + hist_bytes;
  if (!buf) { *bytes = need; return PFB_OK; }
  if (*bytes < need) { *bytes = need; return PFB_ERR_CAPACITY; }
  DeviceGuard g(h->device);
  StateHeader sh{kStateMagic, (uint32_t)h->M, (uint32_t)h->P, (uint32_t)h->D, (uint32_t)h->fmt,
                 (uint32_t)h->hist_samples, h->phase, 0u, h->frame_index};
  std::memcpy(buf, &sh, sizeof(sh));
  HIP_TRY(hipMemcpyAsync(static_cast<char*>(buf) + sizeof(sh), h->d_hist[h->cur], hist_bytes, hipMemcpyDeviceToHost,
                         h->stream));
  HIP_TRY(hipStreamSynchronize(h->stream));
  *bytes = need;
  return PFB_OK;
  });
}

int pfb_set_state(pfb_handle* h, const void* buf, size_t bytes) {
  return pfb::abi_guard([&]() -> int {
  if (!h || !buf || bytes < sizeof(StateHeader)) return PFB_ERR_BAD_ARG;
  StateHeader sh;
  std::memcpy(&sh, buf, sizeof(sh));
  const size_t hist_bytes = (size_t)h->hist_samples * h->bps;
  if (sh.magic != kStateMagic || sh.M != (uint32_t)h->M || sh.P != (uint32_t)h->P || sh.D != (uint32_t)h->D ||
      sh.fmt != (uint32_t)h->fmt || sh.hist_samples != (uint32_t)h->hist_samples || sh.phase >= (uint32_t)h->D ||
      bytes < sizeof(sh) + hist_bytes)
    return PFB_ERR_BAD_ARG;
  DeviceGuard g(h->device);
  HIP_TRY(hipMemcpyAsync(h->d_hist[h->cur], static_cast<const char*>(buf) + sizeof(sh), hist_bytes,
                         hipMemcpyHostToDevice, h->stream));
  HIP_TRY(hipStreamSynchronize(h->stream));
  h->phase = sh.phase;
  h->frame_index = sh.frame_index;
  return PFB_OK;
  });
}

int pfb_set_frame_index(pfb_handle* h, uint64_t next_frame) {
  if (!h) return PFB_ERR_BAD_ARG;
  h->frame_index = next_frame;
  return PFB_OK;
}

int pfb_get_frame_index(const pfb_handle* h, uint64_t* next_frame) {
  if (!h || !next_frame) return PFB_ERR_BAD_ARG;
  *next_frame = h->frame_index;
  return PFB_OK;
}

int pfb_set_option(pfb_handle* h, int option, int64_t value) {
  return pfb::abi_guard([&]() -> int {
  if (!h) return PFB_ERR_BAD_ARG;
  switch (option) {
    case PFB_OPT_KERNEL:
      if (value < 0 || value > 2) return PFB_ERR_BAD_ARG;
      h->opt_kernel = (int)value;
      return PFB_OK;
    case PFB_OPT_FRAMES_PER_BLOCK:
      if (value < 0 || value > (1 << 24)) return PFB_ERR_BAD_ARG;
      h->opt_frames_per_block = (int)value;
      return PFB_OK;
    case PFB_OPT_HOST_CHUNK_SAMPLES:
      if (value < 0) return PFB_ERR_BAD_ARG;
      h->opt_host_chunk = value;
      return PFB_OK;
    case PFB_OPT_NONTEMPORAL:
      h->opt_nontemporal = value ? 1 : 0;
      return PFB_OK;
    case PFB_OPT_SCHEDULE:
      if (value < -1 || value > 13 || value == 1 || value == 5 || value == 10 || value == 12) return PFB_ERR_BAD_ARG;  // (removed studies)
      h->opt_schedule = (int)value;
      return PFB_OK;
    case PFB_OPT_TILE_WAVES:
      if (value < 1 || value > 16) return PFB_ERR_BAD_ARG;
      h->opt_tile_waves = (int)value;
      return PFB_OK;
    case PFB_OPT_GRID:
      if (value < 0 || value > (1 << 22)) return PFB_ERR_BAD_ARG;
      h->opt_grid = (int)value;
      return PFB_OK;
    case PFB_OPT_XCD_REMAP:
      if (value < -1 || value > (1 << 20)) return PFB_ERR_BAD_ARG;
      h->opt_xcd_remap = (int)value;
      return PFB_OK;
    case PFB_OPT_EXPERIMENT:
      if (value < 0 || value > 0xffff) return PFB_ERR_BAD_ARG;
      h->opt_experiment = (int)value;
      return PFB_OK;
    case PFB_OPT_SLAB_FRAMES:
      if (value < 0 || value > (1ll << 32)) return PFB_ERR_BAD_ARG;
      h->opt_slab_frames = value;
      return PFB_OK;
    case PFB_OPT_VARIANT: {
      if (value < 0 || value > 16) return PFB_ERR_BAD_ARG;
      if ((int)value == h->opt_variant) return PFB_OK;
      int row = -1;
      const pfb::FastKernelInfo* f = pfb::find_fast_kernel(h->M, h->P, h->D, h->fmt, (int)value, false, &row);
      if (!f) return PFB_ERR_UNSUPPORTED;
      DeviceGuard g(h->device);
      HIP_TRY(hipStreamSynchronize(h->stream));  // the old tables may still be in use
      float* tl = nullptr;
      float2* tw = nullptr;
      const hipError_t e = make_lane_tables(h, f, &tl, &tw);
      if (e != hipSuccess) return hip_fail(e, "pfb_set_option(PFB_OPT_VARIANT)");
      (void)hipFree(h->d_taps_lane);
      (void)hipFree(h->d_tw_lane);
      h->d_taps_lane = tl;
      h->d_tw_lane = tw;
      h->fast = f;
      (void)pfb_fast_plan_info(row, &h->plan);
      h->opt_variant = (int)value;
      return PFB_OK;
    }
    case PFB_OPT_PROFILE:
      h->opt_profile = value ? 1 : 0;
      h->ev_used = 0;
      return PFB_OK;
    default:
      return PFB_ERR_BAD_ARG;
  }
  });
}

const char* pfb_last_kernel(const pfb_handle* h) { return h ? h->last_kernel : ""; }

int pfb_last_launch(const pfb_handle* h, pfb_launch_report* out) {
  if (!h || !out) return PFB_ERR_BAD_ARG;
  *out = h->last_launch;
  return PFB_OK;
}

static void export_entry(const pfb::KernelEntry& e, pfb_kernel_entry* out) {
  *out = pfb_kernel_entry{e.schedule, e.threads, e.dyn_lds, 0, (uint64_t)e.blocks, reinterpret_cast<uintptr_t>(e.kernel), e.tag};
}

int pfb_last_entry(const pfb_handle* h, pfb_kernel_entry* out) {
  if (!h || !out) return PFB_ERR_BAD_ARG;
  export_entry(h->last_entry, out);
  return PFB_OK;
}

int pfb_plan_entry(const pfb_entry_request* rq, pfb_kernel_entry* out) {
  pfb_fast_plan_desc plan;
  pfb_launch_report rep;
  if (!rq || !out || rq->struct_size != sizeof(pfb_entry_request) ||
      pfb_fast_plan_info(rq->plan_index, &plan) != PFB_OK || pfb_plan_launch(rq->plan_index, &rq->launch, rq->frames, &rep) != PFB_OK)
    return PFB_ERR_BAD_ARG;
  const pfb::FastKernelInfo* fast = pfb::find_fast_kernel(plan.M, plan.P, plan.D, plan.sample_format, plan.variant);
  if (!fast) return PFB_ERR_INTERNAL;
  pfb::KernelParams p{};  // the fields a select may read, as launch_frames and launch_by_slabs fill them
  p.frames = (long long)(rep.by_slabs ? std::min(rep.slab_frames, rq->frames) : rq->frames);
  p.layout = rq->launch.channel_major && !rep.by_slabs ? PFB_LAYOUT_CHANNEL_MAJOR : PFB_LAYOUT_FRAME_MAJOR;
  p.flags = rq->launch.magnitude ? PFB_FLAG_MAGNITUDE : 0u;
  p.out = reinterpret_cast<float2*>((uintptr_t)(rq->out_aligned16 || rep.by_slabs ? 0 : 8));  // (a slab is a device allocation)
  p.nontemporal = rq->nontemporal ? 1 : 0;
  p.experiment = rq->experiment;
  p.grid_override = rq->grid;
  p.tile_waves = rq->tile_waves;
  apply_policy(p, rep);
  export_entry(fast->select(p), out);
  return PFB_OK;
}

int pfb_plan_launch(int plan_index, const pfb_launch_request* rq, uint64_t frames, pfb_launch_report* out) {
  pfb_fast_plan_desc plan;
  if (!rq || !out || rq->struct_size != sizeof(pfb_launch_request) || pfb_fast_plan_info(plan_index, &plan) != PFB_OK)
    return PFB_ERR_BAD_ARG;
  *out = pfb::plan_launch(plan, pfb::LaunchRequest{rq->schedule, rq->frames_per_block, rq->xcd_remap, rq->slab_frames,
                                                   rq->channel_major, rq->magnitude, rq->num_cus}, frames);
  return PFB_OK;
}

int pfb_get_device(const pfb_handle* h, int* device_id) {
  if (!h || !device_id) return PFB_ERR_BAD_ARG;
  *device_id = h->device;
  return PFB_OK;
}

int pfb_get_kernel_times(pfb_handle* h, float* ms_out, int capacity, int* count) {
  return pfb::abi_guard([&]() -> int {
  if (!h || !count || (capacity > 0 && !ms_out)) return PFB_ERR_BAD_ARG;
  DeviceGuard g(h->device);
  HIP_TRY(hipStreamSynchronize(h->stream));
  int n = 0;
  for (size_t i = 0; i < h->ev_used && n < capacity; ++i, ++n)
    HIP_TRY(hipEventElapsedTime(&ms_out[n], h->ev_pool[i].first, h->ev_pool[i].second));
  h->ev_used = 0;
  *count = n;
  return PFB_OK;
  });
}

void* pfb_host_alloc(size_t bytes) {
  void* p = nullptr;
  if (bytes == 0 || hipHostMalloc(&p, bytes, hipHostMallocDefault) != hipSuccess) {
    (void)hipGetLastError();
    return nullptr;
  }
  return p;
}

void pfb_host_free(void* p) {
  if (p) (void)hipHostFree(p);
}

int pfb_measure_stream_copy(int device_id, uint64_t bytes_in, int iters, double* bytes_per_sec) {
  return pfb::abi_guard([&]() -> int {
  if (!bytes_per_sec || iters < 1 || bytes_in < 512) return PFB_ERR_BAD_ARG;
  int dev = 0;
  const int drc = pfb::resolve_device(device_id, &dev);
  if (drc != PFB_OK) return drc;
  DeviceGuard g(dev);
  const long long nvec = (long long)(bytes_in / 512) * 32;  // whole row pairs (512 bytes of input per wave)
  return time_copy("pfb_measure_stream_copy", (size_t)nvec * 16, (size_t)nvec * 32, (double)nvec * 48.0, iters,
                   [&](void* in, void* out) { return pfb::launch_stream_copy(in, out, nvec, nullptr); }, bytes_per_sec);
  });
}

int pfb_measure_mix_copy(int device_id, uint64_t bytes_in, uint32_t write_ratio, uint32_t rows_per_wave, int iters,
                         double* bytes_per_sec) {
  return pfb::abi_guard([&]() -> int {
  if (!bytes_per_sec || iters < 1 || (write_ratio != 2 && write_ratio != 4) || rows_per_wave < 2 || (rows_per_wave & 1))
    return PFB_ERR_BAD_ARG;
  int dev = 0;
  const int drc = pfb::resolve_device(device_id, &dev);
  if (drc != PFB_OK) return drc;
  DeviceGuard g(dev);
  const long long rows = (long long)(bytes_in / 256) / (4ll * rows_per_wave) * (4ll * rows_per_wave);  // whole workgroups
  if (rows <= 0) return PFB_ERR_BAD_ARG;
  return time_copy("pfb_measure_mix_copy", (size_t)rows * 256, (size_t)rows * 256 * write_ratio,
                   (double)rows * 256.0 * (1.0 + write_ratio), iters, [&](void* in, void* out) {
                     return pfb::launch_mix_copy(in, out, rows, (int)write_ratio, (int)rows_per_wave, nullptr);
                   }, bytes_per_sec);
  });
}

}  // extern "C"
