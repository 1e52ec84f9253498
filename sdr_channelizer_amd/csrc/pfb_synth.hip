// pfb_synth.hip -- the pulse-train source (pfb_synth_* in include/pfb_channelizer.h): what the host derives from a
// configuration, the kernel that turns a global sample index into a value, and the record writer.  Restates
// /root/reference/matlab/generate_pulsed_iq.m:27-77 and /root/reference/matlab/generate_training_iq.m:34-62,95-127 as
// the counter-based integer stream of sdr_channelizer_amd/synth.py (_counter_stream): the definition is in the header.
//
// Against the float64 scripts the phase of an ON sample is off by at most 3.4e-6 rad (the 32-bit fcw); the 16-bit table
// index, 9.6e-5 rad, is the resolution that matters.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <functional>
#include <new>
#include <string>
#include <vector>

#include "pfb_common.h"
#include "pfb_host.h"

namespace {

constexpr int kFx = 20;                      // fractional bits of the fixed-point sum
constexpr uint32_t kTabSize = 1u << 16;
constexpr uint32_t kBarkerPlus = 0x159F;     // bit c set: chip c of + + + + + - - + + - + - + adds +offset
constexpr uint32_t kSynthFlags =
    PFB_SYNTH_BARKER13 | PFB_SYNTH_BARKER_DEGREES | PFB_SYNTH_PHASE_FROM_ZERO | PFB_SYNTH_ROUND_MATLAB;
constexpr int kThreads = 256;
constexpr uint64_t kHostChunk = (uint64_t)1 << 22;  // samples per page-locked chunk of the host and record paths

// Kernel-side view of one pfb_synth_generate call.  Sample j of the call is stream sample start + j; for j >= pre its
// index inside the period is (kbase + j) mod pri, and samples j < pre lie before the first pulse.
struct SynthParams {
  void* out;
  const int64_t* tab;
  uint64_t start, n, pre, record, dcw;
  int64_t gain;
  uint32_t kbase, pw, pri, chip, fcw, boff, seed, flags;
  uint32_t head;      // samples before the first 16-byte boundary of `out` (at most n)
  int bit_width;
};

__device__ __forceinline__ uint32_t mix32(uint32_t x) {
  x ^= x >> 16;
  x *= 0x7FEB352Du;
  x ^= x >> 15;
  x *= 0x846CA68Bu;
  return x ^ (x >> 16);
}

__device__ __forceinline__ int32_t noise_of(uint32_t base, uint32_t lane_const) {
  const uint32_t a = mix32(base ^ lane_const);
  const uint32_t b = mix32(a ^ 0x5BD1E995u);
  return (int32_t)((a & 0xFFFFu) + (a >> 16) + (b & 0xFFFFu) + (b >> 16)) - 2 * 65535;
}

// (I, Q) of call sample j, whose index inside the period is k, in 2^-20 LSB fixed point
__device__ __forceinline__ void synth_value(const SynthParams& p, uint64_t j, uint32_t k, int64_t& vi, int64_t& vq) {
  const uint64_t i = p.start + j;
  const uint32_t base = (uint32_t)i ^ ((uint32_t)(i >> 32) * 0x9E3779B1u) ^ p.seed;
  vi = (int64_t)noise_of(base, 0x68E31DA4u) * p.gain;
  vq = (int64_t)noise_of(base, 0x68E31DA4u * 3u) * p.gain;
  bool on = j >= p.pre && k < p.pw;
  if (on && p.record) {  // only pulses that fit the record: s + 1 + pw < record
    const uint64_t s = i - k;
    on = s < p.record && p.record - s > (uint64_t)p.pw + 1;
  }
  if (on) {  // off samples never touch the table
    uint32_t ph = ((p.flags & PFB_SYNTH_PHASE_FROM_ZERO) ? k : k + 1) * p.fcw;
    if (p.dcw) ph += (uint32_t)((((uint64_t)k * (k + 1) / 2) * p.dcw) >> 32);
    if (p.chip) {
      const uint32_t c = k / p.chip;  // k < pw = 13 chip here; the clamp is the definition's
      ph += ((kBarkerPlus >> (c < 12u ? c : 12u)) & 1u) ? p.boff : 0u - p.boff;
    }
    const uint32_t ci = ph >> 16, si = (ci - 16384u) & 65535u;
    vi += p.tab[ci];
    vq += p.tab[si];
  }
}

__device__ __forceinline__ int32_t quantize(const SynthParams& p, int64_t v) {
  const int64_t half = (int64_t)1 << (kFx - 1), full = (int64_t)1 << (p.bit_width - 1);
  const int64_t r = ((p.flags & PFB_SYNTH_ROUND_MATLAB) && v < 0) ? -((-v + half) >> kFx) : (v + half) >> kFx;
  return (int32_t)(r < -full ? -full : (r > full - 1 ? full - 1 : r));
}

template <int FMT> struct Pack;
template <> struct Pack<PFB_FMT_INT16_IQ> {
  using word_t = uint32_t;  // one sample
  static __device__ __forceinline__ word_t make(const SynthParams& p, int64_t vi, int64_t vq) {
    return ((uint32_t)quantize(p, vi) & 0xFFFFu) | ((uint32_t)quantize(p, vq) << 16);
  }
};
template <> struct Pack<PFB_FMT_INT8_IQ> {
  using word_t = uint16_t;
  static __device__ __forceinline__ word_t make(const SynthParams& p, int64_t vi, int64_t vq) {
    return (uint16_t)(((uint32_t)quantize(p, vi) & 0xFFu) | (((uint32_t)quantize(p, vq) & 0xFFu) << 8));
  }
};
template <> struct Pack<PFB_FMT_CF32> {
  using word_t = float2;
  static __device__ __forceinline__ word_t make(const SynthParams& p, int64_t vi, int64_t vq) {
    const double scale = __longlong_as_double((long long)(1023 - (kFx + p.bit_width - 1)) << 52);  // 2^-(20+bw-1)
    return make_float2((float)((double)vi * scale), (float)((double)vq * scale));
  }
};

// One 16-byte store per lane and step over the aligned body (S samples), a grid-stride loop; the up to S-1 samples in
// front of the first 16-byte boundary and the up to S-1 behind the last whole vector go out one by one from the first
// lanes of the grid.  A lane derives its k with one 64-bit remainder and then only compares and subtracts.
template <int FMT>
__global__ __launch_bounds__(kThreads) void synth_kernel(const SynthParams p) {
  using word_t = typename Pack<FMT>::word_t;
  constexpr int S = 16 / (int)sizeof(word_t);
  struct alignas(16) Vec { word_t w[S]; };
  word_t* out = static_cast<word_t*>(p.out);
  const uint64_t nvec = (p.n - p.head) / S;
  const uint64_t tid = (uint64_t)blockIdx.x * kThreads + threadIdx.x, stride = (uint64_t)gridDim.x * kThreads;
  if (tid < nvec) {
    uint64_t j = p.head + tid * S;
    uint32_t k = (uint32_t)((p.kbase + j) % p.pri);
    const uint32_t kstep = (uint32_t)((stride * S) % p.pri);
    for (uint64_t v = tid; v < nvec; v += stride) {
      Vec vec;
      uint32_t kk = k;
#pragma unroll
      for (int e = 0; e < S; ++e) {
        int64_t vi, vq;
        synth_value(p, j + e, kk, vi, vq);
        vec.w[e] = Pack<FMT>::make(p, vi, vq);
        if (++kk == p.pri) kk = 0;
      }
      *reinterpret_cast<Vec*>(out + j) = vec;
      j += stride * S;
      k += kstep;
      if (k >= p.pri) k -= p.pri;
    }
  }
  const uint64_t tail0 = p.head + nvec * S;
  if (tid < p.head + (p.n - tail0)) {
    const uint64_t j = tid < p.head ? tid : tail0 + (tid - p.head);
    int64_t vi, vq;
    synth_value(p, j, (uint32_t)((p.kbase + j) % p.pri), vi, vq);
    out[j] = Pack<FMT>::make(p, vi, vq);
  }
}

// What a configuration derives (the header's table); the checks every entry point makes before the device is touched.
struct Derived {
  pfb_synth_params q{};
  uint32_t pri = 0;
};

int synth_derive(const pfb_synth_config* cfg, Derived* d, int64_t* table_out) {
  if (!cfg || cfg->struct_size != sizeof(pfb_synth_config)) return PFB_ERR_BAD_ARG;
  for (const double v : {cfg->fs, cfg->f0, cfg->lfm_extent_hz, cfg->amplitude, cfg->noise_sigma})
    if (!std::isfinite(v)) return PFB_ERR_BAD_ARG;
  if (cfg->fs <= 0 || cfg->amplitude < 0 || cfg->amplitude > 2 || cfg->noise_sigma < 0 || cfg->noise_sigma > 1)
    return PFB_ERR_BAD_ARG;
  if ((cfg->flags & ~kSynthFlags) || ((cfg->flags & PFB_SYNTH_BARKER_DEGREES) && !(cfg->flags & PFB_SYNTH_BARKER13)))
    return PFB_ERR_BAD_ARG;
  const uint64_t pri = cfg->period_samples;
  uint64_t pw = cfg->pulse_samples, chip = 0;
  if (pw < 1 || pw > pri || pri >= ((uint64_t)1 << 31)) return PFB_ERR_BAD_ARG;
  if (cfg->flags & PFB_SYNTH_BARKER13) {  // "Pulse width adjusted", generate_pulsed_iq.m:33-40
    chip = (uint64_t)std::max<long long>(std::llrint((double)pw / 13.0), 1);
    pw = 13 * chip;
    if (pw > pri) return PFB_ERR_BAD_ARG;
  }
  const double turns = cfg->f0 / cfg->fs, dturns = pw > 1 ? (cfg->lfm_extent_hz / (double)(pw - 1)) / cfg->fs : 0.0;
  if (!(std::fabs(turns) <= 1048576.0) || !(std::fabs(dturns) < 0.5)) return PFB_ERR_BAD_ARG;
  if (cfg->sample_format > PFB_FMT_CF32) return PFB_ERR_BAD_FORMAT;
  const uint32_t bw = cfg->bit_width;
  if (bw < 2 || bw > (cfg->sample_format == PFB_FMT_INT8_IQ ? 8u : 16u)) return PFB_ERR_BAD_FORMAT;

  const double full = std::ldexp(1.0, (int)bw - 1), fx = (double)(1 << kFx);
  d->pri = (uint32_t)pri;
  d->q.pulse_samples = (uint32_t)pw;
  d->q.chip_samples = (uint32_t)chip;
  d->q.fcw = (uint32_t)(uint64_t)std::llrint(turns * 4294967296.0);
  d->q.dcw = (uint64_t)std::llrint(std::ldexp(dturns, 64));
  d->q.noise_gain = std::llrint(cfg->noise_sigma * full * fx / std::sqrt(4.0 * (65536.0 * 65536.0 - 1.0) / 12.0));
  d->q.barker_offset = 0;
  if (chip) {
    // the script adds +-90 to a phase in radians (generate_pulsed_iq.m:50-58,61): 90/(2 pi) turns, less the whole ones
    const double two_pi = 2.0 * 3.141592653589793;
    d->q.barker_offset = (cfg->flags & PFB_SYNTH_BARKER_DEGREES)
                             ? (1u << 30)
                             : (uint32_t)std::llrint(std::fmod(90.0 / two_pi, 1.0) * 4294967296.0);
  }
  if (table_out) {
    const double two_pi = 2.0 * 3.141592653589793;
    for (uint32_t j = 0; j < kTabSize; ++j)
      table_out[j] = std::llrint(cfg->amplitude * full * fx * std::cos(two_pi * (double)j / (double)kTabSize));
  }
  return PFB_OK;
}

}  // namespace

struct pfb_synth_handle {
  pfb_synth_config cfg{};
  Derived d;
  int device = 0;
  int bps = 0;              // bytes per sample
  int max_blocks = 0;       // the grid's cap: 8 workgroups per CU
  int64_t* d_tab = nullptr;
  hipStream_t stream = nullptr;
  hipEvent_t ev_switch = nullptr;
  // host and record paths: two device chunks, two page-locked chunks, one event each (made at the first such call)
  void* d_chunk[2] = {nullptr, nullptr};
  void* h_chunk[2] = {nullptr, nullptr};
  hipEvent_t ev_chunk[2] = {nullptr, nullptr};
};

namespace {

void free_synth(pfb_synth_handle* h) {
  if (!h) return;
  pfb::DeviceGuard g(h->device);
  (void)hipFree(h->d_tab);
  for (int b = 0; b < 2; ++b) {
    (void)hipFree(h->d_chunk[b]);
    if (h->h_chunk[b]) (void)hipHostFree(h->h_chunk[b]);
    if (h->ev_chunk[b]) (void)hipEventDestroy(h->ev_chunk[b]);
  }
  if (h->ev_switch) (void)hipEventDestroy(h->ev_switch);
  delete h;
}

// null handle, overflowing range, null or misaligned output: before anything touches the device
int check_range(const pfb_synth_handle* h, uint64_t start, uint64_t n, const void* out) {
  if (!h || start + n < start || n > ((uint64_t)1 << 62) || (n > 0 && !out)) return PFB_ERR_BAD_ARG;
  if (reinterpret_cast<uintptr_t>(out) % (uintptr_t)h->bps) return PFB_ERR_BAD_ARG;
  return PFB_OK;
}

// one kernel on the handle's stream: samples [start, start + n) into device memory at d_out
int synth_enqueue(pfb_synth_handle* h, uint64_t start, uint64_t n, void* d_out) {
  if (n == 0) return PFB_OK;
  const pfb_synth_config& c = h->cfg;
  SynthParams p{};
  p.out = d_out;
  p.tab = h->d_tab;
  p.start = start;
  p.n = n;
  p.record = c.record_samples;
  p.dcw = h->d.q.dcw;
  p.gain = h->d.q.noise_gain;
  p.pw = h->d.q.pulse_samples;
  p.pri = h->d.pri;
  p.chip = h->d.q.chip_samples;
  p.fcw = h->d.q.fcw;
  p.boff = h->d.q.barker_offset;
  p.seed = c.seed;
  p.flags = c.flags;
  p.bit_width = (int)c.bit_width;
  if (start >= c.first_pulse) {
    p.pre = 0;
    p.kbase = (uint32_t)((start - c.first_pulse) % p.pri);
  } else {  // sample j = pre is the first pulse's first: k = 0 there
    p.pre = c.first_pulse - start;
    p.kbase = (uint32_t)((p.pri - p.pre % p.pri) % p.pri);
  }
  const uint64_t to_boundary = ((16 - reinterpret_cast<uintptr_t>(d_out) % 16) % 16) / (uint64_t)h->bps;
  p.head = (uint32_t)std::min<uint64_t>(to_boundary, n);
  const uint64_t per_vec = 16 / (uint64_t)h->bps, nvec = (n - p.head) / per_vec;
  const uint64_t want = std::max<uint64_t>((nvec + kThreads - 1) / kThreads, 1);  // the scalar lanes need one workgroup
  const dim3 grid((unsigned)std::min<uint64_t>(want, (uint64_t)h->max_blocks));
  switch (c.sample_format) {
    case PFB_FMT_INT8_IQ: hipLaunchKernelGGL(synth_kernel<PFB_FMT_INT8_IQ>, grid, dim3(kThreads), 0, h->stream, p); break;
    case PFB_FMT_INT16_IQ: hipLaunchKernelGGL(synth_kernel<PFB_FMT_INT16_IQ>, grid, dim3(kThreads), 0, h->stream, p); break;
    default: hipLaunchKernelGGL(synth_kernel<PFB_FMT_CF32>, grid, dim3(kThreads), 0, h->stream, p); break;
  }
  HIP_TRY(hipGetLastError());
  return PFB_OK;
}

// Samples [start, start + n) to the host in chunks: chunk c + 1 is generated and copied into its page-locked buffer
// while sink() consumes chunk c.  Returns with nothing left in flight.
int synth_to_host(pfb_synth_handle* h, uint64_t start, uint64_t n,
                  const std::function<int(const char* buf, size_t bytes)>& sink) {
  if (n == 0) return PFB_OK;
  const size_t chunk_bytes = (size_t)kHostChunk * h->bps;
  for (int b = 0; b < 2; ++b) {
    if (!h->d_chunk[b]) HIP_TRY(hipMalloc(&h->d_chunk[b], chunk_bytes));
    if (!h->h_chunk[b]) HIP_TRY(hipHostMalloc(&h->h_chunk[b], chunk_bytes, hipHostMallocDefault));
    if (!h->ev_chunk[b]) HIP_TRY(hipEventCreateWithFlags(&h->ev_chunk[b], hipEventDisableTiming));
  }
  const uint64_t chunks = (n + kHostChunk - 1) / kHostChunk;
  const auto issue = [&](uint64_t c) -> int {
    const int b = (int)(c & 1);
    const uint64_t m = std::min<uint64_t>(kHostChunk, n - c * kHostChunk);
    const int rc = synth_enqueue(h, start + c * kHostChunk, m, h->d_chunk[b]);
    if (rc != PFB_OK) return rc;
    HIP_TRY(hipMemcpyAsync(h->h_chunk[b], h->d_chunk[b], (size_t)m * h->bps, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipEventRecord(h->ev_chunk[b], h->stream));
    return PFB_OK;
  };
  int rc = issue(0);
  for (uint64_t c = 0; c < chunks && rc == PFB_OK; ++c) {
    if (c + 1 < chunks) rc = issue(c + 1);
    if (rc != PFB_OK) break;
    const int b = (int)(c & 1);
    const hipError_t e = hipEventSynchronize(h->ev_chunk[b]);
    if (e != hipSuccess) { rc = pfb::hip_fail(e, "hipEventSynchronize"); break; }
    rc = sink(static_cast<const char*>(h->h_chunk[b]), (size_t)std::min<uint64_t>(kHostChunk, n - c * kHostChunk) * h->bps);
  }
  if (rc != PFB_OK) (void)hipStreamSynchronize(h->stream);
  return rc;
}

}  // namespace

extern "C" int pfb_synth_describe(const pfb_synth_config* cfg, pfb_synth_params* out, int64_t* table_out) {
  return pfb::abi_guard([&]() -> int {
    if (!out) return PFB_ERR_BAD_ARG;
    Derived d;
    const int rc = synth_derive(cfg, &d, table_out);
    if (rc == PFB_OK) *out = d.q;
    return rc;
  });
}

extern "C" int pfb_synth_create(const pfb_synth_config* cfg, pfb_synth_handle** out) {
  return pfb::abi_guard([&]() -> int {
    if (!out) return PFB_ERR_BAD_ARG;
    *out = nullptr;
    std::vector<int64_t> tab(kTabSize);
    Derived d;
    int rc = synth_derive(cfg, &d, tab.data());
    if (rc != PFB_OK) return rc;
    int dev = 0;
    rc = pfb::resolve_device(cfg->device_id, &dev);
    if (rc != PFB_OK) return rc;
    pfb_synth_handle* h = new pfb_synth_handle();
    h->cfg = *cfg;
    h->d = d;
    h->device = dev;
    h->bps = pfb::bytes_per_sample((int)cfg->sample_format);
    pfb::DeviceGuard g(dev);
    int cus = 0;
    hipError_t e = hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
    h->max_blocks = 8 * std::max(cus, 1);
    if (e == hipSuccess) e = hipMalloc((void**)&h->d_tab, kTabSize * sizeof(int64_t));
    if (e == hipSuccess) e = hipMemcpy(h->d_tab, tab.data(), kTabSize * sizeof(int64_t), hipMemcpyHostToDevice);
    if (e != hipSuccess) {
      rc = pfb::hip_fail(e, "pfb_synth_create allocation");
      free_synth(h);
      return rc;
    }
    *out = h;
    return PFB_OK;
  });
}

extern "C" int pfb_synth_destroy(pfb_synth_handle* h) {
  return pfb::abi_guard([&]() -> int {
    if (!h) return PFB_ERR_BAD_ARG;
    free_synth(h);
    return PFB_OK;
  });
}

extern "C" int pfb_synth_set_stream(pfb_synth_handle* h, void* hip_stream) {
  return pfb::abi_guard([&]() -> int {
    if (!h) return PFB_ERR_BAD_ARG;
    return pfb::switch_stream(h->device, &h->stream, &h->ev_switch, static_cast<hipStream_t>(hip_stream));
  });
}

extern "C" int pfb_synth_generate_async(pfb_synth_handle* h, uint64_t start, uint64_t num_samples, void* d_out) {
  return pfb::abi_guard([&]() -> int {
    const int rc = check_range(h, start, num_samples, d_out);
    if (rc != PFB_OK) return rc;
    pfb::DeviceGuard g(h->device);
    return synth_enqueue(h, start, num_samples, d_out);
  });
}

extern "C" int pfb_synth_generate(pfb_synth_handle* h, uint64_t start, uint64_t num_samples, void* out, uint32_t mem) {
  return pfb::abi_guard([&]() -> int {
    int rc = check_range(h, start, num_samples, out);
    if (rc != PFB_OK || mem > PFB_MEM_DEVICE) return PFB_ERR_BAD_ARG;
    pfb::DeviceGuard g(h->device);
    if (mem == PFB_MEM_DEVICE) {
      rc = synth_enqueue(h, start, num_samples, out);
      if (rc != PFB_OK) return rc;
      HIP_TRY(hipStreamSynchronize(h->stream));
      return PFB_OK;
    }
    char* dst = static_cast<char*>(out);
    return synth_to_host(h, start, num_samples, [&](const char* buf, size_t bytes) {
      std::memcpy(dst, buf, bytes);
      dst += bytes;
      return (int)PFB_OK;
    });
  });
}

extern "C" int pfb_synth_sync(pfb_synth_handle* h) {
  return pfb::abi_guard([&]() -> int {
    if (!h) return PFB_ERR_BAD_ARG;
    pfb::DeviceGuard g(h->device);
    HIP_TRY(hipStreamSynchronize(h->stream));
    return PFB_OK;
  });
}

extern "C" int pfb_synth_get_device(const pfb_synth_handle* h, int* device_id) {
  return pfb::abi_guard([&]() -> int {
    if (!h || !device_id) return PFB_ERR_BAD_ARG;
    *device_id = h->device;
    return PFB_OK;
  });
}

extern "C" int pfb_synth_write_iq_file(pfb_synth_handle* h, const char* path, int file_format, uint64_t start,
                                       uint32_t num_samples, const pfb_iq_packet* header_fields) {
  return pfb::abi_guard([&]() -> int {
    if (!h || !path || (file_format != 1 && file_format != 3) || start + num_samples < start) return PFB_ERR_BAD_ARG;
    const pfb_synth_config& c = h->cfg;
    if (c.fs > 4294967295.0) return PFB_ERR_BAD_ARG;  // sampleRateSps is a uint32
    // the record formats hold int8 / int16 pairs; generate_training_iq.m:97-98,125 writes int16 only
    if (c.sample_format == PFB_FMT_CF32 || (file_format == 1 && c.sample_format != PFB_FMT_INT16_IQ))
      return PFB_ERR_BAD_FORMAT;
    pfb_iq_packet pk;
    if (header_fields) {
      pk = *header_fields;
    } else {  // generate_training_iq.m:109-123
      pfb_iq_fill_packet(&pk, 0, 0, (uint32_t)c.fs, (uint32_t)c.fs, 0.0f, 0, 0, "simulated", nullptr, 0.0);
      pk.linkSpeed = file_format == 1 ? 1 : 0;
    }
    pk.endianness = file_format == 1 ? PFB_IQ_MARKER_FMT1 : PFB_IQ_MARKER_FMT3;
    pk.numSamples = num_samples;
    pk.bitWidth = c.bit_width;
    unsigned char head[PFB_IQ_HEADER_BYTES];
    size_t head_bytes = 0;
    int rc = pfb_iq_serialize_header(&pk, file_format, head, sizeof(head), &head_bytes);
    if (rc != PFB_OK) return rc;
    std::FILE* f = std::fopen(path, "wb");
    if (!f) { pfb::g_detail = std::string("cannot create ") + path; return PFB_ERR_BAD_ARG; }
    bool wrote = std::fwrite(head, 1, head_bytes, f) == head_bytes;
    if (wrote) {
      pfb::DeviceGuard g(h->device);
      rc = synth_to_host(h, start, num_samples, [&](const char* buf, size_t bytes) {
        wrote = std::fwrite(buf, 1, bytes, f) == bytes;
        return wrote ? (int)PFB_OK : (int)PFB_ERR_INTERNAL;
      });
    }
    wrote = (std::fclose(f) == 0) && wrote;
    if (!wrote) { pfb::g_detail = std::string("short write to ") + path; return PFB_ERR_INTERNAL; }
    return rc;
  });
}
