// pfb_trace.hip -- magnitude / phase traces and plot envelopes of an I/Q stream (pfb_trace_* in
// include/pfb_channelizer.h, where the arithmetic is defined): the arithmetic of the reference's plotters,
// matlab/plot_my_iq.m:105-111 (iq/2^(bitWidth-1), abs, rad2deg(angle)), as one read of the stream.
//
// Envelope: the call's samples are cut at every bin boundary and at every multiple of kTile samples from a bin's
// start, so that each segment lies in one bin; the grid follows from (samples, bin length, samples the open bin already
// holds) alone.
//   bins shorter than kGroupBins   a group of 1..64 lanes per bin, a wave on 64 .. 1 consecutive bins (env_group_kernel)
//   bins up to kTile               one workgroup per bin: one segment (env_segment_kernel writes the record itself)
//   longer bins                    one workgroup per segment writes a partial to the handle's scratch; env_fold_kernel,
//                                  one wave per bin, folds the bin's partials
// A bin that a call leaves open lives in a device-side carry record (two, written in turn: the bin that reads the old
// one and the bin that writes the new one may be different workgroups); the host keeps only the stream position.
// Everything a fold combines is associative and commutative -- min, the lexicographic (largest power, lowest index)
// and, for the integer formats, a uint64 sum -- so the records do not depend on how the stream is cut; cf32 sums its
// doubles in the fixed order of the grid.  No atomics anywhere.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <new>

#include "pfb_common.h"
#include "pfb_host.h"

namespace {

constexpr int kThreads = 256;
constexpr uint32_t kTile = 4096;         // samples per segment (sdr_channelizer_amd/trace.py: TILE)
constexpr uint32_t kLaneSamples = 16;    // env_group_kernel: a lane takes at most this many samples of its bin
constexpr uint32_t kGroupBins = 64 * kLaneSamples;  // bins shorter than this go to lane groups
constexpr uint64_t kMaxBin = (uint64_t)1 << 31;
constexpr unsigned kMaxGrid = 1u << 22;  // longer calls: every workgroup takes several segments / bins
constexpr uint32_t kNone = 0xFFFFFFFFu;
constexpr uint64_t kStageBytes = (uint64_t)64 << 20;  // per side of the host staging

static_assert(sizeof(pfb_trace_bin) == 48, "the record of include/pfb_channelizer.h");

// A bin's figures over some of its samples, as they travel between kernels and calls.  pmin, pmax and sum hold a uint64
// (integer formats: I^2 + Q^2 and its sum) or the bits of a double (cf32).  count == 0: no sample yet.
struct Part {
  uint64_t peak_sample;
  uint64_t pmin, pmax, sum;
  float peak_i, peak_q;
  uint32_t count, pad;
};

template <int FMT>
struct Pow {  // integer formats
  using raw_t = typename pfb::SampleT<FMT>::raw_t;
  using pow_t = uint32_t;  // up to 2^31: (-32768, -32768)
  using sum_t = uint64_t;
  static __device__ __forceinline__ pow_t power(raw_t v) {
    int i, q;
    comps(v, i, q);
    return (uint32_t)(i * i) + (uint32_t)(q * q);
  }
  static __device__ __forceinline__ void comps(raw_t v, int& i, int& q) {
    if constexpr (FMT == PFB_FMT_INT8_IQ) {
      i = (int)(int8_t)(v & 0xffu);
      q = (int)(int8_t)(v >> 8);
    } else {
      i = (int)(int16_t)(v & 0xffffu);
      q = (int32_t)v >> 16;
    }
  }
  static __device__ __forceinline__ pow_t pow_top() { return 0xFFFFFFFFu; }
  static __device__ __forceinline__ uint64_t bits(uint64_t v) { return v; }
  static __device__ __forceinline__ uint64_t unbits(uint64_t v) { return v; }
  static __device__ __forceinline__ void peak(raw_t v, int bit_width, float& pi, float& pq) {
    int i, q;
    comps(v, i, q);
    const float s = __uint_as_float((uint32_t)(127 - (bit_width - 1)) << 23);  // 2^-(bit_width-1): the products are exact
    pi = (float)i * s;
    pq = (float)q * s;
  }
};
template <>
struct Pow<PFB_FMT_CF32> {
  using raw_t = float2;
  using pow_t = double;
  using sum_t = double;
  static __device__ __forceinline__ pow_t power(raw_t v) {
    return (double)v.x * (double)v.x + (double)v.y * (double)v.y;  // exact products: contraction changes nothing
  }
  static __device__ __forceinline__ pow_t pow_top() { return __longlong_as_double(0x7FF0000000000000ll); }
  static __device__ __forceinline__ uint64_t bits(double v) { return (uint64_t)__double_as_longlong(v); }
  static __device__ __forceinline__ double unbits(uint64_t v) { return __longlong_as_double((long long)v); }
  static __device__ __forceinline__ void peak(raw_t v, int, float& pi, float& pq) {
    pi = v.x;
    pq = v.y;
  }
};

// What one lane gathers.  idx: the sample's offset from the start of the lane's segment, kNone before the first sample;
// a lane visits its samples in rising order, so the strict comparison keeps the first of equal powers.
template <int FMT>
struct Acc {
  using P = Pow<FMT>;
  typename P::pow_t pmin, pmax;
  typename P::sum_t sum;
  uint32_t idx;
  static __device__ __forceinline__ Acc empty() {
    Acc a;
    a.pmin = P::pow_top();
    a.pmax = 0;
    a.sum = 0;
    a.idx = kNone;
    return a;
  }
  __device__ __forceinline__ void add(typename P::raw_t v, uint32_t off) {
    const typename P::pow_t p = P::power(v);
    sum += p;
    pmin = p < pmin ? p : pmin;
    if (p > pmax || idx == kNone) {
      pmax = p;
      idx = off;
    }
  }
  __device__ __forceinline__ void merge(const Acc& b) {  // an empty b (power 0, kNone) never wins
    sum += b.sum;
    pmin = b.pmin < pmin ? b.pmin : pmin;
    if (b.pmax > pmax || (b.pmax == pmax && b.idx < idx)) {
      pmax = b.pmax;
      idx = b.idx;
    }
  }
  __device__ __forceinline__ Acc lane_xor(int mask) const {
    Acc b;
    b.pmin = __shfl_xor(pmin, mask);
    b.pmax = __shfl_xor(pmax, mask);
    b.sum = __shfl_xor(sum, mask);
    b.idx = __shfl_xor(idx, mask);
    return b;
  }
};

template <int FMT>
__device__ __forceinline__ void merge_part(Part& a, const Part& b) {  // global sample indices: any order of folding
  using P = Pow<FMT>;
  if (b.count == 0) return;
  if (a.count == 0) {
    a = b;
    return;
  }
  const auto amin = P::unbits(a.pmin), bmin = P::unbits(b.pmin), amax = P::unbits(a.pmax), bmax = P::unbits(b.pmax);
  a.sum = P::bits(P::unbits(a.sum) + P::unbits(b.sum));
  if (bmin < amin) a.pmin = b.pmin;
  if (bmax > amax || (bmax == amax && b.peak_sample < a.peak_sample)) {
    a.pmax = b.pmax;
    a.peak_sample = b.peak_sample;
    a.peak_i = b.peak_i;
    a.peak_q = b.peak_q;
  }
  a.count += b.count;
}

// The record of a bin whose samples are all in `p`; the one place where integers become doubles.  Runs on the device
// for the bins a call completes and on the host for the bin pfb_trace_flush returns: IEEE conversions, one division and
// multiplications by a power of two give the same bits on both.
__host__ __device__ inline pfb_trace_bin finish_bin(const Part& p, int fmt, int bit_width) {
  pfb_trace_bin r;
  r.peak_sample = p.peak_sample;
  if (fmt == PFB_FMT_CF32) {
    double lo, hi, s;
    memcpy(&lo, &p.pmin, 8);
    memcpy(&hi, &p.pmax, 8);
    memcpy(&s, &p.sum, 8);
    r.power_min = lo;
    r.power_max = hi;
    r.power_mean = s / (double)p.count;
  } else {
    const uint64_t sbits = (uint64_t)(1023 - 2 * (bit_width - 1)) << 52;  // 2^-(2(bit_width-1))
    double scale;
    memcpy(&scale, &sbits, 8);
    r.power_min = (double)p.pmin * scale;
    r.power_max = (double)p.pmax * scale;
    r.power_mean = ((double)p.sum / (double)p.count) * scale;
  }
  r.peak_i = p.peak_i;
  r.peak_q = p.peak_q;
  r.count = p.count;
  r.reserved = 0;
  return r;
}

// Kernel-side view of one envelope call.  "Grid position" g counts from the first sample of the bin that was open when
// the call began: call sample j sits at g = open + j, in local bin g / bin at offset g % bin.
struct EnvParams {
  const void* in;
  uint64_t n;            // samples of this call (> 0)
  uint64_t pos;          // global index of in[0]
  uint64_t bin;          // B
  uint64_t open;         // samples of local bin 0 that earlier calls took (< B); they are in *carry_in
  uint64_t bins;         // local bins the call touches
  uint64_t segs;         // segments of the call (bins of kGroupBins samples and more)
  uint32_t seg_per_bin;  // ceil(B / kTile)
  uint32_t seg0;         // index inside local bin 0 of the call's first segment: open / kTile
  const Part* carry_in;
  Part* carry_out;
  Part* parts;           // one per segment when seg_per_bin > 1
  pfb_trace_bin* out;    // one per completed local bin
  int bit_width;
  int group;             // env_group_kernel: lanes per bin
};

// thread 0 / the group's first lane: the bin's share of this call is in `mine`
template <int FMT>
__device__ __forceinline__ void close_or_carry(const EnvParams& p, uint64_t b, Part mine) {
  if (b == 0 && p.open > 0) {
    Part all = *p.carry_in;
    merge_part<FMT>(all, mine);
    mine = all;
  }
  if ((b + 1) * p.bin <= p.open + p.n)
    p.out[b] = finish_bin(mine, FMT, p.bit_width);
  else
    *p.carry_out = mine;
}

template <int FMT>
__device__ __forceinline__ Part part_of(const EnvParams& p, const Acc<FMT>& a, uint64_t j0, uint32_t count) {
  using P = Pow<FMT>;
  Part r;
  r.pmin = P::bits(a.pmin);
  r.pmax = P::bits(a.pmax);
  r.sum = P::bits(a.sum);
  r.peak_sample = p.pos + j0 + a.idx;
  r.peak_i = r.peak_q = 0.0f;
  // the peak's components: one more read of a sample of this segment (idx can be kNone only next to NaNs)
  if (a.idx < count) P::peak(static_cast<const typename P::raw_t*>(p.in)[j0 + a.idx], p.bit_width, r.peak_i, r.peak_q);
  r.count = count;
  r.pad = 0;
  return r;
}

// Bins of fewer than kGroupBins samples: `group` lanes (a power of two, at least B / 16) share a bin, lane r of the
// group takes the bin's samples r, r + group, ... of this call, so a wave reads one contiguous stretch per step; the
// group's lanes meet by xor shuffles.  One sample per load: a bin's edges fall anywhere inside a 16-byte vector.
template <int FMT>
__global__ __launch_bounds__(kThreads) void env_group_kernel(const EnvParams p) {
  using P = Pow<FMT>;
  const typename P::raw_t* in = static_cast<const typename P::raw_t*>(p.in);
  const uint32_t G = (uint32_t)p.group, per_block = kThreads / G;
  const uint32_t r = threadIdx.x % G;
  const uint64_t end = p.open + p.n;
  // the loop's bounds are the same for every lane of a wave: all of them reach the shuffles
  for (uint64_t b0 = (uint64_t)blockIdx.x * per_block; b0 < p.bins; b0 += (uint64_t)gridDim.x * per_block) {
    const uint64_t b = b0 + threadIdx.x / G;
    Acc<FMT> acc = Acc<FMT>::empty();
    uint64_t j0 = 0;
    uint32_t count = 0;
    if (b < p.bins) {
      const uint64_t g0 = std::max<uint64_t>(b * p.bin, p.open), g1 = std::min<uint64_t>((b + 1) * p.bin, end);
      j0 = g0 - p.open;
      count = (uint32_t)(g1 - g0);
      for (uint32_t o = r; o < count; o += G) acc.add(in[j0 + o], o);
    }
    for (uint32_t m = G >> 1; m > 0; m >>= 1) acc.merge(acc.lane_xor((int)m));
    if (r == 0 && b < p.bins) close_or_carry<FMT>(p, b, part_of<FMT>(p, acc, j0, count));
  }
}

// One workgroup per segment [j0, j0 + len) of the call: the samples before the first 16-byte boundary and behind the
// last whole vector one by one from the first lanes, the body by one 16-byte load per lane and step.
template <int FMT>
__global__ __launch_bounds__(kThreads) void env_segment_kernel(const EnvParams p) {
  using P = Pow<FMT>;
  using raw_t = typename P::raw_t;
  constexpr uint32_t S = 16 / (uint32_t)sizeof(raw_t);
  struct alignas(16) Vec { raw_t w[S]; };
  __shared__ Acc<FMT> s_acc[kThreads / 64];
  const raw_t* in = static_cast<const raw_t*>(p.in);
  const uint32_t t = threadIdx.x;
  const uint64_t end = p.open + p.n;
  for (uint64_t q = blockIdx.x; q < p.segs; q += gridDim.x) {
    const uint64_t qq = q + p.seg0, b = qq / p.seg_per_bin, s = qq % p.seg_per_bin;
    const uint64_t g0 = std::max<uint64_t>(b * p.bin + s * kTile, p.open);
    const uint64_t g1 = std::min<uint64_t>(b * p.bin + std::min<uint64_t>((s + 1) * (uint64_t)kTile, p.bin), end);
    const uint64_t j0 = g0 - p.open;
    const uint32_t len = (uint32_t)(g1 - g0);  // 1 .. kTile
    const raw_t* seg = in + j0;
    const uint32_t to_boundary = (uint32_t)(((16 - reinterpret_cast<uintptr_t>(seg) % 16) % 16) / sizeof(raw_t));
    const uint32_t head = to_boundary < len ? to_boundary : len;
    const uint32_t nvec = (len - head) / S, tail0 = head + nvec * S;
    Acc<FMT> acc = Acc<FMT>::empty();
    if (t < head) acc.add(seg[t], t);
    for (uint32_t v = t; v < nvec; v += kThreads) {
      const uint32_t o = head + v * S;
      const Vec vec = *reinterpret_cast<const Vec*>(seg + o);
#pragma unroll
      for (uint32_t e = 0; e < S; ++e) acc.add(vec.w[e], o + e);
    }
    if (t < len - tail0) acc.add(seg[tail0 + t], tail0 + t);
#pragma unroll
    for (int m = 32; m > 0; m >>= 1) acc.merge(acc.lane_xor(m));
    if (t % 64 == 0) s_acc[t / 64] = acc;
    __syncthreads();
    if (t == 0) {
      for (int w = 1; w < kThreads / 64; ++w) acc.merge(s_acc[w]);
      const Part mine = part_of<FMT>(p, acc, j0, len);
      if (p.seg_per_bin == 1)
        close_or_carry<FMT>(p, b, mine);
      else
        p.parts[q] = mine;
    }
    __syncthreads();  // s_acc is free for the next segment
  }
}

// Bins longer than kTile: one wave per local bin folds its segments' partials, lane l those at l, l + 64, ...
template <int FMT>
__global__ __launch_bounds__(64) void env_fold_kernel(const EnvParams p) {
  using P = Pow<FMT>;
  for (uint64_t b = blockIdx.x; b < p.bins; b += gridDim.x) {
    const uint64_t lo = std::max<uint64_t>(b * p.seg_per_bin, p.seg0) - p.seg0;
    const uint64_t hi = std::min<uint64_t>((b + 1) * (uint64_t)p.seg_per_bin - p.seg0, p.segs);
    Part a{};
    for (uint64_t q = lo + threadIdx.x; q < hi; q += 64) merge_part<FMT>(a, p.parts[q]);
#pragma unroll
    for (int m = 32; m > 0; m >>= 1) {
      Part o;
      o.peak_sample = __shfl_xor((unsigned long long)a.peak_sample, m);
      o.pmin = __shfl_xor((unsigned long long)a.pmin, m);
      o.pmax = __shfl_xor((unsigned long long)a.pmax, m);
      o.sum = __shfl_xor((unsigned long long)a.sum, m);
      o.peak_i = __shfl_xor(a.peak_i, m);
      o.peak_q = __shfl_xor(a.peak_q, m);
      o.count = __shfl_xor(a.count, m);
      o.pad = 0;
      // cf32: both lanes of a pair must add in the same order to hold the same sum
      if (threadIdx.x & (unsigned)m) {
        merge_part<FMT>(o, a);
        a = o;
      } else {
        merge_part<FMT>(a, o);
      }
    }
    if (threadIdx.x == 0) close_or_carry<FMT>(p, b, a);
  }
}

// Full-rate trace: mag = sqrt(power), phase = atan2(Q, I) in degrees, float32.  The input as in synth_kernel: scalar
// head, 16-byte body, scalar tail, grid-stride.  A lane's S results go out as whole vectors where the output pointer
// allows it, else one by one.
struct SampleParams {
  const void* in;
  float* mag;     // may be null
  float* phase;   // may be null
  uint64_t n;
  uint32_t head;  // samples before the first 16-byte boundary of `in` (at most n)
  int mag_vec, phase_vec;  // out + head is 16-byte aligned
  int bit_width;
};

template <int FMT>
__device__ __forceinline__ void mag_phase(typename Pow<FMT>::raw_t v, int bit_width, float& mag, float& phase) {
  constexpr float kDeg = 57.29577951308232f;
  if constexpr (FMT == PFB_FMT_CF32) {
    mag = (float)sqrt(Pow<FMT>::power(v));
    phase = atan2f(v.y, v.x) * kDeg;
  } else {
    int i, q;
    Pow<FMT>::comps(v, i, q);
    const float s = __uint_as_float((uint32_t)(127 - (bit_width - 1)) << 23);
    mag = sqrtf((float)Pow<FMT>::power(v)) * s;
    phase = atan2f((float)q, (float)i) * kDeg;
  }
}

template <int S>
__device__ __forceinline__ void store_run(float* dst, const float (&v)[S], bool vec) {
  if (vec) {
    if constexpr (S == 2) {
      *reinterpret_cast<float2*>(dst) = make_float2(v[0], v[1]);
    } else {
#pragma unroll
      for (int e = 0; e < S; e += 4) *reinterpret_cast<float4*>(dst + e) = make_float4(v[e], v[e + 1], v[e + 2], v[e + 3]);
    }
  } else {
#pragma unroll
    for (int e = 0; e < S; ++e) dst[e] = v[e];
  }
}

template <int FMT>
__global__ __launch_bounds__(kThreads) void trace_samples_kernel(const SampleParams p) {
  using raw_t = typename Pow<FMT>::raw_t;
  constexpr int S = 16 / (int)sizeof(raw_t);
  struct alignas(16) Vec { raw_t w[S]; };
  const raw_t* in = static_cast<const raw_t*>(p.in);
  const uint64_t nvec = (p.n - p.head) / S;
  const uint64_t tid = (uint64_t)blockIdx.x * kThreads + threadIdx.x, stride = (uint64_t)gridDim.x * kThreads;
  for (uint64_t v = tid; v < nvec; v += stride) {
    const uint64_t j = p.head + v * S;
    const Vec vec = *reinterpret_cast<const Vec*>(in + j);
    float m[S], ph[S];
#pragma unroll
    for (int e = 0; e < S; ++e) mag_phase<FMT>(vec.w[e], p.bit_width, m[e], ph[e]);
    if (p.mag) store_run<S>(p.mag + j, m, p.mag_vec != 0);
    if (p.phase) store_run<S>(p.phase + j, ph, p.phase_vec != 0);
  }
  const uint64_t tail0 = p.head + nvec * S;
  if (tid < p.head + (p.n - tail0)) {
    const uint64_t j = tid < p.head ? tid : tail0 + (tid - p.head);
    float m, ph;
    mag_phase<FMT>(in[j], p.bit_width, m, ph);
    if (p.mag) p.mag[j] = m;
    if (p.phase) p.phase[j] = ph;
  }
}

}  // namespace

struct pfb_trace_handle {
  int fmt = 0, bit_width = 0;
  uint64_t bin = 1;
  int device = 0;
  int bps = 0;              // bytes per sample
  int max_blocks = 0;       // pfb_trace_samples' grid cap: 8 workgroups per CU
  uint64_t pos = 0;         // samples since create / reset: the global index of the next one
  uint64_t grid0 = 0;       // where the bin grid starts: 0, or the position of the last flush
  Part* d_carry = nullptr;  // two records; [cur] holds the open bin when (pos - grid0) % bin > 0
  int cur = 0;
  Part* d_parts = nullptr;  // segment partials of the call in flight (grow-only)
  uint64_t parts_cap = 0;
  hipStream_t stream = nullptr;
  hipEvent_t ev_switch = nullptr;
  pfb::HostStage stage;     // host path
};

namespace {

void free_trace(pfb_trace_handle* h) {
  if (!h) return;
  pfb::DeviceGuard g(h->device);
  (void)hipFree(h->d_carry);
  (void)hipFree(h->d_parts);
  h->stage.release();
  if (h->ev_switch) (void)hipEventDestroy(h->ev_switch);
  delete h;
}

int check_config(const pfb_trace_config* cfg) {
  if (!cfg || cfg->struct_size != sizeof(pfb_trace_config)) return PFB_ERR_BAD_ARG;
  if (cfg->bin_samples < 1 || (uint64_t)cfg->bin_samples > kMaxBin || cfg->flags != 0) return PFB_ERR_BAD_ARG;
  if (cfg->sample_format > PFB_FMT_CF32) return PFB_ERR_BAD_FORMAT;
  const uint32_t bw = cfg->bit_width;
  if (cfg->sample_format == PFB_FMT_INT8_IQ && (bw < 1 || bw > 8)) return PFB_ERR_BAD_FORMAT;
  if (cfg->sample_format == PFB_FMT_INT16_IQ && (bw < 1 || bw > 16)) return PFB_ERR_BAD_FORMAT;
  return PFB_OK;
}

int create_trace(const pfb_trace_config* cfg, pfb_trace_handle** out) {
  int rc = check_config(cfg);
  if (rc != PFB_OK) return rc;
  int dev = 0;
  rc = pfb::resolve_device(cfg->device_id, &dev);
  if (rc != PFB_OK) return rc;
  pfb_trace_handle* h = new pfb_trace_handle();
  h->fmt = (int)cfg->sample_format;
  h->bit_width = h->fmt == PFB_FMT_CF32 ? 1 : (int)cfg->bit_width;
  h->bin = cfg->bin_samples;
  h->device = dev;
  h->bps = pfb::bytes_per_sample(h->fmt);
  pfb::DeviceGuard g(dev);
  int cus = 0;
  hipError_t e = hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
  h->max_blocks = 8 * std::max(cus, 1);
  if (e == hipSuccess) e = hipMalloc((void**)&h->d_carry, 2 * sizeof(Part));
  if (e == hipSuccess) e = hipMemset(h->d_carry, 0, 2 * sizeof(Part));
  if (e != hipSuccess) {
    rc = pfb::hip_fail(e, "pfb_trace_create allocation");
    free_trace(h);
    return rc;
  }
  *out = h;
  return PFB_OK;
}

uint64_t open_samples(const pfb_trace_handle* h) { return (h->pos - h->grid0) % h->bin; }
uint64_t bins_for(const pfb_trace_handle* h, uint64_t n) { return (open_samples(h) + n) / h->bin; }

#define PFB_TRACE_LAUNCH(kernel, fmt, grid, block, stream, params)                                            \
  switch (fmt) {                                                                                              \
    case PFB_FMT_INT8_IQ: hipLaunchKernelGGL(kernel<PFB_FMT_INT8_IQ>, grid, block, 0, stream, params); break;   \
    case PFB_FMT_INT16_IQ: hipLaunchKernelGGL(kernel<PFB_FMT_INT16_IQ>, grid, block, 0, stream, params); break; \
    default: hipLaunchKernelGGL(kernel<PFB_FMT_CF32>, grid, block, 0, stream, params); break;                   \
  }

// the kernels of one call and the position update, on the handle's stream; bins_for(n) records land at d_out
int envelope_enqueue(pfb_trace_handle* h, const void* d_in, uint64_t n, pfb_trace_bin* d_out) {
  if (n == 0) return PFB_OK;
  const uint64_t B = h->bin;
  EnvParams p{};
  p.in = d_in;
  p.n = n;
  p.pos = h->pos;
  p.bin = B;
  p.open = open_samples(h);
  p.bins = (p.open + n + B - 1) / B;
  p.carry_in = h->d_carry + h->cur;
  p.carry_out = h->d_carry + (h->cur ^ 1);
  p.out = d_out;
  p.bit_width = h->bit_width;
  if (B < kGroupBins) {
    uint32_t G = 1;
    while ((uint64_t)G * kLaneSamples < B) G <<= 1;  // at most 64
    p.group = (int)G;
    const uint64_t per_block = kThreads / G, want = (p.bins + per_block - 1) / per_block;
    const dim3 grid((unsigned)std::min<uint64_t>(want, kMaxGrid));
    PFB_TRACE_LAUNCH(env_group_kernel, h->fmt, grid, dim3(kThreads), h->stream, p);
    HIP_TRY(hipGetLastError());
  } else {
    p.seg_per_bin = (uint32_t)((B + kTile - 1) / kTile);
    p.seg0 = (uint32_t)(p.open / kTile);
    const uint64_t last = p.open + n - 1;
    p.segs = (last / B) * p.seg_per_bin + (last % B) / kTile + 1 - p.seg0;
    if (p.seg_per_bin > 1) {
      if (p.segs > h->parts_cap) {  // frees only after the device has drained: earlier calls are done with the old one
        (void)hipFree(h->d_parts);
        h->d_parts = nullptr;
        h->parts_cap = 0;
        HIP_TRY(hipMalloc((void**)&h->d_parts, p.segs * sizeof(Part)));
        h->parts_cap = p.segs;
      }
      p.parts = h->d_parts;
    }
    const dim3 grid((unsigned)std::min<uint64_t>(p.segs, kMaxGrid));
    PFB_TRACE_LAUNCH(env_segment_kernel, h->fmt, grid, dim3(kThreads), h->stream, p);
    HIP_TRY(hipGetLastError());
    if (p.seg_per_bin > 1) {
      const dim3 fgrid((unsigned)std::min<uint64_t>(p.bins, kMaxGrid));
      PFB_TRACE_LAUNCH(env_fold_kernel, h->fmt, fgrid, dim3(64), h->stream, p);
      HIP_TRY(hipGetLastError());
    }
  }
  h->pos += n;
  if (open_samples(h) > 0) h->cur ^= 1;  // the call wrote the other carry record
  return PFB_OK;
}

// what every envelope call checks before the device is touched; *f = the bins it completes
int check_envelope(const pfb_trace_handle* h, const void* iq, uint64_t n, const void* out, uint64_t cap,
                   uint64_t* bins_out, bool device, uint64_t* f) {
  if (!h || (n > 0 && !iq) || n > ((uint64_t)1 << 62) || h->pos + n < h->pos) return PFB_ERR_BAD_ARG;
  *f = bins_for(h, n);
  if (bins_out) *bins_out = *f;
  if (*f > cap) return PFB_ERR_CAPACITY;
  if (*f > 0 && !out) return PFB_ERR_BAD_ARG;
  if ((device && reinterpret_cast<uintptr_t>(iq) % (uintptr_t)h->bps) || reinterpret_cast<uintptr_t>(out) % 8)
    return PFB_ERR_BAD_ARG;
  return PFB_OK;
}

// Host buffers through the staged pipeline: a "frame" is one record, a step at most 64 MiB on either side.  Any cut
// of the stream gives the same records (cf32: the same but for the last bits of power_mean).
int envelope_host(pfb_trace_handle* h, const void* iq, uint64_t n, void* out, uint64_t limit = UINT64_MAX) {
  if (n == 0) return PFB_OK;
  uint64_t chunk = std::min<uint64_t>(limit, kStageBytes / (uint64_t)h->bps);
  chunk = std::min<uint64_t>(chunk, (kStageBytes / sizeof(pfb_trace_bin)) * h->bin);
  const pfb::StageSteps steps{
      chunk, (h->bin - 1 + chunk) / h->bin, (size_t)h->bps, sizeof(pfb_trace_bin),
      [h](uint64_t m) { return bins_for(h, m); },
      [h](const void* d_in, uint64_t m, void* d_out, uint64_t, int64_t, int64_t) {
        return envelope_enqueue(h, d_in, m, static_cast<pfb_trace_bin*>(d_out));
      }};
  return pfb::stage_host(h->stage, h->stream, steps, iq, n, pfb::StageOut{out});
}

int samples_enqueue(pfb_trace_handle* h, const void* d_in, uint64_t n, float* d_mag, float* d_phase) {
  if (n == 0 || (!d_mag && !d_phase)) return PFB_OK;
  SampleParams p{};
  p.in = d_in;
  p.mag = d_mag;
  p.phase = d_phase;
  p.n = n;
  p.bit_width = h->bit_width;
  const uint64_t to_boundary = ((16 - reinterpret_cast<uintptr_t>(d_in) % 16) % 16) / (uint64_t)h->bps;
  p.head = (uint32_t)std::min<uint64_t>(to_boundary, n);
  p.mag_vec = (reinterpret_cast<uintptr_t>(d_mag) + 4 * (uintptr_t)p.head) % 16 == 0;
  p.phase_vec = (reinterpret_cast<uintptr_t>(d_phase) + 4 * (uintptr_t)p.head) % 16 == 0;
  const uint64_t per_vec = 16 / (uint64_t)h->bps, nvec = (n - p.head) / per_vec;
  const uint64_t want = std::max<uint64_t>((nvec + kThreads - 1) / kThreads, 1);  // the scalar lanes need one workgroup
  const dim3 grid((unsigned)std::min<uint64_t>(want, (uint64_t)h->max_blocks));
  PFB_TRACE_LAUNCH(trace_samples_kernel, h->fmt, grid, dim3(kThreads), h->stream, p);
  HIP_TRY(hipGetLastError());
  return PFB_OK;
}

// one of the two traces of n host samples into host memory, through the same staging: a "frame" is one float
int samples_host(pfb_trace_handle* h, const void* iq, uint64_t n, float* out, bool phase) {
  const uint64_t chunk = kStageBytes / (uint64_t)std::max(h->bps, 4);
  const pfb::StageSteps steps{
      chunk, chunk, (size_t)h->bps, sizeof(float), [](uint64_t m) { return m; },
      [h, phase](const void* d_in, uint64_t m, void* d_out, uint64_t, int64_t, int64_t) {
        float* o = static_cast<float*>(d_out);
        return samples_enqueue(h, d_in, m, phase ? nullptr : o, phase ? o : nullptr);
      }};
  return pfb::stage_host(h->stage, h->stream, steps, iq, n, pfb::StageOut{out});
}

}  // namespace

extern "C" int pfb_trace_create(const pfb_trace_config* cfg, pfb_trace_handle** out) {
  return pfb::abi_guard([&]() -> int {
    if (!out) return PFB_ERR_BAD_ARG;
    *out = nullptr;
    return create_trace(cfg, out);
  });
}

extern "C" int pfb_trace_destroy(pfb_trace_handle* h) {
  return pfb::abi_guard([&]() -> int {
    if (!h) return PFB_ERR_BAD_ARG;
    free_trace(h);
    return PFB_OK;
  });
}

extern "C" int pfb_trace_reset(pfb_trace_handle* h) {
  return pfb::abi_guard([&]() -> int {
    if (!h) return PFB_ERR_BAD_ARG;
    h->pos = h->grid0 = 0;  // no open bin: the carry record is never read again
    return PFB_OK;
  });
}

extern "C" int pfb_trace_set_stream(pfb_trace_handle* h, void* hip_stream) {
  return pfb::abi_guard([&]() -> int {
    if (!h) return PFB_ERR_BAD_ARG;
    return pfb::switch_stream(h->device, &h->stream, &h->ev_switch, static_cast<hipStream_t>(hip_stream));
  });
}

extern "C" int pfb_trace_sync(pfb_trace_handle* h) {
  return pfb::abi_guard([&]() -> int {
    if (!h) return PFB_ERR_BAD_ARG;
    pfb::DeviceGuard g(h->device);
    HIP_TRY(hipStreamSynchronize(h->stream));
    return PFB_OK;
  });
}

extern "C" int pfb_trace_get_device(const pfb_trace_handle* h, int* device_id) {
  return pfb::abi_guard([&]() -> int {
    if (!h || !device_id) return PFB_ERR_BAD_ARG;
    *device_id = h->device;
    return PFB_OK;
  });
}

extern "C" int pfb_trace_bins_for(const pfb_trace_handle* h, uint64_t num_samples, uint64_t* bins_out) {
  return pfb::abi_guard([&]() -> int {
    if (!h || !bins_out || num_samples > ((uint64_t)1 << 62)) return PFB_ERR_BAD_ARG;
    *bins_out = bins_for(h, num_samples);
    return PFB_OK;
  });
}

extern "C" int pfb_trace_envelope_async(pfb_trace_handle* h, const void* d_iq, uint64_t num_samples, pfb_trace_bin* d_out,
                                        uint64_t capacity_bins, uint64_t* bins_out) {
  return pfb::abi_guard([&]() -> int {
    uint64_t f = 0;
    const int rc = check_envelope(h, d_iq, num_samples, d_out, capacity_bins, bins_out, true, &f);
    if (rc != PFB_OK) return rc;
    pfb::DeviceGuard g(h->device);
    return envelope_enqueue(h, d_iq, num_samples, d_out);
  });
}

extern "C" int pfb_trace_envelope(pfb_trace_handle* h, const void* iq, uint64_t num_samples, pfb_trace_bin* out,
                                  uint64_t capacity_bins, uint64_t* bins_out, uint32_t mem) {
  return pfb::abi_guard([&]() -> int {
    if (mem > PFB_MEM_DEVICE) return PFB_ERR_BAD_ARG;
    uint64_t f = 0;
    int rc = check_envelope(h, iq, num_samples, out, capacity_bins, bins_out, mem == PFB_MEM_DEVICE, &f);
    if (rc != PFB_OK) return rc;
    pfb::DeviceGuard g(h->device);
    if (mem == PFB_MEM_HOST) return envelope_host(h, iq, num_samples, out);
    rc = envelope_enqueue(h, iq, num_samples, out);
    if (rc != PFB_OK) return rc;
    HIP_TRY(hipStreamSynchronize(h->stream));
    return PFB_OK;
  });
}

extern "C" int pfb_trace_flush(pfb_trace_handle* h, pfb_trace_bin* out_host, int32_t* have) {
  return pfb::abi_guard([&]() -> int {
    if (!h || !out_host || !have) return PFB_ERR_BAD_ARG;
    *have = 0;
    if (open_samples(h) > 0) {
      pfb::DeviceGuard g(h->device);
      Part open;
      HIP_TRY(hipMemcpyAsync(&open, h->d_carry + h->cur, sizeof(Part), hipMemcpyDeviceToHost, h->stream));
      HIP_TRY(hipStreamSynchronize(h->stream));
      *out_host = finish_bin(open, h->fmt, h->bit_width);
      *have = 1;
    }
    h->grid0 = h->pos;  // the next sample starts a bin
    return PFB_OK;
  });
}

extern "C" int pfb_trace_samples(pfb_trace_handle* h, const void* iq, uint64_t num_samples, float* mag, float* phase_deg,
                                 uint32_t mem) {
  return pfb::abi_guard([&]() -> int {
    if (!h || (num_samples > 0 && !iq) || num_samples > ((uint64_t)1 << 62) || mem > PFB_MEM_DEVICE) return PFB_ERR_BAD_ARG;
    if (reinterpret_cast<uintptr_t>(mag) % 4 || reinterpret_cast<uintptr_t>(phase_deg) % 4) return PFB_ERR_BAD_ARG;
    if (mem == PFB_MEM_DEVICE && reinterpret_cast<uintptr_t>(iq) % (uintptr_t)h->bps) return PFB_ERR_BAD_ARG;
    if (num_samples == 0 || (!mag && !phase_deg)) return PFB_OK;
    pfb::DeviceGuard g(h->device);
    if (mem == PFB_MEM_DEVICE) {
      const int rc = samples_enqueue(h, iq, num_samples, mag, phase_deg);
      if (rc != PFB_OK) return rc;
      HIP_TRY(hipStreamSynchronize(h->stream));
      return PFB_OK;
    }
    // one pass of the staging per trace asked for
    int rc = mag ? samples_host(h, iq, num_samples, mag, false) : (int)PFB_OK;
    if (rc == PFB_OK && phase_deg) rc = samples_host(h, iq, num_samples, phase_deg, true);
    return rc;
  });
}

extern "C" int pfb_trace_choose_bin(uint64_t num_samples, uint32_t max_bins, uint32_t* bin_samples) {
  return pfb::abi_guard([&]() -> int {
    if (!bin_samples || max_bins == 0) return PFB_ERR_BAD_ARG;
    const uint64_t b = std::max<uint64_t>(1, num_samples / max_bins + (num_samples % max_bins != 0));
    if (b > kMaxBin) return PFB_ERR_BAD_ARG;
    // 2^31 itself fits the uint32 of pfb_trace_config
    *bin_samples = (uint32_t)b;
    return PFB_OK;
  });
}

extern "C" int pfb_trace_envelope_from_iq_file(const char* path, uint32_t max_bins, pfb_trace_bin* out,
                                               uint64_t capacity_bins, uint64_t* bins_out, uint32_t* bin_samples_out,
                                               pfb_iq_info* info_out, int32_t device_id) {
  return pfb::abi_guard([&]() -> int {
    if (!path || !bins_out || !bin_samples_out || max_bins == 0 || (capacity_bins > 0 && !out) ||
        reinterpret_cast<uintptr_t>(out) % 8)
      return PFB_ERR_BAD_ARG;
    int dev = 0;
    int rc = pfb::resolve_device(device_id, &dev);
    if (rc != PFB_OK) return rc;
    pfb::Record rec;
    rc = rec.open(path);
    if (info_out) *info_out = rec.info;
    if (rc != PFB_OK) return rc;
    const uint64_t n = rec.info.packet.numSamples;
    pfb_trace_config cfg{};
    cfg.struct_size = sizeof(cfg);
    cfg.sample_format = rec.info.sample_format;
    cfg.bit_width = rec.info.packet.bitWidth;
    cfg.device_id = dev;
    rc = pfb_trace_choose_bin(n, max_bins, &cfg.bin_samples);
    if (rc != PFB_OK) return rc;
    *bin_samples_out = cfg.bin_samples;
    const uint64_t need = (n + cfg.bin_samples - 1) / cfg.bin_samples;  // the final partial bin included
    *bins_out = need;
    if (need > capacity_bins) return PFB_ERR_CAPACITY;
    pfb_trace_handle* h = nullptr;
    rc = create_trace(&cfg, &h);
    if (rc != PFB_OK) return rc;
    // the payload in record chunks of 2^24 samples, each staged in steps of at most 2^22 (pfb_stft_process_iq_file)
    uint64_t done = 0;
    rc = rec.read((uint64_t)1 << 24, [&](const char* buf, uint64_t, uint64_t m) {
      const uint64_t f = bins_for(h, m);
      pfb::DeviceGuard g(h->device);
      const int r = envelope_host(h, buf, m, out + done, (uint64_t)1 << 22);
      done += f;
      return r;
    });
    if (rc == PFB_OK && done < need) {
      int32_t have = 0;
      rc = pfb_trace_flush(h, out + done, &have);
      done += (uint64_t)have;
    }
    *bins_out = done;
    free_trace(h);
    return rc;
  });
}
