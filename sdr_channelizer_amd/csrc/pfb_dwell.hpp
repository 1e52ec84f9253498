// pfb_dwell.hpp -- dwell analysis (include/pfb_channelizer.h, pfb_dwell_analyze; the entry point is in pfb_pdw.hip) on
// the raw extractor's sample source, stage and edge stage (pfb_pdw_raw.hpp).
//
// Restates the per-dwell part of the reference's event predictor on the raw recorder stream:
//   matlab/predict_event.m:53-121       MEDIAN: the raw extractor with one threshold for both edges -- extract_raw itself
//   cpp/usrp_predict_event.cpp:287-343  MEAN: noise floor = mean |x| (:288-289), amplitude = mean |x| from the leading
//                                       sample up to, not including, the trailing one (:311,:334,:325)
// and the gain finders' saturation scan (cpp/usrp_find_max_unsaturated_gain.cpp:146,
// cpp/blade_find_max_unsaturated_gain.cpp:268) as one pass over the stream:
//
//   stats   dwell_stats_kernel  one read: sum |x|, max |x|^2, max |component|, components past the saturation limits.
//                               Every workgroup leaves one record; the host adds the records in index order.  No
//                               floating-point atomics and a grid that depends on n alone: same buffer, same bits.
//   masks   pdw_raw_mask_kernel at lead == trail == threshold (launch_raw_masks)
//   edges   edges_and_pulses, with
//   pulses  dwell_pulse_mean_kernel: one workgroup per pulse, a strided double sum per thread folded by a fixed tree.
//
// The MEAN route reads the stream twice (stats, masks) plus the pulses' own samples; it has no radix select.
#pragma once

#include "pfb_pdw_raw.hpp"

namespace {
struct DwellPartial {  // what one workgroup of the stats pass saw
  double sum;    // of sqrt(I^2 + Q^2), raw units (integers: the 2^-(bit_width-1) scale is applied once, to the total)
  double m2max;  // largest I^2 + Q^2 (exact in double for every format)
  double cmax;   // largest |I|, |Q|
  unsigned long long nsat;
};

constexpr int kDwellChunk = 1024;      // samples per workgroup step: four per thread, one 16-byte load for int16
constexpr int kDwellMaxBlocks = 2048;  // 8 workgroups of 4 waves on each of 256 CUs; longer streams are grid-strided

unsigned dwell_stats_grid(long long n) {
  return (unsigned)std::min<long long>(kDwellMaxBlocks, (n + kDwellChunk - 1) / kDwellChunk);
}

// a thread's running figures.  Integer formats compare the raw components with integer limits (c <= lo is
// c <= floor(lo) for an integer c: the host rounds the double limits outwards), cf32 compares in double.
template <int FMT>
struct DwellAcc {
  double sum = 0.0;
  long long k_max = 0;
  int c_max = 0;
  unsigned long long nsat = 0ull;
  int lo, hi;
  __device__ DwellAcc(double sat_lo, double sat_hi) : lo((int)sat_lo), hi((int)sat_hi) {}
  __device__ __forceinline__ void add(int re, int im) {
    const long long k = (long long)re * re + (long long)im * im;
    sum += sqrt((double)k);
    k_max = k > k_max ? k : k_max;
    const int a = re < 0 ? -re : re, b = im < 0 ? -im : im;
    c_max = a > c_max ? a : c_max;
    c_max = b > c_max ? b : c_max;
    nsat += (unsigned)(re <= lo || re >= hi) + (unsigned)(im <= lo || im >= hi);
  }
  // samples 4q .. 4q+3 from one 8-byte (int8) or 16-byte (int16) load; p 16-byte aligned
  __device__ __forceinline__ void add4(const void* p, long long q) {
    if constexpr (FMT == PFB_FMT_INT8_IQ) {
      const int2 w = static_cast<const int2*>(p)[q];
      const int v[2] = {w.x, w.y};
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int half = (v[j >> 1] >> (16 * (j & 1))) & 0xffff;
        add((int)(signed char)(half & 0xff), (int)(signed char)(half >> 8));
      }
    } else {
      const int4 w = static_cast<const int4*>(p)[q];
      const int v[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
      for (int j = 0; j < 4; ++j) add((int)(short)(v[j] & 0xffff), (int)(short)(v[j] >> 16));
    }
  }
  __device__ __forceinline__ void add1(const void* p, long long i) {
    if constexpr (FMT == PFB_FMT_INT8_IQ) {
      const char2 v = static_cast<const char2*>(p)[i];
      add((int)v.x, (int)v.y);
    } else {
      const short2 v = static_cast<const short2*>(p)[i];
      add((int)v.x, (int)v.y);
    }
  }
  __device__ __forceinline__ double m2max() const { return (double)k_max; }
  __device__ __forceinline__ double cmax() const { return (double)c_max; }
};

template <>
struct DwellAcc<PFB_FMT_CF32> {
  double sum = 0.0, m2_max = 0.0;
  float c_max = 0.0f;
  unsigned long long nsat = 0ull;
  double lo, hi;
  __device__ DwellAcc(double sat_lo, double sat_hi) : lo(sat_lo), hi(sat_hi) {}
  __device__ __forceinline__ void add(float re, float im) {
    const double m2 = mag2_of(make_float2(re, im));
    sum += sqrt(m2);
    m2_max = fmax(m2_max, m2);
    c_max = fmaxf(c_max, fmaxf(fabsf(re), fabsf(im)));
    nsat += (unsigned)((double)re <= lo || (double)re >= hi) + (unsigned)((double)im <= lo || (double)im >= hi);
  }
  __device__ __forceinline__ void add4(const void* p, long long q) {  // two 16-byte loads
    const float4 a = static_cast<const float4*>(p)[2 * q], b = static_cast<const float4*>(p)[2 * q + 1];
    add(a.x, a.y); add(a.z, a.w); add(b.x, b.y); add(b.z, b.w);
  }
  __device__ __forceinline__ void add1(const void* p, long long i) {
    const float2 v = static_cast<const float2*>(p)[i];
    add(v.x, v.y);
  }
  __device__ __forceinline__ double m2max() const { return m2_max; }
  __device__ __forceinline__ double cmax() const { return (double)c_max; }
};

// One read of the stream.  A workgroup takes chunks blockIdx.x, blockIdx.x + gridDim.x, ... of kDwellChunk samples: a
// whole chunk of a 16-byte aligned stream by wide loads (thread t: samples 4t .. 4t+3), anything else -- a misaligned
// stream, the ragged last chunk -- by one sample per load, lanes on consecutive samples.  The threads' figures meet
// in LDS and are folded by a fixed tree; thread 0 writes the workgroup's record.
template <class Src, bool VEC>
__global__ void __launch_bounds__(256) dwell_stats_kernel(Src src, long long n, double sat_lo, double sat_hi, DwellPartial* out) {
  using Acc = DwellAcc<Src::kFmt>;
  Acc acc(sat_lo, sat_hi);
  const long long step = (long long)gridDim.x * kDwellChunk;
  for (long long i0 = (long long)blockIdx.x * kDwellChunk; i0 < n; i0 += step) {
    if (VEC && i0 + kDwellChunk <= n) {
      acc.add4(src.p, (i0 >> 2) + threadIdx.x);
    } else {
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const long long i = i0 + u * 256 + threadIdx.x;
        if (i < n) acc.add1(src.p, i);
      }
    }
  }
  __shared__ double s_sum[256], s_m2[256], s_c[256];
  __shared__ unsigned long long s_n[256];
  const int t = threadIdx.x;
  s_sum[t] = acc.sum; s_m2[t] = acc.m2max(); s_c[t] = acc.cmax(); s_n[t] = acc.nsat;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if (t < w) {
      s_sum[t] += s_sum[t + w];
      s_m2[t] = fmax(s_m2[t], s_m2[t + w]);
      s_c[t] = fmax(s_c[t], s_c[t + w]);
      s_n[t] += s_n[t + w];
    }
    __syncthreads();
  }
  if (t == 0) {
    DwellPartial r;
    r.sum = s_sum[0]; r.m2max = s_m2[0]; r.cmax = s_c[0]; r.nsat = s_n[0];
    out[blockIdx.x] = r;
  }
}

// Median of the wrapped phase steps (degrees) over samples toa .. toa + n - 1 (predict_event.m:102-105); the whole
// workgroup calls it with the same arguments.  cache, hist, pick, scratch, mid: the caller's LDS.  This is
// pdw_pulse_kernel's phase block, word for word: that kernel keeps its own copy, because calling a shared function
// from it changes its register allocation, and the existing extractors' device code stays as it is.
template <class Src, int CACHE, int THREADS>
__device__ __forceinline__ double phase_step_median(const Src& src, long long toa, long long n, int pcol, double* cache /* [CACHE] */,
                                    unsigned* hist /* [256] */, unsigned long long* pick /* [2] */,
                                    unsigned long long* scratch /* [kCountingMedian] */, double* mid /* [2] */) {
  auto dphi = [&](long long i) {
    double d = src.phase(toa + i + 1, pcol) - src.phase(toa + i, pcol);
    if (d < -180.0) d += 360.0;
    if (d > 180.0) d -= 360.0;
    return d;
  };
  double med;
  if (n <= CACHE) {  // one atan2 per sample: phases into the cache, steps into registers, steps back into the cache
    constexpr int PER = (CACHE + THREADS - 1) / THREADS;
    for (long long i = threadIdx.x; i < n; i += blockDim.x) cache[i] = src.phase(toa + i, pcol);
    __syncthreads();
    double step[PER];
#pragma unroll
    for (int j = 0; j < PER; ++j) {
      const long long i = threadIdx.x + (long long)j * THREADS;
      if (i < n - 1) {
        double d = cache[i + 1] - cache[i];
        if (d < -180.0) d += 360.0;
        if (d > 180.0) d -= 360.0;
        step[j] = d;
      }
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < PER; ++j) {
      const long long i = threadIdx.x + (long long)j * THREADS;
      if (i < n - 1) cache[i] = step[j];
    }
    __syncthreads();
    med = (n - 1 <= kCountingMedian) ? cached_median(cache, (int)(n - 1), mid)
                                     : block_median([&](long long i) { return cache[i]; }, n - 1, hist, pick, scratch);
  } else {
    med = block_median(dphi, n - 1, hist, pick, scratch);
  }
  __syncthreads();
  return med;
}

// One workgroup per pulse (usrp_predict_event.cpp:306-342); i0 = starts[pulse] is the leading sample, j = ends[pulse]
// the trailing one.  amp = (sum of |x_i|, i0 <= i < j) / (j - i0) (:311 amp = mag(toa), :334 the samples in between,
// :325): thread t adds samples i0 + t, i0 + t + THREADS, ... in that order, whatever the pulse's length, and the
// threads' sums are folded by a fixed tree.  sat: the samples strictly inside (:336).  FREQ: the median wrapped phase
// step over i0 .. j as pdw_pulse_kernel takes it; without it the kernel needs no cache and freq is NaN.
template <class Src, bool FREQ>
__global__ void __launch_bounds__(Src::kThreads) dwell_pulse_mean_kernel(Src src, const long long* starts, const long long* ends,
                                                                         const double* nf, double fs, double fc, double t0,
                                                                         pfb_pdw* out) {
  constexpr int THREADS = Src::kThreads, CACHE = FREQ ? Src::kCache : THREADS;
  static_assert(CACHE >= THREADS && CACHE >= kCountingMedian, "the cache holds the threads' sums, and doubles as the bucket");
  __shared__ double cache[CACHE];
  __shared__ unsigned hist[FREQ ? 256 : 1];
  __shared__ unsigned long long pick[2];
  __shared__ double mid[2];
  __shared__ unsigned long long bucket_store[FREQ && CACHE > kCountingMedian ? kCountingMedian : 1];
  __shared__ int sat_flag;
  const long long toa = starts[blockIdx.x], jj = ends[blockIdx.x];
  const int t = threadIdx.x;
  if (t == 0) sat_flag = 0;
  __syncthreads();
  double s = 0.0;
  int sat = 0;
  for (long long i = toa + t; i < jj; i += THREADS) {
    s += src.mag(i, 0);
    if (i > toa) sat |= src.saturated(i, 0);
  }
  if (sat) atomicOr(&sat_flag, 1);
  cache[t] = s;
  __syncthreads();
  for (int w = THREADS / 2; w > 0; w >>= 1) {
    if (t < w) cache[t] += cache[t + w];
    __syncthreads();
  }
  const double amp = cache[0] / (double)(jj - toa);
  __syncthreads();
  double freq = __longlong_as_double(0x7ff8000000000000ll);
  if constexpr (FREQ) {
    unsigned long long* scratch = CACHE > kCountingMedian ? bucket_store : reinterpret_cast<unsigned long long*>(cache);
    const double med = phase_step_median<Src, CACHE, THREADS>(src, toa, jj - toa + 1, 0, cache, hist, pick, scratch, mid);
    freq = fc + (fs / (360.0 / med));
  }
  if (t == 0) {
    pfb_pdw o;
    o.toa = ((double)toa / fs) + t0;     // :321 (0-based index)
    o.snr = 10.0 * log10(amp / nf[0]);   // :329
    o.pw = (double)(jj - toa) / fs;
    o.freq = freq;
    o.sat = sat_flag;
    o.bin = 0;
    o.mag = amp;
    out[blockIdx.x] = o;
  }
}

struct MeanPulse {  // edges_and_pulses' per-pulse stage of the MEAN statistic
  template <class Src>
  static void launch(Src src, const long long* starts, const long long* ends, const double* nf, double fs, double fc, double t0,
                     unsigned flags, pfb_pdw* out, unsigned long long n_out, hipStream_t st) {
    with_bool(!(flags & PFB_DWELL_SKIP_FREQ), [&](auto freq) {
      hipLaunchKernelGGL((dwell_pulse_mean_kernel<Src, decltype(freq)::value>), dim3((unsigned)n_out), dim3(Src::kThreads), 0, st, src,
                         starts, ends, nf, fs, fc, t0, out);
    });
  }
};

struct DwellStage : RawStage {  // device buffers of one call, all inside arena 0
  DwellPartial* part;  // [kDwellMaxBlocks]
};

template <int FMT>
int dwell_run(PdwCall& call, const pfb_dwell_config& c, const DwellStage& d, pfb_pdw* out, uint64_t capacity, uint64_t* count,
              pfb_dwell_stats* stats) {
  const hipStream_t st = call.st;
  const long long n = d.n;
  const int full_bits = (int)c.bit_width - 1;
  const double inv_scale = d.inv_scale;
  const double gain = std::pow(10.0, c.snr_threshold_db / 10.0);
  const RawSrc<FMT> src{d.d_iq, inv_scale};
  const unsigned grid = dwell_stats_grid(n);
  const double sf = c.sat_fraction == 0.0 ? 0.98 : c.sat_fraction;
  // the gain finders' limits; for the integer formats rounded outwards to the integers the kernel compares with
  double sat_lo = -sf, sat_hi = sf;
  if (FMT != PFB_FMT_CF32) {
    const double full = std::ldexp(1.0, full_bits);
    sat_lo = std::floor(sf * -full);
    sat_hi = std::ceil(sf * (full - 1.0));
  }
  *count = 0;
  with_bool(d.vec, [&](auto vec) {
    hipLaunchKernelGGL((dwell_stats_kernel<RawSrc<FMT>, decltype(vec)::value>), dim3(grid), dim3(256), 0, st, src, n, sat_lo, sat_hi,
                       d.part);
  });
  PDW_TRY(hipGetLastError());
  std::vector<DwellPartial> part(grid);
  PDW_TRY(hipMemcpyAsync(part.data(), d.part, grid * sizeof(DwellPartial), hipMemcpyDeviceToHost, st));
  PDW_TRY(hipStreamSynchronize(st));
  double sum = 0.0, m2max = 0.0, cmax = 0.0;
  unsigned long long nsat = 0ull;
  for (const DwellPartial& p : part) {  // index order
    sum += p.sum;
    m2max = std::max(m2max, p.m2max);
    cmax = std::max(cmax, p.cmax);
    nsat += p.nsat;
  }
  stats->num_samples = (uint64_t)n;
  stats->saturated_components = nsat;
  stats->mean_mag = sum * inv_scale / (double)n;
  stats->peak_mag = std::sqrt(m2max) * inv_scale;
  stats->peak_component = cmax * inv_scale;
  double nf = 0.0;
  int rc;
  if (c.statistic == PFB_DWELL_STAT_MEDIAN) {  // predict_event.m:64-121 is create_pdws.m with one threshold
    rc = extract_raw<FMT>(call, d, RawParams{c.fs, c.fc, c.sample_start_time, c.snr_threshold_db, c.snr_threshold_db, out, capacity,
                                             count, &nf});
  } else {
    nf = stats->mean_mag;  // usrp_predict_event.cpp:288-289
    PDW_TRY(hipMemcpyAsync(d.e.nf, &nf, sizeof(double), hipMemcpyHostToDevice, st));
    PDW_TRY(hipStreamSynchronize(st));  // nf lives on this stack frame
    launch_raw_masks<FMT>(src, d, nf * gain, nf * gain, st);  // :291, :306, :316
    PDW_TRY(hipGetLastError());
    rc = edges_and_pulses<RawSrc<FMT>, MeanPulse>(src, 1, d.ntiles, d.tile_words, d.e, call, c.fs, c.fc, c.sample_start_time, c.flags,
                                                  out, capacity, count);
  }
  stats->noise_floor = nf;
  stats->threshold = nf * gain;
  stats->pulses = *count;
  stats->any_pulse_saturated = 0;
  stats->reserved = 0;
  if (rc == PFB_OK)
    for (uint64_t i = 0; i < std::min<uint64_t>(*count, capacity); ++i) stats->any_pulse_saturated |= out[i].sat != 0;
  return rc;
}

int dwell_analyze_impl(const pfb_dwell_config* cfg, const void* iq, uint64_t num_samples, pfb_pdw* out, uint64_t capacity,
                       uint64_t* count, pfb_dwell_stats* stats, void* hip_stream) {
  if (!iq || !count || !stats || num_samples < 2 || (capacity && !out)) return PFB_ERR_BAD_ARG;
  int rc = pfb::dwell_check_config(cfg, false);
  if (rc != PFB_OK) return rc;
  PdwCall call(cfg->device_id, hip_stream);
  if (call.rc != PFB_OK) return call.rc;
  DwellStage d{};
  rc = raw_stage(call, iq, num_samples, cfg->sample_format, cfg->bit_width, cfg->mem, d,
                 [&](Arena& a) { d.part = take<DwellPartial>(a, kDwellMaxBlocks); });
  if (rc != PFB_OK) return rc;
  return with_format(cfg->sample_format, [&](auto fmt) {
    return dwell_run<decltype(fmt)::value>(call, *cfg, d, out, capacity, count, stats);
  });
}
}  // namespace
