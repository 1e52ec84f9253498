// pfb_pdw_pulse.hpp -- sample sources (where a (sample index, channel) pair finds its complex value: the channelizer
// output, or the raw recorder stream of create_pdws.m:30-33) and the per-pulse kernel over either
// (create_pdws_channelized.m:98-132, create_pdws.m:66-102).
#pragma once

#include "pfb_pdw_select.hpp"

namespace {
struct ChanSrc {  // F x M channelizer output, frame-major complex64
  static constexpr int kCache = kPulseCache;
  static constexpr int kThreads = 64;  // pulses are tens of frames and a pulse's workgroup is a chain of memory round trips: many small workgroups per CU
  const float2* y;
  int M;
  __device__ __forceinline__ double mag(long long i, int col) const { return mag_of(y[i * M + col]); }
  __device__ __forceinline__ double phase(long long i, int col) const { return phase_deg(y[i * M + col]); }
  __device__ __forceinline__ bool saturated(long long i, int col) const {
    const float2 v = y[i * M + col];
    return (fabs((double)v.x) >= 0.9999) || (fabs((double)v.y) >= 0.9999);
  }
};

// the raw recorder stream (create_pdws.m:30-33): x = (I + jQ) / 2^(bit_width-1), one column.
// |x|^2 orders like I^2 + Q^2, which is an exact integer for the integer formats.
template <int FMT>
struct RawSrc {
  static constexpr int kCache = kPulseCacheRaw;
  static constexpr int kFmt = FMT;
  static constexpr int kThreads = 512;  // 256: 0.84 ms for 4794 pulses of 5600 samples, 512: 0.66, 1024: 1.09 (one workgroup per CU)
  const void* p;
  double inv_scale;  // 2^-(bit_width-1); 1 for cf32
  __device__ __forceinline__ void reim(long long i, double& re, double& im) const {
    if constexpr (FMT == PFB_FMT_INT8_IQ) {
      const char2 v = static_cast<const char2*>(p)[i];
      re = (double)v.x * inv_scale; im = (double)v.y * inv_scale;
    } else if constexpr (FMT == PFB_FMT_INT16_IQ) {
      const short2 v = static_cast<const short2*>(p)[i];
      re = (double)v.x * inv_scale; im = (double)v.y * inv_scale;
    } else {
      const float2 v = static_cast<const float2*>(p)[i];
      re = (double)v.x; im = (double)v.y;
    }
  }
  // order-preserving key of |x_i|^2 and the magnitude it stands for
  __device__ __forceinline__ unsigned long long key(long long i) const {
    if constexpr (FMT == PFB_FMT_INT8_IQ) {
      const char2 v = static_cast<const char2*>(p)[i];
      return (unsigned long long)((int)v.x * (int)v.x + (int)v.y * (int)v.y);
    } else if constexpr (FMT == PFB_FMT_INT16_IQ) {
      const short2 v = static_cast<const short2*>(p)[i];
      return (unsigned long long)((long long)v.x * v.x + (long long)v.y * v.y);
    } else {
      return dkey(mag2_of(static_cast<const float2*>(p)[i]));
    }
  }
  // keys of samples 4q .. 4q+3 from one 16-byte (int16), 8-byte (int8) or two 16-byte (cf32) loads; p 16-byte aligned
  __device__ __forceinline__ void key4(long long q, unsigned long long (&k)[4]) const {
    if constexpr (FMT == PFB_FMT_INT8_IQ) {
      const int2 w = static_cast<const int2*>(p)[q];
      const int v[2] = {w.x, w.y};
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int half = (v[j >> 1] >> (16 * (j & 1))) & 0xffff;
        const int re = (int)(signed char)(half & 0xff), im = (int)(signed char)(half >> 8);
        k[j] = (unsigned long long)(re * re + im * im);
      }
    } else if constexpr (FMT == PFB_FMT_INT16_IQ) {
      const int4 w = static_cast<const int4*>(p)[q];
      const int v[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const long long re = (short)(v[j] & 0xffff), im = (short)(v[j] >> 16);
        k[j] = (unsigned long long)(re * re + im * im);
      }
    } else {
      const float4 a = static_cast<const float4*>(p)[2 * q], b = static_cast<const float4*>(p)[2 * q + 1];
      k[0] = dkey(mag2_of(make_float2(a.x, a.y))); k[1] = dkey(mag2_of(make_float2(a.z, a.w)));
      k[2] = dkey(mag2_of(make_float2(b.x, b.y))); k[3] = dkey(mag2_of(make_float2(b.z, b.w)));
    }
  }
  __device__ __forceinline__ double key_mag(unsigned long long k) const {
    if constexpr (FMT == PFB_FMT_CF32) return sqrt(dkey_inv(k));
    else return sqrt((double)k) * inv_scale;
  }
  __device__ __forceinline__ double mag(long long i, int) const { return key_mag(key(i)); }
  __device__ __forceinline__ double phase(long long i, int) const {
    double re, im;
    reim(i, re, im);
    return atan2(im, re) * kRadToDeg;
  }
  __device__ __forceinline__ bool saturated(long long i, int) const {
    double re, im;
    reim(i, re, im);
    return (fabs(re) >= 0.9999) || (fabs(im) >= 0.9999);
  }
};

// ---- per pulse ------------------------------------------------------------------
template <class Src, int CACHE, int THREADS>
__global__ void __launch_bounds__(THREADS) pdw_pulse_kernel(Src src, int M, const long long* starts, const long long* ends,
                                                        const unsigned long long* base_s, const unsigned long long* base_e,
                                                        const double* nf, const double* bin_freqs, double fs, double fc,
                                                        double t0, unsigned flags, pfb_pdw* out, unsigned long long capacity) {
  __shared__ unsigned hist[256];
  __shared__ unsigned long long pick[2];
  __shared__ double cache[CACHE];
  __shared__ double mid[2];
  __shared__ int sat_flag;
  // the bucket of block_median: its own array when cached pulses can be longer than the counting median handles,
  // otherwise the cache itself (block_median then only runs for pulses too long to be cached)
  __shared__ unsigned long long bucket_store[CACHE > kCountingMedian ? kCountingMedian : 1];
  static_assert(CACHE >= kCountingMedian, "the cache doubles as the bucket");
  unsigned long long* scratch = CACHE > kCountingMedian ? bucket_store : reinterpret_cast<unsigned long long*>(cache);
  const unsigned long long pid = blockIdx.x;
  if (pid >= capacity) return;
  // channel of this pulse: base_e is the exclusive prefix of tot_e over channels, so the pulse's channel is the largest
  // one whose base <= pid (every later base is > pid).  Wave 0 counts those bases 64 at a time -- one memory round trip
  // for M <= 64 lanes' worth, where a binary search would chain log2(M) of them.
  __shared__ int chan;
  if (threadIdx.x < 64) {
    int cnt_le = 0;
    for (int c0 = 0; c0 < M; c0 += 64) {
      const int c = c0 + (int)threadIdx.x;
      cnt_le += __popcll(__ballot(c < M && base_e[c] <= pid));
    }
    if (threadIdx.x == 0) chan = cnt_le - 1;  // base_e[0] = 0 <= pid
  }
  __syncthreads();
  const int b = chan;
  const unsigned long long k = pid - base_e[b];
  const long long toa = starts[base_s[b] + k], jj = ends[base_e[b] + k];
  const long long n = jj - toa + 1;
  const int pcol = (flags & PFB_PDW_MATLAB_QUIRKS) ? 0 : b;  // :114 phase(toa:jj) linear-indexes column 1
  if (threadIdx.x == 0) sat_flag = 0;
  __syncthreads();

  // :130-132 / create_pdws.m:100-102 saturation: samples strictly inside the pulse (the edge samples take
  // the other branches)
  int sat = 0;
  for (long long i = toa + 1 + threadIdx.x; i < jj; i += blockDim.x) sat |= src.saturated(i, b);
  if (sat) atomicOr(&sat_flag, 1);

  // :101 / :70 amplitude = median magnitude over toa..jj
  double amp;
  if (n <= CACHE) {
    for (long long i = threadIdx.x; i < n; i += blockDim.x) cache[i] = src.mag(toa + i, b);
    __syncthreads();
    amp = (n <= kCountingMedian) ? cached_median(cache, (int)n, mid)
                                 : block_median([&](long long i) { return cache[i]; }, n, hist, pick, scratch);
  } else {
    amp = block_median([&](long long i) { return src.mag(toa + i, b); }, n, hist, pick, scratch);
  }
  __syncthreads();

  // :114-117 / :83-86 median of the wrapped phase steps (degrees)
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
  if (threadIdx.x == 0) {
    pfb_pdw o;
    o.toa = ((double)(toa + 1) / fs) + t0;            // :98 / :67 (1-based index)
    o.snr = 10.0 * log10(amp / nf[b]);                // :105 / :74
    o.pw = (double)(jj - toa) / fs;                   // :110 / :79
    // :80 binFreqs(bin), bin = column of the fftshift-ed matrix: the column's true centre frequency, or -- with
    // PFB_PDW_BINFREQ_UNSHIFTED -- the FFT-ordered list indexed by the shifted column (what the script computes if
    // MathWorks' centerFrequencies returns the unshifted list; unpinned).  bin_freqs is FFT-ordered; the raw script has no bins
    const double fbin = !bin_freqs ? 0.0
                        : (flags & PFB_PDW_BINFREQ_UNSHIFTED) ? bin_freqs[b] : bin_freqs[(b + (M + 1) / 2) % M];
    o.freq = (fc + fbin) + (fs / (360.0 / med));      // :122 / :91
    o.sat = sat_flag;
    o.bin = b;
    o.mag = amp;
    out[pid] = o;
  }
}
}  // namespace
