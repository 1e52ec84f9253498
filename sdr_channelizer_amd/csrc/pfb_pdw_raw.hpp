// pfb_pdw_raw.hpp -- the raw-stream extractor (matlab/create_pdws.m:30-105, pfb_pdw_extract_raw): noise floor (:44) and
// masks (:45-47, :57, :63), time-parallel (one column, so lanes are consecutive samples), and their host side: RawStage
// (what a raw call prepares, shared with the dwell analysis), launch_raw_masks and extract_raw.  Edges and pulses are
// pfb_pdw_stage.hpp's.
#pragma once

#include <cmath>
#include <vector>

#include "pfb_pdw_stage.hpp"

namespace {
constexpr int kRawBits = 11, kRawBins = 1 << kRawBits;

// one digit pass of the radix select of the stream's median |x|^2 key: digit = (key >> shift) & (bins-1)
// among keys whose bits above the digit equal `prefix`
// below_out (optional): also count the keys whose bits above the digit are SMALLER than prefix's -- what a pass that
// starts from a predicted prefix needs to turn the stream's rank into a rank inside the bucket
template <class Src, bool VEC>
__global__ void __launch_bounds__(256) pdw_raw_hist_kernel(Src src, long long n, int shift, unsigned bins_mask,
                                                           unsigned long long prefix, unsigned long long prefix_mask,
                                                           unsigned* hist, unsigned long long* below_out) {
  __shared__ unsigned h[kRawBins];
  for (int i = threadIdx.x; i < kRawBins; i += 256) h[i] = 0u;
  __syncthreads();
  unsigned long long nbelow = 0ull;
  const long long step = (long long)gridDim.x * 1024;
  for (long long i0 = (long long)blockIdx.x * 1024; i0 < n; i0 += step) {  // four samples per thread in flight
    unsigned long long k[4];
    bool in[4];
    if (VEC && i0 + 1024 <= n) {  // one wide load: samples i0 + 4 tid .. + 3
      src.key4((i0 >> 2) + threadIdx.x, k);
#pragma unroll
      for (int u = 0; u < 4; ++u) in[u] = true;
    } else {
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const long long i = i0 + u * 256 + threadIdx.x;
        in[u] = i < n;
        k[u] = in[u] ? src.key(i) : 0ull;
      }
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      hist_add(h, (unsigned)(k[u] >> shift) & bins_mask, in[u] && ((k[u] & prefix_mask) == prefix));
      nbelow += (unsigned long long)(in[u] && (k[u] & prefix_mask) < prefix);
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < kRawBins; i += 256)
    if (h[i]) atomicAdd(&hist[i], h[i]);
  if (below_out) {
    for (int d = 32; d > 0; d >>= 1) nbelow += __shfl_xor(nbelow, d);
    if ((threadIdx.x & 63) == 0 && nbelow) atomicAdd(below_out, nbelow);
  }
}

// keys of ns samples spread over the stream (hashed positions, as the channelized sample): the host predicts the
// median's leading digits from them
template <class Src>
__global__ void __launch_bounds__(256) pdw_raw_sample_kernel(Src src, long long stride, int ns, unsigned long long* keys) {
  const int q = blockIdx.x * 256 + threadIdx.x;
  if (q < ns) keys[q] = src.key(sample_row(q, stride));
}

// number of keys below `pivot` and the largest of them (the lower middle value of an even-length median)
template <class Src, bool VEC>
__global__ void __launch_bounds__(256) pdw_raw_below_kernel(Src src, long long n, unsigned long long pivot,
                                                            unsigned long long* below, unsigned long long* max_below) {
  unsigned long long nb = 0ull, best = 0ull;
  bool any = false;
  const long long step = (long long)gridDim.x * 1024;
  for (long long i0 = (long long)blockIdx.x * 1024; i0 < n; i0 += step) {  // four samples per thread in flight
    unsigned long long k[4];
    if (VEC && i0 + 1024 <= n) {
      src.key4((i0 >> 2) + threadIdx.x, k);
    } else {
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const long long i = i0 + u * 256 + threadIdx.x;
        k[u] = (i < n) ? src.key(i) : ~0ull;
      }
    }
#pragma unroll
    for (int u = 0; u < 4; ++u)
      if (k[u] < pivot) { ++nb; best = (any && best > k[u]) ? best : k[u]; any = true; }
  }
  if (any) { atomicAdd(below, nb); atomicMax(max_below, best); }
}

// OR of x over the 16 lanes of a DPP row, left in every lane of the row (row_ror 1, 2, 4, 8)
__device__ __forceinline__ unsigned row_or(unsigned x) {
  x |= (unsigned)__builtin_amdgcn_update_dpp(0, (int)x, 0x121, 0xf, 0xf, false);
  x |= (unsigned)__builtin_amdgcn_update_dpp(0, (int)x, 0x122, 0xf, 0xf, false);
  x |= (unsigned)__builtin_amdgcn_update_dpp(0, (int)x, 0x124, 0xf, 0xf, false);
  x |= (unsigned)__builtin_amdgcn_update_dpp(0, (int)x, 0x128, 0xf, 0xf, false);
  return x;
}

// comparison masks of the raw stream.  A wave covers 64 consecutive words: in step i every lane compares
// sample 64 * (w0 + i) + lane (one coalesced load), the wave votes, lane i keeps the word.  The magnitude is a
// monotone function of the sample's |x|^2 key (sqrt, then an exact power-of-two scale), so `mag >= lead` and
// `mag > trail` are comparisons of the KEY with the first key whose magnitude passes -- found by the host with the
// same float64 operations -- and the pass does no float64 arithmetic at all.  key_max: the largest key that is a
// number (an infinity passes every threshold, a NaN none, as with the magnitudes themselves).
template <class Src, bool VEC>
__global__ void __launch_bounds__(256) pdw_raw_mask_kernel(Src src, long long n, unsigned long long key_ge,
                                                           unsigned long long key_gt, unsigned long long key_max,
                                                           unsigned long long* f0, unsigned long long* f1, long long words) {
  const int lane = threadIdx.x & 63;
  const long long w0 = ((long long)blockIdx.x * 4 + (threadIdx.x >> 6)) * 64;
  if (w0 >= words) return;
  unsigned long long a = 0ull, b = 0ull;
  if (VEC && (w0 + 64) * 64 <= n) {
    // wide loads: in step u the wave reads 256 consecutive samples, four per lane (one 16-byte load for int16); a lane's
    // four comparison bits go to their place in the word its 16-lane row is building, the row ORs itself together
    // (DPP rotations), and lanes 4u .. 4u+3 keep the four finished words
#pragma unroll 1
    for (int u0 = 0; u0 < 16; u0 += 8) {  // eight loads in flight per lane
      unsigned long long k[8][4];
#pragma unroll
      for (int u = 0; u < 8; ++u) src.key4(((w0 * 64) >> 2) + (long long)(u0 + u) * 64 + lane, k[u]);
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        unsigned na = 0u, nb = 0u;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          na |= (unsigned)(k[u][j] >= key_ge && k[u][j] <= key_max) << j;
          nb |= (unsigned)(k[u][j] >= key_gt && k[u][j] <= key_max) << j;
        }
        // lanes 0-7 of a row fill the word's low half, lanes 8-15 the high half; OR over the row by DPP rotations
        const int sh = 4 * (lane & 7);
        const bool upper = (lane & 8) != 0;
        const unsigned a_lo = row_or(upper ? 0u : na << sh), a_hi = row_or(upper ? na << sh : 0u);
        const unsigned b_lo = row_or(upper ? 0u : nb << sh), b_hi = row_or(upper ? nb << sh : 0u);
#pragma unroll
        for (int j = 0; j < 4; ++j) {  // row j holds word 4 (u0 + u) + j
          const unsigned long long wa = ((unsigned long long)(unsigned)__builtin_amdgcn_readlane((int)a_hi, 16 * j) << 32) |
                                        (unsigned)__builtin_amdgcn_readlane((int)a_lo, 16 * j);
          const unsigned long long wb = ((unsigned long long)(unsigned)__builtin_amdgcn_readlane((int)b_hi, 16 * j) << 32) |
                                        (unsigned)__builtin_amdgcn_readlane((int)b_lo, 16 * j);
          if (lane == 4 * (u0 + u) + j) { a = wa; b = wb; }
        }
      }
    }
  } else {
    for (int i0 = 0; i0 < 64; i0 += 16) {  // sixteen loads in flight per lane
      bool ge[16], gt[16];
#pragma unroll
      for (int u = 0; u < 16; ++u) {
        const long long sidx = (w0 + i0 + u) * 64 + lane;
        ge[u] = false; gt[u] = true;  // past the end: identity
        if (sidx < n) {
          const unsigned long long k = src.key(sidx);
          ge[u] = k >= key_ge && k <= key_max;
          gt[u] = k >= key_gt && k <= key_max;
        }
      }
#pragma unroll
      for (int u = 0; u < 16; ++u) {
        const unsigned long long wa = __ballot(ge[u]), wb = __ballot(gt[u]);
        if (lane == i0 + u) { a = wa; b = wb; }
      }
    }
  }
  if (w0 + lane < words) { f0[w0 + lane] = a; f1[w0 + lane] = b; }
}

// ---- host side ------------------------------------------------------------------------------------

// host twins of dkey_inv and RawSrc::key_mag, same float64 operations: thresholds as keys, the noise floor's finish
double dkey_inv_host(unsigned long long k) {
  const unsigned long long b = (k >> 63) ? (k & 0x7fffffffffffffffull) : ~k;
  double d;
  std::memcpy(&d, &b, sizeof d);
  return d;
}
template <int FMT>
double key_mag_host(unsigned long long k, double inv_scale) {
  return (FMT == PFB_FMT_CF32) ? std::sqrt(dkey_inv_host(k)) : std::sqrt((double)k) * inv_scale;
}

// What a raw call prepares before its format is a template argument: geometry of the edge scan, the scale, the stream
// on the device (the caller's pointer, or the copy staged in arena 0) and the buffers in arena 0.
constexpr int kRawSampleKeys = 4096;  // keys of the sample that predicts the median's leading digits, behind the histogram
struct RawStage {
  long long n, ntiles, words;
  int tile_words;
  double inv_scale;  // 2^-(bit_width-1); 1 for cf32
  const void* d_iq;
  bool vec;          // d_iq is 16-byte aligned: wide loads in the counting passes
  unsigned* hist;            // [kRawBins], then kRawSampleKeys 64-bit keys
  unsigned long long* pair;  // [2]
  EdgeStage e;
};
// extra(arena): buffers of the caller's own, between pair and the edge stage
template <class Extra>
int raw_stage(PdwCall& call, const void* iq, uint64_t num_samples, uint32_t sample_format, uint32_t bit_width, uint32_t mem,
              RawStage& r, Extra&& extra) {
  r.n = (long long)num_samples;
  r.tile_words = tile_words_for(r.n, 1);
  r.ntiles = (r.n + 64ll * r.tile_words - 1) / (64ll * r.tile_words);
  r.words = r.ntiles * r.tile_words;
  r.inv_scale = sample_format == PFB_FMT_CF32 ? 1.0 : std::ldexp(1.0, -((int)bit_width - 1));
  static_assert(PFB_FMT_INT8_IQ == 0 && PFB_FMT_INT16_IQ == 1 && PFB_FMT_CF32 == 2, "a sample is 2 << format bytes");
  const size_t bytes = (size_t)r.n * ((size_t)2 << sample_format);
  char* own = nullptr;
  PDW_TRY(arena_layout(call.ws, [&](Arena& a) {
    if (mem == PFB_MEM_HOST) own = take<char>(a, bytes);
    r.hist = take<unsigned>(a, kRawBins + kRawSampleKeys * sizeof(unsigned long long) / sizeof(unsigned));
    r.pair = take<unsigned long long>(a, 2);
    extra(a);
    r.e = take_edge_stage(a, r.words, r.ntiles, 1, false);
  }));
  r.d_iq = own ? own : iq;
  r.vec = (reinterpret_cast<uintptr_t>(r.d_iq) % 16) == 0;
  if (own) PDW_TRY(hipMemcpyAsync(own, iq, bytes, hipMemcpyHostToDevice, call.st));
  return PFB_OK;
}

// comparison masks of the raw stream at the magnitudes `lead` and `trail`.  The thresholds as keys: the first key whose
// magnitude is >= lead / > trail, found with the float64 operations the device's key_mag uses
template <int FMT>
void launch_raw_masks(const RawSrc<FMT>& src, const RawStage& r, double lead, double trail, hipStream_t st) {
  const unsigned long long k_lo = (FMT == PFB_FMT_CF32) ? 0x8000000000000000ull : 0ull;               // |x|^2 = 0
  const unsigned long long k_hi = (FMT == PFB_FMT_CF32) ? 0xFFF0000000000000ull : (1ull << 33);       // +inf / above any sample
  auto first_key = [&](auto pred) {  // smallest key in [k_lo, k_hi] that passes, k_hi + 1 if none (pred is monotone)
    if (!pred(k_hi)) return k_hi + 1;
    unsigned long long lo = k_lo, hi = k_hi;  // invariant: pred(hi)
    while (lo < hi) {
      const unsigned long long mid = lo + (hi - lo) / 2;
      if (pred(mid)) hi = mid; else lo = mid + 1;
    }
    return lo;
  };
  const unsigned long long key_ge = first_key([&](unsigned long long k) { return key_mag_host<FMT>(k, r.inv_scale) >= lead; });
  const unsigned long long key_gt = first_key([&](unsigned long long k) { return key_mag_host<FMT>(k, r.inv_scale) > trail; });
  with_bool(r.vec, [&](auto vec) {
    hipLaunchKernelGGL((pdw_raw_mask_kernel<RawSrc<FMT>, decltype(vec)::value>), dim3((unsigned)((r.words + 255) / 256)), dim3(256), 0,
                       st, src, r.n, key_ge, key_gt, k_hi, r.e.f0, r.e.f1, r.words);
  });
}

struct RawParams {  // what an extraction asks for; lead_db == trail_db in the dwell analysis
  double fs, fc, t0, lead_db, trail_db;
  pfb_pdw* out;
  uint64_t capacity, *count;
  double* noise_floor_out;  // optional
};

template <int FMT>
int extract_raw(PdwCall& call, const RawStage& r, const RawParams& p) {
  const hipStream_t st = call.st;
  const long long n = r.n;
  const RawSrc<FMT> src{r.d_iq, r.inv_scale};
  // ---- noise floor (:44): radix select of rank n/2 on the |x|^2 keys, 11-bit digits
  struct Pass { int shift, bits; };
  static const Pass kIntPasses[] = {{22, 11}, {11, 11}, {0, 11}};                            // keys < 2^33
  static const Pass kF32Passes[] = {{53, 11}, {42, 11}, {31, 11}, {20, 11}, {9, 11}, {0, 9}};  // 64-bit double keys
  const Pass* pass = (FMT == PFB_FMT_CF32) ? kF32Passes : kIntPasses;
  const int npass = (FMT == PFB_FMT_CF32) ? 6 : 3;
  const unsigned grid = (unsigned)std::min<long long>(4096, std::max<long long>(1, (n + 2047) / 2048));
  std::vector<unsigned> h_hist(kRawBins);
  unsigned long long prefix = 0ull, rank = (unsigned long long)(n / 2), h_pair[2] = {0ull, 0ull};
  // The leading digits of the median are predictable: the keys of a few thousand samples spread over the stream bracket
  // it (5 sigma either side of the sample's middle), and the digits both bracket ends share are, almost surely, the
  // median's.  The select starts below them -- for noise-dominated int16 data the first two of the three passes see
  // every key in one bucket -- and the first pass it does run also counts the keys below the predicted bucket, which
  // both turns the rank into a rank inside the bucket and PROVES the prediction (the rank must fall inside); if it
  // does not, the select starts over from the top.
  int first_pass = 0;
  if (n >= (1ll << 22)) {
    constexpr int kNs = kRawSampleKeys;
    const long long stride = n / kNs;
    std::vector<unsigned long long> sk(kNs);
    unsigned long long* d_sk = reinterpret_cast<unsigned long long*>(r.hist + kRawBins);  // room behind the histogram
    hipLaunchKernelGGL(pdw_raw_sample_kernel<RawSrc<FMT>>, dim3(kNs / 256), dim3(256), 0, st, src, stride, kNs, d_sk);
    PDW_TRY(hipGetLastError());
    PDW_TRY(hipMemcpyAsync(sk.data(), d_sk, kNs * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
    PDW_TRY(hipStreamSynchronize(st));
    const int delta = (int)std::ceil(2.5 * std::sqrt((double)kNs)) + 2;
    std::nth_element(sk.begin(), sk.begin() + (kNs / 2 - delta), sk.end());
    const unsigned long long k_lo = sk[kNs / 2 - delta];
    std::nth_element(sk.begin(), sk.begin() + (kNs / 2 + delta), sk.end());
    const unsigned long long k_hi = sk[kNs / 2 + delta];
    while (first_pass < npass - 1) {  // passes whose digit (and everything above) both bracket ends share
      const int sh = pass[first_pass].shift;
      if ((k_lo >> sh) != (k_hi >> sh)) break;
      ++first_pass;
    }
    if (first_pass > 0) prefix = k_lo & (~0ull << pass[first_pass - 1].shift);
  }
  for (int ps = first_pass; ps < npass; ++ps) {
    const int top = pass[ps].shift + pass[ps].bits;
    const unsigned long long pmask = top >= 64 ? 0ull : (~0ull << top);
    const bool check = first_pass > 0 && ps == first_pass;  // the first pass after a prediction
    PDW_TRY(hipMemsetAsync(r.hist, 0, kRawBins * sizeof(unsigned), st));
    if (check) PDW_TRY(hipMemsetAsync(r.pair, 0, sizeof(unsigned long long), st));
    with_bool(r.vec, [&](auto vec) {
      hipLaunchKernelGGL((pdw_raw_hist_kernel<RawSrc<FMT>, decltype(vec)::value>), dim3(grid), dim3(256), 0, st, src, n, pass[ps].shift,
                         (1u << pass[ps].bits) - 1u, prefix, pmask, r.hist, check ? r.pair : nullptr);
    });
    PDW_TRY(hipGetLastError());
    PDW_TRY(hipMemcpyAsync(h_hist.data(), r.hist, kRawBins * sizeof(unsigned), hipMemcpyDeviceToHost, st));
    if (check) PDW_TRY(hipMemcpyAsync(h_pair, r.pair, sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
    PDW_TRY(hipStreamSynchronize(st));
    if (check) {
      unsigned long long in_bucket = 0;
      for (int d = 0; d < kRawBins; ++d) in_bucket += h_hist[d];
      const unsigned long long below_pred = h_pair[0];
      h_pair[0] = 0ull;
      if (below_pred > rank || rank - below_pred >= in_bucket) {  // the median is not in the predicted bucket: from the top
        first_pass = 0;
        prefix = 0ull;
        rank = (unsigned long long)(n / 2);
        ps = -1;
        continue;
      }
      rank -= below_pred;
    }
    unsigned long long cum = 0;
    int d = 0;
    const int last = (1 << pass[ps].bits) - 1;
    for (; d < last; ++d) {
      if (cum + h_hist[d] > rank) break;
      cum += h_hist[d];
    }
    prefix |= (unsigned long long)d << pass[ps].shift;
    rank -= cum;
  }
  unsigned long long v0 = prefix;
  if ((n & 1) == 0 && rank == 0) {
    // even count and the pivot is the first of its value in the order: the lower middle value is the largest key below
    // it.  All of the pivot's bits are decided, so the last pass's histogram (h_hist: the lowest digit among the keys
    // that share every higher bit) usually names it -- the nearest occupied digit below the pivot's; only when that
    // bucket holds nothing smaller does the data have to be read once more.
    const int dl = (int)((prefix >> pass[npass - 1].shift) & ((1u << pass[npass - 1].bits) - 1u));
    int dn = dl - 1;
    while (dn >= 0 && h_hist[dn] == 0u) --dn;
    if (dn >= 0) {
      v0 = (prefix & ~((unsigned long long)((1u << pass[npass - 1].bits) - 1u) << pass[npass - 1].shift)) |
           ((unsigned long long)dn << pass[npass - 1].shift);
    } else {
      PDW_TRY(hipMemsetAsync(r.pair, 0, 2 * sizeof(unsigned long long), st));
      with_bool(r.vec, [&](auto vec) {
        hipLaunchKernelGGL((pdw_raw_below_kernel<RawSrc<FMT>, decltype(vec)::value>), dim3(grid), dim3(256), 0, st, src, n, prefix,
                           r.pair, r.pair + 1);
      });
      PDW_TRY(hipGetLastError());
      PDW_TRY(hipMemcpyAsync(h_pair, r.pair, 2 * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
      PDW_TRY(hipStreamSynchronize(st));
      if (h_pair[0] == (unsigned long long)(n / 2)) v0 = h_pair[1];
    }
  }  // (rank > 0: the pivot's value repeats below the middle, v0 = the pivot)
  const double m1 = key_mag_host<FMT>(prefix, r.inv_scale);
  const double nf = (n & 1) ? m1 : 0.5 * (key_mag_host<FMT>(v0, r.inv_scale) + m1);
  const double lead = nf * std::pow(10.0, p.lead_db / 10.0);    // :45-46
  const double trail = nf * std::pow(10.0, p.trail_db / 10.0);  // :47
  if (p.noise_floor_out) *p.noise_floor_out = nf;
  PDW_TRY(hipMemcpyAsync(r.e.nf, &nf, sizeof(double), hipMemcpyHostToDevice, st));
  PDW_TRY(hipStreamSynchronize(st));  // nf lives on this stack frame
  // ---- edges (:54-105) and pulses
  launch_raw_masks<FMT>(src, r, lead, trail, st);
  PDW_TRY(hipGetLastError());
  return edges_and_pulses(src, 1, r.ntiles, r.tile_words, r.e, call, p.fs, p.fc, p.t0, 0u, p.out, p.capacity, p.count);
}
}  // namespace
