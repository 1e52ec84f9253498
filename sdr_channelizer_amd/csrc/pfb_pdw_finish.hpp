// pfb_pdw_finish.hpp -- end of the sampled bracket path (create_pdws_channelized.m:73-75): the exact median among the
// bracket's candidates, split over several workgroups per channel, and the patch of the provisional masks (:87, :94).
#pragma once

#include "pfb_pdw_bracket.hpp"

namespace {
// exact order statistics among the gathered candidates; one workgroup per channel.  The median's rank
// must fall inside the candidate set -- that is the proof the sampled bracket held it.  The leading bits
// lo and hi share are known, so the select starts right below them: ONE histogram pass over the candidates on the
// next 8 bits, a second pass that moves that digit's bucket (1/100 of them or so) into LDS, and the
// remaining bits are decided there.  The lower middle value of an even count is the largest candidate below
// the upper one unless that one repeats.  Also checks that the threshold really lies inside the band the
// provisional masks assumed (flag 8 if not).
constexpr int kFinishLds = 4096;  // bucket members held in LDS; a larger bucket (heavily tied data) keeps selecting in memory

// The select is split over gridDim.y workgroups per channel (one workgroup scanning a channel's 84 000 candidates twice
// was 0.12 ms on 128 of the 256 CUs, and 1 ms for the 670 000 candidates of an M = 8 matrix on 8 of them):
// pdw_finish_hist_kernel -- every part histograms its share of the candidates on the first undecided digit into
// fin.hist; pdw_bracket_finish_kernel -- every part finds the median's digit in that histogram, moves its share of
// that digit's bucket into fin.bucket, and the LAST part to arrive (a ticket) holds the bucket in LDS and finishes.
constexpr int kFinishBits = 11, kFinishBins = 1 << kFinishBits;  // the first digit: wide enough to leave <= kFinishLds members of 4 M candidates
struct FinishShared {
  unsigned* hist;               // [M][kFinishBins] first-digit histogram of the candidates
  unsigned long long* bucket;   // [M][kFinishLds] keys of the median's bucket
  unsigned* bucket_n;           // [M]
  unsigned long long* lt_max;   // [M] largest candidate key below the bucket
  unsigned* ticket;             // [M]
};

// what every part derives from the channel's counters; false: the bracket did not hold the median (or overflowed)
struct FinishSetup {
  unsigned long long n, lo, hi;
  long long r0;
  int shared_bits;
};
__device__ __forceinline__ bool finish_setup(int col, long long F, unsigned cap, const unsigned* cand_n,
                                             const unsigned long long* below, const unsigned long long* pre_lo,
                                             const unsigned long long* pre_hi, FinishSetup& q) {
  constexpr unsigned long long kLow = (1ull << (64 - 8 * kSamplePasses)) - 1ull;
  const unsigned long long b = below[col], target = (unsigned long long)(F / 2);
  q.n = cand_n[col];
  if (q.n > cap || b > target || target - b >= q.n) return false;
  q.lo = pre_lo[col] & ~kLow;
  q.hi = pre_hi[col] | kLow;
  q.shared_bits = q.lo == q.hi ? 64 : __clzll((long long)(q.lo ^ q.hi));  // leading bits every candidate has
  q.r0 = (long long)(target - b);  // the upper middle value's rank among the candidates
  return true;
}

__global__ void __launch_bounds__(1024) pdw_finish_hist_kernel(long long F, const double* cand, unsigned cap,
                                                               const unsigned* cand_n, const unsigned long long* below,
                                                               const unsigned long long* pre_lo,
                                                               const unsigned long long* pre_hi, FinishShared fin) {
  __shared__ unsigned hist[kFinishBins];
  const int col = blockIdx.x;
  FinishSetup q;
  if (!finish_setup(col, F, cap, cand_n, below, pre_lo, pre_hi, q) || q.shared_bits == 64) return;  // uniform
  const int width = 64 - q.shared_bits < kFinishBits ? 64 - q.shared_bits : kFinishBits, shift = 64 - q.shared_bits - width;
  const unsigned dmask = (1u << width) - 1u;
  const double* v = cand + (size_t)col * cap;
  const long long i_begin = (long long)(q.n * blockIdx.y / gridDim.y), i_end = (long long)(q.n * (blockIdx.y + 1) / gridDim.y);
  for (int i = threadIdx.x; i < kFinishBins; i += blockDim.x) hist[i] = 0u;
  __syncthreads();
  for (long long i0 = i_begin; i0 < i_end; i0 += 8ll * blockDim.x) {  // uniform trip count: hist_add uses wave-wide votes
    unsigned long long kk[8];
    bool in[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const long long i = i0 + (long long)u * blockDim.x + threadIdx.x;
      in[u] = i < i_end;
      kk[u] = in[u] ? dkey(v[i]) : 0ull;
    }
#pragma unroll
    for (int u = 0; u < 8; ++u) hist_add(hist, (unsigned)(kk[u] >> shift) & dmask, in[u]);
  }
  __syncthreads();
  for (int i = threadIdx.x; i < kFinishBins; i += blockDim.x)
    if (hist[i]) atomicAdd(&fin.hist[(size_t)col * kFinishBins + i], hist[i]);
}

__global__ void __launch_bounds__(1024) pdw_bracket_finish_kernel(long long F, const double* cand, unsigned cap,
                                                                  const unsigned* cand_n, const unsigned long long* below,
                                                                  const unsigned long long* max_below,
                                                                  const unsigned long long* pre_lo,
                                                                  const unsigned long long* pre_hi, double gain, double* nf,
                                                                  unsigned* flags, FinishShared fin) {
  __shared__ unsigned hist[256];
  __shared__ unsigned long long pick[2];
  __shared__ unsigned long long lt_count, lt_max;
  __shared__ unsigned long long members[kFinishLds];
  __shared__ unsigned members_n, my_ticket;
  const int col = blockIdx.x, part = blockIdx.y, parts = gridDim.y;
  FinishSetup q;
  if (!finish_setup(col, F, cap, cand_n, below, pre_lo, pre_hi, q)) {  // uniform over the workgroup
    if (part == 0 && threadIdx.x == 0) { atomicOr(flags, 2u); nf[col] = 0.0; }
    return;
  }
  const unsigned long long n = q.n, lo = q.lo, hi = q.hi;
  const int shared_bits = q.shared_bits;
  const long long r0 = q.r0;
  const double* v = cand + (size_t)col * cap;
  auto getkey = [&](long long i) { return dkey(v[i]); };
  const bool even = (F & 1) == 0;
  if (threadIdx.x == 0) { lt_count = 0ull; lt_max = 0ull; members_n = 0u; }
  unsigned long long k1;
  bool lower_known = false;  // lt_count / lt_max already hold the candidates below k1
  if (shared_bits == 64) {
    if (part != 0) return;
    k1 = lo;
  } else {
    long long r = r0;
    int db = shared_bits;  // bits decided so far
    unsigned long long pfx = db ? lo & (~0ull << (64 - db)) : 0ull;
    unsigned bucket;
    {  // the first digit (kFinishBits wide): every part reads the histogram all the parts built (pdw_finish_hist_kernel)
      const int width = 64 - db < kFinishBits ? 64 - db : kFinishBits, shift = 64 - db - width;
      if (threadIdx.x < 64) {  // wave 0: kFinishBins / 64 bins per lane, a shuffle scan, the owning lane walks its bins
        constexpr int PER = kFinishBins / 64;
        const unsigned* hc = fin.hist + (size_t)col * kFinishBins + threadIdx.x * PER;
        unsigned long long sum = 0ull;
        for (int j = 0; j < PER; ++j) sum += hc[j];
        unsigned long long inc = sum;
        for (int d = 1; d < 64; d <<= 1) {
          const unsigned long long prev = __shfl_up(inc, d);
          if ((int)threadIdx.x >= d) inc += prev;
        }
        unsigned long long cum = inc - sum;
        const unsigned long long kk = (unsigned long long)r;
        if (cum <= kk && kk < inc) {  // exactly one lane
          int j = 0;
          for (; j < PER - 1; ++j) {
            if (kk < cum + hc[j]) break;
            cum += hc[j];
          }
          pick[0] = (unsigned long long)(threadIdx.x * PER + j);
          pick[1] = cum;
          lt_count = hc[j];  // (borrowed until the setup below: the bucket's size)
        }
      }
      __syncthreads();
      pfx |= pick[0] << shift;
      r -= (long long)pick[1];
      db += width;
      bucket = (unsigned)lt_count;
      __syncthreads();
      if (threadIdx.x == 0) lt_count = 0ull;
    }
    if (bucket > (unsigned)kFinishLds && part != 0) return;  // heavily tied data: part 0 keeps selecting in memory, alone
    // further passes over all the candidates until the bucket fits LDS (the 8 bits right below the shared ones spread
    // the bracket's population over up to 256 buckets, so this loop does not run as a rule)
    const bool alone = bucket > (unsigned)kFinishLds || parts == 1;
    while (db < 64 && bucket > (unsigned)kFinishLds) {  // uniform
      const int width = 64 - db < 8 ? 64 - db : 8;
      block_digit_pass<16>(getkey, (long long)n, r, hist, pick, db, width, pfx, false);
      bucket = hist[(unsigned)(pfx >> (64 - db)) & ((1u << width) - 1u)];
      __syncthreads();
    }
    if (db == 64) {
      k1 = pfx;
    } else {
      // move the bucket out of the candidates: this part's share (everything when it works alone), slots claimed per
      // wave; remember the largest candidate below the bucket
      const unsigned long long dmask = db == 0 ? 0ull : ~0ull << (64 - db);
      const int lane = threadIdx.x & 63;
      const long long i_begin = alone ? 0 : (long long)(n * part / parts), i_end = alone ? (long long)n : (long long)(n * (part + 1) / parts);
      unsigned long long* dst = members;  // LDS first (a returning global atomic per vote would chain memory round trips)
      unsigned* dst_n = &members_n;
      unsigned long long mx = 0ull;
      for (long long i0 = i_begin; i0 < i_end; i0 += 8ll * blockDim.x) {  // uniform trip count: wave-wide votes
        unsigned long long kk[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {  // eight candidates in flight per thread
          const long long i = i0 + (long long)u * blockDim.x + threadIdx.x;
          kk[u] = i < i_end ? getkey(i) : ~0ull;  // ~0 is neither a member nor below
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) {
          const unsigned long long k = kk[u];
          const bool in = k != ~0ull && (k & dmask) == pfx;
          if (k != ~0ull && k < pfx) mx = k > mx ? k : mx;
          const unsigned long long vote = __ballot(in);
          if (vote) {
            const int leader = __ffsll((long long)vote) - 1;
            unsigned base = 0u;
            if (lane == leader) base = atomicAdd(dst_n, (unsigned)__popcll(vote));
            base = (unsigned)__shfl((int)base, leader);
            if (in) dst[base + (unsigned)__popcll(vote & ((1ull << lane) - 1ull))] = k;
          }
        }
      }
      if (mx) atomicMax(&lt_max, mx);
      __syncthreads();
      if (!alone) {
        // hand over: this part's members go to the channel's bucket in memory (one slot claim per part), and the last
        // part to arrive finds every part's members and maxima there
        if (threadIdx.x == 0) my_ticket = members_n ? atomicAdd(&fin.bucket_n[col], members_n) : 0u;  // (borrowed: the base)
        __syncthreads();
        {
          unsigned long long* gb = fin.bucket + (size_t)col * kFinishLds + my_ticket;
          for (unsigned i = threadIdx.x; i < members_n; i += blockDim.x) gb[i] = members[i];
        }
        __syncthreads();  // (the workgroup's stores have left for L2)
        if (threadIdx.x == 0) {
          if (lt_max) atomicMax(&fin.lt_max[col], lt_max);
          __threadfence();  // one release per workgroup: L2 written back before the ticket is drawn (a fence per
                            // thread made this kernel 0.43 ms)
          my_ticket = atomicAdd(&fin.ticket[col], 1u);
          if (my_ticket == (unsigned)parts - 1u) __threadfence();  // the last part: acquire before it reads the others' members
        }
        __syncthreads();
        if (my_ticket != (unsigned)parts - 1u) return;  // uniform
        const volatile unsigned long long* src = fin.bucket + (size_t)col * kFinishLds;
        for (unsigned i = threadIdx.x; i < bucket; i += blockDim.x) members[i] = src[i];
        if (threadIdx.x == 0) lt_max = *reinterpret_cast<const volatile unsigned long long*>(&fin.lt_max[col]);
        __syncthreads();
      }
      const long long r_in = r;  // rank inside the bucket
      bool first = true;
      while (db < 64) {  // the remaining bits, decided among the members
        const int width = 64 - db < 8 ? 64 - db : 8;
        block_digit_pass([&](long long i) { return members[i]; }, (long long)bucket, r, hist, pick, db, width, pfx, first);
        first = false;
      }
      k1 = pfx;
      if (even && r0 > 0) {
        unsigned long long c = 0ull, m2 = 0ull;
        for (unsigned i = threadIdx.x; i < bucket; i += blockDim.x) {
          const unsigned long long k = members[i];
          if (k < k1) { ++c; m2 = k > m2 ? k : m2; }
        }
        if (c) { atomicAdd(&lt_count, c); atomicMax(&lt_max, m2); }  // members outrank everything below the bucket
        __syncthreads();
        if (threadIdx.x == 0) lt_count += (unsigned long long)(r0 - r_in);  // candidates in the lower buckets
        __syncthreads();
        lower_known = true;
      }
    }
  }
  const double v1 = dkey_inv(k1);
  double res;
  if (!even) {
    res = sqrt(v1);
  } else {
    double v0;
    if (r0 == 0) {
      const unsigned long long mb = max_below[col];
      if (mb == 0ull && threadIdx.x == 0) atomicOr(flags, 2u);  // nothing near the bracket's lower edge was seen exactly: redo
      v0 = dkey_inv(mb);
    } else {
      if (!lower_known) {
        __syncthreads();
        unsigned long long c = 0ull, mx = 0ull;
        for (long long i = threadIdx.x; i < (long long)n; i += blockDim.x) {
          const unsigned long long k = getkey(i);
          if (k < k1) { ++c; mx = k > mx ? k : mx; }
        }
        if (c) { atomicAdd(&lt_count, c); atomicMax(&lt_max, mx); }
        __syncthreads();
      }
      v0 = (lt_count == (unsigned long long)r0) ? dkey_inv(lt_max) : v1;
    }
    res = 0.5 * (sqrt(v0) + sqrt(v1));
  }
  if (threadIdx.x == 0) {
    nf[col] = res;
    const double t2 = (res * gain) * (res * gain);
    const double g2 = gain * gain;
    if (!(t2 >= dkey_inv(lo) * g2 * (1.0 - 1e-10) && t2 <= dkey_inv(hi) * g2 * (1.0 + 1e-10))) atomicOr(flags, 8u);
  }
}

// classify the listed samples now that the thresholds are known: set their bits in the masks
__global__ void __launch_bounds__(256) pdw_patch_kernel(const float2* y, int M, const double* thr,
                                                        const unsigned long long* undecided, const unsigned* und_n,
                                                        unsigned long long* f0, unsigned long long* f1) {
  const unsigned n = *und_n < (unsigned)kUndecided ? *und_n : (unsigned)kUndecided;
  for (unsigned u = blockIdx.x * 256 + threadIdx.x; u < n; u += gridDim.x * 256) {
    const unsigned long long idx = undecided[u];
    const long long row = (long long)(idx / (unsigned long long)M);
    const int col = (int)(idx % (unsigned long long)M);
    const double m = mag_of(y[idx]), t = thr[col];
    const unsigned long long bit = 1ull << (row & 63);
    if (m >= t) atomicOr(&f0[(row >> 6) * M + col], bit);
    if (m > t) atomicOr(&f1[(row >> 6) * M + col], bit);
  }
}
}  // namespace
