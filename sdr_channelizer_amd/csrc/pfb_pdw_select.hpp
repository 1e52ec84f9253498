// pfb_pdw_select.hpp -- what every selection of pfb_pdw.hip stands on: the unit's constants, the exact float64 |y|^2 and
// its order-preserving key, one digit of a workgroup radix select, and the two MATLAB medians of a workgroup (the
// `median` of create_pdws_channelized.m:73,:98-132 and create_pdws.m:44) by bucket select and by rank counting.
#pragma once

#include <hip/hip_runtime.h>

#include "pfb_channelizer.h"

namespace {
constexpr int kTile = 512;        // smallest tile of the edge scan, in frames (tiles grow with the stream, see tile_words_for)
constexpr int kCand = 2048;       // candidate capacity per channel for the exact median finish
constexpr int kPulseCache = 512;  // per-pulse values cached in LDS up to this many (channelized: pulses are tens of frames)
constexpr int kPulseCacheRaw = 7168; // same for the raw stream, whose pulses are thousands of samples (56 KB of LDS)
constexpr int kCountingMedian = 512; // cached pulses up to this long take the O(n^2 / threads) counting median
constexpr int kSampleRows = 65536; // rows sampled to bracket the median (below 8x this the full select runs)
constexpr int kSamplePasses = 3;   // digits resolved on the sample: bracket edges to 2^-12 relative
constexpr int kUndecided = 1 << 20; // samples too close to the threshold's bracket to classify before the median is known
constexpr int kBracketRows = 1024; // rows per workgroup of the bracket pass
constexpr int kBracketInFlight = 16; // rows each lane of the bracket pass has in flight
constexpr double kRadToDeg = 57.295779513082320876798154814105;

// |y|^2 of a complex64 is EXACT in float64 (two 48-bit products, 49-bit sum), so selecting on it is
// selecting on the true magnitude, and sqrt() of it is the correctly rounded magnitude.
__device__ __forceinline__ double mag2_of(float2 v) { return fma((double)v.x, (double)v.x, (double)v.y * (double)v.y); }
__device__ __forceinline__ double mag_of(float2 v) { return sqrt(mag2_of(v)); }
__device__ __forceinline__ double phase_deg(float2 v) { return atan2((double)v.y, (double)v.x) * kRadToDeg; }

// order-preserving 64-bit key of a finite double
__device__ __forceinline__ unsigned long long dkey(double d) {
  const unsigned long long b = (unsigned long long)__double_as_longlong(d);
  return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
__device__ __forceinline__ double dkey_inv(unsigned long long k) {
  const unsigned long long b = (k >> 63) ? (k & 0x7fffffffffffffffull) : ~k;
  return __longlong_as_double((long long)b);
}

// histogram increment with wave aggregation of the most likely digit: the lanes that share the first
// participating lane's digit (all of them while the decided prefix is still common to every value, most
// of them on noise-dominated data) are counted by one atomic instead of serialising on one LDS word; the
// others add themselves.  Lanes with pred == false do not count.  Call with the whole wave converged.
__device__ __forceinline__ void hist_add(unsigned* h, unsigned digit, bool pred) {
  const unsigned long long act = __ballot(pred);
  if (!act) return;
  const int leader = __ffsll((long long)act) - 1;
  const unsigned d0 = (unsigned)__shfl((int)digit, leader);
  const unsigned long long same = __ballot(pred && digit == d0);
  if ((int)(threadIdx.x & 63) == leader) atomicAdd(&h[d0], (unsigned)__popcll(same));
  else if (pred && digit != d0) atomicAdd(&h[digit], 1u);
}

// one wave: the digit of a 256-bin histogram that holds rank k (0 <= k < total count) -> pick[0], and the count of
// everything in lower digits -> pick[1].  Four counters per lane, a shuffle scan, one lane owns the answer.
__device__ __forceinline__ void find_digit(const unsigned* hist, unsigned long long k, unsigned long long* pick) {
  const int l = threadIdx.x & 63;
  const unsigned long long c0 = hist[4 * l], c1 = hist[4 * l + 1], c2 = hist[4 * l + 2], c3 = hist[4 * l + 3];
  const unsigned long long sum = c0 + c1 + c2 + c3;
  unsigned long long inc = sum;
  for (int d = 1; d < 64; d <<= 1) {
    const unsigned long long prev = __shfl_up(inc, d);
    if (l >= d) inc += prev;
  }
  unsigned long long cum = inc - sum;
  if (cum <= k && k < inc) {  // exactly one lane
    int d = 4 * l;
    if (k >= cum + c0) { cum += c0; ++d;
      if (k >= cum + c1) { cum += c1; ++d;
        if (k >= cum + c2) { cum += c2; ++d; } } }
    pick[0] = (unsigned long long)d;
    pick[1] = cum;
  }
}

// One digit of a radix select over n 64-bit keys produced by getkey(i); the whole workgroup cooperates (every thread
// must call it, with the same arguments).  The top `db` bits are decided (prefix holds them, lower bits zero); the digit
// is the next `width` (<= 8) bits.  Keys whose decided bits differ from prefix do not count (all_share: the caller
// knows that every key has them).  On return prefix has the digit, db has grown by width, k is the rank inside the
// digit's bucket and hist[digit] is still that bucket's size.  The digit holding rank k is found by wave 0.
template <int INFLIGHT = 4, class GetKey>
__device__ void block_digit_pass(GetKey getkey, long long n, long long& k, unsigned* hist /* [256] shared */,
                                 unsigned long long* pick /* [2] shared */, int& db, int width, unsigned long long& prefix,
                                 bool all_share) {
  const int shift = 64 - db - width;
  const unsigned dmask = (1u << width) - 1u;
  for (int i = threadIdx.x; i < 256; i += blockDim.x) hist[i] = 0u;
  __syncthreads();
  const bool nofilter = db == 0 || all_share;
  for (long long i0 = 0; i0 < n; i0 += (long long)INFLIGHT * blockDim.x) {  // uniform trip count: hist_add uses wave-wide votes
    unsigned long long key[INFLIGHT];
    bool in[INFLIGHT];
#pragma unroll
    for (int u = 0; u < INFLIGHT; ++u) {  // values in flight per thread
      const long long i = i0 + (long long)u * blockDim.x + threadIdx.x;
      in[u] = i < n;
      key[u] = in[u] ? getkey(i) : 0ull;
    }
#pragma unroll
    for (int u = 0; u < INFLIGHT; ++u)
      hist_add(hist, (unsigned)(key[u] >> shift) & dmask,
               in[u] && (nofilter || (key[u] >> (64 - db)) == (prefix >> (64 - db))));
  }
  __syncthreads();
  if (threadIdx.x < 64) find_digit(hist, (unsigned long long)k, pick);
  __syncthreads();
  prefix |= pick[0] << shift;
  k -= (long long)pick[1];
  db += width;
  __syncthreads();
}

// MATLAB median of n doubles produced by get(i) (any order; called by the whole workgroup with the same n).
// One scan finds the smallest and the largest key, whose common leading bits every key shares; the 8 bits right below
// spread the values over up to 256 buckets, so ONE digit pass usually leaves the middle value's bucket with a few dozen
// members (further passes only while it holds more than kCountingMedian); a third scan moves the bucket into
// `scratch` and remembers the largest key below it; the two middle order statistics are then found among the members
// by rank counting (every member counts the smaller ones).  Three scans instead of the nine of a full 8-digit select
// plus its counting pass.
template <class Get>
__device__ double block_median(Get get, long long n, unsigned* hist /* [256] shared */, unsigned long long* pick /* [2] shared */,
                               unsigned long long* scratch /* [kCountingMedian] shared */) {
  __shared__ unsigned long long s_min, s_max, s_ltmax, s_hi, s_lo;
  __shared__ unsigned s_n;
  if (threadIdx.x == 0) { s_min = ~0ull; s_max = 0ull; s_ltmax = 0ull; s_n = 0u; s_hi = 0ull; s_lo = 0ull; }
  __syncthreads();
  auto getkey = [&](long long i) { return dkey(get(i)); };
  {
    unsigned long long mn = ~0ull, mx = 0ull;
    for (long long i = threadIdx.x; i < n; i += blockDim.x) {
      const unsigned long long k = getkey(i);
      mn = k < mn ? k : mn;
      mx = k > mx ? k : mx;
    }
    atomicMin(&s_min, mn);
    atomicMax(&s_max, mx);
  }
  __syncthreads();
  const unsigned long long kmin = s_min, kmax = s_max;
  long long r = n / 2;  // rank of the upper middle value
  int db = kmin == kmax ? 64 : __clzll((long long)(kmin ^ kmax));  // bits every key shares
  unsigned long long pfx = db == 64 ? kmin : (db ? kmin & (~0ull << (64 - db)) : 0ull);
  unsigned long long bucket = (unsigned long long)n;
  bool first = true;
  while (db < 64 && bucket > (unsigned long long)kCountingMedian) {  // uniform
    const int width = 64 - db < 8 ? 64 - db : 8;
    block_digit_pass(getkey, n, r, hist, pick, db, width, pfx, first);
    first = false;
    bucket = hist[(unsigned)(pfx >> (64 - db)) & ((1u << width) - 1u)];
    __syncthreads();
  }
  unsigned long long khi, klo;
  if (db == 64) {  // the bucket is one value (all keys equal, or heavy ties)
    khi = pfx;
    klo = pfx;
    if (r == 0 && (n & 1) == 0) {  // the lower middle value is the largest key below
      unsigned long long mx = 0ull;
      for (long long i = threadIdx.x; i < n; i += blockDim.x) {
        const unsigned long long k = getkey(i);
        if (k < pfx) mx = k > mx ? k : mx;
      }
      if (mx) atomicMax(&s_ltmax, mx);
      __syncthreads();
      klo = s_ltmax;
    }
  } else {
    const unsigned long long dmask = db == 0 ? 0ull : ~0ull << (64 - db);
    const int lane = threadIdx.x & 63;
    unsigned long long mx = 0ull;
    for (long long i0 = 0; i0 < n; i0 += blockDim.x) {  // uniform trip count: wave-wide votes
      const long long i = i0 + threadIdx.x;
      const unsigned long long k = i < n ? getkey(i) : 0ull;
      const bool in = i < n && (k & dmask) == pfx;
      if (i < n && k < pfx) mx = k > mx ? k : mx;
      const unsigned long long vote = __ballot(in);
      if (vote) {
        const int leader = __ffsll((long long)vote) - 1;
        unsigned base = 0u;
        if (lane == leader) base = atomicAdd(&s_n, (unsigned)__popcll(vote));
        base = (unsigned)__shfl((int)base, leader);
        if (in) scratch[base + (unsigned)__popcll(vote & ((1ull << lane) - 1ull))] = k;
      }
    }
    if (mx) atomicMax(&s_ltmax, mx);
    __syncthreads();
    const int m = (int)bucket;
    for (int i = threadIdx.x; i < m; i += blockDim.x) {
      const unsigned long long ki = scratch[i];
      long long rank = 0;
      for (int j = 0; j < m; ++j) {
        const unsigned long long kj = scratch[j];
        rank += (kj < ki) || (kj == ki && j < i);
      }
      if (rank == r) s_hi = ki;
      if (rank == r - 1) s_lo = ki;
    }
    __syncthreads();
    khi = s_hi;
    klo = r > 0 ? s_lo : s_ltmax;
  }
  const double hi = dkey_inv(khi);
  const double res = (n & 1) ? hi : 0.5 * (dkey_inv(klo) + hi);
  __syncthreads();  // the shared words are free for the next call
  return res;
}

// median of the n <= kCountingMedian values in v[] (LDS) by rank counting: element i has rank
// #{v_j < v_i} + #{j < i : v_j == v_i}; the two middle ranks announce themselves.  No passes, two barriers.
__device__ double cached_median(const double* v, int n, double* mid /* [2] shared */) {
  const int kh = n / 2, kl = kh - 1;
  for (int i = threadIdx.x; i < n; i += blockDim.x) {
    const double vi = v[i];
    int rank = 0;
    for (int j = 0; j < n; ++j) {
      const double vj = v[j];
      rank += (vj < vi) || (vj == vi && j < i);
    }
    if (rank == kh) mid[1] = vi;
    if (rank == kl) mid[0] = vi;
  }
  __syncthreads();
  const double r = (n & 1) ? mid[1] : 0.5 * (mid[0] + mid[1]);
  __syncthreads();
  return r;
}
}  // namespace
