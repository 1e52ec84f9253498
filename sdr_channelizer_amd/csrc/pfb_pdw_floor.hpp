// pfb_pdw_floor.hpp -- noise floor of the channelized extractor (create_pdws_channelized.m:73-75), the route that always
// works: full MSB-first radix select of rank[col] over the column's magnitudes, exact finish, thresholds.
#pragma once

#include "pfb_pdw_select.hpp"

namespace {
// q-th sampled row: one row out of every `stride`, at a hashed offset inside its stride block (a fixed
// offset could alias with a periodic signal)
__device__ __forceinline__ long long sample_row(long long q, long long stride) {
  if (stride == 1) return q;
  unsigned long long h = (unsigned long long)q * 0x9E3779B97F4A7C15ull;
  h ^= h >> 29;
  return q * stride + (long long)(((h >> 40) * (unsigned long long)stride) >> 24);
}

// one 8-bit digit histogram pass over F rows (row q -> sample_row(q, stride)).
// grid = (column groups of 64, row blocks, selects); block = 256 (4 waves).  blockIdx.z picks one of several
// independent selects over the same rows (prefix[z][M], hist[z][M][256]): the two bracket ranks run together.
__global__ void __launch_bounds__(256) pdw_hist_kernel(const float2* y, long long F, long long stride, int M, int pass,
                                                       const unsigned long long* prefix, unsigned* hist) {
  prefix += (size_t)blockIdx.z * M;
  hist += (size_t)blockIdx.z * M * 256;
  __shared__ unsigned h[256][64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int i = threadIdx.x; i < 256 * 64; i += 256) (&h[0][0])[i] = 0u;
  __syncthreads();
  const int col = blockIdx.x * 64 + lane;
  const bool valid = col < M;
  const int shift = 56 - 8 * pass;
  const unsigned long long pre = valid ? prefix[col] : 0ull;
  const long long rows_per_block = (F + gridDim.y - 1) / gridDim.y;
  const long long r0 = (long long)blockIdx.y * rows_per_block;
  const long long r1 = (r0 + rows_per_block < F) ? r0 + rows_per_block : F;
  if (valid) {
    auto count = [&](float2 v) {
      const unsigned long long k = dkey(mag2_of(v));  // ordered like the magnitude, no sqrt
      const bool in_bucket = (pass == 0) || ((k >> (shift + 8)) == (pre >> (shift + 8)));
      if (in_bucket) atomicAdd(&h[(unsigned)(k >> shift) & 255u][lane], 1u);
    };
    long long r = r0 + wave;
    for (; r + 28 < r1; r += 32) {  // eight rows in flight per lane: the sampled rows are far apart, each a fresh HBM line
      float2 v[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) v[u] = y[sample_row(r + 4 * u, stride) * M + col];
#pragma unroll
      for (int u = 0; u < 8; ++u) count(v[u]);
    }
    for (; r < r1; r += 4) count(y[sample_row(r, stride) * M + col]);
  }
  __syncthreads();
  for (int i = threadIdx.x; i < 256 * 64; i += 256) {
    const int d = i >> 6, c = i & 63;
    const unsigned v = h[d][c];
    if (v && (int)(blockIdx.x * 64) + c < M) atomicAdd(&hist[(size_t)(blockIdx.x * 64 + c) * 256 + d], v);
  }
}

// thr = noise floor * 10^(SNR/10) on the device, so the edge stage can be queued before the host has seen the medians
__global__ void pdw_thr_kernel(const double* nf, double gain, double* thr, int M) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < M) thr[i] = nf[i] * gain;
}

// choose the digit holding rank[col]; one wave per column (four counters per lane, a shuffle scan, one lane owns
// the answer), four columns per workgroup
__global__ void __launch_bounds__(256) pdw_pick_kernel(int M, int pass, unsigned* hist, unsigned long long* prefix,
                                                       unsigned long long* rank, unsigned* bucket, unsigned long long* below) {
  const int col = blockIdx.x * 4 + (threadIdx.x >> 6), l = threadIdx.x & 63;
  if (col >= M) return;
  unsigned* hc = hist + (size_t)col * 256;
  const uint4 c4 = *reinterpret_cast<const uint4*>(hc + 4 * l);
  const unsigned long long c0 = c4.x, c1 = c4.y, c2 = c4.z, c3 = c4.w, sum = c0 + c1 + c2 + c3;
  unsigned long long inc = sum;
  for (int d = 1; d < 64; d <<= 1) {
    const unsigned long long prev = __shfl_up(inc, d);
    if (l >= d) inc += prev;
  }
  unsigned long long cum = inc - sum;
  const unsigned long long r = rank[col];
  // the lane whose counters hold rank r; a rank past the total (cannot happen: r < count) would fall to digit 255
  const bool last = (l == 63) && r >= inc;
  if ((cum <= r && r < inc) || last) {
    int d = 4 * l;
    unsigned cnt = (unsigned)c0;
    if (r >= cum + c0) { cum += c0; ++d; cnt = (unsigned)c1;
      if (r >= cum + c1) { cum += c1; ++d; cnt = (unsigned)c2;
        if (r >= cum + c2) { cum += c2; ++d; cnt = (unsigned)c3; } } }
    prefix[col] |= (unsigned long long)d << (56 - 8 * pass);
    rank[col] = r - cum;        // rank inside the chosen bucket
    below[col] += cum;          // elements strictly below the bucket so far
    bucket[col] = cnt;
  }
  *reinterpret_cast<uint4*>(hc + 4 * l) = make_uint4(0u, 0u, 0u, 0u);
}

// gather the bucket's exact values, and the largest value below the bucket (for the lower median)
__global__ void __launch_bounds__(256) pdw_collect_kernel(const float2* y, long long F, int M, int passes_done,
                                                          const unsigned long long* prefix, double* cand,
                                                          unsigned* cand_n, unsigned long long* max_below) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int col = blockIdx.x * 64 + lane;
  if (col >= M) return;
  const int low_bits = 64 - 8 * passes_done;  // undecided low bits
  const unsigned long long pre = prefix[col];
  const long long rows_per_block = (F + gridDim.y - 1) / gridDim.y;
  const long long r0 = (long long)blockIdx.y * rows_per_block;
  const long long r1 = (r0 + rows_per_block < F) ? r0 + rows_per_block : F;
  unsigned long long best = 0ull;
  for (long long r = r0 + wave; r < r1; r += 4) {
    const double m = mag2_of(y[r * M + col]);
    const unsigned long long k = dkey(m);
    const unsigned long long hi = (low_bits >= 64) ? 0ull : (k >> low_bits), phi = (low_bits >= 64) ? 0ull : (pre >> low_bits);
    if (hi == phi) {
      const unsigned slot = atomicAdd(&cand_n[col], 1u);
      if (slot < (unsigned)kCand) cand[(size_t)col * kCand + slot] = m;
    } else if (hi < phi) {
      best = k > best ? k : best;
    }
  }
  if (best) atomicMax(&max_below[col], best);
}

// exact finish: sort the candidates of one column (bitonic in LDS), pick the two middle values
__global__ void __launch_bounds__(256) pdw_median_finish_kernel(long long F, int passes_done, const double* cand,
                                                                const unsigned* cand_n, const unsigned long long* prefix,
                                                                const unsigned long long* rank,
                                                                const unsigned long long* max_below, double* nf) {
  __shared__ double v[kCand];
  const int col = blockIdx.x;
  const unsigned n = cand_n[col];
  const unsigned long long r = rank[col];
  double v1, v0;
  if (n > (unsigned)kCand) {
    // only reachable when all 64 key bits are decided: the whole bucket is one value
    v1 = dkey_inv(prefix[col]);
    v0 = (r > 0) ? v1 : dkey_inv(max_below[col]);
  } else {
    for (int i = threadIdx.x; i < kCand; i += 256) v[i] = (i < (int)n) ? cand[(size_t)col * kCand + i] : INFINITY;
    __syncthreads();
    for (int k = 2; k <= kCand; k <<= 1)
      for (int j = k >> 1; j > 0; j >>= 1) {
        for (int i = threadIdx.x; i < kCand; i += 256) {
          const int l = i ^ j;
          if (l > i) {
            const bool up = (i & k) == 0;
            const double a = v[i], b = v[l];
            if ((a > b) == up) { v[i] = b; v[l] = a; }
          }
        }
        __syncthreads();
      }
    v1 = v[r];
    v0 = (r > 0) ? v[r - 1] : dkey_inv(max_below[col]);
  }
  (void)passes_done;
  // the candidates are squared magnitudes; MATLAB median: mean of the two middle values
  if (threadIdx.x == 0) nf[col] = (F & 1) ? sqrt(v1) : 0.5 * (sqrt(v0) + sqrt(v1));
}
}  // namespace
