// pfb_pdw_bracket.hpp -- noise floor of the channelized extractor (create_pdws_channelized.m:73), the sampled bracket
// path: gather a hashed row sample, select the bracket's two ranks on it, and the one pass over the data that counts,
// gathers the bracket's candidates and leaves provisional masks.  pfb_pdw_finish.hpp picks the median among them.
#pragma once

#include "pfb_pdw_floor.hpp"  // sample_row

namespace {
// The sampled rows are read ONCE: the top 32 bits of every sampled |y|^2 key (the sample decides kSamplePasses = 3
// digits = 24 bits) go to keys[channel][sample], transposed through LDS so that the per-channel select streams them.
// grid = (column groups of 64, sample blocks of 64 rows); sixteen far-apart rows in flight per lane.
__global__ void __launch_bounds__(256) pdw_sample_gather_kernel(const float2* y, long long ns, long long stride, int M,
                                                                unsigned* keys, long long ld) {
  __shared__ unsigned tile[64][65];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int col = blockIdx.x * 64 + lane;
  const long long q0 = (long long)blockIdx.y * 64;
  float2 v[16];
#pragma unroll
  for (int u = 0; u < 16; ++u) {
    const long long q = q0 + wave * 16 + u;
    v[u] = (col < M && q < ns) ? y[sample_row(q, stride) * M + col] : make_float2(0.f, 0.f);
  }
#pragma unroll
  for (int u = 0; u < 16; ++u) tile[wave * 16 + u][lane] = (unsigned)(dkey(mag2_of(v[u])) >> 32);
  __syncthreads();
  for (int c = wave; c < 64; c += 4) {
    const int gc = blockIdx.x * 64 + c;
    const long long q = q0 + lane;
    if (gc < M && q < ns) keys[(size_t)gc * ld + q] = tile[lane][c];
  }
}

// both bracket ranks of one channel's sample, kSamplePasses digits each; one workgroup per channel.  The channel's
// keys (ns <= 1024 * kSampleKeysPerThread, guaranteed by F >= 8 * kSampleRows) are read once into registers; every
// pass counts both selects (two histograms), wave 0 and wave 1 find their digits side by side.
constexpr int kSampleKeysPerThread = 72;
static_assert(1024ll * kSampleKeysPerThread >= (long long)kSampleRows * 9 / 8, "ns < kSampleRows * (stride + 1) / stride, stride >= 8");
__global__ void __launch_bounds__(1024) pdw_sample_select_kernel(const unsigned* keys, long long ns, long long ld,
                                                                 unsigned long long rank_lo, unsigned long long rank_hi,
                                                                 unsigned long long* pre_lo, unsigned long long* pre_hi) {
  __shared__ unsigned hist[2][256];
  __shared__ unsigned long long pick[2][2];
  const uint4* k4 = reinterpret_cast<const uint4*>(keys + (size_t)blockIdx.x * ld);
  constexpr int kQuads = kSampleKeysPerThread / 4;
  uint4 kq[kQuads];
#pragma unroll
  for (int j = 0; j < kQuads; ++j) {
    const long long q = (long long)j * 1024 + threadIdx.x;
    kq[j] = (q * 4 < ld) ? k4[q] : make_uint4(0u, 0u, 0u, 0u);
  }
  unsigned pre[2] = {0u, 0u};                       // decided digits of the two 32-bit key prefixes
  unsigned long long rk[2] = {rank_lo, rank_hi};
#pragma unroll 1
  for (int pass = 0; pass < kSamplePasses; ++pass) {
    const int shift = 24 - 8 * pass;
    for (int i = threadIdx.x; i < 512; i += 1024) (&hist[0][0])[i] = 0u;
    __syncthreads();
    const unsigned hmask = pass ? ~0u << (shift + 8) : 0u;  // the digits already decided
    const bool split = pre[0] != pre[1];  // the two ranks sit in one bucket until their digits part: one histogram serves both
#pragma unroll
    for (int j = 0; j < kQuads; ++j) {
      const long long base = ((long long)j * 1024 + threadIdx.x) * 4;
      const unsigned kk[4] = {kq[j].x, kq[j].y, kq[j].z, kq[j].w};
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const bool valid = base + u < ns;
        const unsigned digit = (kk[u] >> shift) & 255u;
        hist_add(hist[0], digit, valid && (kk[u] & hmask) == pre[0]);
        if (split) hist_add(hist[1], digit, valid && (kk[u] & hmask) == pre[1]);  // uniform over the workgroup
      }
    }
    __syncthreads();
    if (threadIdx.x < 128) find_digit(hist[split ? threadIdx.x >> 6 : 0], rk[threadIdx.x >> 6], pick[threadIdx.x >> 6]);
    __syncthreads();
#pragma unroll
    for (int z = 0; z < 2; ++z) {
      pre[z] |= (unsigned)pick[z][0] << shift;
      rk[z] -= pick[z][1];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    pre_lo[blockIdx.x] = (unsigned long long)pre[0] << 32;
    pre_hi[blockIdx.x] = (unsigned long long)pre[1] << 32;
  }
}

// One pass over the data with the bracket [lo, hi] of every channel (key prefixes from the sample, low
// bits cleared / set): count what lies below, gather what lies inside.
//
// The same pass writes the edge machine's comparison masks.  The threshold is gain * median, and the
// median lies in [sqrt(lo), sqrt(hi)], so |y|^2 below lo * gain^2 is certainly under the threshold and
// above hi * gain^2 certainly over it (both with a 1e-9 guard band); the few samples in between are
// listed and classified exactly once the median is known (pdw_patch_kernel).  One word (64 frames)
// per wave at a time, lane = channel.
//
// Every sample is SCREENED in float32: m32 = fl(x^2 + y^2) is within 2^-23 of the exact |y|^2, and four
// per-channel float32 limits set 2^-19 outside lo / hi / t2lo / t2hi tell "surely below the bracket", "surely
// above it" and "surely over / under the threshold" in a dozen instructions.  A sample inside the bracket's
// zone (the 2 % candidates plus a 4e-6 wide rim) is parked as it is, 8 bytes, in a staging column that belongs
// to its (wave, lane, channel) -- a register counts the slots, no atomics -- and the float64 classification
// (below / inside / above, exactly as the unscreened pass did) happens once per workgroup when the columns are
// flushed: one channel per wave at a time, lanes = (source wave, slot), candidates appended as one contiguous
// run per channel.  A full column (16 slots; ~5 expected) classifies on the spot.  Samples inside the
// threshold's zone are a handful: reloaded and classified exactly.  max_below covers the zone only: it is the
// true maximum below lo whenever it is non-zero, and the finish kernel asks for a redo in the (never seen)
// case that needs it and finds it zero.
__device__ __forceinline__ void bracket_screen(double lo, double hi, float& a, float& b) {
  if (lo > 1e-30 && hi < 1e30) {  // float32 keeps its relative accuracy here
    a = (float)(lo * (1.0 - 0x1p-19));
    b = (float)(hi * (1.0 + 0x1p-19));
  } else {  // everything is "inside the zone": the exact route decides
    a = 0.0f;
    b = INFINITY;
  }
}

constexpr int kBracketSlots = 16;  // staging slots per (wave, channel): 4 waves x 16 slots = the 64 lanes of the flush

// grid = (column groups of 64, a few workgroups per CU); a workgroup walks row groups of kBracketRows frames
// (long-lived workgroups read faster than thousands of short ones), flushing its staging columns after each.
// LPR = lanes per row.  64: lane = channel, column groups of 64 (blockIdx.x).  8 / 16 / 32 for M <= LPR (the small
// banks: numBands = fs * 1e-6 at 8 ... 32 Msps): a wave-load covers 64 / LPR consecutive rows, lane (sub, channel) owns
// rows sub, sub + RPW, ... of a 64-row word -- every lane loads, where lane = channel would leave 7 of 8 idle at M = 8 --
// and the word of a channel is the OR of its RPW lanes' bits.
template <int LPR>
__global__ void __launch_bounds__(256) pdw_bracket_kernel(const float2* y, long long F, int M,
                                                          const unsigned long long* pre_lo, const unsigned long long* pre_hi,
                                                          double gain2, double* cand, unsigned cap, unsigned* cand_n,
                                                          unsigned long long* below, unsigned long long* max_below,
                                                          unsigned long long* f0, unsigned long long* f1, long long words,
                                                          unsigned long long* undecided, unsigned* und_n, unsigned* flags,
                                                          int row_groups) {
  constexpr int RPW = 64 / LPR;                                            // rows per wave-load
  constexpr int kBatch = kBracketInFlight < LPR ? kBracketInFlight : LPR;  // a lane owns LPR rows of a word
  // (rows of 65: the flush reads one column c with lanes = (wave, slot) -- 64 rows -- and with rows of 64 float2 every
  // one of those reads hit the same bank pair, a 32-way conflict: 38 % of the LDS's active cycles in round 2's counters)
  __shared__ float2 stage[4][kBracketSlots][65];
  __shared__ unsigned char cnt[4][64];
  __shared__ unsigned cand_cnt[64], cand_base[64];
  __shared__ unsigned long long below_acc[64];  // per channel of this workgroup: "below" counts, sent out once at the end
  if (threadIdx.x < 64) below_acc[threadIdx.x] = 0ull;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int sub = lane / LPR;                                              // 0 when LPR == 64
  const int col = LPR == 64 ? blockIdx.x * 64 + lane : lane % LPR;
  const int lane_off = sub * M + col;                                      // element offset of this lane inside a wave-load
  auto chan_of = [&](int c) { return LPR == 64 ? (int)blockIdx.x * 64 + c : c % LPR; };  // channel of staging column c
  const bool valid = col < M;
  constexpr unsigned long long kLow = (1ull << (64 - 8 * kSamplePasses)) - 1ull;
  constexpr int kWordsPerBlock = kBracketRows / 64;
  const unsigned long long lo = valid ? pre_lo[col] & ~kLow : 0ull, hi = valid ? pre_hi[col] | kLow : 0ull;
  const double t2lo = dkey_inv(lo) * gain2 * (1.0 - 1e-9), t2hi = dkey_inv(hi) * gain2 * (1.0 + 1e-9);
  float sA, sB, sC, sD;
  bracket_screen(dkey_inv(lo), dkey_inv(hi), sA, sB);
  bracket_screen(t2lo, t2hi, sC, sD);
  unsigned long long nb = 0ull, best = 0ull;
  const int ws = lane / kBracketSlots, sl = lane % kBracketSlots;  // the flush's view of a lane

  for (int rgi = blockIdx.y; rgi < row_groups; rgi += gridDim.y) {
    // last rows first: when the matrix has just been written (the channelizer ran right before), its tail is still in
    // the 256 MB Infinity Cache (tools/mall_probe.py: a 256 MB buffer reads back 1.4x faster than a large one)
    const int rg = row_groups - 1 - rgi;
    unsigned n = 0u, nb32 = 0u;
    if (valid) {
      for (int wi = wave; wi < kWordsPerBlock; wi += 4) {
        const long long w = (long long)rg * kWordsPerBlock + wi;
        if (w >= words) break;
        const long long r0 = w * 64;
        // the same number for the scalar unit (w depends on the wave only)
        const long long r0s = (long long)(((unsigned long long)(unsigned)__builtin_amdgcn_readfirstlane((int)(r0 >> 32)) << 32) |
                                          (unsigned)__builtin_amdgcn_readfirstlane((int)r0));
        unsigned long long over = 0ull;
        // the float64 route, on the spot: a full staging column, the threshold's zone, the ragged last word
        auto exact = [&](float2 v, int i, bool for_median, bool for_mask) {
          const double m = mag2_of(v);
          if (for_median) {
            const unsigned long long k = dkey(m);
            if (k < lo) {
              ++nb;
              best = k > best ? k : best;
            } else if (k <= hi) {
              const unsigned g = atomicAdd(&cand_n[col], 1u);
              if (g < cap) cand[(size_t)col * cap + g] = m;
              else atomicOr(flags, 1u);
            }
          }
          if (for_mask) {
            if (m > t2hi) {
              over |= 1ull << i;
            } else if (m >= t2lo) {
              const unsigned u = atomicAdd(und_n, 1u);
              if (u < (unsigned)kUndecided) undecided[u] = (unsigned long long)(r0 + i) * (unsigned long long)M + (unsigned)col;
              else atomicOr(flags, 4u);
            }
          }
        };
        unsigned long long pad = 0ull;  // frames past F: identity (f0 = 0, f1 = 1)
        if (r0 + 64 <= F) {
          // The row address is wave-uniform arithmetic on the scalar unit (a 64-bit multiply by M per load on the vector
          // unit otherwise), and the two threshold screens of a sample are one running maximum per batch: only a lane
          // whose batch reaches the threshold's lower limit looks at its samples again.  A third fewer vector instructions
          // -- and no faster (905 against 910 us in the same process): the pass is bound by its access shape.
          const float2* rows = y + r0s * M;
          for (int i = 0; i < LPR; i += kBatch) {  // the lane's rows r0 + (i + u) RPW + sub, kBatch of them in flight
            float2 v[kBatch];
#pragma unroll
            for (int u = 0; u < kBatch; ++u) v[u] = (rows + (long long)((i + u) * RPW) * M)[lane_off];
            unsigned ov = 0u, ub = 0u, sb = 0u;
            float mx = 0.0f;
#pragma unroll
            for (int u = 0; u < kBatch; ++u) {
              const float m32 = __fmaf_rn(v[u].x, v[u].x, __fmul_rn(v[u].y, v[u].y));
              const bool is_below = m32 < sA;
              nb32 += (unsigned)is_below;
              if (!is_below && !(m32 > sB)) {
                if (n < (unsigned)kBracketSlots) stage[wave][n][lane] = v[u];
                else sb |= 1u << u;
                ++n;
              }
              mx = fmaxf(mx, m32);  // (a NaN is skipped: it would pass neither threshold comparison anyway)
            }
            if (!(mx < sC)) {
#pragma unroll
              for (int u = 0; u < kBatch; ++u) {
                const float m32 = __fmaf_rn(v[u].x, v[u].x, __fmul_rn(v[u].y, v[u].y));
                ov |= (unsigned)(m32 > sD) << u;
                ub |= (unsigned)(!(m32 < sC) && !(m32 > sD)) << u;
              }
            }
            if constexpr (RPW == 1) {
              over |= (unsigned long long)ov << i;
            } else {
              while (ov) {  // bit u of the batch is row (i + u) RPW + sub of the word
                const int u = __ffs((int)ov) - 1;
                ov &= ov - 1u;
                over |= 1ull << ((i + u) * RPW + sub);
              }
            }
            unsigned bits = ub | sb;
            while (bits) {  // the threshold's zone, a full column: reload (the line is in cache) and classify exactly
              const int u = __ffs((int)bits) - 1;
              bits &= bits - 1u;
              const int row = (i + u) * RPW + sub;
              exact(y[(r0 + row) * M + col], row, (sb >> u) & 1u, (ub >> u) & 1u);
            }
          }
        } else {
          for (int t = 0; t < LPR; ++t) {
            const int row = t * RPW + sub;
            if (r0 + row < F) exact(y[(r0 + row) * M + col], row, true, true);
            else pad |= 1ull << row;
          }
        }
        if constexpr (RPW > 1) {  // a channel's word = its RPW lanes' rows
#pragma unroll
          for (int d = LPR; d < 64; d <<= 1) {
            over |= __shfl_xor(over, d);
            pad |= __shfl_xor(pad, d);
          }
        }
        if (sub == 0) {
          f0[w * M + col] = over;
          f1[w * M + col] = over | pad;
        }
      }
    }
    nb += nb32;
    cnt[wave][lane] = (unsigned char)(n < (unsigned)kBracketSlots ? n : (unsigned)kBracketSlots);
    __syncthreads();
    // flush: one channel per wave at a time, lane = (source wave, slot); exact classification of the parked samples.
    // Counting first, then ONE round of appends to the global candidate counters for all the channels at once (a
    // returning atomic per channel inside the loop would serialise sixteen memory round trips per wave), then the stores.
    auto classify = [&](int c, int gc, double& m, unsigned long long& k, bool& is_below, bool& is_cand) {
      const bool has = ws < 4 && sl < (int)cnt[ws < 4 ? ws : 0][c];
      const unsigned long long klo = pre_lo[gc] & ~kLow, khi = pre_hi[gc] | kLow;
      const float2 v = has ? stage[ws < 4 ? ws : 0][sl][c] : make_float2(0.f, 0.f);
      m = mag2_of(v);
      k = dkey(m);
      is_below = has && k < klo;
      is_cand = has && k >= klo && k <= khi;
    };
    for (int c = wave; c < 64; c += 4) {
      const int gc = chan_of(c);
      if (gc >= M) {  // uniform over the wave
        if (lane == 0) cand_cnt[c] = 0u;
        continue;
      }
      double m;
      unsigned long long k;
      bool is_below, is_cand;
      classify(c, gc, m, k, is_below, is_cand);
      const unsigned long long vb = __ballot(is_below), vc = __ballot(is_cand);
      if (lane == 0) cand_cnt[c] = (unsigned)__popcll(vc);
      if (vb) {
        if (lane == __ffsll((long long)vb) - 1) atomicAdd(&below_acc[c % LPR], (unsigned long long)__popcll(vb));
        if (is_below) atomicMax(&max_below[gc], k);
      }
    }
    __syncthreads();
    // one append per CHANNEL and workgroup (64 / LPR staging columns share a channel when rows are packed: with a
    // returning atomic per column the eight channels of an M = 8 bank took 2 M of them each -- 5.9 ms for 2 GB)
    if (threadIdx.x < LPR) {
      const int gc = chan_of((int)threadIdx.x);
      unsigned tot = 0u;
#pragma unroll
      for (int j = 0; j < RPW; ++j) tot += cand_cnt[threadIdx.x + j * LPR];
      unsigned b0 = (gc < M && tot) ? atomicAdd(&cand_n[gc], tot) : 0u;
#pragma unroll
      for (int j = 0; j < RPW; ++j) {
        cand_base[threadIdx.x + j * LPR] = b0;
        b0 += cand_cnt[threadIdx.x + j * LPR];
      }
    }
    __syncthreads();
    for (int c = wave; c < 64; c += 4) {
      const int gc = chan_of(c);
      if (gc >= M || cand_cnt[c] == 0u) continue;  // uniform over the wave
      double m;
      unsigned long long k;
      bool is_below, is_cand;
      classify(c, gc, m, k, is_below, is_cand);
      const unsigned long long vc = __ballot(is_cand);
      if (is_cand) {
        const unsigned pos = cand_base[c] + (unsigned)__popcll(vc & ((1ull << lane) - 1ull));
        if (pos < cap) cand[(size_t)gc * cap + pos] = m;
        else atomicOr(flags, 1u);
      }
    }
    __syncthreads();  // the staging columns are free again
  }
  if (valid) {
    if (nb) atomicAdd(&below_acc[lane % LPR], nb);
    if (best) atomicMax(&max_below[col], best);
  }
  __syncthreads();
  if (threadIdx.x < LPR) {
    const int gc = chan_of((int)threadIdx.x);
    if (gc < M && below_acc[threadIdx.x]) atomicAdd(&below[gc], below_acc[threadIdx.x]);
  }
}
}  // namespace
