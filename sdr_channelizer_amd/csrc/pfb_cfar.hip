// pfb_cfar.hip -- a CFAR detector on a compressed stream (pfb_cfar_* in include/pfb_channelizer.h, where the arithmetic
// is defined): block sums, per-block thresholds, over-bit words, runs and their peaks, kernels and host side.
// A step takes up to 2^24 new cells.  The cells it reads are a view of two segments, the device-side carry (the
// undecided cells of earlier calls, starting on a block boundary) and the call's own buffer, which is never copied:
//   cfar_sum<E>        S[b] of the blocks the step completes.  A lane adds four cells, (a0+a1)+(a2+a3), from one
//                      16-byte load (two for bank cells) when the address allows it; xor-butterflies 1, 2, 4, ... join
//                      the C/4 lanes of a block.  Tiers: lane groups (C <= 128, 64*4/C blocks per wave), one wave
//                      (C = 256), one wave and two or four sub-sums, (s0+s1)+(s2+s3) (C = 512, 1024).
//   cfar_threshold     one thread per decided block: the 2T float64 adds, noise, alpha * noise, the one-sided flag
//   cfar_mask<E>       the second read of the cells, four to a lane as in the sum pass: 64-cell words of over bits,
//                      the 16 lanes of a word joining their four bits by xor-butterflies
//   run stage, on the words alone (1/64 of the cells):
//     cfar_tile_last   per tile of 256 words: its last over cell, its over count
//     cfar_tile_scan   one workgroup: exclusive max-scan of the tiles, seeded with the carried run's last over cell
//     cfar_word_starts per word: the over cell before it (block max-scan) and how many of its over cells start a run
//                      (the cell before them lies more than g+1 back); per-tile counts
//     cfar_start_scan  one workgroup: exclusive sum of the tile counts; what closes, the call's record count, the stats
//     cfar_write_starts the list of (start, over cell before it), in order: run k ends where run k+1's predecessor is
//     cfar_runs<E>     one wave per run: re-reads its over cells for the peak (largest p, lowest index), merges the
//                      carried partial record, writes the record at its place or, for the run still open, the carry
//   cfar_carry<E>      the cells and block sums the next step needs, into the other carry slot
// No atomics: every count is a scan, every record has one writer.  Grids are capped and stride.
// Cost: the stream is read twice (sum, mask); everything else is O(1/C) or O(1/64) of it.  A run of many dense over
// cells is walked by a single wave: correct, and slow only for input that is all detections.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <new>
#include <type_traits>

#include "pfb_common.h"
#include "pfb_host.h"

namespace {

using namespace pfb;

constexpr uint64_t kStepCells = (uint64_t)1 << 24;  // cells per step, and per staging step of a host buffer
constexpr unsigned kMaxGrid = 1u << 16;
constexpr int kTileWords = 256;
constexpr int kNone = -(1 << 30);  // "no over cell before": any local index minus this exceeds every g + 1

struct RunState {
  pfb_cfar_det d;
  uint32_t open, pad;
};
struct DevState {      // what the device keeps between calls besides cells and block sums
  RunState run[2];     // [rs] the open run's partial record; a step writes the other
  unsigned long long cells_over, detections, dropped;
  unsigned long long call_count;  // runs the current call has closed so far
};
struct StepScalars {   // from the two scan kernels to the kernels behind them
  int last_all;        // local index of the last over cell, the carried run's included; kNone without one
  int num_starts, candidates, closed;
  unsigned long long base_count;  // call_count before this step
};

struct CfarParams {
  const void* call;    // the step's cells
  const void* carry;   // carry_len cells; [0] is global cell `base`, a block boundary
  void* carry_out;
  float* S;            // S[b - sb]
  float* S_out;
  float* noise;        // per decided block
  float* thr;
  uint32_t* bflags;
  unsigned long long* words;
  int* word_prev;
  int* word_off;
  int* tile_last;
  int* tile_over;
  int* tile_prev;
  int* tile_starts;
  int* tile_off;
  int2* starts;
  DevState* st;
  StepScalars* sc;
  pfb_cfar_det* det_out;
  unsigned long long capacity;
  unsigned long long base;  // global index of view cell 0
  long long D;              // global block of view cell 0: the first undecided one
  long long sb;             // global block of S[0]
  long long nbc0, nbc1;     // complete blocks before and after the step
  int carry_len, view_len;
  int C, logC, G, T, method;
  float alpha, min_power;
  int dec_cells, dec_blocks, nwords, ntiles;
  int flush, g, rs;
  int keep_from, keep_len, s_from, s_keep;
};

// ---------------------------------------------------------------------------------
// the two-segment view

template <int E>
__device__ __forceinline__ const void* cell_ptr(const CfarParams& p, int i) {
  using T = std::conditional_t<E == PFB_CFAR_POWER, float, float2>;
  return i < p.carry_len ? static_cast<const void*>(static_cast<const T*>(p.carry) + i)
                         : static_cast<const void*>(static_cast<const T*>(p.call) + (i - p.carry_len));
}
template <int E>
__device__ __forceinline__ float cell_power(const CfarParams& p, int i) {
  return *static_cast<const float*>(cell_ptr<E>(p, i));  // a bank cell starts with its power
}
template <int E>
__device__ __forceinline__ int cell_hyp(const CfarParams& p, int i) {
  if constexpr (E == PFB_CFAR_POWER) return -1;
  else return __float_as_int(static_cast<const float2*>(cell_ptr<E>(p, i))->y);
}

// cells i .. i+3 of the view, i a multiple of 4: one or two 16-byte loads when all four lie in one segment at an
// aligned address (the carry's always do), single cells otherwise
template <int E>
__device__ __forceinline__ void load4(const CfarParams& p, int i, float& a0, float& a1, float& a2, float& a3) {
  const bool one_segment = i >= p.carry_len || i + 4 <= p.carry_len;
  const void* q = cell_ptr<E>(p, i);
  if (one_segment && (reinterpret_cast<uintptr_t>(q) & 15) == 0) {
    if constexpr (E == PFB_CFAR_POWER) {
      const float4 v = *static_cast<const float4*>(q);
      a0 = v.x; a1 = v.y; a2 = v.z; a3 = v.w;
    } else {
      const float4 v = static_cast<const float4*>(q)[0], w = static_cast<const float4*>(q)[1];
      a0 = v.x; a1 = v.z; a2 = w.x; a3 = w.z;
    }
  } else {
    a0 = cell_power<E>(p, i);
    a1 = cell_power<E>(p, i + 1);
    a2 = cell_power<E>(p, i + 2);
    a3 = cell_power<E>(p, i + 3);
  }
}

// ---------------------------------------------------------------------------------
// block scans over 256 threads (int): exclusive prefix and the total

struct OpMax { __device__ int operator()(int a, int b) const { return a > b ? a : b; } };
struct OpAdd { __device__ int operator()(int a, int b) const { return a + b; } };

template <class Op>
__device__ int block_scan_excl(int v, int ident, Op op, int* sh, int& total) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, waves = blockDim.x >> 6;
  int inc = v;
  for (int d = 1; d < 64; d <<= 1) {
    const int o = __shfl_up(inc, d, 64);
    if (lane >= d) inc = op(o, inc);
  }
  int exc = __shfl_up(inc, 1, 64);
  if (lane == 0) exc = ident;
  __syncthreads();  // sh is free again
  if (lane == 63) sh[wv] = inc;
  __syncthreads();
  int pre = ident;
  total = ident;
  for (int k = 0; k < waves; ++k) {
    if (k < wv) pre = op(pre, sh[k]);
    total = op(total, sh[k]);
  }
  return op(pre, exc);
}

// ---------------------------------------------------------------------------------
// kernels

template <int E>
__global__ void __launch_bounds__(256) cfar_sum(const CfarParams p) {
  const int lanes = min(p.C >> 2, 64);  // lanes that share one block (one 256-cell sub-sum of it)
  const int subs = max(1, p.C >> 8);
  const int per_wave = 64 / lanes;      // blocks a wave takes at once
  const int lane = threadIdx.x & 63;
  const long long wave = ((long long)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const long long nwaves = ((long long)gridDim.x * blockDim.x) >> 6;
  const long long groups = (p.nbc1 - p.nbc0 + per_wave - 1) / per_wave;
  for (long long gi = wave; gi < groups; gi += nwaves) {  // uniform per wave: the shuffles see all 64 lanes
    const long long b = p.nbc0 + gi * per_wave + lane / lanes;
    const bool live = b < p.nbc1;
    float s[4] = {0.f, 0.f, 0.f, 0.f};
    for (int q = 0; q < subs; ++q) {
      float v = 0.f;
      if (live) {
        float a0, a1, a2, a3;
        load4<E>(p, (int)((b - p.D) << p.logC) + q * 256 + (lane % lanes) * 4, a0, a1, a2, a3);
        v = (a0 + a1) + (a2 + a3);
      }
      for (int d = 1; d < lanes; d <<= 1) v += __shfl_xor(v, d, 64);
      s[q] = v;
    }
    const float total = subs == 1 ? s[0] : subs == 2 ? s[0] + s[1] : (s[0] + s[1]) + (s[2] + s[3]);
    if (live && lane % lanes == 0) p.S[b - p.sb] = total;
  }
}

__global__ void __launch_bounds__(256) cfar_threshold(const CfarParams p) {
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (long long k = (long long)blockIdx.x * blockDim.x + threadIdx.x; k < p.dec_blocks; k += stride) {
    const long long b = p.D + k;
    const long long l0 = max(b - p.G - p.T, 0ll), l1 = b - p.G;            // lead: [l0, l1)
    const long long r0 = b + p.G + 1, r1 = min(b + p.G + p.T + 1, p.nbc1);  // lag:  [r0, r1)
    double sum_l = 0.0, sum_r = 0.0;
    int nl = 0, nr = 0;
    for (long long j = l0; j < l1; ++j, ++nl) sum_l += (double)p.S[j - p.sb];
    for (long long j = r0; j < r1; ++j, ++nr) sum_r += (double)p.S[j - p.sb];
    const double C = (double)p.C;
    double m = std::numeric_limits<double>::quiet_NaN();  // no noise: no comparison with it holds
    if (p.method == PFB_CFAR_CA) {
      if (nl + nr > 0) m = (sum_l + sum_r) / ((double)(nl + nr) * C);
    } else if (nl > 0 && nr > 0) {
      const double a = sum_l / ((double)nl * C), c = sum_r / ((double)nr * C);
      if (a == a && c == c) m = p.method == PFB_CFAR_GO ? (a > c ? a : c) : (a < c ? a : c);
    } else if (nl > 0) {
      m = sum_l / ((double)nl * C);
    } else if (nr > 0) {
      m = sum_r / ((double)nr * C);
    }
    const float noise = (float)m;
    p.noise[k] = noise;
    p.thr[k] = p.alpha * noise;
    p.bflags[k] = nl + nr < 2 * p.T ? PFB_CFAR_DET_ONE_SIDED : 0u;
  }
}

template <int E>
__global__ void __launch_bounds__(256) cfar_mask(const CfarParams p) {
  const int lane = threadIdx.x & 63;
  const long long wave = ((long long)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const long long nwaves = ((long long)gridDim.x * blockDim.x) >> 6;
  const long long groups = ((long long)p.nwords + 3) / 4;  // a wave takes 256 cells at a time: four words
  for (long long gi = wave; gi < groups; gi += nwaves) {    // uniform per wave
    const int i = (int)(gi << 8) + lane * 4;                 // four cells of one block: C >= 4
    unsigned nibble = 0;
    if (i < p.dec_cells) {
      float a[4];
      if (i + 4 <= p.dec_cells) {
        load4<E>(p, i, a[0], a[1], a[2], a[3]);
      } else {
        for (int k = 0; k < 4; ++k) a[k] = i + k < p.dec_cells ? cell_power<E>(p, i + k) : -1.f;  // min_power >= 0
      }
      const float t = p.thr[i >> p.logC];
      for (int k = 0; k < 4; ++k) nibble |= ((a[k] > t) && (a[k] > p.min_power) ? 1u : 0u) << k;
    }
    unsigned long long m = (unsigned long long)nibble << (4 * (lane & 15));  // the 16 lanes of a word join their bits
    for (int d = 1; d < 16; d <<= 1) m |= __shfl_xor(m, d, 64);
    const long long w = gi * 4 + (lane >> 4);
    if ((lane & 15) == 0 && w < p.nwords) p.words[w] = m;
  }
}

__global__ void __launch_bounds__(256) cfar_tile_last(const CfarParams p) {
  __shared__ int sh[8];
  for (int t = blockIdx.x; t < p.ntiles; t += gridDim.x) {
    const int j = t * kTileWords + threadIdx.x;
    const unsigned long long w = j < p.nwords ? p.words[j] : 0ull;
    int total_last, total_over;
    block_scan_excl(w ? (j << 6) + 63 - __clzll(w) : kNone, kNone, OpMax(), sh, total_last);
    block_scan_excl(__popcll(w), 0, OpAdd(), sh, total_over);
    if (threadIdx.x == 0) {
      p.tile_last[t] = total_last;
      p.tile_over[t] = total_over;
    }
  }
}

__global__ void __launch_bounds__(256) cfar_tile_scan(const CfarParams p) {
  __shared__ int sh[8];
  const RunState& carried = p.st->run[p.rs];
  int running = carried.open ? (int)((long long)carried.d.last_index - (long long)p.base) : kNone;
  unsigned long long over = 0;
  for (int t0 = 0; t0 < p.ntiles; t0 += blockDim.x) {
    const int t = t0 + threadIdx.x;
    int total, sum;
    const int exc = block_scan_excl(t < p.ntiles ? p.tile_last[t] : kNone, kNone, OpMax(), sh, total);
    if (t < p.ntiles) p.tile_prev[t] = max(running, exc);
    running = max(running, total);
    block_scan_excl(t < p.ntiles ? p.tile_over[t] : 0, 0, OpAdd(), sh, sum);
    over += (unsigned long long)sum;
  }
  if (threadIdx.x == 0) {
    p.sc->last_all = running;
    p.st->cells_over += over;
  }
}

// the over cells of word j that start a run, given the over cell before the word; f(local index, cell before it)
template <class F>
__device__ __forceinline__ int for_each_start(unsigned long long w, int j, int prev, int g, F&& f) {
  int n = 0;
  while (w) {
    const int i = (j << 6) + __ffsll((long long)w) - 1;
    if (i - prev > g + 1) {
      f(n, i, prev);
      ++n;
    }
    prev = i;
    w &= w - 1;
  }
  return n;
}

__global__ void __launch_bounds__(256) cfar_word_starts(const CfarParams p) {
  __shared__ int sh[8];
  for (int t = blockIdx.x; t < p.ntiles; t += gridDim.x) {
    const int j = t * kTileWords + threadIdx.x;
    const unsigned long long w = j < p.nwords ? p.words[j] : 0ull;
    int total;
    const int exc = block_scan_excl(w ? (j << 6) + 63 - __clzll(w) : kNone, kNone, OpMax(), sh, total);
    const int prev = max(p.tile_prev[t], exc);
    const int n = for_each_start(w, j, prev, p.g, [](int, int, int) {});
    const int off = block_scan_excl(n, 0, OpAdd(), sh, total);
    if (j < p.nwords) {
      p.word_prev[j] = prev;
      p.word_off[j] = off;
    }
    if (threadIdx.x == 0) p.tile_starts[t] = total;
  }
}

__global__ void __launch_bounds__(256) cfar_start_scan(const CfarParams p) {
  __shared__ int sh[8];
  int running = 0;
  for (int t0 = 0; t0 < p.ntiles; t0 += blockDim.x) {
    const int t = t0 + threadIdx.x;
    int total;
    const int exc = block_scan_excl(t < p.ntiles ? p.tile_starts[t] : 0, 0, OpAdd(), sh, total);
    if (t < p.ntiles) p.tile_off[t] = running + exc;
    running += total;
  }
  if (threadIdx.x == 0) {
    DevState& st = *p.st;
    StepScalars& sc = *p.sc;
    const int candidates = (int)st.run[p.rs].open + running;
    // the last candidate closes once g + 1 decided cells follow its last over cell, or at flush
    const bool closes = p.flush || (long long)p.dec_cells - 1 - (long long)sc.last_all >= (long long)p.g + 1;
    const int closed = candidates == 0 ? 0 : candidates - (closes ? 0 : 1);
    sc.num_starts = running;
    sc.candidates = candidates;
    sc.closed = closed;
    sc.base_count = st.call_count;
    const unsigned long long after = st.call_count + (unsigned long long)closed;
    st.dropped += max(after, p.capacity) - max(st.call_count, p.capacity);
    st.detections += (unsigned long long)closed;
    st.call_count = after;
    st.run[p.rs ^ 1].open = candidates > closed ? 1u : 0u;
  }
}

__global__ void __launch_bounds__(256) cfar_write_starts(const CfarParams p) {
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (long long j = (long long)blockIdx.x * blockDim.x + threadIdx.x; j < p.nwords; j += stride) {
    const unsigned long long w = p.words[j];
    if (!w) continue;
    int2* dst = p.starts + p.tile_off[j / kTileWords] + p.word_off[j];
    for_each_start(w, (int)j, p.word_prev[j], p.g, [dst](int n, int i, int prev) { dst[n] = make_int2(i, prev); });
  }
}

struct Peak {
  float p;
  int i;  // local index; INT_MAX: none yet
};
__device__ __forceinline__ bool peak_beats(const Peak& a, const Peak& b) {  // a before b: larger p, then lower index
  if (a.i == INT_MAX) return false;
  if (b.i == INT_MAX) return true;
  return a.p > b.p || (a.p == b.p && a.i < b.i);
}

template <int E>
__global__ void __launch_bounds__(64) cfar_runs(const CfarParams p) {
  const StepScalars sc = *p.sc;
  const RunState& carried = p.st->run[p.rs];
  const int open0 = (int)carried.open;
  const int lane = threadIdx.x;
  for (int c = blockIdx.x; c < sc.candidates; c += gridDim.x) {
    const int k = c - open0;  // the run that starts at starts[k]; -1: the carried one
    const int begin = k < 0 ? 0 : p.starts[k].x;
    const int end = c == sc.candidates - 1 ? sc.last_all : p.starts[k + 1].y;  // < 0: no over cell in this step
    Peak best{0.f, INT_MAX};
    unsigned long long count = 0;
    if (end >= begin) {
      for (int j = (begin >> 6) + lane; j <= (end >> 6); j += 64) {
        unsigned long long w = p.words[j];
        const int lo = j << 6;
        if (lo < begin) w &= ~0ull << (begin - lo);
        if (lo + 63 > end) w &= ~0ull >> (63 - (end - lo));
        count += (unsigned long long)__popcll(w);
        while (w) {
          const int i = lo + __ffsll((long long)w) - 1;
          const Peak x{cell_power<E>(p, i), i};
          if (peak_beats(x, best)) best = x;
          w &= w - 1;
        }
      }
    }
    for (int d = 32; d >= 1; d >>= 1) {
      const Peak o{__shfl_xor(best.p, d, 64), __shfl_xor(best.i, d, 64)};
      if (peak_beats(o, best)) best = o;
      count += __shfl_xor(count, d, 64);
    }
    if (lane == 0) {
      pfb_cfar_det d;
      if (k < 0) {
        d = carried.d;
      } else {
        d.first_index = p.base + (unsigned long long)begin;
        d.cells_over = 0;
        d.reserved = 0;
      }
      if (best.i != INT_MAX) {
        if (k >= 0 || best.p > d.peak_power) {  // a tie with the carried peak stays with it: the lower index
          const int blk = best.i >> p.logC;
          d.peak_index = p.base + (unsigned long long)best.i;
          d.peak_power = best.p;
          d.noise = p.noise[blk];
          d.hypothesis = cell_hyp<E>(p, best.i);
          d.flags = p.bflags[blk];
        }
        d.last_index = p.base + (unsigned long long)end;
        d.cells_over = (uint32_t)min((unsigned long long)d.cells_over + count, 0xffffffffull);
      }
      if (c < sc.closed) {
        const unsigned long long pos = sc.base_count + (unsigned long long)c;
        if (pos < p.capacity) p.det_out[pos] = d;
      } else {
        p.st->run[p.rs ^ 1].d = d;  // .open is cfar_start_scan's
      }
    }
  }
}

template <int E>
__global__ void __launch_bounds__(256) cfar_carry(const CfarParams p) {
  using T = std::conditional_t<E == PFB_CFAR_POWER, float, float2>;
  const long long stride = (long long)gridDim.x * blockDim.x;
  const long long t0 = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  T* dst = static_cast<T*>(p.carry_out);
  for (long long i = t0; i < p.keep_len; i += stride) dst[i] = *static_cast<const T*>(cell_ptr<E>(p, p.keep_from + (int)i));
  for (long long i = t0; i < p.s_keep; i += stride) p.S_out[i] = p.S[p.s_from + i];
}

// ---------------------------------------------------------------------------------
// host: checks and plan

const char* sum_tier(uint32_t C, uint32_t element) {
  const bool cell = element == PFB_CFAR_BANK_CELL;
  if (C <= 128) return cell ? "pfb_cfar_sum<lanes,cell>" : "pfb_cfar_sum<lanes,power>";
  if (C == 256) return cell ? "pfb_cfar_sum<wave,cell>" : "pfb_cfar_sum<wave,power>";
  return cell ? "pfb_cfar_sum<subsums,cell>" : "pfb_cfar_sum<subsums,power>";
}

size_t elem_bytes(uint32_t element) { return element == PFB_CFAR_BANK_CELL ? 8 : 4; }

// Everything pfb_cfar_describe and pfb_cfar_create check before the device, in the order the header states
int cfar_check(const pfb_cfar_config* cfg, pfb_cfar_plan* plan) {
  if (!cfg || !plan || cfg->struct_size != sizeof(pfb_cfar_config)) return PFB_ERR_BAD_ARG;
  if (cfg->element > PFB_CFAR_BANK_CELL || cfg->method > PFB_CFAR_SO) return PFB_ERR_BAD_ARG;
  const uint32_t C = cfg->block_cells;
  if (C < 4 || C > 1024 || (C & (C - 1))) return PFB_ERR_BAD_ARG;
  if (cfg->guard_blocks > 64 || cfg->train_blocks < 1 || cfg->train_blocks > 32) return PFB_ERR_BAD_ARG;
  if (cfg->merge_gap > (1u << 20)) return PFB_ERR_BAD_ARG;
  if (!std::isfinite(cfg->alpha) || !(cfg->alpha > 0.f)) return PFB_ERR_BAD_ARG;
  if (!(cfg->min_power >= 0.f)) return PFB_ERR_BAD_ARG;  // NaN included
  if (cfg->flags != 0) return PFB_ERR_BAD_ARG;
  const uint64_t GT = (uint64_t)cfg->guard_blocks + cfg->train_blocks;
  plan->latency_cells = (GT + 1) * C;
  plan->training_cells = 2ull * cfg->train_blocks * C;
  plan->carry_bytes = (GT + 1) * C * elem_bytes(cfg->element) + (2 * GT + 2) * sizeof(float);
  std::memset(plan->sum_kernel, 0, sizeof(plan->sum_kernel));
  std::snprintf(plan->sum_kernel, sizeof(plan->sum_kernel), "%s", sum_tier(C, cfg->element));
  return PFB_OK;
}

struct HostCounters {  // all the host knows of the stream
  uint64_t n = 0;      // cells taken
  uint64_t D = 0;      // blocks decided
  uint64_t without_noise = 0;
  int slot = 0;        // carry slot (cells, S) in use
  int rs = 0;          // run-state slot in use
  bool flushed = false;
};

}  // namespace

struct pfb_cfar_handle {
  pfb_cfar_config cfg{};
  int device = 0;
  int logC = 0;
  size_t eb = 4;
  hipStream_t stream = nullptr;
  hipEvent_t ev_switch = nullptr;
  HostCounters hc;
  // device: carry slots 0 and 1, slot 2 the copy pfb_cfar_process restores from when the caller's buffer is too small
  void* d_cells[3] = {nullptr, nullptr, nullptr};
  float* d_S[3] = {nullptr, nullptr, nullptr};
  DevState* d_state = nullptr;  // [0] live, [1] the copy
  StepScalars* d_sc = nullptr;
  float* d_noise = nullptr;
  float* d_thr = nullptr;
  uint32_t* d_bflags = nullptr;
  unsigned long long* d_words = nullptr;
  int* d_word = nullptr;  // word_prev, word_off
  int* d_tile = nullptr;  // tile_last, tile_over, tile_prev, tile_starts, tile_off
  int2* d_starts = nullptr;
  size_t max_words = 0, max_tiles = 0;
  void* d_stage = nullptr;  // host cells on their way in
  size_t stage_bytes = 0;
  pfb_cfar_det* d_det = nullptr;  // records on their way out to a host buffer
  size_t det_cap = 0;
  const char* last_kernel = "";
};

namespace {

void free_cfar(pfb_cfar_handle* h) {
  if (!h) return;
  DeviceGuard g(h->device);
  for (int i = 0; i < 3; ++i) {
    (void)hipFree(h->d_cells[i]);
    (void)hipFree(h->d_S[i]);
  }
  (void)hipFree(h->d_state);
  (void)hipFree(h->d_sc);
  (void)hipFree(h->d_noise);
  (void)hipFree(h->d_thr);
  (void)hipFree(h->d_bflags);
  (void)hipFree(h->d_words);
  (void)hipFree(h->d_word);
  (void)hipFree(h->d_tile);
  (void)hipFree(h->d_starts);
  (void)hipFree(h->d_stage);
  (void)hipFree(h->d_det);
  if (h->ev_switch) (void)hipEventDestroy(h->ev_switch);
  delete h;
}

hipError_t allocate_cfar(pfb_cfar_handle* h) {
  const pfb_cfar_config& c = h->cfg;
  const uint64_t C = c.block_cells, GT = (uint64_t)c.guard_blocks + c.train_blocks;
  const uint64_t carry_cells = (GT + 1) * C;
  const uint64_t view = carry_cells + kStepCells;  // the longest view of one step
  const uint64_t blocks = view / C + 2;
  h->max_words = (size_t)(view / 64 + 2);
  h->max_tiles = h->max_words / kTileWords + 2;
  hipError_t e = hipSuccess;
  auto alloc = [&e](auto** p, size_t bytes) {
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(p), bytes);
  };
  for (int i = 0; i < 3; ++i) {
    alloc(&h->d_cells[i], carry_cells * h->eb);
    alloc(&h->d_S[i], (2 * GT + 2 + blocks) * sizeof(float));
  }
  alloc(&h->d_state, 2 * sizeof(DevState));
  alloc(&h->d_sc, sizeof(StepScalars));
  alloc(&h->d_noise, blocks * sizeof(float));
  alloc(&h->d_thr, blocks * sizeof(float));
  alloc(&h->d_bflags, blocks * sizeof(uint32_t));
  alloc(&h->d_words, h->max_words * sizeof(unsigned long long));
  alloc(&h->d_word, 2 * h->max_words * sizeof(int));
  alloc(&h->d_tile, 5 * h->max_tiles * sizeof(int));
  alloc(&h->d_starts, (view / ((uint64_t)c.merge_gap + 2) + 2) * sizeof(int2));  // starts lie more than g + 1 apart
  if (e == hipSuccess) e = hipMemset(h->d_state, 0, 2 * sizeof(DevState));
  return e;
}

int create_cfar(const pfb_cfar_config* cfg, pfb_cfar_handle** out) {
  pfb_cfar_plan plan{};
  int rc = cfar_check(cfg, &plan);
  if (rc != PFB_OK) return rc;
  int dev = 0;
  rc = pfb::resolve_device(cfg->device_id, &dev);
  if (rc != PFB_OK) return rc;
  pfb_cfar_handle* h = new pfb_cfar_handle();
  h->cfg = *cfg;
  h->device = dev;
  h->eb = elem_bytes(cfg->element);
  while ((1u << h->logC) < cfg->block_cells) ++h->logC;
  DeviceGuard g(dev);
  const hipError_t e = allocate_cfar(h);
  if (e != hipSuccess) {
    rc = pfb::hip_fail(e, "pfb_cfar_create allocation");
    free_cfar(h);
    return rc;
  }
  *out = h;
  return PFB_OK;
}

template <int E>
void launch_step(const CfarParams& p, bool sums, bool decide, bool carry, hipStream_t s) {
  if (sums) hipLaunchKernelGGL((cfar_sum<E>), dim3(grid_for((uint64_t)(p.nbc1 - p.nbc0) * std::max(p.C / 4, 1), 256, kMaxGrid)), dim3(256), 0, s, p);
  if (decide) {
    if (p.dec_blocks > 0) {
      hipLaunchKernelGGL(cfar_threshold, dim3(grid_for(p.dec_blocks, 256, kMaxGrid)), dim3(256), 0, s, p);
      hipLaunchKernelGGL((cfar_mask<E>), dim3(grid_for(((uint64_t)p.nwords + 3) / 4, 4, kMaxGrid)), dim3(256), 0, s, p);
    }
    const unsigned tiles = grid_for(p.ntiles, 1, kMaxGrid);
    hipLaunchKernelGGL(cfar_tile_last, dim3(tiles), dim3(256), 0, s, p);
    hipLaunchKernelGGL(cfar_tile_scan, dim3(1), dim3(256), 0, s, p);
    hipLaunchKernelGGL(cfar_word_starts, dim3(tiles), dim3(256), 0, s, p);
    hipLaunchKernelGGL(cfar_start_scan, dim3(1), dim3(256), 0, s, p);
    hipLaunchKernelGGL(cfar_write_starts, dim3(grid_for(p.nwords, 256, kMaxGrid)), dim3(256), 0, s, p);
    hipLaunchKernelGGL((cfar_runs<E>), dim3(1024), dim3(64), 0, s, p);
  }
  if (carry) hipLaunchKernelGGL((cfar_carry<E>), dim3(grid_for(std::max(p.keep_len, p.s_keep), 256, kMaxGrid)), dim3(256), 0, s, p);
}

// One step: m <= 2^24 device cells (or the flush), queued on the handle's stream; the host counters advance
int cfar_step(pfb_cfar_handle* h, const void* d_cells, uint64_t m, bool flush, pfb_cfar_det* d_det, uint64_t capacity) {
  HostCounters& hc = h->hc;
  const pfb_cfar_config& c = h->cfg;
  const uint64_t C = c.block_cells, GT = (uint64_t)c.guard_blocks + c.train_blocks;
  const uint64_t n1 = hc.n + m, nbc0 = hc.n >> h->logC, nbc1 = n1 >> h->logC;
  const uint64_t D1 = std::max(hc.D, nbc1 > GT ? nbc1 - GT : 0);
  const uint64_t base = hc.D * C, sb = hc.D > GT ? hc.D - GT : 0;
  const uint64_t view = n1 - base;
  CfarParams p{};
  p.call = d_cells;
  p.carry = h->d_cells[hc.slot];
  p.carry_out = h->d_cells[hc.slot ^ 1];
  p.S = h->d_S[hc.slot];
  p.S_out = h->d_S[hc.slot ^ 1];
  p.noise = h->d_noise;
  p.thr = h->d_thr;
  p.bflags = h->d_bflags;
  p.words = h->d_words;
  p.word_prev = h->d_word;
  p.word_off = h->d_word + h->max_words;
  p.tile_last = h->d_tile;
  p.tile_over = h->d_tile + h->max_tiles;
  p.tile_prev = h->d_tile + 2 * h->max_tiles;
  p.tile_starts = h->d_tile + 3 * h->max_tiles;
  p.tile_off = h->d_tile + 4 * h->max_tiles;
  p.starts = h->d_starts;
  p.st = h->d_state;
  p.sc = h->d_sc;
  p.det_out = d_det;
  p.capacity = capacity;
  p.base = base;
  p.D = (long long)hc.D;
  p.sb = (long long)sb;
  p.nbc0 = (long long)nbc0;
  p.nbc1 = (long long)nbc1;
  p.carry_len = (int)(hc.n - base);
  p.view_len = (int)view;
  p.C = (int)C;
  p.logC = h->logC;
  p.G = (int)c.guard_blocks;
  p.T = (int)c.train_blocks;
  p.method = (int)c.method;
  p.alpha = c.alpha;
  p.min_power = c.min_power;
  p.dec_cells = flush ? (int)view : (int)((D1 - hc.D) * C);
  p.dec_blocks = flush ? (int)((view + C - 1) / C) : (int)(D1 - hc.D);
  p.nwords = (p.dec_cells + 63) / 64;
  p.ntiles = (p.nwords + kTileWords - 1) / kTileWords;
  p.flush = flush ? 1 : 0;
  p.g = (int)c.merge_gap;
  p.rs = hc.rs;
  const uint64_t sb1 = D1 > GT ? D1 - GT : 0;
  p.keep_from = p.dec_cells;
  p.keep_len = (int)view - p.dec_cells;
  p.s_from = (int)(sb1 - sb);
  p.s_keep = flush ? 0 : (int)(nbc1 - sb1);
  const bool sums = nbc1 > nbc0, decide = flush || p.dec_cells > 0, carry = p.keep_len > 0 || p.s_keep > 0;
  if (c.element == PFB_CFAR_POWER) launch_step<PFB_CFAR_POWER>(p, sums, decide, carry, h->stream);
  else launch_step<PFB_CFAR_BANK_CELL>(p, sums, decide, carry, h->stream);
  HIP_TRY(hipGetLastError());
  if (sums) h->last_kernel = sum_tier(c.block_cells, c.element);
  if (flush) {  // blocks with both training sets empty: no lead block (b <= G), no complete block past the guard
    const uint64_t last = (n1 + C - 1) / C;
    for (uint64_t b = hc.D; b < last && b <= c.guard_blocks; ++b)
      if (nbc1 <= b + c.guard_blocks + 1) hc.without_noise += std::min(C, n1 - b * C);
    hc.flushed = true;
  }
  hc.n = n1;
  hc.D = flush ? (n1 + C - 1) / C : D1;
  if (carry) hc.slot ^= 1;
  if (decide) hc.rs ^= 1;
  return PFB_OK;
}

// the cells of one call in steps, device pointers, no host sync; the call's count ends in d_state->call_count
int cfar_enqueue(pfb_cfar_handle* h, const void* d_cells, uint64_t n, pfb_cfar_det* d_det, uint64_t capacity) {
  HIP_TRY(hipMemsetAsync(&h->d_state->call_count, 0, sizeof(unsigned long long), h->stream));
  for (uint64_t done = 0; done < n;) {
    const uint64_t m = std::min(kStepCells, n - done);
    const int rc = cfar_step(h, static_cast<const char*>(d_cells) + done * h->eb, m, false, d_det, capacity);
    if (rc != PFB_OK) return rc;
    done += m;
  }
  return PFB_OK;
}

int save_state(pfb_cfar_handle* h) {  // into slot 2, queued
  const HostCounters& hc = h->hc;
  const uint64_t C = h->cfg.block_cells, GT = (uint64_t)h->cfg.guard_blocks + h->cfg.train_blocks;
  const uint64_t cells = hc.flushed ? 0 : hc.n - hc.D * C, sums = hc.flushed ? 0 : (hc.n >> h->logC) - (hc.D > GT ? hc.D - GT : 0);
  if (cells) HIP_TRY(hipMemcpyAsync(h->d_cells[2], h->d_cells[hc.slot], cells * h->eb, hipMemcpyDeviceToDevice, h->stream));
  if (sums) HIP_TRY(hipMemcpyAsync(h->d_S[2], h->d_S[hc.slot], sums * sizeof(float), hipMemcpyDeviceToDevice, h->stream));
  HIP_TRY(hipMemcpyAsync(h->d_state + 1, h->d_state, sizeof(DevState), hipMemcpyDeviceToDevice, h->stream));
  return PFB_OK;
}

int restore_state(pfb_cfar_handle* h, const HostCounters& saved) {
  h->hc = saved;
  const HostCounters& hc = h->hc;
  const uint64_t C = h->cfg.block_cells, GT = (uint64_t)h->cfg.guard_blocks + h->cfg.train_blocks;
  const uint64_t cells = hc.flushed ? 0 : hc.n - hc.D * C, sums = hc.flushed ? 0 : (hc.n >> h->logC) - (hc.D > GT ? hc.D - GT : 0);
  if (cells) HIP_TRY(hipMemcpyAsync(h->d_cells[hc.slot], h->d_cells[2], cells * h->eb, hipMemcpyDeviceToDevice, h->stream));
  if (sums) HIP_TRY(hipMemcpyAsync(h->d_S[hc.slot], h->d_S[2], sums * sizeof(float), hipMemcpyDeviceToDevice, h->stream));
  HIP_TRY(hipMemcpyAsync(h->d_state, h->d_state + 1, sizeof(DevState), hipMemcpyDeviceToDevice, h->stream));
  HIP_TRY(hipStreamSynchronize(h->stream));
  return PFB_OK;
}

// pfb_cfar_process and pfb_cfar_flush: the steps, the count, and the state back where it was when the count does not fit
int cfar_sync_call(pfb_cfar_handle* h, const void* cells, uint64_t n, bool flush, pfb_cfar_det* det_out, uint64_t capacity,
                   uint64_t* count_out, uint32_t mem) {
  DeviceGuard g(h->device);
  const bool host = mem == PFB_MEM_HOST;
  const HostCounters saved = h->hc;
  int rc = save_state(h);
  if (rc != PFB_OK) return rc;
  pfb_cfar_det* d_det = det_out;
  uint64_t cap_dev = capacity;
  if (host) {  // no call closes more runs than it decides cells, plus the carried one
    cap_dev = std::min<uint64_t>(capacity, n + (saved.n - saved.D * h->cfg.block_cells) + 1);
    size_t have = h->det_cap * sizeof(pfb_cfar_det);
    rc = grow(reinterpret_cast<void**>(&h->d_det), &have, (size_t)std::max<uint64_t>(cap_dev, 1) * sizeof(pfb_cfar_det));
    h->det_cap = have / sizeof(pfb_cfar_det);
    if (rc == PFB_OK && n > 0) rc = grow(&h->d_stage, &h->stage_bytes, (size_t)std::min(n, kStepCells) * h->eb);
    if (rc != PFB_OK) return rc;
    d_det = h->d_det;
  }
  auto fail = [&](int code) {
    (void)hipStreamSynchronize(h->stream);
    (void)restore_state(h, saved);
    return code;
  };
  // from here on every failure goes through fail(): the state is put back before the call returns
  if (flush || host) {
    const hipError_t e0 = hipMemsetAsync(&h->d_state->call_count, 0, sizeof(unsigned long long), h->stream);
    if (e0 != hipSuccess) return fail(pfb::hip_fail(e0, "pfb_cfar_process"));
  }
  if (flush) {
    rc = cfar_step(h, nullptr, 0, true, d_det, cap_dev);
  } else if (!host) {
    rc = cfar_enqueue(h, cells, n, d_det, cap_dev);
  } else {
    for (uint64_t done = 0; done < n && rc == PFB_OK;) {
      const uint64_t m = std::min(kStepCells, n - done);
      hipError_t e = hipMemcpyAsync(h->d_stage, static_cast<const char*>(cells) + done * h->eb, m * h->eb, hipMemcpyHostToDevice, h->stream);
      if (e != hipSuccess) return fail(pfb::hip_fail(e, "pfb_cfar_process staging"));
      rc = cfar_step(h, h->d_stage, m, false, d_det, cap_dev);
      e = hipStreamSynchronize(h->stream);  // the one staging buffer is free again
      if (e != hipSuccess) return fail(pfb::hip_fail(e, "pfb_cfar_process"));
      done += m;
    }
  }
  if (rc != PFB_OK) return fail(rc);
  unsigned long long count = 0;
  hipError_t e = hipMemcpyAsync(&count, &h->d_state->call_count, sizeof(count), hipMemcpyDeviceToHost, h->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
  if (e != hipSuccess) return fail(pfb::hip_fail(e, "pfb_cfar_process"));
  *count_out = count;
  if (count > capacity) {
    rc = restore_state(h, saved);
    return rc != PFB_OK ? rc : PFB_ERR_CAPACITY;
  }
  if (host && count > 0) {
    e = hipMemcpy(det_out, d_det, (size_t)count * sizeof(pfb_cfar_det), hipMemcpyDeviceToHost);
    if (e != hipSuccess) return fail(pfb::hip_fail(e, "pfb_cfar_process records"));  // nothing delivered: nothing taken
  }
  return PFB_OK;
}

// what every process call checks before the device is touched
int cfar_check_call(const pfb_cfar_handle* h, const void* cells, uint64_t n, const void* det, uint64_t capacity,
                    const void* count_out, bool device) {
  if (!h || !count_out || (n > 0 && !cells) || (capacity > 0 && !det)) return PFB_ERR_BAD_ARG;
  if (n > ((uint64_t)1 << 62) || capacity > ((uint64_t)1 << 56) || h->hc.flushed) return PFB_ERR_BAD_ARG;
  if (device && ((reinterpret_cast<uintptr_t>(cells) % h->eb) || (reinterpret_cast<uintptr_t>(det) % 8))) return PFB_ERR_BAD_ARG;
  return PFB_OK;
}

}  // namespace

extern "C" int pfb_cfar_describe(const pfb_cfar_config* cfg, pfb_cfar_plan* plan_out) {
  return pfb::abi_guard([&]() -> int {
    pfb_cfar_plan plan{};
    const int rc = cfar_check(cfg, plan_out ? &plan : nullptr);
    if (rc == PFB_OK) *plan_out = plan;
    return rc;
  });
}

extern "C" int pfb_cfar_alpha(double pfa, uint64_t training_cells, double* alpha_out) {
  return pfb::abi_guard([&]() -> int {
    if (!alpha_out || !(pfa > 0.0 && pfa < 1.0) || training_cells < 1) return PFB_ERR_BAD_ARG;
    const double N = (double)training_cells;
    *alpha_out = N * (std::pow(pfa, -1.0 / N) - 1.0);
    return PFB_OK;
  });
}

extern "C" int pfb_cfar_create(const pfb_cfar_config* cfg, pfb_cfar_handle** out) {
  return pfb::abi_guard([&]() -> int {
    if (!out) return PFB_ERR_BAD_ARG;
    *out = nullptr;
    return create_cfar(cfg, out);
  });
}

extern "C" int pfb_cfar_destroy(pfb_cfar_handle* h) {
  return pfb::abi_guard([&]() -> int {
    if (!h) return PFB_ERR_BAD_ARG;
    free_cfar(h);
    return PFB_OK;
  });
}

extern "C" int pfb_cfar_reset(pfb_cfar_handle* h) {
  return pfb::abi_guard([&]() -> int {
    if (!h) return PFB_ERR_BAD_ARG;
    DeviceGuard g(h->device);
    HIP_TRY(hipMemsetAsync(h->d_state, 0, sizeof(DevState), h->stream));
    h->hc = HostCounters();
    return PFB_OK;
  });
}

extern "C" int pfb_cfar_set_stream(pfb_cfar_handle* h, void* hip_stream) {
  return pfb::abi_guard([&]() -> int {
    if (!h) return PFB_ERR_BAD_ARG;
    return pfb::switch_stream(h->device, &h->stream, &h->ev_switch, static_cast<hipStream_t>(hip_stream));
  });
}

extern "C" int pfb_cfar_sync(pfb_cfar_handle* h) {
  return pfb::abi_guard([&]() -> int {
    if (!h) return PFB_ERR_BAD_ARG;
    DeviceGuard g(h->device);
    HIP_TRY(hipStreamSynchronize(h->stream));
    return PFB_OK;
  });
}

extern "C" int pfb_cfar_get_device(const pfb_cfar_handle* h, int* device_id) {
  return pfb::abi_guard([&]() -> int {
    if (!h || !device_id) return PFB_ERR_BAD_ARG;
    *device_id = h->device;
    return PFB_OK;
  });
}

extern "C" int pfb_cfar_next_index(const pfb_cfar_handle* h, uint64_t* index_out) {
  return pfb::abi_guard([&]() -> int {
    if (!h || !index_out) return PFB_ERR_BAD_ARG;
    *index_out = h->hc.n;
    return PFB_OK;
  });
}

extern "C" int pfb_cfar_get_stats(pfb_cfar_handle* h, pfb_cfar_stats* stats_out) {
  return pfb::abi_guard([&]() -> int {
    if (!h || !stats_out) return PFB_ERR_BAD_ARG;
    DeviceGuard g(h->device);
    DevState st;
    HIP_TRY(hipMemcpyAsync(&st, h->d_state, sizeof(st), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    const HostCounters& hc = h->hc;
    stats_out->cells_in = hc.n;
    stats_out->cells_decided = hc.flushed ? hc.n : hc.D * h->cfg.block_cells;
    stats_out->cells_over = st.cells_over;
    stats_out->cells_without_noise = hc.without_noise;
    stats_out->detections = st.detections;
    stats_out->dropped = st.dropped;
    stats_out->open_run = st.run[hc.rs].open;
    return PFB_OK;
  });
}

extern "C" int pfb_cfar_process(pfb_cfar_handle* h, const void* cells, uint64_t num_cells, pfb_cfar_det* det_out,
                                uint64_t capacity, uint64_t* count_out, uint32_t mem) {
  return pfb::abi_guard([&]() -> int {
    if (mem > PFB_MEM_DEVICE) return PFB_ERR_BAD_ARG;
    const int rc = cfar_check_call(h, cells, num_cells, det_out, capacity, count_out, mem == PFB_MEM_DEVICE);
    if (rc != PFB_OK) return rc;
    return cfar_sync_call(h, cells, num_cells, false, det_out, capacity, count_out, mem);
  });
}

extern "C" int pfb_cfar_flush(pfb_cfar_handle* h, pfb_cfar_det* det_out, uint64_t capacity, uint64_t* count_out, uint32_t mem) {
  return pfb::abi_guard([&]() -> int {
    if (mem > PFB_MEM_DEVICE || !h || !count_out || (capacity > 0 && !det_out) || capacity > ((uint64_t)1 << 56))
      return PFB_ERR_BAD_ARG;
    if (mem == PFB_MEM_DEVICE && reinterpret_cast<uintptr_t>(det_out) % 8) return PFB_ERR_BAD_ARG;
    if (h->hc.flushed) {  // nothing is left
      *count_out = 0;
      return PFB_OK;
    }
    return cfar_sync_call(h, nullptr, 0, true, det_out, capacity, count_out, mem);
  });
}

extern "C" int pfb_cfar_process_async(pfb_cfar_handle* h, const void* d_cells, uint64_t num_cells, pfb_cfar_det* d_det_out,
                                      uint64_t capacity, uint64_t* d_count_out) {
  return pfb::abi_guard([&]() -> int {
    int rc = cfar_check_call(h, d_cells, num_cells, d_det_out, capacity, d_count_out, true);
    if (rc != PFB_OK) return rc;
    if (reinterpret_cast<uintptr_t>(d_count_out) % 8) return PFB_ERR_BAD_ARG;
    DeviceGuard g(h->device);
    rc = cfar_enqueue(h, d_cells, num_cells, d_det_out, capacity);
    if (rc != PFB_OK) return rc;
    HIP_TRY(hipMemcpyAsync(d_count_out, &h->d_state->call_count, sizeof(uint64_t), hipMemcpyDeviceToDevice, h->stream));
    return PFB_OK;
  });
}

extern "C" int pfb_cfar_to_pdw(const pfb_cfar_det* dets, uint64_t n, double fs, double fc, double sample_start_time,
                               double bin_hz, int32_t first_bin, uint32_t bin_step, pfb_pdw* pdw_out) {
  return pfb::abi_guard([&]() -> int {
    if ((n > 0 && (!dets || !pdw_out)) || !std::isfinite(fs) || !(fs > 0.0)) return PFB_ERR_BAD_ARG;
    for (uint64_t k = 0; k < n; ++k) {
      const pfb_cfar_det& d = dets[k];
      pfb_pdw& w = pdw_out[k];
      w.toa = (double)(d.peak_index + 1) / fs + sample_start_time;
      w.pw = (double)(d.last_index - d.first_index + 1) / fs;
      w.snr = 10.0 * std::log10((double)d.peak_power / (double)d.noise);
      w.mag = std::sqrt((double)d.peak_power);
      w.freq = d.hypothesis >= 0 ? fc + ((double)first_bin + (double)d.hypothesis) * (double)bin_step * bin_hz : fc;
      w.sat = 0;
      w.bin = d.hypothesis;
    }
    return PFB_OK;
  });
}

extern "C" const char* pfb_cfar_last_kernel(const pfb_cfar_handle* h) { return h ? h->last_kernel : ""; }
