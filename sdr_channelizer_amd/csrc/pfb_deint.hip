// pfb_deint.hip -- PDW deinterleaver (pfb_deint_* in include/pfb_channelizer.h, where every figure is defined): emitters
// from a time-ordered list of arrival ticks, kernels and host side.
//   deint_count / list_scan / deint_scatter   the alive list of a round: flags (label == -1), a scan of the workgroups'
//                     counts, an ordered scatter of (tick, original index).  The first round's count pass also checks
//                     the list's order and the ticks' bound.
//   deint_hist<LDS>   a workgroup stages tiles of 1024 consecutive alive ticks plus Lv more in LDS (16-byte loads) and
//                     walks the levels; at one level its lanes take consecutive i, so the LDS reads are conflict free.
//                     The list is sorted: once no pair of a tile is within pmax at a level, none is at a deeper one,
//                     and the workgroup leaves the tile.  LDS = true counts in a private LDS histogram that is added to
//                     the global one once, when the workgroup has walked all its tiles; LDS = false adds straight into
//                     the global one.  Integer adds commute: the counts do not depend on the order.
//   deint_succ        one lane per alive pulse: the first entry at or over each target by a probe of the next 8 entries
//                     and then a galloping binary search (the list is L2 resident), its left neighbour, the lowest
//                     index among duplicates.
//   deint_double      pointer doubling over (jump, hops, periods), 16 bytes an entry, from one table into the other; a
//                     pulse without a successor points to itself with 0 hops, so that a jump past the end stays there.
//   deint_argmax / deint_pick   the largest (hops, lowest index) as one 64-bit key, reduced per workgroup and then by
//                     an integer atomic max; one lane turns the key into the record's figures.
//   deint_mark_tables / deint_mark_walk   the labels of b's chain: lane q takes the q-th pulse of the chain by the bits
//                     of q through the kept jump tables of every doubling round (what the library runs: 2 to 50 times
//                     faster over a whole search), or one lane along succ
//                     (pfb_deint_set_tier, for tests and meter).
// The decision of every round (candidates, accept or refuse) is taken on the host from the copied histogram.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <new>
#include <numeric>
#include <string>
#include <vector>

#include "pfb_list.hpp"

namespace {

constexpr uint32_t kMaxPulses = 1u << 20, kMaxBins = 1u << 16, kMaxLevel = 256;
constexpr uint32_t kLdsBins = 8192;      // the LDS tier's bound
constexpr uint32_t kTile = 1024;         // alive pulses of one histogram tile, and of one compaction workgroup
constexpr unsigned kHistGrid = 1024;     // workgroups of the histogram at most: four to a CU
constexpr u64 kMaxTick = 1ull << 62;
constexpr int kMaxRounds = 20;           // doubling rounds for 2^20 pulses

struct Control {            // what a round hands back to the host
  u64 first, last;          // a[0], a[n-1] of the alive list
  u64 best;                 // deint_argmax's key
  uint32_t bad, pad;        // the list is out of order or holds a tick >= 2^62
  // deint_pick
  u64 first_tick, last_tick;
  uint32_t b, hops, per, first_pulse;
};
static_assert(sizeof(Control) == 64, "deint_scatter, deint_argmax and deint_pick write it by these offsets");

struct CompactParams {
  const u64* t;             // the caller's list
  const int32_t* labels;    // -1: alive
  uint32_t* counts;         // alive pulses of every workgroup, then (list_scan) those before it
  u64* a;                   // the alive ticks ...
  uint32_t* idx;            // ... and their indices in the caller's list
  Control* ctl;
  uint32_t n, alive, check;
};
static_assert(sizeof(CompactParams) == 64, "the kernels' parameter layout");

// a lane takes 4 consecutive pulses, a workgroup kTile
__device__ __forceinline__ void alive_of(const CompactParams& p, uint32_t i0, bool live[4]) {
  const int4 l = *reinterpret_cast<const int4*>(p.labels + i0);  // the labels are padded to a whole tile
  live[0] = i0 + 0 < p.n && l.x < 0;
  live[1] = i0 + 1 < p.n && l.y < 0;
  live[2] = i0 + 2 < p.n && l.z < 0;
  live[3] = i0 + 3 < p.n && l.w < 0;
}

__global__ void __launch_bounds__(kThreads) deint_count(const CompactParams p) {
  const uint32_t i0 = blockIdx.x * kTile + threadIdx.x * 4;
  bool live[4];
  alive_of(p, i0, live);
  if (p.check) {
    bool bad = false;
    for (uint32_t k = 0; k < 4; ++k) {
      const uint32_t i = i0 + k;
      if (i >= p.n) break;
      const u64 v = p.t[i];
      bad |= v >= kMaxTick || (i > 0 && v < p.t[i - 1]);
    }
    if (bad) atomicOr(&p.ctl->bad, 1u);
  }
  uint32_t total;
  (void)block_scan((uint32_t)live[0] + live[1] + live[2] + live[3], &total);
  if (threadIdx.x == 0) p.counts[blockIdx.x] = total;
}

__global__ void __launch_bounds__(kThreads) deint_scatter(const CompactParams p) {
  const uint32_t i0 = blockIdx.x * kTile + threadIdx.x * 4;
  bool live[4];
  alive_of(p, i0, live);
  uint32_t total;
  uint32_t at = p.counts[blockIdx.x] + block_scan((uint32_t)live[0] + live[1] + live[2] + live[3], &total);
  for (uint32_t k = 0; k < 4; ++k) {
    if (!live[k]) continue;
    const u64 v = p.t[i0 + k];
    p.a[at] = v;
    p.idx[at] = i0 + k;
    if (at == 0) p.ctl->first = v;
    if (at == p.alive - 1) p.ctl->last = v;
    ++at;
  }
}

struct HistParams {
  const u64* a;             // the alive ticks, 16-byte aligned
  uint32_t* C;              // NB counts, zeroed
  uint32_t n, tiles;
  uint32_t pmin, W, NB, Lv;
  u64 pmax;
};
static_assert(sizeof(HistParams) == 48, "the kernels' parameter layout");

template <bool LDS>
__global__ void __launch_bounds__(kThreads) deint_hist(const HistParams p) {
  __shared__ u64 s_t[kTile + kMaxLevel];
  __shared__ uint32_t s_h[LDS ? kLdsBins : 1];
  if (LDS)
    for (uint32_t k = threadIdx.x; k < p.NB; k += kThreads) s_h[k] = 0;
  for (uint32_t tile = blockIdx.x; tile < p.tiles; tile += gridDim.x) {
    const uint32_t base = tile * kTile;
    const uint32_t staged = min(kTile + p.Lv, p.n - base);
    const uint32_t mine = min(kTile, p.n - base);
    __syncthreads();  // the tile before is read, the histogram is zero
    const u64* src = p.a + base;  // base is even: 16-byte aligned
    for (uint32_t v = threadIdx.x; 2 * v < staged; v += kThreads) {
      if (2 * v + 1 < staged) {
        const ulonglong2 w = *reinterpret_cast<const ulonglong2*>(src + 2 * v);
        s_t[2 * v] = w.x;
        s_t[2 * v + 1] = w.y;
      } else {
        s_t[2 * v] = src[2 * v];
      }
    }
    __syncthreads();
    for (uint32_t level = 1; level <= p.Lv; ++level) {
      int near = 0;  // a pair of this level within pmax
      for (uint32_t i = threadIdx.x; i < mine; i += kThreads) {
        const uint32_t j = i + level;
        if (j >= staged) break;
        const u64 d = s_t[j] - s_t[i];
        if (d > p.pmax) continue;
        near = 1;
        if (d < p.pmin) continue;
        const uint32_t k = ((uint32_t)d - p.pmin) / p.W;
        if (LDS) atomicAdd(&s_h[k], 1u); else atomicAdd(&p.C[k], 1u);
      }
      if (!__syncthreads_or(near)) break;  // sorted: no deeper level has one either
    }
  }
  if (LDS) {
    __syncthreads();
    for (uint32_t k = threadIdx.x; k < p.NB; k += kThreads)
      if (s_h[k]) atomicAdd(&p.C[k], s_h[k]);
  }
}

// the first index in [lo, n) with a[index] >= key, n when there is none: most successors lie a few entries on
__device__ __forceinline__ uint32_t first_at_or_over(const u64* a, uint32_t lo, uint32_t n, u64 key) {
  for (int k = 0; k < 8; ++k) {
    if (lo >= n || a[lo] >= key) return lo;
    ++lo;
  }
  uint32_t width = 16;  // every entry before lo is under key
  while (lo + width <= n && a[lo + width - 1] < key) {
    lo += width;
    width <<= 1;
  }
  uint32_t hi = min(lo + width, n);
  while (lo < hi) {
    const uint32_t mid = (lo + hi) >> 1;
    if (a[mid] < key) lo = mid + 1; else hi = mid;
  }
  return lo;
}

struct SuccParams {
  const u64* a;
  int32_t* succ;   // -1: none
  int32_t* step;   // 0: none
  int4* table;     // (jump, hops, periods, 0) of one step
  u64 tau, e;
  uint32_t n, X;
};
static_assert(sizeof(SuccParams) == 56, "the kernels' parameter layout");

__global__ void __launch_bounds__(kThreads) deint_succ(const SuccParams p) {
  const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
  if (i >= p.n) return;
  const u64 ai = p.a[i];
  int32_t s = -1, st = 0;
  uint32_t from = i + 1;
  for (uint32_t m = 0; m <= p.X; ++m) {
    const u64 target = ai + (u64)(m + 1) * p.tau, w = (u64)(m + 1) * p.e;
    const uint32_t at = first_at_or_over(p.a, from, p.n, target);
    from = at;  // the next target lies further on
    u64 dist = ~0ull;
    if (at < p.n && p.a[at] - target <= w) {  // the smallest value at or over the target, at its lowest index
      s = (int32_t)at;
      dist = p.a[at] - target;
    }
    if (at > i + 1) {  // the largest value under the target; inside the window it lies after a[i]
      const u64 v = p.a[at - 1];
      if (target - v <= w && target - v <= dist) {  // a tie goes to the lower index
        uint32_t q = at - 1;
        if (q > i + 1 && p.a[q - 1] == v) q = first_at_or_over(p.a, i + 1, q, v);  // duplicates: the lowest of them
        s = (int32_t)q;
      }
    }
    if (s >= 0) {
      st = (int32_t)(m + 1);
      break;
    }
  }
  p.succ[i] = s;
  p.step[i] = st;
  p.table[i] = make_int4(s < 0 ? (int)i : s, s < 0 ? 0 : 1, st, 0);
}

// out = in after twice the hops; level (when kept): in's jumps
__global__ void __launch_bounds__(kThreads) deint_double(const int4* in, int4* out, int32_t* level, uint32_t n) {
  const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
  if (i >= n) return;
  const int4 x = in[i];
  const int4 y = in[x.x];
  out[i] = make_int4(y.x, x.y + y.y, x.z + y.z, 0);
  if (level) level[i] = x.x;
}

__global__ void __launch_bounds__(kThreads) deint_argmax(const int4* table, uint32_t n, Control* ctl) {
  __shared__ u64 sh[kThreads / 64];
  u64 best = 0;
  for (uint32_t i = blockIdx.x * kThreads + threadIdx.x; i < n; i += gridDim.x * kThreads) {
    const u64 key = ((u64)(uint32_t)table[i].y << 32) | (0xffffffffu - i);  // more hops, then the lower index
    best = max(best, key);
  }
  for (int d = 32; d >= 1; d >>= 1) best = max(best, (u64)__shfl_xor(best, d, 64));
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = best;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int k = 1; k < kThreads / 64; ++k) best = max(best, sh[k]);
    atomicMax(&ctl->best, best);
  }
}

__global__ void deint_pick(const int4* table, const u64* a, const uint32_t* idx, Control* ctl) {
  const uint32_t b = 0xffffffffu - (uint32_t)(ctl->best & 0xffffffffu);
  const int4 x = table[b];
  ctl->b = b;
  ctl->hops = (uint32_t)x.y;
  ctl->per = (uint32_t)x.z;
  ctl->first_pulse = idx[b];
  ctl->first_tick = a[b];
  ctl->last_tick = a[x.x];
}

__global__ void deint_mark_walk(const int32_t* succ, const uint32_t* idx, int32_t* labels, uint32_t b, int32_t E) {
  for (int32_t j = (int32_t)b; j >= 0; j = succ[j]) labels[idx[j]] = E;
}

// lane q labels the q-th pulse of b's chain: a jump of 2^k for every bit k of q; levels[k] holds the jumps of 2^k
__global__ void __launch_bounds__(kThreads) deint_mark_tables(const int32_t* levels, uint32_t stride, int rounds,
                                                              const int4* table, const uint32_t* idx, int32_t* labels,
                                                              uint32_t b, uint32_t hops, int32_t E) {
  const uint32_t q = blockIdx.x * kThreads + threadIdx.x;
  if (q > hops) return;
  int32_t j = (int32_t)b;
  if (q == hops) {
    j = table[b].x;  // the end: hops may be 2^rounds itself
  } else {
    for (int k = 0; k < rounds; ++k)
      if ((q >> k) & 1) j = levels[(size_t)k * stride + j];
  }
  labels[idx[j]] = E;
}

__global__ void __launch_bounds__(kThreads) deint_lengths(const int4* table, int32_t* len, uint32_t n) {
  const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
  if (i < n) len[i] = table[i].y + 1;
}

// ---------------------------------------------------------------------------------
// host: checks and plan

enum { kMarkAuto = 0, kMarkWalk = 1, kMarkTables = 2 };  // the histogram's tiers are kTier*

struct Settings {
  uint32_t pmin = 0, W = 0, NB = 0, Lv = 0, detect = 0, min_pulses = 0, X = 0, fill = 0, max_emitters = 0;
  u64 pmax = 0, e = 0;
};

struct Arrays {             // a handle's scratch
  u64* t;                   // a host list on its way in
  int32_t* labels;          // -1: alive; padded to a whole kTile
  u64* a;                   // the alive ticks ...
  uint32_t* idx;            // ... and their indices in the caller's list
  int32_t* succ;
  int32_t* step;
  int32_t* len;
  int4* table0;             // the doubling goes from one table into the other
  int4* table1;
  uint32_t* counts;         // alive pulses of every compaction workgroup
  uint32_t* hist;           // NB counts
  Control* ctl;
};

// the carving of a handle's scratch for lists of up to cap pulses, cap a multiple of kTile: every array once
Arrays carve(Carver& c, size_t cap, uint32_t NB) {
  Arrays s{};
  s.t = c.array<u64>(cap);
  s.labels = c.array<int32_t>(cap);
  s.a = c.array<u64>(cap);
  s.idx = c.array<uint32_t>(cap);
  s.succ = c.array<int32_t>(cap);
  s.step = c.array<int32_t>(cap);
  s.len = c.array<int32_t>(cap);
  s.table0 = c.array<int4>(cap);
  s.table1 = c.array<int4>(cap);
  s.counts = c.array<uint32_t>(kMaxPulses / kTile);
  s.hist = c.array<uint32_t>(NB);
  s.ctl = c.array<Control>(1);
  return s;
}

size_t scratch_bytes(size_t cap, uint32_t NB) {
  Carver c;
  carve(c, cap, NB);
  return c.bytes();
}

size_t capacity_for(uint64_t n) { return round_up(std::max<uint64_t>(n, 1), kTile); }
// the jump tables of every doubling round, kept for the marking pass of pfb_deint_run
size_t level_bytes(size_t cap) { return (size_t)kMaxRounds * cap * sizeof(int32_t); }

const char* hist_name(bool lds) { return lds ? "pfb_deint_hist_lds" : "pfb_deint_hist_global"; }
const char* mark_name(bool tables) { return tables ? "pfb_deint_mark_tables" : "pfb_deint_mark_walk"; }

// Everything pfb_deint_describe and pfb_deint_create check before the device, in the order the header states
int deint_check(const pfb_deint_config* cfg, Settings* s) {
  if (!cfg || !s || cfg->struct_size != sizeof(pfb_deint_config)) return PFB_ERR_BAD_ARG;
  if (cfg->min_period < 1 || cfg->max_period < cfg->min_period || cfg->max_period > (1u << 31)) return PFB_ERR_BAD_ARG;
  if (cfg->bin_ticks < 1) return PFB_ERR_BAD_ARG;
  const uint64_t NB = (uint64_t)(cfg->max_period - cfg->min_period) / cfg->bin_ticks + 1;
  if (NB > kMaxBins) return PFB_ERR_BAD_ARG;
  if (cfg->max_level < 1 || cfg->max_level > kMaxLevel) return PFB_ERR_BAD_ARG;
  if (cfg->detect_percent < 1 || cfg->detect_percent > 100) return PFB_ERR_BAD_ARG;
  if (cfg->min_pulses < 3 || cfg->min_pulses > kMaxPulses) return PFB_ERR_BAD_ARG;
  if (cfg->max_missing > 8) return PFB_ERR_BAD_ARG;
  const uint64_t e = cfg->tolerance ? cfg->tolerance : cfg->bin_ticks;
  if (e * (2 * (uint64_t)cfg->max_missing + 3) >= cfg->min_period) return PFB_ERR_BAD_ARG;
  if (cfg->fill_percent < 1 || cfg->fill_percent > 100) return PFB_ERR_BAD_ARG;
  if (cfg->max_emitters < 1 || cfg->max_emitters > 1024) return PFB_ERR_BAD_ARG;
  if (cfg->flags != 0) return PFB_ERR_BAD_ARG;
  s->pmin = cfg->min_period;
  s->pmax = cfg->max_period;
  s->W = cfg->bin_ticks;
  s->NB = (uint32_t)NB;
  s->Lv = cfg->max_level;
  s->detect = cfg->detect_percent;
  s->min_pulses = cfg->min_pulses;
  s->X = cfg->max_missing;
  s->e = e;
  s->fill = cfg->fill_percent;
  s->max_emitters = cfg->max_emitters;
  return PFB_OK;
}

}  // namespace

struct pfb_deint_handle : ListHandle {
  Settings s;
  int hist_tier = kTierAuto, mark_tier = kMarkAuto;
  int32_t* d_levels = nullptr;  // the marking tables: kMaxRounds x level_cap jumps
  size_t level_cap = 0;
  pfb_deint_stats stats{};
  std::vector<uint32_t> hist;   // a round's histogram on the host
  void release() {
    DeviceGuard g(device);
    (void)hipFree(d_levels);
    ListHandle::release();
  }
};

namespace {

bool runs_lds(const pfb_deint_handle* h) { return h->hist_tier == kTierAuto ? h->s.NB <= kLdsBins : h->hist_tier == kTierLds; }
// the kept tables wherever they were measured, which is everywhere; kMarkWalk is for tests and meter
bool runs_tables(const pfb_deint_handle* h) { return h->mark_tier != kMarkWalk; }

// one call's view of the scratch
struct Call : ListCall {
  pfb_deint_handle* h;
  Arrays scr;
  const u64* d_t = nullptr;  // the list on the device
  uint32_t n = 0;
  Call(pfb_deint_handle* hh) : h(hh) {
    Carver c{hh->d_scratch};
    scr = carve(c, hh->cap, hh->s.NB);
  }
};

// the scratch for a list of n pulses; levels: the marking tables too
int reserve(pfb_deint_handle* h, uint64_t n, bool levels = false) {
  const size_t cap = capacity_for(n);
  const int rc = cap > h->cap ? h->ensure(cap, scratch_bytes(cap, h->s.NB)) : PFB_OK;  // the size only when it grows
  if (rc != PFB_OK) return rc;
  if (levels && runs_tables(h) && h->level_cap < h->cap) {
    (void)hipFree(h->d_levels);
    h->d_levels = nullptr;
    h->level_cap = 0;
    HIP_TRY(hipMalloc(reinterpret_cast<void**>(&h->d_levels), level_bytes(h->cap)));
    h->level_cap = h->cap;
  }
  return PFB_OK;
}

// the alive list of a round: `alive` pulses have label -1.  check: the first round, which also reads the list's order
int compact(Call& c, uint32_t alive, bool check) {
  CompactParams p{};
  p.t = c.d_t;
  p.labels = c.scr.labels;
  p.counts = c.scr.counts;
  p.a = c.scr.a;
  p.idx = c.scr.idx;
  p.ctl = c.scr.ctl;
  p.n = c.n;
  p.alive = alive;
  p.check = check ? 1u : 0u;
  const unsigned blocks = (c.n + kTile - 1) / kTile;
  hipLaunchKernelGGL(deint_count, dim3(blocks), dim3(kThreads), 0, c.h->stream, p);
  hipLaunchKernelGGL(list_scan<false>, dim3(1), dim3(kThreads), 0, c.h->stream, p.counts, blocks, (uint32_t*)nullptr);
  hipLaunchKernelGGL(deint_scatter, dim3(blocks), dim3(kThreads), 0, c.h->stream, p);
  HIP_TRY(hipGetLastError());
  c.ran("pfb_deint_compact");
  return PFB_OK;
}

// The list onto the device, every label -1, the first alive list; PFB_ERR_BAD_ARG for a list the device refuses
int begin_call(Call& c, const uint64_t* ticks, uint64_t n, uint32_t mem, Control* ctl) {
  pfb_deint_handle* h = c.h;
  c.n = (uint32_t)n;
  if (mem == PFB_MEM_HOST) {
    HIP_TRY(hipMemcpyAsync(c.scr.t, ticks, n * sizeof(u64), hipMemcpyHostToDevice, h->stream));
    c.d_t = c.scr.t;
  } else {
    c.d_t = reinterpret_cast<const u64*>(ticks);
  }
  HIP_TRY(hipMemsetAsync(c.scr.labels, 0xff, h->cap * sizeof(int32_t), h->stream));
  HIP_TRY(hipMemsetAsync(c.scr.ctl, 0, sizeof(Control), h->stream));
  int rc = compact(c, c.n, true);
  if (rc != PFB_OK) return rc;
  rc = fetch(c.h->stream, c.scr.ctl, ctl);
  if (rc != PFB_OK) return rc;
  return ctl->bad ? PFB_ERR_BAD_ARG : PFB_OK;
}

int histogram(Call& c, uint32_t alive) {
  pfb_deint_handle* h = c.h;
  HistParams p{};
  p.a = c.scr.a;
  p.C = c.scr.hist;
  p.n = alive;
  p.tiles = (alive + kTile - 1) / kTile;
  p.pmin = h->s.pmin;
  p.pmax = h->s.pmax;
  p.W = h->s.W;
  p.NB = h->s.NB;
  p.Lv = h->s.Lv;
  HIP_TRY(hipMemsetAsync(p.C, 0, (size_t)p.NB * sizeof(uint32_t), h->stream));
  if (alive == 0) return PFB_OK;
  const dim3 grid(std::min(p.tiles, kHistGrid)), block(kThreads);
  const bool lds = runs_lds(h);
  if (lds) hipLaunchKernelGGL(deint_hist<true>, grid, block, 0, h->stream, p);
  else hipLaunchKernelGGL(deint_hist<false>, grid, block, 0, h->stream, p);
  HIP_TRY(hipGetLastError());
  c.ran(hist_name(lds));
  return PFB_OK;
}

// steps 3 and 4 at one period on the alive list: the final table (jump = end, hops, periods) is the one returned
int chains(Call& c, uint32_t alive, u64 tau, u64 span, bool keep, const int4** table_out, int* rounds_out) {
  pfb_deint_handle* h = c.h;
  SuccParams p{};
  p.a = c.scr.a;
  p.succ = c.scr.succ;
  p.step = c.scr.step;
  p.table = c.scr.table0;
  p.tau = tau;
  p.e = h->s.e;
  p.n = alive;
  p.X = h->s.X;
  const dim3 grid((alive + kThreads - 1) / kThreads), block(kThreads);
  hipLaunchKernelGGL(deint_succ, grid, block, 0, h->stream, p);
  // a hop advances by tau - e at least: no chain has more than span / (tau - e) of them
  const u64 most = std::min<u64>(alive - 1, span / (tau - h->s.e));
  int rounds = 0;
  while ((1ull << rounds) < most) ++rounds;
  int4* in = c.scr.table0;
  int4* out = c.scr.table1;
  for (int r = 0; r < rounds; ++r) {
    hipLaunchKernelGGL(deint_double, grid, block, 0, h->stream, in, out, keep ? h->d_levels + (size_t)r * h->level_cap : nullptr,
                       alive);
    std::swap(in, out);
  }
  HIP_TRY(hipGetLastError());
  c.ran("pfb_deint_succ");
  if (rounds) c.ran("pfb_deint_double");
  *table_out = in;
  *rounds_out = rounds;
  return PFB_OK;
}

// ceil(floor(span / tau) percent / 100) without leaving 64 bits
u64 expected_pairs(u64 span, u64 tau, uint32_t percent) {
  const u64 q = span / tau;
  return (q / 100) * percent + ((q % 100) * percent + 99) / 100;
}

int run(pfb_deint_handle* h, const uint64_t* ticks, uint64_t n, uint32_t mem, pfb_deint_emitter* emitters_out,
        uint64_t capacity, uint64_t* count_out, int32_t* labels_out) {
  const Settings& s = h->s;
  DeviceGuard g(h->device);
  std::vector<pfb_deint_emitter> found;
  pfb_deint_stats stats{};
  if (n == 0) {
    *count_out = 0;
    h->stats = stats;
    h->last_kernel.clear();
    return PFB_OK;
  }
  int rc = reserve(h, n, true);
  if (rc != PFB_OK) return rc;
  Call c(h);
  Control ctl{};
  rc = begin_call(c, ticks, n, mem, &ctl);
  if (rc != PFB_OK) return rc;
  uint32_t alive = (uint32_t)n;
  h->hist.resize(s.NB);
  for (bool first = true; found.size() < s.max_emitters && alive >= s.min_pulses; first = false) {
    if (!first) {
      rc = compact(c, alive, false);
      if (rc != PFB_OK) return rc;
    }
    rc = histogram(c, alive);
    if (rc != PFB_OK) return rc;
    HIP_TRY(hipMemcpyAsync(h->hist.data(), c.scr.hist, (size_t)s.NB * sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream));
    rc = fetch(c.h->stream, c.scr.ctl, &ctl);
    if (rc != PFB_OK) return rc;
    ++stats.rounds;
    const u64 span = ctl.last - ctl.first;
    const std::vector<uint32_t>& C = h->hist;
    bool accepted = false;
    for (uint32_t k = 0; k < s.NB && !accepted; ++k) {
      const u64 left = k > 0 ? C[k - 1] : 0, right = k + 1 < s.NB ? C[k + 1] : 0;
      if (!(C[k] > left && C[k] >= right)) continue;
      const u64 tau = (u64)s.pmin + (u64)k * s.W + s.W / 2, sum = left + C[k] + right;
      if (sum < std::max<u64>(s.min_pulses - 1, expected_pairs(span, tau, s.detect))) continue;
      ++stats.candidates_tried;
      const int4* table = nullptr;
      int rounds = 0;
      rc = chains(c, alive, tau, span, runs_tables(h), &table, &rounds);
      if (rc != PFB_OK) return rc;
      HIP_TRY(hipMemsetAsync(&c.scr.ctl->best, 0, sizeof(u64), h->stream));
      hipLaunchKernelGGL(deint_argmax, dim3(std::min((alive + kThreads - 1) / kThreads, 1024u)), dim3(kThreads), 0, h->stream,
                         table, alive, c.scr.ctl);
      hipLaunchKernelGGL(deint_pick, dim3(1), dim3(1), 0, h->stream, table, c.scr.a, c.scr.idx, c.scr.ctl);
      HIP_TRY(hipGetLastError());
      c.ran("pfb_deint_argmax");
      rc = fetch(c.h->stream, c.scr.ctl, &ctl);
      if (rc != PFB_OK) return rc;
      const u64 len = (u64)ctl.hops + 1;
      if (len < s.min_pulses || 100 * (len - 1) < (u64)s.fill * ctl.per) {
        ++stats.candidates_refused;
        continue;
      }
      const int32_t E = (int32_t)found.size();
      int32_t* labels = c.scr.labels;
      if (runs_tables(h))
        hipLaunchKernelGGL(deint_mark_tables, dim3((unsigned)((len + kThreads - 1) / kThreads)), dim3(kThreads), 0, h->stream,
                           h->d_levels, (uint32_t)h->level_cap, rounds, table, c.scr.idx, labels, ctl.b,
                           ctl.hops, E);
      else
        hipLaunchKernelGGL(deint_mark_walk, dim3(1), dim3(1), 0, h->stream, c.scr.succ, c.scr.idx, labels, ctl.b, E);
      HIP_TRY(hipGetLastError());
      c.ran(mark_name(runs_tables(h)));
      pfb_deint_emitter rec{};
      rec.first_tick = ctl.first_tick;
      rec.last_tick = ctl.last_tick;
      rec.period = (double)(ctl.last_tick - ctl.first_tick) / (double)ctl.per;
      rec.pulses = (uint32_t)len;
      rec.periods = ctl.per;
      rec.bin = k;
      rec.candidate_period = (uint32_t)tau;
      rec.first_pulse = ctl.first_pulse;
      rec.hist_count = (uint32_t)sum;
      found.push_back(rec);
      alive -= (uint32_t)len;
      stats.pulses_assigned += len;
      accepted = true;
    }
    if (!accepted) break;
  }
  *count_out = found.size();
  if (found.size() > capacity) {
    HIP_TRY(hipStreamSynchronize(h->stream));
    return PFB_ERR_CAPACITY;
  }
  if (!found.empty()) {
    if (mem == PFB_MEM_DEVICE)
      HIP_TRY(hipMemcpyAsync(emitters_out, found.data(), found.size() * sizeof(pfb_deint_emitter), hipMemcpyHostToDevice,
                             h->stream));
    else
      std::memcpy(emitters_out, found.data(), found.size() * sizeof(pfb_deint_emitter));
  }
  rc = copy_out(h->stream, labels_out, c.scr.labels, n * sizeof(int32_t), mem);
  if (rc != PFB_OK) return rc;
  HIP_TRY(hipStreamSynchronize(h->stream));
  h->stats = stats;
  h->last_kernel = c.kernels;
  return PFB_OK;
}

}  // namespace

extern "C" int pfb_deint_describe(const pfb_deint_config* cfg, uint64_t n, pfb_deint_plan* plan_out) {
  return pfb::abi_guard([&]() -> int {
    Settings s;
    const int rc = deint_check(cfg, plan_out ? &s : nullptr);
    if (rc != PFB_OK) return rc;
    if (n > kMaxPulses) return PFB_ERR_BAD_ARG;
    pfb_deint_plan plan{};
    plan.scratch_bytes = scratch_bytes(capacity_for(n), s.NB) + level_bytes(capacity_for(n));
    plan.num_bins = s.NB;
    plan.lds_bins = kLdsBins;
    plan.tile_pulses = kTile;
    const bool lds = s.NB <= kLdsBins;
    plan.lds_bytes = (kTile + kMaxLevel) * 8 + (lds ? kLdsBins * 4 : 4);
    plan.successor_threads = kThreads;
    std::snprintf(plan.histogram_kernel, sizeof(plan.histogram_kernel), "%s", hist_name(lds));
    std::snprintf(plan.successor_kernel, sizeof(plan.successor_kernel), "%s", "pfb_deint_succ");
    std::snprintf(plan.marking_kernel, sizeof(plan.marking_kernel), "%s", mark_name(true));
    *plan_out = plan;
    return PFB_OK;
  });
}

extern "C" int pfb_deint_create(const pfb_deint_config* cfg, pfb_deint_handle** out) {
  return pfb::abi_guard([&]() -> int {
    if (!out) return PFB_ERR_BAD_ARG;
    *out = nullptr;
    Settings s;
    int rc = deint_check(cfg, &s);
    if (rc != PFB_OK) return rc;
    int dev = 0;
    rc = pfb::resolve_device(cfg->device_id, &dev);
    if (rc != PFB_OK) return rc;
    pfb_deint_handle* h = new pfb_deint_handle();
    h->device = dev;
    h->s = s;
    *out = h;
    return PFB_OK;
  });
}

extern "C" int pfb_deint_destroy(pfb_deint_handle* h) {
  return pfb::abi_guard([&]() -> int {
    return destroy_list(h);
  });
}

extern "C" int pfb_deint_set_stream(pfb_deint_handle* h, void* hip_stream) {
  return pfb::abi_guard([&]() -> int {
    return set_list_stream(h, hip_stream);
  });
}

extern "C" int pfb_deint_sync(pfb_deint_handle* h) {
  return pfb::abi_guard([&]() -> int {
    return sync_list(h);
  });
}

extern "C" int pfb_deint_get_device(const pfb_deint_handle* h, int* device_id) {
  return pfb::abi_guard([&]() -> int {
    return list_device(h, device_id);
  });
}

extern "C" int pfb_deint_set_tier(pfb_deint_handle* h, int histogram_tier, int marking_tier) {
  return pfb::abi_guard([&]() -> int {
    if (!h || histogram_tier < kTierAuto || histogram_tier > kTierGlobal) return PFB_ERR_BAD_ARG;
    if (marking_tier < kMarkAuto || marking_tier > kMarkTables) return PFB_ERR_BAD_ARG;
    if (histogram_tier == kTierLds && h->s.NB > kLdsBins) return PFB_ERR_UNSUPPORTED;
    h->hist_tier = histogram_tier;
    h->mark_tier = marking_tier;
    return PFB_OK;
  });
}

extern "C" int pfb_deint_run(pfb_deint_handle* h, const uint64_t* ticks, uint64_t n, uint32_t mem,
                             pfb_deint_emitter* emitters_out, uint64_t capacity, uint64_t* count_out, int32_t* labels_out) {
  return pfb::abi_guard([&]() -> int {
    const int rc = check_list(h, ticks, n, kMaxPulses, mem, 8);
    if (rc != PFB_OK) return rc;
    if (!count_out || (capacity > 0 && !emitters_out) || (n > 0 && !labels_out)) return PFB_ERR_BAD_ARG;
    if (mem == PFB_MEM_DEVICE && (misaligned(emitters_out, 8) || misaligned(labels_out, 4))) return PFB_ERR_BAD_ARG;
    return run(h, ticks, n, mem, emitters_out, capacity, count_out, labels_out);
  });
}

extern "C" int pfb_deint_histogram(pfb_deint_handle* h, const uint64_t* ticks, uint64_t n, uint32_t mem,
                                   uint32_t* counts_out, uint64_t capacity_bins) {
  return pfb::abi_guard([&]() -> int {
    int rc = check_list(h, ticks, n, kMaxPulses, mem, 8);
    if (rc != PFB_OK) return rc;
    if (!counts_out || (mem == PFB_MEM_DEVICE && misaligned(counts_out, 4))) return PFB_ERR_BAD_ARG;
    if (capacity_bins < h->s.NB) return PFB_ERR_CAPACITY;
    DeviceGuard g(h->device);
    rc = reserve(h, n);
    if (rc != PFB_OK) return rc;
    Call c(h);
    if (n > 0) {
      Control ctl{};
      rc = begin_call(c, ticks, n, mem, &ctl);
      if (rc != PFB_OK) return rc;
    }
    rc = histogram(c, (uint32_t)n);
    if (rc != PFB_OK) return rc;
    rc = copy_out(h->stream, counts_out, c.scr.hist, (size_t)h->s.NB * sizeof(uint32_t), mem);
    if (rc != PFB_OK) return rc;
    HIP_TRY(hipStreamSynchronize(h->stream));
    h->last_kernel = c.kernels;
    return PFB_OK;
  });
}

extern "C" int pfb_deint_successors(pfb_deint_handle* h, const uint64_t* ticks, uint64_t n, uint32_t mem, uint64_t period,
                                    int32_t* succ_out, int32_t* step_out, int32_t* len_out) {
  return pfb::abi_guard([&]() -> int {
    int rc = check_list(h, ticks, n, kMaxPulses, mem, 8);
    if (rc != PFB_OK) return rc;
    if (n > 0 && (!succ_out || !step_out || !len_out)) return PFB_ERR_BAD_ARG;
    if (mem == PFB_MEM_DEVICE && (misaligned(succ_out, 4) || misaligned(step_out, 4) || misaligned(len_out, 4)))
      return PFB_ERR_BAD_ARG;
    if (period < 1 || period > 0xffffffffull || h->s.e * (2 * (uint64_t)h->s.X + 3) >= period) return PFB_ERR_BAD_ARG;
    if (n == 0) {
      h->last_kernel.clear();
      return PFB_OK;
    }
    DeviceGuard g(h->device);
    rc = reserve(h, n);
    if (rc != PFB_OK) return rc;
    Call c(h);
    Control ctl{};
    rc = begin_call(c, ticks, n, mem, &ctl);
    if (rc != PFB_OK) return rc;
    const int4* table = nullptr;
    int rounds = 0;
    rc = chains(c, (uint32_t)n, period, ctl.last - ctl.first, false, &table, &rounds);
    if (rc != PFB_OK) return rc;
    hipLaunchKernelGGL(deint_lengths, dim3(((unsigned)n + kThreads - 1) / kThreads), dim3(kThreads), 0, h->stream,
                       table, c.scr.len, (uint32_t)n);
    HIP_TRY(hipGetLastError());
    const size_t bytes = n * sizeof(int32_t);
    if ((rc = copy_out(h->stream, succ_out, c.scr.succ, bytes, mem)) != PFB_OK) return rc;
    if ((rc = copy_out(h->stream, step_out, c.scr.step, bytes, mem)) != PFB_OK) return rc;
    if ((rc = copy_out(h->stream, len_out, c.scr.len, bytes, mem)) != PFB_OK) return rc;
    HIP_TRY(hipStreamSynchronize(h->stream));
    h->last_kernel = c.kernels;
    return PFB_OK;
  });
}

extern "C" const char* pfb_deint_last_kernel(const pfb_deint_handle* h) { return h ? h->last_kernel.c_str() : ""; }

extern "C" int pfb_deint_get_stats(const pfb_deint_handle* h, pfb_deint_stats* stats_out) {
  return pfb::abi_guard([&]() -> int {
    return list_stats(h, stats_out);
  });
}

extern "C" int pfb_deint_ticks_from_toa(const double* toa, uint64_t stride_bytes, uint64_t n, double t0, double tick_rate,
                                        uint64_t* ticks_out, uint32_t* order_out) {
  return pfb::abi_guard([&]() -> int {
    if ((n > 0 && (!toa || !ticks_out || !order_out)) || stride_bytes < sizeof(double) || n > (1ull << 31))
      return PFB_ERR_BAD_ARG;
    if (!std::isfinite(tick_rate) || tick_rate <= 0 || !std::isfinite(t0)) return PFB_ERR_BAD_ARG;
    std::vector<uint64_t> tick(n);
    const char* at = reinterpret_cast<const char*>(toa);
    for (uint64_t i = 0; i < n; ++i, at += stride_bytes) {
      double v;
      std::memcpy(&v, at, sizeof(v));
      const double r = std::rint((v - t0) * tick_rate);  // to nearest, ties to even: llrint without its range trouble
      if (!std::isfinite(r) || r < 0 || r >= 4611686018427387904.0) return PFB_ERR_BAD_ARG;
      tick[i] = (uint64_t)r;
    }
    std::vector<uint32_t> order(n);
    std::iota(order.begin(), order.end(), 0u);
    std::stable_sort(order.begin(), order.end(), [&tick](uint32_t x, uint32_t y) { return tick[x] < tick[y]; });
    for (uint64_t i = 0; i < n; ++i) {
      order_out[i] = order[i];
      ticks_out[i] = tick[order[i]];
    }
    return PFB_OK;
  });
}
