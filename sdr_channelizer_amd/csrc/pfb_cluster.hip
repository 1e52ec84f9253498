// pfb_cluster.hip -- PDW clustering (pfb_cluster_* in include/pfb_channelizer.h, where every figure is defined): cells of
// two integer features, dense cells joined into clusters, a stable partition of the items by cluster; kernels and host side.
//   cluster_hist<LDS>   one lane per item, kHistTile items a workgroup.  A wave first combines the lanes that hit the cell
//                       of its first remaining lane (twice), then adds: into a private LDS histogram that the workgroup
//                       adds to the global one once (LDS = true, U V <= kLdsCells), or straight into the global one.
//   cluster_init        one lane per cell: label = g for a dense cell, -1 otherwise; the per-root slots cleared.
//   cluster_hook        one lane per cell, a workgroup a block of bu x bv cells whose labels it stages with a halo of the
//                       reach in LDS: where the labels of a linked pair differ, an atomicMin on the larger label's entry
//                       of the NEW labels with the smaller.  All pairs of a round read the old labels.
//   cluster_jump        label[g] = label[label[g]], in place: a read gives the old or the new entry, both ancestors.
//   cluster_border      one lane per cell: the cell's root -- its label, or for a border cell the lowest label in its box.
//   cluster_cells       one lane per cell: integer add / min / max into the root's slots, a 64-bit max of (H << 32 | ~g).
//   cluster_count / list_scan / cluster_scatter   the clusters' numbers: flags (a root with pulses >= min_pulses), a
//                       scan of the workgroups' counts, an ordered scatter that also clears the cluster's item sums.
//   cluster_label       one lane per item: its cluster through the cell tables, wave-combined adds into sum_u / sum_v and
//                       a min into first_item.
//   cluster_emit        one lane per cluster: the 64-byte record.
//   cluster_offsets     one workgroup: the scan of the clusters' pulses, G + 2 offsets.
//   part_hist / part_scan / part_scatter   one pass of the LSD radix over the label: digit counts per tile, the scan over
//                       (digit, tile), the stable rank inside the tile from wave ballots and LDS counts of the waves.
//   cluster_gather4/8   dst[k] = src[order[k]].
// Whether a round hooked is read by the host, one flag a round.  No float on the device.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <new>
#include <string>

#include "pfb_list.hpp"

namespace {

constexpr uint32_t kMaxItems = 1u << 20, kMaxCells = 1u << 20, kMaxReach = 8, kMaxClusters = 65535;
constexpr uint32_t kMaxCount = 1u << 20;
constexpr uint32_t kLdsCells = 8192;     // the LDS histogram's bound
constexpr uint32_t kHistTile = 4096;     // items of one histogram workgroup: 16 to a lane
constexpr uint32_t kLabelTile = 256;     // items of one label workgroup: one to a lane
constexpr uint32_t kPartTile = 1024;     // items of one partition workgroup: four steps of one to a lane
constexpr uint32_t kNumTile = 1024;      // cells of one workgroup of the numbering: four to a lane
constexpr uint32_t kDigits = 256;
constexpr uint32_t kSlots = 65536;       // per-cluster slots: numbers past them are counted, not stored
constexpr uint32_t kHalo = 4624;         // labels the hook stages at most: (256 / bv + 16) (bv + 16) is largest at bv = 1
constexpr int kCombine = 2;              // cells a wave combines before its lanes add alone
constexpr int kMaxRounds = 64;           // after which the host gives up

struct Control {            // what a call hands back to the host
  u64 outside, unassigned, dense, border, components;
  uint32_t groups, pad;
  uint32_t hooked[kMaxRounds];
};

struct Arrays {             // all in the handle's scratch
  // per cell
  uint32_t* H;
  int32_t* label;           // padded to a whole kNumTile
  int32_t* next;            // the new labels of a round
  int32_t* croot;           // the cell's root after the border step, padded to a whole kNumTile
  int32_t* cnum;            // the root's cluster number, -1 for none
  uint32_t* c_pulses;       // per root: indexed by the root's g
  uint32_t* c_cells;
  int32_t* c_umin;
  int32_t* c_umax;
  int32_t* c_vmin;
  int32_t* c_vmax;
  u64* c_peak;
  uint32_t* counts;         // clusters of every numbering workgroup, then (list_scan) those before it
  // per cluster, by its number
  uint32_t* root;
  u64* sum_u;
  u64* sum_v;
  uint32_t* first;
  pfb_cluster_group* records;
  // per item
  int32_t* labels;
  uint32_t* order_a;
  uint32_t* order_b;
  uint32_t* table;          // kDigits x tiles digit counts of a partition pass
  uint32_t* offsets;        // kSlots + 2
  Control* ctl;
  uint32_t n, U, V, cells, ru, rv, minc, minp, border;
};
static_assert(sizeof(Control) == 304 && sizeof(Arrays) == 232, "the kernels' parameter layout");

__device__ __forceinline__ u64 lanes_below() { return (1ull << (threadIdx.x & 63)) - 1; }

__device__ __forceinline__ u64 wave_sum(u64 v) {
  for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
  return v;
}

// g of an item, or -1 outside the grid
__device__ __forceinline__ int32_t cell_of(int2 it, uint32_t U, uint32_t V) {
  return ((uint32_t)it.x < U && (uint32_t)it.y < V) ? (int32_t)((uint32_t)it.x * V + (uint32_t)it.y) : -1;
}

template <bool LDS>
__global__ void __launch_bounds__(kThreads) cluster_hist(const int2* items, const Arrays a) {
  __shared__ uint32_t s_h[LDS ? kLdsCells : 1];
  if (LDS) {
    for (uint32_t k = threadIdx.x; k < a.cells; k += kThreads) s_h[k] = 0;  // cells <= kLdsCells: the host's tier rule
    __syncthreads();
  }
  const uint32_t base = blockIdx.x * kHistTile;
  uint32_t outside = 0;
  for (uint32_t s = 0; s < kHistTile / kThreads; ++s) {  // the trip count is the same for every lane
    const uint32_t i = base + s * kThreads + threadIdx.x;
    int32_t g = -1;
    if (i < a.n) {
      g = cell_of(items[i], a.U, a.V);
      outside += g < 0;
    }
    bool todo = g >= 0;
    u64 left = __ballot(todo);
    for (int k = 0; k < kCombine && left; ++k) {  // `left` is the wave's: every lane goes round together
      const int lead = __ffsll((long long)left) - 1;
      const int32_t gl = __shfl(g, lead, 64);
      const u64 same = __ballot(todo && g == gl);
      if ((int)(threadIdx.x & 63) == lead) {
        if (LDS) atomicAdd(&s_h[gl], (uint32_t)__popcll(same));  // 0 <= gl < cells
        else atomicAdd(&a.H[gl], (uint32_t)__popcll(same));
      }
      if (todo && g == gl) todo = false;
      left &= ~same;
    }
    if (todo) {
      if (LDS) atomicAdd(&s_h[g], 1u);
      else atomicAdd(&a.H[g], 1u);
    }
  }
  outside = (uint32_t)wave_sum(outside);
  if ((threadIdx.x & 63) == 0 && outside) atomicAdd(&a.ctl->outside, (u64)outside);
  if (LDS) {
    __syncthreads();
    for (uint32_t k = threadIdx.x; k < a.cells; k += kThreads) {
      const uint32_t c = s_h[k];
      if (c) atomicAdd(&a.H[k], c);
    }
  }
}

__global__ void __launch_bounds__(kThreads) cluster_init(const Arrays a) {
  const uint32_t g = blockIdx.x * kThreads + threadIdx.x;
  bool dense = false;
  if (g < a.cells) {
    dense = a.H[g] >= a.minc;
    a.label[g] = dense ? (int32_t)g : -1;
    a.c_pulses[g] = 0;
    a.c_cells[g] = 0;
    a.c_umin[g] = 0x7fffffff;
    a.c_umax[g] = (int32_t)0x80000000;
    a.c_vmin[g] = 0x7fffffff;
    a.c_vmax[g] = (int32_t)0x80000000;
    a.c_peak[g] = 0;
  }
  const u64 m = __ballot(dense);
  if ((threadIdx.x & 63) == 0 && m) atomicAdd(&a.ctl->dense, (u64)__popcll(m));
}

// A workgroup takes the block (blockIdx / blocks_v, blockIdx mod blocks_v) of bu x bv cells, bu bv = kThreads.
__global__ void __launch_bounds__(kThreads) cluster_hook(const Arrays a, uint32_t bu, uint32_t bv, uint32_t blocks_v,
                                                         uint32_t round) {
  __shared__ int32_t s_l[kHalo];
  const int ru = (int)a.ru, rv = (int)a.rv;
  const int su = (int)bu + 2 * ru, sv = (int)bv + 2 * rv;  // su sv <= kHalo: bv is a power of two up to 16, bu = 256 / bv
  const int u0 = (int)((blockIdx.x / blocks_v) * bu), v0 = (int)((blockIdx.x % blocks_v) * bv);
  for (int k = threadIdx.x; k < su * sv; k += kThreads) {
    const int gu = u0 - ru + k / sv, gv = v0 - rv + k % sv;
    s_l[k] = (gu >= 0 && gu < (int)a.U && gv >= 0 && gv < (int)a.V) ? a.label[(uint32_t)gu * a.V + (uint32_t)gv] : -1;
  }
  __syncthreads();
  const int tu = (int)(threadIdx.x / bv), tv = (int)(threadIdx.x % bv);
  const int32_t ri = s_l[(tu + ru) * sv + tv + rv];  // -1 outside the grid and for a cell that is not dense
  if (ri < 0) return;
  bool hooked = false;
  for (int du = 0; du <= 2 * ru; ++du) {
    for (int dv = 0; dv <= 2 * rv; ++dv) {
      const int32_t rj = s_l[(tu + du) * sv + tv + dv];
      if (rj < 0 || rj == ri) continue;
      // both are cells of the pair's component and each entry is at most its index: the entry only decreases
      atomicMin(&a.next[max(ri, rj)], min(ri, rj));
      hooked = true;
    }
  }
  if (hooked) a.ctl->hooked[round] = 1u;
}

__global__ void __launch_bounds__(kThreads) cluster_jump(int32_t* label, uint32_t cells) {
  const uint32_t g = blockIdx.x * kThreads + threadIdx.x;
  if (g >= cells) return;
  const int32_t p = label[g];
  if (p < 0) return;
  const int32_t q = label[p];  // 0 <= q <= p <= g: p is a dense cell
  if (q != p) label[g] = q;
}

__global__ void __launch_bounds__(kThreads) cluster_border(const Arrays a) {
  const uint32_t g = blockIdx.x * kThreads + threadIdx.x;
  bool joined = false;
  if (g < a.cells) {
    int32_t r = a.label[g];
    const uint32_t h = a.H[g];
    if (a.border && h > 0 && h < a.minc) {
      const int u = (int)(g / a.V), v = (int)(g % a.V);
      const int ulo = max(u - (int)a.ru, 0), uhi = min(u + (int)a.ru, (int)a.U - 1);
      const int vlo = max(v - (int)a.rv, 0), vhi = min(v + (int)a.rv, (int)a.V - 1);
      int32_t best = 0x7fffffff;
      for (int x = ulo; x <= uhi; ++x)
        for (int y = vlo; y <= vhi; ++y) {
          const int32_t l = a.label[(uint32_t)x * a.V + (uint32_t)y];  // of a dense cell: its root; -1 otherwise
          if (l >= 0) best = min(best, l);
        }
      if (best != 0x7fffffff) {
        r = best;
        joined = true;
      }
    }
    a.croot[g] = r;
  }
  const u64 m = __ballot(joined);
  if ((threadIdx.x & 63) == 0 && m) atomicAdd(&a.ctl->border, (u64)__popcll(m));
}

__global__ void __launch_bounds__(kThreads) cluster_cells(const Arrays a) {
  const uint32_t g = blockIdx.x * kThreads + threadIdx.x;
  bool is_root = false;
  if (g < a.cells) {
    const int32_t r = a.croot[g];
    if (r >= 0) {
      const uint32_t h = a.H[g];
      const int32_t u = (int32_t)(g / a.V), v = (int32_t)(g % a.V);
      is_root = r == (int32_t)g;
      atomicAdd(&a.c_pulses[r], h);
      atomicAdd(&a.c_cells[r], 1u);
      atomicMin(&a.c_umin[r], u);
      atomicMax(&a.c_umax[r], u);
      atomicMin(&a.c_vmin[r], v);
      atomicMax(&a.c_vmax[r], v);
      atomicMax(&a.c_peak[r], ((u64)h << 32) | (0xffffffffu - g));
    }
  }
  const u64 m = __ballot(is_root);
  if ((threadIdx.x & 63) == 0 && m) atomicAdd(&a.ctl->components, (u64)__popcll(m));
}

// a lane takes 4 consecutive cells, a workgroup kNumTile; croot is padded with -1 to a whole tile
__device__ __forceinline__ void clusters_of(const Arrays& a, uint32_t g0, bool is[4]) {
  const int4 r = *reinterpret_cast<const int4*>(a.croot + g0);
  const int32_t rr[4] = {r.x, r.y, r.z, r.w};
  for (uint32_t k = 0; k < 4; ++k) is[k] = g0 + k < a.cells && rr[k] == (int32_t)(g0 + k) && a.c_pulses[g0 + k] >= a.minp;
}

__global__ void __launch_bounds__(kThreads) cluster_count(const Arrays a) {
  bool is[4];
  clusters_of(a, blockIdx.x * kNumTile + threadIdx.x * 4, is);
  uint32_t total;
  (void)block_scan((uint32_t)is[0] + is[1] + is[2] + is[3], &total);
  if (threadIdx.x == 0) a.counts[blockIdx.x] = total;
}

__global__ void __launch_bounds__(kThreads) cluster_scatter(const Arrays a) {
  const uint32_t g0 = blockIdx.x * kNumTile + threadIdx.x * 4;
  bool is[4];
  clusters_of(a, g0, is);
  uint32_t total;
  uint32_t at = a.counts[blockIdx.x] + block_scan((uint32_t)is[0] + is[1] + is[2] + is[3], &total);
  for (uint32_t k = 0; k < 4; ++k) {
    if (g0 + k >= a.cells) break;
    int32_t number = -1;
    if (is[k]) {
      if (at < kSlots) {  // past them the call is refused: only the count matters
        a.root[at] = g0 + k;
        a.sum_u[at] = 0;
        a.sum_v[at] = 0;
        a.first[at] = 0xffffffffu;
        number = (int32_t)at;
      }
      ++at;
    }
    a.cnum[g0 + k] = number;
  }
}

__global__ void __launch_bounds__(kThreads) cluster_label(const int2* items, const Arrays a, int32_t* labels_out) {
  const uint32_t i = blockIdx.x * kLabelTile + threadIdx.x;
  int32_t c = -1;
  int2 it = make_int2(0, 0);
  bool lost = false;
  if (i < a.n) {
    it = items[i];
    const int32_t g = cell_of(it, a.U, a.V);
    if (g >= 0) {
      const int32_t r = a.croot[g];
      if (r >= 0) c = a.cnum[r];
      lost = c < 0;
    }
    labels_out[i] = c;
    a.labels[i] = c;
  }
  // in the grid: u, v >= 0
  const u64 su = (u64)(uint32_t)it.x, sv = (u64)(uint32_t)it.y;
  bool todo = c >= 0;
  u64 left = __ballot(todo);
  for (int k = 0; k < kCombine && left; ++k) {  // `left` is the wave's: every lane goes round together
    const int lead = __ffsll((long long)left) - 1;
    const int32_t cl = __shfl(c, lead, 64);
    const bool mine = todo && c == cl;
    const u64 same = __ballot(mine);
    const u64 tu = wave_sum(mine ? su : 0), tv = wave_sum(mine ? sv : 0);
    if ((int)(threadIdx.x & 63) == lead) {  // the lowest lane of them: its index is their lowest
      atomicAdd(&a.sum_u[cl], tu);
      atomicAdd(&a.sum_v[cl], tv);
      atomicMin(&a.first[cl], i);
    }
    if (mine) todo = false;
    left &= ~same;
  }
  if (todo) {
    atomicAdd(&a.sum_u[c], su);
    atomicAdd(&a.sum_v[c], sv);
    atomicMin(&a.first[c], i);
  }
  const u64 m = __ballot(lost);
  if ((threadIdx.x & 63) == 0 && m) atomicAdd(&a.ctl->unassigned, (u64)__popcll(m));
}

__global__ void __launch_bounds__(kThreads) cluster_emit(const Arrays a, uint32_t groups) {
  const uint32_t e = blockIdx.x * kThreads + threadIdx.x;
  if (e >= groups) return;
  const uint32_t g = a.root[e];
  const u64 peak = a.c_peak[g];
  const uint32_t pg = 0xffffffffu - (uint32_t)(peak & 0xffffffffu);
  pfb_cluster_group r;
  r.root_u = (int32_t)(g / a.V);
  r.root_v = (int32_t)(g % a.V);
  r.pulses = a.c_pulses[g];
  r.cells = a.c_cells[g];
  r.u_min = a.c_umin[g];
  r.u_max = a.c_umax[g];
  r.v_min = a.c_vmin[g];
  r.v_max = a.c_vmax[g];
  r.sum_u = (int64_t)a.sum_u[e];
  r.sum_v = (int64_t)a.sum_v[e];
  r.peak_u = (int32_t)(pg / a.V);
  r.peak_v = (int32_t)(pg % a.V);
  r.peak_count = (uint32_t)(peak >> 32);
  r.first_item = a.first[e];
  a.records[e] = r;
}

// one workgroup: offsets[c] = the pulses of the clusters before c, offsets[G] = the assigned, offsets[G + 1] = n
__global__ void __launch_bounds__(kThreads) cluster_offsets(const Arrays a, uint32_t groups) {
  const uint32_t per = (groups + kThreads - 1) / kThreads;  // <= 256
  const uint32_t lo = min(threadIdx.x * per, groups), hi = min(lo + per, groups);
  uint32_t sum = 0;
  for (uint32_t c = lo; c < hi; ++c) sum += a.c_pulses[a.root[c]];
  uint32_t total;
  uint32_t at = block_scan(sum, &total);
  for (uint32_t c = lo; c < hi; ++c) {
    a.offsets[c] = at;
    at += a.c_pulses[a.root[c]];
  }
  if (threadIdx.x == 0) {
    a.offsets[groups] = total;
    a.offsets[groups + 1] = a.n;
  }
}

// ---- the partition: one pass of the radix ----
// item k of the pass is src[k], or k itself in the first pass; its digit is 8 bits of its label, -1 taken as `groups`
__device__ __forceinline__ uint32_t digit_of(const Arrays& a, const uint32_t* src, uint32_t k, uint32_t groups, uint32_t shift,
                                             uint32_t* index) {
  const uint32_t i = src ? src[k] : k;
  const int32_t l = a.labels[i];
  *index = i;
  return (((l < 0) ? groups : (uint32_t)l) >> shift) & (kDigits - 1);
}

__global__ void __launch_bounds__(kThreads) part_hist(const Arrays a, const uint32_t* src, uint32_t groups, uint32_t shift,
                                                      uint32_t tiles) {
  __shared__ uint32_t s_c[kDigits];
  s_c[threadIdx.x] = 0;  // kThreads == kDigits
  __syncthreads();
  for (uint32_t s = 0; s < kPartTile / kThreads; ++s) {
    const uint32_t k = blockIdx.x * kPartTile + s * kThreads + threadIdx.x;
    if (k < a.n) {
      uint32_t index;
      atomicAdd(&s_c[digit_of(a, src, k, groups, shift, &index)], 1u);  // a count: the order is free
    }
  }
  __syncthreads();
  a.table[threadIdx.x * tiles + blockIdx.x] = s_c[threadIdx.x];
}

// one workgroup: table[0 .. total) becomes the sum of the entries before each
__global__ void __launch_bounds__(kThreads) part_scan(uint32_t* table, uint32_t total) {
  const uint32_t per = (total + kThreads - 1) / kThreads;
  const uint32_t lo = min(threadIdx.x * per, total), hi = min(lo + per, total);
  uint32_t sum = 0;
  for (uint32_t k = lo; k < hi; ++k) sum += table[k];
  uint32_t all;
  uint32_t at = block_scan(sum, &all);
  for (uint32_t k = lo; k < hi; ++k) {
    const uint32_t v = table[k];
    table[k] = at;
    at += v;
  }
}

__global__ void __launch_bounds__(kThreads) part_scatter(const Arrays a, const uint32_t* src, uint32_t* dst, uint32_t groups,
                                                         uint32_t shift, uint32_t tiles) {
  __shared__ uint32_t s_base[kDigits];                   // where the next item of each digit goes
  __shared__ uint32_t s_wave[kThreads / 64][kDigits];    // items of each digit in each wave of this step
  const int wv = threadIdx.x >> 6;
  s_base[threadIdx.x] = a.table[threadIdx.x * tiles + blockIdx.x];
  for (int w = 0; w < kThreads / 64; ++w) s_wave[w][threadIdx.x] = 0;
  __syncthreads();
  for (uint32_t s = 0; s < kPartTile / kThreads; ++s) {  // every lane makes every trip: the barriers are the workgroup's
    const uint32_t k = blockIdx.x * kPartTile + s * kThreads + threadIdx.x;
    const bool live = k < a.n;
    uint32_t index = 0, d = 0;
    if (live) d = digit_of(a, src, k, groups, shift, &index);
    u64 same = __ballot(live);                           // the live lanes of this wave with this lane's digit
    for (uint32_t b = 0; b < 8; ++b) {
      const u64 bal = __ballot(live && ((d >> b) & 1u));
      same &= ((d >> b) & 1u) ? bal : ~bal;
    }
    const uint32_t below = (uint32_t)__popcll(same & lanes_below());
    if (live && below == 0) s_wave[wv][d] = (uint32_t)__popcll(same);  // the lowest lane of its digit writes
    __syncthreads();
    if (live) {
      uint32_t at = s_base[d] + below;
      for (int w = 0; w < wv; ++w) at += s_wave[w][d];
      dst[at] = index;                                   // at < n: the scan of the counts of exactly these items
    }
    __syncthreads();
    uint32_t step = 0;
    for (int w = 0; w < kThreads / 64; ++w) {
      step += s_wave[w][threadIdx.x];
      s_wave[w][threadIdx.x] = 0;
    }
    s_base[threadIdx.x] += step;
    __syncthreads();
  }
}

template <class T>
__global__ void __launch_bounds__(kThreads) cluster_gather(const T* src, const uint32_t* order, uint32_t n, T* dst) {
  const uint32_t k = blockIdx.x * kThreads + threadIdx.x;
  if (k < n) dst[k] = src[order[k]];
}

// ---------------------------------------------------------------------------------
// host: checks and plan

struct Settings {
  uint32_t U = 0, V = 0, cells = 0, ru = 0, rv = 0, minc = 0, minp = 0, border = 0;
  uint32_t bu = 0, bv = 0;  // the component kernels' block
};

size_t cells_padded(size_t cells) { return round_up(cells, kNumTile); }

// the carving of a handle's scratch for lists of up to cap items (a multiple of kPartTile) on a grid of `cells`: every
// array once.  *items: where a host list is staged
Arrays carve(Carver& c, size_t cap, size_t cells, pfb_cluster_item** items) {
  const size_t padded = cells_padded(cells), slots = std::min<size_t>(cells, kSlots);
  Arrays a{};
  *items = c.array<pfb_cluster_item>(cap);
  a.H = c.array<uint32_t>(cells);
  a.label = c.array<int32_t>(padded);
  a.next = c.array<int32_t>(padded);
  a.croot = c.array<int32_t>(padded);
  a.cnum = c.array<int32_t>(cells);
  a.c_pulses = c.array<uint32_t>(cells);
  a.c_cells = c.array<uint32_t>(cells);
  a.c_umin = c.array<int32_t>(cells);
  a.c_umax = c.array<int32_t>(cells);
  a.c_vmin = c.array<int32_t>(cells);
  a.c_vmax = c.array<int32_t>(cells);
  a.c_peak = c.array<u64>(cells);
  a.counts = c.array<uint32_t>(kMaxCells / kNumTile);
  a.root = c.array<uint32_t>(slots);
  a.sum_u = c.array<u64>(slots);
  a.sum_v = c.array<u64>(slots);
  a.first = c.array<uint32_t>(slots);
  a.records = c.array<pfb_cluster_group>(slots);
  a.labels = c.array<int32_t>(cap);
  a.order_a = c.array<uint32_t>(cap);
  a.order_b = c.array<uint32_t>(cap);
  a.table = c.array<uint32_t>((size_t)kDigits * (cap / kPartTile));
  a.offsets = c.array<uint32_t>(kSlots + 2);
  a.ctl = c.array<Control>(1);
  return a;
}

size_t scratch_bytes(size_t cap, size_t cells) {
  Carver c;
  pfb_cluster_item* items;
  carve(c, cap, cells, &items);
  return c.bytes();
}

size_t capacity_for(uint64_t n) { return round_up(std::max<uint64_t>(n, 1), kPartTile); }

const char* hist_name(bool lds) { return lds ? "pfb_cluster_hist_lds" : "pfb_cluster_hist_global"; }

// Everything pfb_cluster_describe and pfb_cluster_create check before the device, in the order the header states
int cluster_check(const pfb_cluster_config* cfg, Settings* s) {
  if (!cfg || !s || cfg->struct_size != sizeof(pfb_cluster_config)) return PFB_ERR_BAD_ARG;
  if (cfg->cells_u < 1 || cfg->cells_v < 1) return PFB_ERR_BAD_ARG;
  if ((uint64_t)cfg->cells_u * cfg->cells_v > kMaxCells) return PFB_ERR_BAD_ARG;
  if (cfg->reach_u > kMaxReach || cfg->reach_v > kMaxReach) return PFB_ERR_BAD_ARG;
  if (cfg->min_cell_count < 1 || cfg->min_cell_count > kMaxCount) return PFB_ERR_BAD_ARG;
  if (cfg->min_pulses < 1 || cfg->min_pulses > kMaxCount) return PFB_ERR_BAD_ARG;
  if (cfg->flags & ~PFB_CLUSTER_BORDER) return PFB_ERR_BAD_ARG;
  s->U = cfg->cells_u;
  s->V = cfg->cells_v;
  s->cells = cfg->cells_u * cfg->cells_v;
  s->ru = cfg->reach_u;
  s->rv = cfg->reach_v;
  s->minc = cfg->min_cell_count;
  s->minp = cfg->min_pulses;
  s->border = cfg->flags & PFB_CLUSTER_BORDER;
  s->bv = 1;  // the smallest power of two that covers V, 16 at the most
  while (s->bv < 16 && s->bv < s->V) s->bv *= 2;
  s->bu = kThreads / s->bv;
  return PFB_OK;
}

}  // namespace

struct pfb_cluster_handle : ListHandle {
  Settings s;
  int tier = kTierAuto;
  pfb_cluster_stats stats{};
};

namespace {

bool runs_lds(const pfb_cluster_handle* h) {
  return h->tier == kTierAuto ? h->s.cells <= kLdsCells : h->tier == kTierLds;
}

unsigned blocks_for(uint32_t n, uint32_t per) { return (n + per - 1) / per; }

// one call's view of the scratch
struct Call : ListCall {
  pfb_cluster_handle* h;
  pfb_cluster_item* staged = nullptr;  // where a host list is staged
  Arrays a;
  const int2* d_items = nullptr;
  Call(pfb_cluster_handle* hh, uint32_t n) : h(hh) {
    Carver c{hh->d_scratch};
    a = carve(c, hh->cap, hh->s.cells, &staged);
    a.n = n;
    a.U = hh->s.U;
    a.V = hh->s.V;
    a.cells = hh->s.cells;
    a.ru = hh->s.ru;
    a.rv = hh->s.rv;
    a.minc = hh->s.minc;
    a.minp = hh->s.minp;
    a.border = hh->s.border;
  }
};

int reserve(pfb_cluster_handle* h, uint64_t n) {
  const size_t cap = capacity_for(n);
  return cap > h->cap ? h->ensure(cap, scratch_bytes(cap, h->s.cells)) : PFB_OK;  // the size only when it grows
}

// step 1: the list onto the device and the histogram
int histogram(Call& c, const pfb_cluster_item* items, uint32_t mem) {
  pfb_cluster_handle* h = c.h;
  const uint32_t n = c.a.n;
  c.d_items = reinterpret_cast<const int2*>(items);
  if (mem == PFB_MEM_HOST && n > 0) {
    HIP_TRY(hipMemcpyAsync(c.staged, items, (size_t)n * sizeof(pfb_cluster_item), hipMemcpyHostToDevice, h->stream));
    c.d_items = reinterpret_cast<const int2*>(c.staged);
  }
  HIP_TRY(hipMemsetAsync(c.a.H, 0, (size_t)c.a.cells * 4, h->stream));
  HIP_TRY(hipMemsetAsync(c.a.ctl, 0, sizeof(Control), h->stream));
  if (n > 0) {
    const bool lds = runs_lds(h);
    const dim3 grid(blocks_for(n, kHistTile)), block(kThreads);
    if (lds) hipLaunchKernelGGL(cluster_hist<true>, grid, block, 0, h->stream, c.d_items, c.a);
    else hipLaunchKernelGGL(cluster_hist<false>, grid, block, 0, h->stream, c.d_items, c.a);
    HIP_TRY(hipGetLastError());
    c.ran(hist_name(lds));
  }
  return PFB_OK;
}

// steps 2 to 4: croot of every cell; *rounds: the rounds made
int components(Call& c, Control* ctl, uint64_t* rounds) {
  pfb_cluster_handle* h = c.h;
  const uint32_t cells = c.a.cells;
  const dim3 block(kThreads), grid(blocks_for(cells, kThreads));
  // the padding of the labels and roots is never a root: -1 is no cell
  HIP_TRY(hipMemsetAsync(c.a.label, 0xff, cells_padded(cells) * 4, h->stream));
  HIP_TRY(hipMemsetAsync(c.a.croot, 0xff, cells_padded(cells) * 4, h->stream));
  hipLaunchKernelGGL(cluster_init, grid, block, 0, h->stream, c.a);
  HIP_TRY(hipGetLastError());
  c.ran("pfb_cluster_init");
  int rc = fetch(h->stream, c.a.ctl, ctl);
  if (rc != PFB_OK) return rc;
  *rounds = 0;
  if (ctl->dense > 0) {
    int passes = 1;  // ceil(log2 cells) + 1: a chain of roots is shorter than the cells
    while ((1ull << (passes - 1)) < cells) ++passes;
    const uint32_t blocks_u = blocks_for(h->s.U, h->s.bu), blocks_v = blocks_for(h->s.V, h->s.bv);
    rc = hook_until_still(h->stream, c.a.ctl->hooked, kMaxRounds, [&](uint32_t round) -> int {
      HIP_TRY(hipMemcpyAsync(c.a.next, c.a.label, (size_t)cells * 4, hipMemcpyDeviceToDevice, h->stream));
      hipLaunchKernelGGL(cluster_hook, dim3(blocks_u * blocks_v), block, 0, h->stream, c.a, h->s.bu, h->s.bv, blocks_v, round);
      for (int p = 0; p < passes; ++p) hipLaunchKernelGGL(cluster_jump, grid, block, 0, h->stream, c.a.next, cells);
      HIP_TRY(hipGetLastError());
      std::swap(c.a.label, c.a.next);
      return PFB_OK;
    });
    if (rc < 0) return rc;
    *rounds = (uint64_t)rc;
    c.ran("pfb_cluster_hook");
    c.ran("pfb_cluster_jump");
  }
  hipLaunchKernelGGL(cluster_border, grid, block, 0, h->stream, c.a);
  HIP_TRY(hipGetLastError());
  c.ran("pfb_cluster_border");
  return PFB_OK;
}

int run(pfb_cluster_handle* h, const pfb_cluster_item* items, uint64_t n64, uint32_t mem, pfb_cluster_group* groups_out,
        uint64_t capacity, uint64_t* count_out, int32_t* labels_out, uint32_t* order_out, uint32_t* offsets_out) {
  DeviceGuard g(h->device);
  int rc = reserve(h, n64);
  if (rc != PFB_OK) return rc;
  const uint32_t n = (uint32_t)n64, cells = h->s.cells;
  Call c(h, n);
  Control ctl{};
  uint64_t rounds = 0;
  if ((rc = histogram(c, items, mem)) != PFB_OK) return rc;
  if ((rc = components(c, &ctl, &rounds)) != PFB_OK) return rc;
  const dim3 block(kThreads);
  hipLaunchKernelGGL(cluster_cells, dim3(blocks_for(cells, kThreads)), block, 0, h->stream, c.a);
  const unsigned blocks = blocks_for(cells, kNumTile);
  hipLaunchKernelGGL(cluster_count, dim3(blocks), block, 0, h->stream, c.a);
  hipLaunchKernelGGL(list_scan<true>, dim3(1), block, 0, h->stream, c.a.counts, blocks, &c.a.ctl->groups);
  hipLaunchKernelGGL(cluster_scatter, dim3(blocks), block, 0, h->stream, c.a);
  HIP_TRY(hipGetLastError());
  c.ran("pfb_cluster_cells");
  c.ran("pfb_cluster_number");
  if ((rc = fetch(h->stream, c.a.ctl, &ctl)) != PFB_OK) return rc;
  const uint32_t G = ctl.groups;
  *count_out = G;
  if (G > capacity || G > kMaxClusters) return PFB_ERR_CAPACITY;
  if (n > 0) {
    // the scratch copy is what the partition reads, and what goes to a caller's host memory
    int32_t* d_labels = mem == PFB_MEM_DEVICE ? labels_out : c.a.labels;
    hipLaunchKernelGGL(cluster_label, dim3(blocks_for(n, kLabelTile)), block, 0, h->stream, c.d_items, c.a, d_labels);
    HIP_TRY(hipGetLastError());
    c.ran("pfb_cluster_label");
    if (mem == PFB_MEM_HOST && (rc = copy_out(h->stream, labels_out, d_labels, (size_t)n * 4, mem)) != PFB_OK) return rc;
  }
  if (G > 0) {
    hipLaunchKernelGGL(cluster_emit, dim3(blocks_for(G, kThreads)), block, 0, h->stream, c.a, G);
    HIP_TRY(hipGetLastError());
    c.ran("pfb_cluster_emit");
    if ((rc = copy_out(h->stream, groups_out, c.a.records, (size_t)G * sizeof(pfb_cluster_group), mem)) != PFB_OK) return rc;
  }
  if (order_out) {
    hipLaunchKernelGGL(cluster_offsets, dim3(1), block, 0, h->stream, c.a, G);
    HIP_TRY(hipGetLastError());
    if ((rc = copy_out(h->stream, offsets_out, c.a.offsets, (size_t)(G + 2) * 4, mem)) != PFB_OK) return rc;
    if (n > 0) {
      const uint32_t tiles = blocks_for(n, kPartTile);
      const bool two = G + 1 > kDigits;
      // the last pass writes the caller's array where that is device memory
      uint32_t* d_order = mem == PFB_MEM_DEVICE ? order_out : (two ? c.a.order_b : c.a.order_a);
      const uint32_t* src = nullptr;
      for (int pass = 0; pass < (two ? 2 : 1); ++pass) {
        const uint32_t shift = 8 * pass;
        const uint32_t digits = pass == 0 ? std::min(G + 1, kDigits) : (G >> 8) + 1;  // the digits that occur
        uint32_t* dst = (two && pass == 0) ? c.a.order_a : d_order;
        hipLaunchKernelGGL(part_hist, dim3(tiles), block, 0, h->stream, c.a, src, G, shift, tiles);
        hipLaunchKernelGGL(part_scan, dim3(1), block, 0, h->stream, c.a.table, digits * tiles);
        hipLaunchKernelGGL(part_scatter, dim3(tiles), block, 0, h->stream, c.a, src, dst, G, shift, tiles);
        HIP_TRY(hipGetLastError());
        src = dst;
      }
      c.ran(two ? "pfb_cluster_part2" : "pfb_cluster_part1");
      if (mem == PFB_MEM_HOST && (rc = copy_out(h->stream, order_out, d_order, (size_t)n * 4, mem)) != PFB_OK) return rc;
    }
  }
  if ((rc = fetch(h->stream, c.a.ctl, &ctl)) != PFB_OK) return rc;
  pfb_cluster_stats stats{};
  stats.outside = ctl.outside;
  stats.unassigned = ctl.unassigned;
  stats.dense_cells = ctl.dense;
  stats.border_cells = ctl.border;
  stats.components = ctl.components;
  stats.hook_rounds = rounds;
  h->stats = stats;
  h->last_kernel = c.kernels;
  return PFB_OK;
}

}  // namespace

extern "C" int pfb_cluster_describe(const pfb_cluster_config* cfg, uint64_t n, pfb_cluster_plan* plan_out) {
  return pfb::abi_guard([&]() -> int {
    Settings s;
    const int rc = cluster_check(cfg, plan_out ? &s : nullptr);
    if (rc != PFB_OK) return rc;
    if (n > kMaxItems) return PFB_ERR_BAD_ARG;
    pfb_cluster_plan plan{};
    plan.scratch_bytes = scratch_bytes(capacity_for(n), s.cells);
    plan.cells = s.cells;
    plan.lds_cells = kLdsCells;
    plan.hist_tile = kHistTile;
    plan.label_tile = kLabelTile;
    plan.part_tile = kPartTile;
    plan.block_u = s.bu;
    plan.block_v = s.bv;
    plan.lds_bytes = s.cells <= kLdsCells ? kLdsCells * 4 : 0;  // a static array of the tier's whole bound
    plan.max_clusters = kMaxClusters;
    std::snprintf(plan.histogram_kernel, sizeof(plan.histogram_kernel), "%s", hist_name(s.cells <= kLdsCells));
    std::snprintf(plan.component_kernel, sizeof(plan.component_kernel), "%s", "pfb_cluster_hook");
    std::snprintf(plan.partition_kernel, sizeof(plan.partition_kernel), "%s", "pfb_cluster_part1");
    *plan_out = plan;
    return PFB_OK;
  });
}

extern "C" int pfb_cluster_create(const pfb_cluster_config* cfg, pfb_cluster_handle** out) {
  return pfb::abi_guard([&]() -> int {
    if (!out) return PFB_ERR_BAD_ARG;
    *out = nullptr;
    Settings s;
    int rc = cluster_check(cfg, &s);
    if (rc != PFB_OK) return rc;
    int dev = 0;
    rc = pfb::resolve_device(cfg->device_id, &dev);
    if (rc != PFB_OK) return rc;
    pfb_cluster_handle* h = new pfb_cluster_handle();
    h->device = dev;
    h->s = s;
    *out = h;
    return PFB_OK;
  });
}

extern "C" int pfb_cluster_destroy(pfb_cluster_handle* h) {
  return pfb::abi_guard([&]() -> int {
    return destroy_list(h);
  });
}

extern "C" int pfb_cluster_set_stream(pfb_cluster_handle* h, void* hip_stream) {
  return pfb::abi_guard([&]() -> int {
    return set_list_stream(h, hip_stream);
  });
}

extern "C" int pfb_cluster_sync(pfb_cluster_handle* h) {
  return pfb::abi_guard([&]() -> int {
    return sync_list(h);
  });
}

extern "C" int pfb_cluster_get_device(const pfb_cluster_handle* h, int* device_id) {
  return pfb::abi_guard([&]() -> int {
    return list_device(h, device_id);
  });
}

extern "C" int pfb_cluster_set_tier(pfb_cluster_handle* h, int tier) {
  return pfb::abi_guard([&]() -> int {
    if (!h || tier < kTierAuto || tier > kTierGlobal) return PFB_ERR_BAD_ARG;
    if (tier == kTierLds && h->s.cells > kLdsCells) return PFB_ERR_UNSUPPORTED;
    h->tier = tier;
    return PFB_OK;
  });
}

extern "C" int pfb_cluster_run(pfb_cluster_handle* h, const pfb_cluster_item* items, uint64_t n, uint32_t mem,
                               pfb_cluster_group* groups_out, uint64_t capacity, uint64_t* count_out, int32_t* labels_out,
                               uint32_t* order_out, uint32_t* offsets_out) {
  return pfb::abi_guard([&]() -> int {
    const int rc = check_list(h, items, n, kMaxItems, mem, 8);
    if (rc != PFB_OK) return rc;
    if (!count_out || (capacity > 0 && !groups_out) || (n > 0 && !labels_out)) return PFB_ERR_BAD_ARG;
    if (!order_out != !offsets_out) return PFB_ERR_BAD_ARG;
    if (mem == PFB_MEM_DEVICE && (misaligned(groups_out, 8) || misaligned(labels_out, 4) || misaligned(order_out, 4) ||
                                  misaligned(offsets_out, 4)))
      return PFB_ERR_BAD_ARG;
    return run(h, items, n, mem, groups_out, capacity, count_out, labels_out, order_out, offsets_out);
  });
}

extern "C" int pfb_cluster_histogram(pfb_cluster_handle* h, const pfb_cluster_item* items, uint64_t n, uint32_t mem,
                                     uint32_t* counts_out, uint64_t capacity_cells) {
  return pfb::abi_guard([&]() -> int {
    int rc = check_list(h, items, n, kMaxItems, mem, 8);
    if (rc != PFB_OK) return rc;
    if (!counts_out) return PFB_ERR_BAD_ARG;
    if (mem == PFB_MEM_DEVICE && misaligned(counts_out, 4)) return PFB_ERR_BAD_ARG;
    if (capacity_cells < h->s.cells) return PFB_ERR_CAPACITY;
    DeviceGuard g(h->device);
    if ((rc = reserve(h, n)) != PFB_OK) return rc;
    Call c(h, (uint32_t)n);
    if ((rc = histogram(c, items, mem)) != PFB_OK) return rc;
    if ((rc = copy_out(h->stream, counts_out, c.a.H, (size_t)h->s.cells * 4, mem)) != PFB_OK) return rc;
    HIP_TRY(hipStreamSynchronize(h->stream));
    h->last_kernel = c.kernels;
    return PFB_OK;
  });
}

extern "C" int pfb_cluster_cell_roots(pfb_cluster_handle* h, const pfb_cluster_item* items, uint64_t n, uint32_t mem,
                                      int32_t* roots_out, uint64_t capacity_cells) {
  return pfb::abi_guard([&]() -> int {
    int rc = check_list(h, items, n, kMaxItems, mem, 8);
    if (rc != PFB_OK) return rc;
    if (!roots_out) return PFB_ERR_BAD_ARG;
    if (mem == PFB_MEM_DEVICE && misaligned(roots_out, 4)) return PFB_ERR_BAD_ARG;
    if (capacity_cells < h->s.cells) return PFB_ERR_CAPACITY;
    DeviceGuard g(h->device);
    if ((rc = reserve(h, n)) != PFB_OK) return rc;
    Call c(h, (uint32_t)n);
    Control ctl{};
    uint64_t rounds = 0;
    if ((rc = histogram(c, items, mem)) != PFB_OK) return rc;
    if ((rc = components(c, &ctl, &rounds)) != PFB_OK) return rc;
    if ((rc = copy_out(h->stream, roots_out, c.a.croot, (size_t)h->s.cells * 4, mem)) != PFB_OK) return rc;
    HIP_TRY(hipStreamSynchronize(h->stream));
    h->last_kernel = c.kernels;
    return PFB_OK;
  });
}

extern "C" int pfb_cluster_gather(pfb_cluster_handle* h, const void* src, uint32_t elem_bytes, const uint32_t* order,
                                  uint64_t n, void* dst) {
  return pfb::abi_guard([&]() -> int {
    if (!h || (elem_bytes != 4 && elem_bytes != 8) || n > kMaxItems) return PFB_ERR_BAD_ARG;
    if (n > 0 && (!src || !order || !dst)) return PFB_ERR_BAD_ARG;
    if (misaligned(src, elem_bytes) || misaligned(dst, elem_bytes) || misaligned(order, 4)) return PFB_ERR_BAD_ARG;
    if (n == 0) return PFB_OK;
    DeviceGuard g(h->device);
    const dim3 grid(blocks_for((uint32_t)n, kThreads)), block(kThreads);
    if (elem_bytes == 4)
      hipLaunchKernelGGL(cluster_gather<uint32_t>, grid, block, 0, h->stream, static_cast<const uint32_t*>(src), order,
                         (uint32_t)n, static_cast<uint32_t*>(dst));
    else
      hipLaunchKernelGGL(cluster_gather<u64>, grid, block, 0, h->stream, static_cast<const u64*>(src), order, (uint32_t)n,
                         static_cast<u64*>(dst));
    HIP_TRY(hipGetLastError());
    h->last_kernel = "pfb_cluster_gather";
    return PFB_OK;
  });
}

extern "C" const char* pfb_cluster_last_kernel(const pfb_cluster_handle* h) { return h ? h->last_kernel.c_str() : ""; }

extern "C" int pfb_cluster_get_stats(const pfb_cluster_handle* h, pfb_cluster_stats* stats_out) {
  return pfb::abi_guard([&]() -> int {
    return list_stats(h, stats_out);
  });
}

extern "C" int pfb_cluster_items_from_pdws(const pfb_pdw* pdws, uint64_t n, uint64_t stride_bytes, double freq0,
                                           double freq_step, double pw_step, pfb_cluster_item* items_out) {
  return pfb::abi_guard([&]() -> int {
    if ((n > 0 && (!pdws || !items_out)) || n > (1ull << 31)) return PFB_ERR_BAD_ARG;
    if (stride_bytes < sizeof(pfb_pdw) || stride_bytes % 8) return PFB_ERR_BAD_ARG;
    if (!std::isfinite(freq0) || !std::isfinite(freq_step) || freq_step <= 0) return PFB_ERR_BAD_ARG;
    if (!std::isfinite(pw_step) || pw_step < 0) return PFB_ERR_BAD_ARG;
    const char* at = reinterpret_cast<const char*>(pdws);
    auto fits = [](double x) { return std::isfinite(x) && x >= -2147483648.0 && x <= 2147483647.0; };
    for (uint64_t i = 0; i < n; ++i, at += stride_bytes) {
      pfb_pdw p;
      std::memcpy(&p, at, sizeof(p));
      const double u = std::floor((p.freq - freq0) / freq_step);
      const double v = pw_step > 0 ? std::floor(p.pw / pw_step) : 0.0;
      if (fits(u) && fits(v)) {
        items_out[i].u = (int32_t)u;
        items_out[i].v = (int32_t)v;
      } else {
        items_out[i].u = INT32_MIN;
        items_out[i].v = 0;
      }
    }
    return PFB_OK;
  });
}
