// pfb_assoc.hip -- PDW association (pfb_assoc_* in include/pfb_channelizer.h, where every figure is defined): one record
// per pulse from a time-ordered list of (start, length, cell, weight) rows, kernels and host side.
//   assoc_prep        one lane per item: the 24-byte items become separate arrays (start, end + g, cell, length, weight
//                     key), the order of the starts and the bound 2^62 are checked, label[i] = i.
//   assoc_link<LDS>   one lane per item walks the item's window: the lowest linked j, the number of linked j, whether
//                     the window clipped the search.  LDS = true: the workgroup stages start and cell of its kTile items
//                     and of the K + 1 behind them, and its own end + g, in LDS with coalesced loads; at one step of the
//                     walk the lanes of a wave read consecutive entries, so the LDS reads are conflict free.
//                     LDS = false reads the same arrays through the caches.
//   assoc_hook        one lane per item that has links walks them again: where the labels of the two ends differ, an
//                     atomicMin on the larger label's entry with the smaller.  Sets the round's flag when it hooked.
//   assoc_jump        label[i] = label[label[i]], in place: a read gives the old or the new entry, both ancestors.
//   assoc_count / list_scan / assoc_scatter   the groups' numbers: root flags (label[i] == i), a scan of the
//                     workgroups' counts, an ordered scatter that also clears the group's accumulators.
//   assoc_gather      one lane per item: its group's number into the output labels, integer min / max / add into the
//                     group's accumulators, one 64-bit max of (key << 32 | ~index) for the best member.
//   assoc_emit        one lane per group: the 48-byte record, and the run's largest group and linked items.
// Whether a round hooked is read by the host, one flag a round.
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

constexpr uint32_t kMaxItems = 1u << 20, kMaxReach = 64, kMaxWindow = 4096;
constexpr uint32_t kMaxSlack = 0x7fffffffu;
constexpr uint32_t kLdsWindow = 1024;    // the LDS tier's bound
constexpr uint32_t kTile = 256;          // items of one workgroup of the edge pass: one to a lane
constexpr uint32_t kNumTile = 1024;      // items of one workgroup of the numbering: four to a lane
constexpr uint32_t kStaged = kTile + kLdsWindow + 4;  // entries the LDS tier stages at most (K + 1 behind the tile), in whole 16 bytes
constexpr u64 kMaxTick = 1ull << 62;
constexpr int kMaxRounds = 64;           // after which the host gives up

struct Control {            // what a call hands back to the host
  u64 edges, clipped, largest, linked;
  uint32_t groups, bad;     // bad: the list is out of order or holds an end + g >= 2^62
  uint32_t hooked[kMaxRounds];
};

struct Arrays {             // the items as separate arrays, and what the passes write; all in the handle's scratch
  u64* start;
  u64* lim;                 // end + g
  int32_t* cell;
  uint32_t* length;
  uint32_t* key;            // the weight's order-preserving key
  int32_t* label;           // padded to a whole kNumTile
  int32_t* first;           // the lowest linked j, -1 for none
  int32_t* count;           // linked j
  int32_t* group;           // the output labels
  uint32_t* counts;         // roots of every numbering workgroup, then (list_scan) those before it
  // per group, by its number
  uint32_t* root;
  u64* acc_end;
  u64* acc_sum;
  u64* acc_best;
  uint32_t* acc_members;
  int32_t* acc_lo;
  int32_t* acc_hi;
  pfb_assoc_group* records;
  Control* ctl;
  uint32_t n, K, Rc;
};
static_assert(sizeof(Control) == 296 && sizeof(Arrays) == 168, "the kernels' parameter layout");

// the order of the floats, -0 under +0, as the order of unsigned integers
__host__ __device__ __forceinline__ uint32_t weight_key(uint32_t bits) {
  return (bits & 0x80000000u) ? ~bits : bits ^ 0x80000000u;
}

__global__ void __launch_bounds__(kThreads) assoc_prep(const u64* items, const Arrays a, u64 g) {
  const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
  if (i >= a.n) return;
  const u64* it = items + 3 * (size_t)i;  // 24 bytes an item, 8-byte aligned
  const u64 start = it[0], w1 = it[1], w2 = it[2];
  const uint32_t length = (uint32_t)w1;
  // start < 2^62 first: the sum below cannot wrap then
  bool bad = start >= kMaxTick || start + length + g >= kMaxTick;
  if (i > 0) bad |= start < it[-3];
  if (bad) atomicOr(&a.ctl->bad, 1u);
  a.start[i] = start;
  a.lim[i] = start + length + g;
  a.cell[i] = (int32_t)(w1 >> 32);
  a.length[i] = length;
  a.key[i] = weight_key((uint32_t)w2);
  a.label[i] = (int32_t)i;
}

__device__ __forceinline__ bool cells_within(int32_t x, int32_t y, uint32_t Rc) {
  const long long d = (long long)x - (long long)y;
  return (d < 0 ? -d : d) <= (long long)Rc;
}

template <bool LDS>
__global__ void __launch_bounds__(kThreads) assoc_link(const Arrays a) {
  __shared__ u64 s_start[LDS ? kStaged : 1];
  __shared__ int32_t s_cell[LDS ? kStaged : 1];
  __shared__ u64 s_lim[LDS ? kTile : 1];
  const uint32_t base = blockIdx.x * kTile;  // base < n: the grid is ceil(n / kTile)
  const uint32_t i = base + threadIdx.x;
  if (LDS) {
    // K <= kLdsWindow here (the host refuses the tier otherwise): staged <= kStaged
    const uint32_t staged = min(kTile + a.K + 1, a.n - base);
    for (uint32_t k = threadIdx.x; k < staged; k += kThreads) {  // at most ceil(kStaged / kThreads) trips
      s_start[k] = a.start[base + k];
      s_cell[k] = a.cell[base + k];
    }
    if (i < a.n) s_lim[threadIdx.x] = a.lim[i];
    __syncthreads();
  }
  uint32_t links = 0, clip = 0;
  if (i < a.n) {
    const u64 lim = LDS ? s_lim[threadIdx.x] : a.lim[i];
    const int32_t ci = LDS ? s_cell[threadIdx.x] : a.cell[i];
    const uint32_t last = min(i + a.K, a.n - 1);
    int32_t first = -1;
    for (uint32_t j = i + 1; j <= last; ++j) {  // at most K trips
      const u64 sj = LDS ? s_start[j - base] : a.start[j];
      if (sj > lim) break;  // sorted: none behind j starts sooner
      const int32_t cj = LDS ? s_cell[j - base] : a.cell[j];
      if (!cells_within(ci, cj, a.Rc)) continue;
      if (first < 0) first = (int32_t)j;
      ++links;
    }
    const uint32_t over = i + a.K + 1;  // <= 2^20 + 4096: no wrap
    if (over < a.n) clip = (LDS ? s_start[over - base] : a.start[over]) <= lim;
    a.first[i] = first;
    a.count[i] = (int32_t)links;
  }
  // the wave's sums, one atomic each
  for (int d = 32; d >= 1; d >>= 1) {
    links += __shfl_xor(links, d, 64);
    clip += __shfl_xor(clip, d, 64);
  }
  if ((threadIdx.x & 63) == 0) {
    if (links) atomicAdd(&a.ctl->edges, (u64)links);
    if (clip) atomicAdd(&a.ctl->clipped, (u64)clip);
  }
}

__global__ void __launch_bounds__(kThreads) assoc_hook(const Arrays a, uint32_t round) {
  const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
  if (i >= a.n) return;
  int32_t left = a.count[i];
  if (left == 0) return;
  const u64 lim = a.lim[i];
  const int32_t ci = a.cell[i];
  const int32_t ri = a.label[i];
  const uint32_t last = min(i + a.K, a.n - 1);
  bool hooked = false;
  for (uint32_t j = (uint32_t)a.first[i]; j <= last && left > 0; ++j) {  // at most K trips
    if (a.start[j] > lim) break;
    if (!cells_within(ci, a.cell[j], a.Rc)) continue;
    --left;
    const int32_t rj = a.label[j];
    if (ri == rj) continue;
    // both are indices of the edge's component and each entry is at most its index: the entry only decreases
    atomicMin(&a.label[max(ri, rj)], min(ri, rj));
    hooked = true;
  }
  if (hooked) a.ctl->hooked[round] = 1u;
}

__global__ void __launch_bounds__(kThreads) assoc_jump(int32_t* label, uint32_t n) {
  const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
  if (i >= n) return;
  const int32_t p = label[i];
  const int32_t q = label[p];  // 0 <= q <= p <= i
  if (q != p) label[i] = q;
}

// a lane takes 4 consecutive items, a workgroup kNumTile; the labels are padded to a whole tile
__device__ __forceinline__ void roots_of(const Arrays& a, uint32_t i0, bool root[4]) {
  const int4 l = *reinterpret_cast<const int4*>(a.label + i0);
  root[0] = i0 + 0 < a.n && l.x == (int32_t)(i0 + 0);
  root[1] = i0 + 1 < a.n && l.y == (int32_t)(i0 + 1);
  root[2] = i0 + 2 < a.n && l.z == (int32_t)(i0 + 2);
  root[3] = i0 + 3 < a.n && l.w == (int32_t)(i0 + 3);
}

__global__ void __launch_bounds__(kThreads) assoc_count(const Arrays a) {
  bool root[4];
  roots_of(a, blockIdx.x * kNumTile + threadIdx.x * 4, root);
  uint32_t total;
  (void)block_scan((uint32_t)root[0] + root[1] + root[2] + root[3], &total);
  if (threadIdx.x == 0) a.counts[blockIdx.x] = total;
}

__global__ void __launch_bounds__(kThreads) assoc_scatter(const Arrays a) {
  const uint32_t i0 = blockIdx.x * kNumTile + threadIdx.x * 4;
  bool root[4];
  roots_of(a, i0, root);
  uint32_t total;
  uint32_t at = a.counts[blockIdx.x] + block_scan((uint32_t)root[0] + root[1] + root[2] + root[3], &total);
  for (uint32_t k = 0; k < 4; ++k) {
    if (!root[k]) continue;
    a.root[at] = i0 + k;  // at < the number of roots <= n
    a.acc_end[at] = 0;
    a.acc_sum[at] = 0;
    a.acc_best[at] = 0;
    a.acc_members[at] = 0;
    a.acc_lo[at] = 0x7fffffff;
    a.acc_hi[at] = (int32_t)0x80000000;
    a.group[i0 + k] = (int32_t)at;  // the root's own number: what assoc_gather looks up
    ++at;
  }
}

__global__ void __launch_bounds__(kThreads) assoc_gather(const Arrays a, int32_t* labels_out, u64 g) {
  const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
  if (i >= a.n) return;
  const uint32_t e = (uint32_t)a.group[a.label[i]];  // the labels are flat: label[i] is a root
  labels_out[i] = (int32_t)e;
  const int32_t c = a.cell[i];
  atomicMax(&a.acc_end[e], a.lim[i] - g);
  atomicAdd(&a.acc_sum[e], (u64)a.length[i]);
  atomicMax(&a.acc_best[e], ((u64)a.key[i] << 32) | (0xffffffffu - i));
  atomicAdd(&a.acc_members[e], 1u);
  atomicMin(&a.acc_lo[e], c);
  atomicMax(&a.acc_hi[e], c);
}

__global__ void __launch_bounds__(kThreads) assoc_emit(const Arrays a, uint32_t groups) {
  const uint32_t e = blockIdx.x * kThreads + threadIdx.x;
  uint32_t members = 0;
  if (e < groups) {
    const uint32_t root = a.root[e];
    const uint32_t best = 0xffffffffu - (uint32_t)(a.acc_best[e] & 0xffffffffu);
    members = a.acc_members[e];
    pfb_assoc_group r;
    r.first_tick = a.start[root];
    r.end_tick = a.acc_end[e];
    r.length_sum = a.acc_sum[e];
    r.members = members;
    r.first_item = root;
    r.best_item = best;
    r.best_cell = a.cell[best];
    r.cell_lo = a.acc_lo[e];
    r.cell_hi = a.acc_hi[e];
    a.records[e] = r;
  }
  uint32_t most = members, linked = members >= 2 ? members : 0;
  for (int d = 32; d >= 1; d >>= 1) {
    most = max(most, (uint32_t)__shfl_xor(most, d, 64));
    linked += __shfl_xor(linked, d, 64);
  }
  if ((threadIdx.x & 63) == 0) {
    atomicMax(&a.ctl->largest, (u64)most);
    if (linked) atomicAdd(&a.ctl->linked, (u64)linked);
  }
}

// ---------------------------------------------------------------------------------
// host: checks and plan

struct Settings {
  uint32_t Rc = 0, g = 0, K = 0;
};

// the carving of a handle's scratch for lists of up to cap items, cap a multiple of kNumTile: every array once.
// *items: where a host list is staged
Arrays carve(Carver& c, size_t cap, pfb_assoc_item** items) {
  Arrays a{};
  *items = c.array<pfb_assoc_item>(cap);
  a.start = c.array<u64>(cap);
  a.lim = c.array<u64>(cap);
  a.cell = c.array<int32_t>(cap);
  a.length = c.array<uint32_t>(cap);
  a.key = c.array<uint32_t>(cap);
  a.label = c.array<int32_t>(cap);
  a.first = c.array<int32_t>(cap);
  a.count = c.array<int32_t>(cap);
  a.group = c.array<int32_t>(cap);
  a.counts = c.array<uint32_t>(kMaxItems / kNumTile);
  a.root = c.array<uint32_t>(cap);
  a.acc_end = c.array<u64>(cap);
  a.acc_sum = c.array<u64>(cap);
  a.acc_best = c.array<u64>(cap);
  a.acc_members = c.array<uint32_t>(cap);
  a.acc_lo = c.array<int32_t>(cap);
  a.acc_hi = c.array<int32_t>(cap);
  a.records = c.array<pfb_assoc_group>(cap);
  a.ctl = c.array<Control>(1);
  return a;
}

size_t scratch_bytes(size_t cap) {
  Carver c;
  pfb_assoc_item* items;
  carve(c, cap, &items);
  return c.bytes();
}

size_t capacity_for(uint64_t n) { return round_up(std::max<uint64_t>(n, 1), kNumTile); }

const char* link_name(bool lds) { return lds ? "pfb_assoc_link_lds" : "pfb_assoc_link_global"; }

uint32_t lds_bytes_for(uint32_t K) {
  return K <= kLdsWindow ? kStaged * 12 + kTile * 8 : 0;  // static arrays of the tier's whole bound; the global tier has none
}

// Everything pfb_assoc_describe and pfb_assoc_create check before the device, in the order the header states
int assoc_check(const pfb_assoc_config* cfg, Settings* s) {
  if (!cfg || !s || cfg->struct_size != sizeof(pfb_assoc_config)) return PFB_ERR_BAD_ARG;
  if (cfg->cell_reach > kMaxReach) return PFB_ERR_BAD_ARG;
  if (cfg->slack_ticks > kMaxSlack) return PFB_ERR_BAD_ARG;
  if (cfg->window_items < 1 || cfg->window_items > kMaxWindow) return PFB_ERR_BAD_ARG;
  if (cfg->flags != 0) return PFB_ERR_BAD_ARG;
  s->Rc = cfg->cell_reach;
  s->g = cfg->slack_ticks;
  s->K = cfg->window_items;
  return PFB_OK;
}

}  // namespace

struct pfb_assoc_handle : ListHandle {
  Settings s;
  int tier = kTierAuto;
  pfb_assoc_stats stats{};
};

namespace {

bool runs_lds(const pfb_assoc_handle* h) { return h->tier == kTierAuto ? h->s.K <= kLdsWindow : h->tier == kTierLds; }

// one call's view of the scratch
struct Call : ListCall {
  pfb_assoc_handle* h;
  pfb_assoc_item* items = nullptr;  // where a host list is staged
  Arrays a;
  Call(pfb_assoc_handle* hh, uint32_t n) : h(hh) {
    Carver c{hh->d_scratch};
    a = carve(c, hh->cap, &items);
    a.n = n;
    a.K = hh->s.K;
    a.Rc = hh->s.Rc;
  }
};

int reserve(pfb_assoc_handle* h, uint64_t n) {
  const size_t cap = capacity_for(n);
  return cap > h->cap ? h->ensure(cap, scratch_bytes(cap)) : PFB_OK;  // the size only when it grows
}

// The list onto the device, the first pass and the edge pass; PFB_ERR_BAD_ARG for a list the device refuses.  n > 0
int begin_call(Call& c, const pfb_assoc_item* items, uint32_t mem, Control* ctl) {
  pfb_assoc_handle* h = c.h;
  const uint32_t n = c.a.n;
  const u64* d_items = reinterpret_cast<const u64*>(items);
  if (mem == PFB_MEM_HOST) {
    HIP_TRY(hipMemcpyAsync(c.items, items, (size_t)n * sizeof(pfb_assoc_item), hipMemcpyHostToDevice, h->stream));
    d_items = reinterpret_cast<const u64*>(c.items);
  }
  // the padding of the labels is never a root: -1 is no index
  HIP_TRY(hipMemsetAsync(c.a.label, 0xff, h->cap * sizeof(int32_t), h->stream));
  HIP_TRY(hipMemsetAsync(c.a.ctl, 0, sizeof(Control), h->stream));
  const dim3 block(kThreads);
  hipLaunchKernelGGL(assoc_prep, dim3((n + kThreads - 1) / kThreads), block, 0, h->stream, d_items, c.a, (u64)h->s.g);
  const dim3 tiles((n + kTile - 1) / kTile);
  const bool lds = runs_lds(h);
  if (lds) hipLaunchKernelGGL(assoc_link<true>, tiles, block, 0, h->stream, c.a);
  else hipLaunchKernelGGL(assoc_link<false>, tiles, block, 0, h->stream, c.a);
  HIP_TRY(hipGetLastError());
  c.ran("pfb_assoc_prep");
  c.ran(link_name(lds));
  const int rc = fetch(h->stream, c.a.ctl, ctl);
  if (rc != PFB_OK) return rc;
  return ctl->bad ? PFB_ERR_BAD_ARG : PFB_OK;
}

int run(pfb_assoc_handle* h, const pfb_assoc_item* items, uint64_t n64, uint32_t mem, pfb_assoc_group* groups_out,
        uint64_t capacity, uint64_t* count_out, int32_t* labels_out) {
  DeviceGuard g(h->device);
  if (n64 == 0) {
    *count_out = 0;
    h->stats = pfb_assoc_stats{};
    h->last_kernel.clear();
    return PFB_OK;
  }
  int rc = reserve(h, n64);
  if (rc != PFB_OK) return rc;
  const uint32_t n = (uint32_t)n64;
  Call c(h, n);
  Control ctl{};
  rc = begin_call(c, items, mem, &ctl);
  if (rc != PFB_OK) return rc;
  const dim3 block(kThreads), grid((n + kThreads - 1) / kThreads);
  int passes = 1;  // ceil(log2 n) + 1: a chain of roots is shorter than n
  while ((1ull << (passes - 1)) < n) ++passes;
  int rounds = 0;
  if (ctl.edges > 0) {
    rounds = hook_until_still(h->stream, c.a.ctl->hooked, kMaxRounds, [&](uint32_t round) -> int {
      hipLaunchKernelGGL(assoc_hook, grid, block, 0, h->stream, c.a, round);
      for (int p = 0; p < passes; ++p) hipLaunchKernelGGL(assoc_jump, grid, block, 0, h->stream, c.a.label, n);
      HIP_TRY(hipGetLastError());
      return PFB_OK;
    });
    if (rounds < 0) return rounds;
    c.ran("pfb_assoc_hook");
    c.ran("pfb_assoc_jump");
  }
  const unsigned blocks = (n + kNumTile - 1) / kNumTile;
  hipLaunchKernelGGL(assoc_count, dim3(blocks), block, 0, h->stream, c.a);
  hipLaunchKernelGGL(list_scan<true>, dim3(1), block, 0, h->stream, c.a.counts, blocks, &c.a.ctl->groups);
  hipLaunchKernelGGL(assoc_scatter, dim3(blocks), block, 0, h->stream, c.a);
  HIP_TRY(hipGetLastError());
  c.ran("pfb_assoc_number");
  rc = fetch(h->stream, c.a.ctl, &ctl);
  if (rc != PFB_OK) return rc;
  *count_out = ctl.groups;
  if (ctl.groups > capacity) return PFB_ERR_CAPACITY;
  // the numbers go to a scratch array when the caller's labels are host memory
  int32_t* d_labels = mem == PFB_MEM_DEVICE ? labels_out : c.a.first;
  hipLaunchKernelGGL(assoc_gather, grid, block, 0, h->stream, c.a, d_labels, (u64)h->s.g);
  hipLaunchKernelGGL(assoc_emit, dim3((ctl.groups + kThreads - 1) / kThreads), block, 0, h->stream, c.a, ctl.groups);
  HIP_TRY(hipGetLastError());
  c.ran("pfb_assoc_gather");
  if (mem == PFB_MEM_HOST && (rc = copy_out(h->stream, labels_out, d_labels, (size_t)n * sizeof(int32_t), mem)) != PFB_OK) return rc;
  rc = copy_out(h->stream, groups_out, c.a.records, (size_t)ctl.groups * sizeof(pfb_assoc_group), mem);
  if (rc != PFB_OK) return rc;
  rc = fetch(h->stream, c.a.ctl, &ctl);
  if (rc != PFB_OK) return rc;
  pfb_assoc_stats stats{};
  stats.groups = ctl.groups;
  stats.edges = ctl.edges;
  stats.clipped = ctl.clipped;
  stats.largest_group = ctl.largest;
  stats.linked_items = ctl.linked;
  stats.rounds = rounds;
  h->stats = stats;
  h->last_kernel = c.kernels;
  return PFB_OK;
}

}  // namespace

extern "C" int pfb_assoc_describe(const pfb_assoc_config* cfg, uint64_t n, pfb_assoc_plan* plan_out) {
  return pfb::abi_guard([&]() -> int {
    Settings s;
    const int rc = assoc_check(cfg, plan_out ? &s : nullptr);
    if (rc != PFB_OK) return rc;
    if (n > kMaxItems) return PFB_ERR_BAD_ARG;
    pfb_assoc_plan plan{};
    plan.scratch_bytes = scratch_bytes(capacity_for(n));
    plan.tile_items = kTile;
    plan.lds_window = kLdsWindow;
    plan.lds_bytes = lds_bytes_for(s.K);
    std::snprintf(plan.link_kernel, sizeof(plan.link_kernel), "%s", link_name(s.K <= kLdsWindow));
    std::snprintf(plan.component_kernel, sizeof(plan.component_kernel), "%s", "pfb_assoc_hook");
    std::snprintf(plan.record_kernel, sizeof(plan.record_kernel), "%s", "pfb_assoc_gather");
    *plan_out = plan;
    return PFB_OK;
  });
}

extern "C" int pfb_assoc_create(const pfb_assoc_config* cfg, pfb_assoc_handle** out) {
  return pfb::abi_guard([&]() -> int {
    if (!out) return PFB_ERR_BAD_ARG;
    *out = nullptr;
    Settings s;
    int rc = assoc_check(cfg, &s);
    if (rc != PFB_OK) return rc;
    int dev = 0;
    rc = pfb::resolve_device(cfg->device_id, &dev);
    if (rc != PFB_OK) return rc;
    pfb_assoc_handle* h = new pfb_assoc_handle();
    h->device = dev;
    h->s = s;
    *out = h;
    return PFB_OK;
  });
}

extern "C" int pfb_assoc_destroy(pfb_assoc_handle* h) {
  return pfb::abi_guard([&]() -> int {
    return destroy_list(h);
  });
}

extern "C" int pfb_assoc_set_stream(pfb_assoc_handle* h, void* hip_stream) {
  return pfb::abi_guard([&]() -> int {
    return set_list_stream(h, hip_stream);
  });
}

extern "C" int pfb_assoc_sync(pfb_assoc_handle* h) {
  return pfb::abi_guard([&]() -> int {
    return sync_list(h);
  });
}

extern "C" int pfb_assoc_get_device(const pfb_assoc_handle* h, int* device_id) {
  return pfb::abi_guard([&]() -> int {
    return list_device(h, device_id);
  });
}

extern "C" int pfb_assoc_set_tier(pfb_assoc_handle* h, int tier) {
  return pfb::abi_guard([&]() -> int {
    if (!h || tier < kTierAuto || tier > kTierGlobal) return PFB_ERR_BAD_ARG;
    if (tier == kTierLds && h->s.K > kLdsWindow) return PFB_ERR_UNSUPPORTED;
    h->tier = tier;
    return PFB_OK;
  });
}

extern "C" int pfb_assoc_run(pfb_assoc_handle* h, const pfb_assoc_item* items, uint64_t n, uint32_t mem,
                             pfb_assoc_group* groups_out, uint64_t capacity, uint64_t* count_out, int32_t* labels_out) {
  return pfb::abi_guard([&]() -> int {
    const int rc = check_list(h, items, n, kMaxItems, mem, 8);
    if (rc != PFB_OK) return rc;
    if (!count_out || (capacity > 0 && !groups_out) || (n > 0 && !labels_out)) return PFB_ERR_BAD_ARG;
    if (mem == PFB_MEM_DEVICE && (misaligned(groups_out, 8) || misaligned(labels_out, 4)))
      return PFB_ERR_BAD_ARG;
    return run(h, items, n, mem, groups_out, capacity, count_out, labels_out);
  });
}

extern "C" int pfb_assoc_links(pfb_assoc_handle* h, const pfb_assoc_item* items, uint64_t n, uint32_t mem,
                               int32_t* first_link_out, int32_t* link_count_out) {
  return pfb::abi_guard([&]() -> int {
    int rc = check_list(h, items, n, kMaxItems, mem, 8);
    if (rc != PFB_OK) return rc;
    if (n > 0 && (!first_link_out || !link_count_out)) return PFB_ERR_BAD_ARG;
    if (mem == PFB_MEM_DEVICE &&
        (misaligned(first_link_out, 4) || misaligned(link_count_out, 4)))
      return PFB_ERR_BAD_ARG;
    if (n == 0) {
      h->last_kernel.clear();
      return PFB_OK;
    }
    DeviceGuard g(h->device);
    rc = reserve(h, n);
    if (rc != PFB_OK) return rc;
    Call c(h, (uint32_t)n);
    Control ctl{};
    rc = begin_call(c, items, mem, &ctl);
    if (rc != PFB_OK) return rc;
    const size_t bytes = n * sizeof(int32_t);
    if ((rc = copy_out(h->stream, first_link_out, c.a.first, bytes, mem)) != PFB_OK) return rc;
    if ((rc = copy_out(h->stream, link_count_out, c.a.count, bytes, mem)) != PFB_OK) return rc;
    HIP_TRY(hipStreamSynchronize(h->stream));
    h->last_kernel = c.kernels;
    return PFB_OK;
  });
}

extern "C" const char* pfb_assoc_last_kernel(const pfb_assoc_handle* h) { return h ? h->last_kernel.c_str() : ""; }

extern "C" int pfb_assoc_get_stats(const pfb_assoc_handle* h, pfb_assoc_stats* stats_out) {
  return pfb::abi_guard([&]() -> int {
    return list_stats(h, stats_out);
  });
}

extern "C" int pfb_assoc_items_from_pdws(const pfb_pdw* pdws, uint64_t n, double t0, double tick_rate,
                                         pfb_assoc_item* items_out, uint32_t* order_out) {
  return pfb::abi_guard([&]() -> int {
    if ((n > 0 && (!pdws || !items_out || !order_out)) || n > (1ull << 31)) return PFB_ERR_BAD_ARG;
    if (!std::isfinite(tick_rate) || tick_rate <= 0 || !std::isfinite(t0)) return PFB_ERR_BAD_ARG;
    std::vector<pfb_assoc_item> item(n);
    for (uint64_t i = 0; i < n; ++i) {
      // to nearest, ties to even: llrint without its range trouble
      const double s = std::rint((pdws[i].toa - t0) * tick_rate), l = std::rint(pdws[i].pw * tick_rate);
      if (!std::isfinite(s) || s < 0 || s >= 4611686018427387904.0) return PFB_ERR_BAD_ARG;
      if (!std::isfinite(l) || l < 0 || l >= 4294967296.0) return PFB_ERR_BAD_ARG;
      item[i].start = (uint64_t)s;
      item[i].length = (uint32_t)l;
      item[i].cell = pdws[i].bin;
      item[i].weight = (float)pdws[i].mag;
      item[i].reserved = 0;
    }
    std::vector<uint32_t> order(n);
    std::iota(order.begin(), order.end(), 0u);
    std::stable_sort(order.begin(), order.end(), [&item](uint32_t x, uint32_t y) { return item[x].start < item[y].start; });
    for (uint64_t i = 0; i < n; ++i) {
      order_out[i] = order[i];
      items_out[i] = item[order[i]];
    }
    return PFB_OK;
  });
}
