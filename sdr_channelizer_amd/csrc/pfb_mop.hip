// pfb_mop.hip -- modulation on pulse (pfb_mop_* in include/pfb_channelizer.h, where every figure is defined): per pulse
// of a list the sums of lag products that give its mid frequency, its sweep and its phase flips; kernels and host side.
//   mop_prep          one lane per pulse: the pulse's geometry (n, flags, where u[0] lies) unless the host route has
//                     made it already, and the work lists of the tiers that take more than a wave (integer atomics:
//                     the order of a list decides only which workgroup takes which pulse).
//   mop_wave          one wave per pulse, four pulses to a workgroup.  The wave's lanes take 64 consecutive i at a time:
//                     the loads of u[i], u[i+1], u[i+2] and of u[i+L], u[i+L+1] are two coalesced streams whose overlap
//                     hits cache.  Negatives are listed in ascending order by a ballot and a count of the lanes below.
//   mop_group         one workgroup per pulse: each wave takes a quarter of the range as mop_wave takes a pulse, the
//                     four partial results are merged in wave order.
//   mop_split + mop_join   a pulse cut into parts of kPart indices, a workgroup per part as mop_group takes a pulse;
//                     the partial results and each part's first max_negatives negatives go to scratch, and a second
//                     kernel merges them in part order.
// Every tier is the same wave_range() over another range, and every merge goes in ascending order of i, so that the
// doubles of a cf32 pulse are summed in one fixed order per tier.  The integer sums are exact in any order.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <type_traits>
#include <vector>

#include "pfb_common.h"
#include "pfb_host.h"

// the definition's terms are single IEEE operations: a product and a sum never become one fused multiply-add
#pragma clang fp contract(off)

namespace {

using namespace pfb;
using u64 = unsigned long long;
using i64 = long long;

constexpr uint32_t kMaxN = 1u << 20, kMaxNegs = 128, kMaxTrim = 1u << 19, kNone = 0xffffffffu;
constexpr u64 kMaxPulses = 1ull << 24;
constexpr int kThreads = 256, kWaves = kThreads / 64;
// tools/mop_rate.py on one MI355X (profiles/mop_rate.jsonl)
constexpr uint32_t kGroupMin = 4096;      // the least n of mop_group
constexpr uint32_t kSplitMin = 1u << 15;  // the least n of mop_split
constexpr uint32_t kPart = 1u << 14;      // indices of one part of a split pulse
constexpr uint32_t kMaxParts = kMaxN / kPart;
constexpr uint32_t kGridCap = 2048;       // workgroups of a launch: eight to a CU
constexpr uint32_t kSlice = 1u << 16;     // pulses of one round of launches: what the fixed scratch is carved for
constexpr uint32_t kSlots = 256;          // split pulses of one mop_split launch
constexpr u64 kStageBytes = 32ull << 20;  // the host route's staging chunk
enum { kAuto = 0, kWave = 1, kGroup = 2, kSplit = 3 };

struct Work {      // a pulse as the measuring kernels see it
  u64 elem0;       // element of u[0]: (start - base_index + t) ld + column
  uint32_t n, flags;
};

__host__ __device__ inline Work geometry(const pfb_mop_pulse& p, u64 num_samples, u64 ld, u64 base, uint32_t trim) {
  Work w{0, 0, 0};
  const bool inside = p.column < ld && p.start >= base && p.start - base <= num_samples &&
                      (u64)p.length <= num_samples - (p.start - base);
  if (!inside) {
    w.flags = PFB_MOP_OUTSIDE | PFB_MOP_SHORT;
    return w;
  }
  if (p.length > 2 * trim) {
    const uint32_t m = p.length - 2 * trim;
    w.n = m < kMaxN ? m : kMaxN;
    if (m > kMaxN) w.flags |= PFB_MOP_TRUNCATED;
  }
  if (w.n < 3) w.flags |= PFB_MOP_SHORT;
  w.elem0 = (p.start - base + trim) * ld + p.column;
  return w;
}

struct Tiers {  // which kernel takes a pulse of n samples
  int forced;
  uint32_t group_min, split_min;
  __host__ __device__ int of(uint32_t n) const {
    if (forced != kAuto) return forced;
    return n < group_min ? kWave : n < split_min ? kGroup : kSplit;
  }
};

// sample e of the series as the definition's (I, Q)
template <int FMT> struct Fmt;
template <> struct Fmt<PFB_FMT_INT8_IQ> {
  using T = i64;
  struct alignas(2) E { int8_t i, q; };
};
template <> struct Fmt<PFB_FMT_INT16_IQ> {
  using T = i64;
  struct alignas(4) E { int16_t i, q; };
};
template <> struct Fmt<PFB_FMT_CF32> {
  using T = double;
  struct alignas(8) E { float i, q; };
};

// What a range of i contributes.  T = i64: s2re / s2im are the high limbs (term >> 32), s2re_lo / s2im_lo the low ones
// (term & 0xffffffff); T = double: the low limbs stay 0.
template <class T>
struct Acc {
  T energy, s1re, s1im, s2re, s2im, s2re_lo, s2im_lo;
  T peak;  // -1: no winner yet
  uint32_t peak_i, negs, first, last;
};
static_assert(sizeof(Acc<i64>) == 80 && sizeof(Acc<double>) == 80, "one partial slot fits both");

template <class T>
__device__ __forceinline__ Acc<T> empty_acc() {
  Acc<T> a;
  a.energy = a.s1re = a.s1im = a.s2re = a.s2im = a.s2re_lo = a.s2im_lo = T(0);
  a.peak = T(-1);
  a.peak_i = a.first = a.last = kNone;
  a.negs = 0;
  return a;
}

template <class T>
__device__ __forceinline__ void add_sums(Acc<T>& a, const Acc<T>& b) {
  a.energy += b.energy;
  a.s1re += b.s1re;
  a.s1im += b.s1im;
  a.s2re += b.s2re;
  a.s2im += b.s2im;
  a.s2re_lo += b.s2re_lo;
  a.s2im_lo += b.s2im_lo;
}

template <class T>
__device__ __forceinline__ void take_peak(Acc<T>& a, T peak, uint32_t at) {
  if (peak > a.peak || (peak == a.peak && at < a.peak_i)) {
    a.peak = peak;
    a.peak_i = at;
  }
}

// b covers the i after a's
template <class T>
__device__ __forceinline__ void merge(Acc<T>& a, const Acc<T>& b) {
  add_sums(a, b);
  take_peak(a, b.peak, b.peak_i);
  if (b.negs) {
    if (!a.negs) a.first = b.first;
    a.last = b.last;
  }
  a.negs += b.negs;
}

template <class T>
__device__ __forceinline__ void add_s2(Acc<T>& a, T re, T im) {
  if constexpr (std::is_same_v<T, double>) {
    a.s2re += re;
    a.s2im += im;
  } else {
    a.s2re += re >> 32;
    a.s2re_lo += re & 0xffffffffLL;
    a.s2im += im >> 32;
    a.s2im_lo += im & 0xffffffffLL;
  }
}

// One wave over i in [lo, hi) of a pulse of n samples whose u[0] is element elem0; every lane returns the wave's result.
// The first maxneg negatives of the range go to negs (LDS or global; may be null) in ascending order.
template <int FMT>
__device__ Acc<typename Fmt<FMT>::T> wave_range(const void* x, u64 elem0, u64 ld, uint32_t n, uint32_t lo, uint32_t hi,
                                                uint32_t* negs, uint32_t maxneg) {
  using T = typename Fmt<FMT>::T;
  using E = typename Fmt<FMT>::E;
  const E* u = reinterpret_cast<const E*>(x) + elem0;
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t L = n ? (n - 1) / 2 : 0;
  Acc<T> acc = empty_acc<T>();
  for (uint32_t i0 = lo; i0 < hi; i0 += 64) {  // uniform over the wave: the ballot sees every lane
    const uint32_t i = i0 + lane;
    bool neg = false;
    if (i < hi) {
      const E e0 = u[(u64)i * ld];
      const T I0 = (T)e0.i, Q0 = (T)e0.q;
      const T pw = I0 * I0 + Q0 * Q0;
      acc.energy += pw;
      if (pw > acc.peak) {  // a lane's i ascend: the first of equals stays
        acc.peak = pw;
        acc.peak_i = i;
      }
      if (i + 1 < n) {
        const E e1 = u[(u64)(i + 1) * ld];
        const T I1 = (T)e1.i, Q1 = (T)e1.q;
        const T a0 = I1 * I0 + Q1 * Q0, b0 = Q1 * I0 - I1 * Q0;
        acc.s1re += a0;
        acc.s1im += b0;
        if (i + 2 < n) {
          const E e2 = u[(u64)(i + 2) * ld];
          const T I2 = (T)e2.i, Q2 = (T)e2.q;
          const T a1 = I2 * I1 + Q2 * Q1, b1 = Q2 * I1 - I2 * Q1;
          neg = a1 * a0 + b1 * b0 < T(0);
        }
        if (i + L + 1 < n) {
          const E f0 = u[(u64)(i + L) * ld], f1 = u[(u64)(i + L + 1) * ld];
          const T J0 = (T)f0.i, R0 = (T)f0.q, J1 = (T)f1.i, R1 = (T)f1.q;
          const T aL = J1 * J0 + R1 * R0, bL = R1 * J0 - J1 * R0;
          add_s2<T>(acc, aL * a0 + bL * b0, bL * a0 - aL * b0);
        }
      }
    }
    const u64 mask = __ballot(neg);
    if (mask) {
      if (!acc.negs) acc.first = i0 + (uint32_t)__ffsll((i64)mask) - 1;
      acc.last = i0 + 63 - (uint32_t)__clzll((i64)mask);
      const uint32_t at = acc.negs + (uint32_t)__popcll(mask & ((1ull << lane) - 1));
      if (neg && negs && at < maxneg) negs[at] = i;
      acc.negs += (uint32_t)__popcll(mask);
    }
  }
  // the lanes' sums and peaks; negs, first and last are the wave's already
  for (int d = 32; d >= 1; d >>= 1) {
    Acc<T> o;
    o.energy = __shfl_xor(acc.energy, d, 64);
    o.s1re = __shfl_xor(acc.s1re, d, 64);
    o.s1im = __shfl_xor(acc.s1im, d, 64);
    o.s2re = __shfl_xor(acc.s2re, d, 64);
    o.s2im = __shfl_xor(acc.s2im, d, 64);
    o.s2re_lo = __shfl_xor(acc.s2re_lo, d, 64);
    o.s2im_lo = __shfl_xor(acc.s2im_lo, d, 64);
    const T peak = __shfl_xor(acc.peak, d, 64);
    const uint32_t at = __shfl_xor(acc.peak_i, d, 64);
    add_sums(acc, o);
    take_peak(acc, peak, at);
  }
  return acc;
}

template <class T>
struct GroupLds {
  Acc<T> acc[kWaves];
  uint32_t negs[kWaves][kMaxNegs];
};

// One workgroup over i in [lo, hi): each wave a quarter, merged in wave order; every thread returns the result.  The
// first maxneg negatives go to dst[0 .. maxneg) (global; may be null), the entries past the count kNone.
template <int FMT>
__device__ Acc<typename Fmt<FMT>::T> group_range(GroupLds<typename Fmt<FMT>::T>& s, const void* x, u64 elem0, u64 ld,
                                                 uint32_t n, uint32_t lo, uint32_t hi, uint32_t* dst, uint32_t maxneg) {
  using T = typename Fmt<FMT>::T;
  const uint32_t wv = threadIdx.x >> 6;
  const uint32_t seg = (((hi - lo) + kWaves - 1) / kWaves + 63) & ~63u;
  const uint32_t wlo = min(hi, lo + wv * seg), whi = min(hi, wlo + seg);
  const Acc<T> mine = wave_range<FMT>(x, elem0, ld, n, wlo, whi, s.negs[wv], maxneg);
  if ((threadIdx.x & 63) == 0) s.acc[wv] = mine;
  __syncthreads();
  Acc<T> all = s.acc[0];
  for (int k = 1; k < kWaves; ++k) merge(all, s.acc[k]);
  if (dst && threadIdx.x < maxneg) {
    uint32_t v = kNone, before = 0;
    for (int k = 0; k < kWaves; ++k) {
      const uint32_t cnt = min(s.acc[k].negs, maxneg);
      if (threadIdx.x >= before && threadIdx.x < before + cnt) v = s.negs[k][threadIdx.x - before];
      before += cnt;
    }
    dst[threadIdx.x] = v;
  }
  __syncthreads();  // the next unit of work writes the LDS again
  return all;
}

template <class T>
__device__ void write_record(pfb_mop_record* out, const pfb_mop_pulse& p, const Work& w, const Acc<T>& a, uint32_t maxneg) {
  pfb_mop_record r;
  r.start = p.start;
  r.length = p.length;
  r.column = p.column;
  r.n = w.n;
  r.flags = w.flags | (a.negs > maxneg ? (uint32_t)PFB_MOP_NEGS_CLIPPED : 0u);
  r.neg_count = a.negs;
  r.first_neg = a.first;
  r.last_neg = a.last;
  r.peak_index = a.peak_i;
  r.negs_listed = min(a.negs, maxneg);
  r.reserved = 0;
  r.energy = (double)a.energy;
  r.peak_power = a.peak_i == kNone ? 0.0 : (double)a.peak;
  r.s1_re = (double)a.s1re;
  r.s1_im = (double)a.s1im;
  if constexpr (std::is_same_v<T, double>) {
    r.s2_re = a.s2re;
    r.s2_im = a.s2im;
  } else {  // hi 2^32 is exact, the sum rounds once
    r.s2_re = (double)a.s2re * 4294967296.0 + (double)a.s2re_lo;
    r.s2_im = (double)a.s2im * 4294967296.0 + (double)a.s2im_lo;
  }
  *out = r;
}

struct PrepParams {
  const pfb_mop_pulse* pulses;  // null: the work is there already (host route)
  Work* work;
  uint32_t count, trim;
  u64 num_samples, ld, base;
  Tiers tiers;
  uint32_t* glist;  // pulses of mop_group, of mop_split
  uint32_t* slist;
  uint32_t* ctl;    // their counts, zeroed
};

__global__ void __launch_bounds__(kThreads) mop_prep(const PrepParams p) {
  const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
  if (i >= p.count) return;
  Work w;
  if (p.pulses) {
    w = geometry(p.pulses[i], p.num_samples, p.ld, p.base, p.trim);
    p.work[i] = w;
  } else {
    w = p.work[i];
  }
  const int tier = p.tiers.of(w.n);
  if (tier == kGroup) p.glist[atomicAdd(&p.ctl[0], 1u)] = i;
  if (tier == kSplit) p.slist[atomicAdd(&p.ctl[1], 1u)] = i;
}

struct MopParams {
  const void* x;
  u64 ld;
  const Work* work;
  const pfb_mop_pulse* pulses;  // what the records echo
  pfb_mop_record* rec;
  uint32_t* negs;               // may be null
  uint32_t count, maxneg;
  Tiers tiers;
  const uint32_t* list;         // mop_group, mop_split, mop_join: the tier's pulses ...
  const uint32_t* list_count;   // ... and how many
  uint32_t first_slot, slots;   // mop_split, mop_join: entries [first_slot, first_slot + slots) of the list
  void* partial;                // slots x kMaxParts Acc
  uint32_t* part_negs;          // slots x kMaxParts x maxneg
};

template <int FMT>
__global__ void __launch_bounds__(kThreads) mop_wave(const MopParams p) {
  using T = typename Fmt<FMT>::T;
  const uint32_t lane = threadIdx.x & 63;
  for (u64 q = (u64)blockIdx.x * kWaves + (threadIdx.x >> 6); q < p.count; q += (u64)gridDim.x * kWaves) {
    const Work w = p.work[q];
    if (p.tiers.of(w.n) != kWave) continue;
    uint32_t* negs = p.negs ? p.negs + q * p.maxneg : nullptr;
    const Acc<T> acc = wave_range<FMT>(p.x, w.elem0, p.ld, w.n, 0, w.n, negs, p.maxneg);
    if (negs)
      for (uint32_t j = lane; j < p.maxneg; j += 64)
        if (j >= acc.negs) negs[j] = kNone;
    if (lane == 0) write_record(p.rec + q, p.pulses[q], w, acc, p.maxneg);
  }
}

template <int FMT>
__global__ void __launch_bounds__(kThreads) mop_group(const MopParams p) {
  using T = typename Fmt<FMT>::T;
  __shared__ GroupLds<T> s;
  const uint32_t total = min(*p.list_count, p.count);
  for (uint32_t k = blockIdx.x; k < total; k += gridDim.x) {
    const uint32_t q = p.list[k];
    const Work w = p.work[q];
    const Acc<T> acc = group_range<FMT>(s, p.x, w.elem0, p.ld, w.n, 0, w.n, p.negs ? p.negs + (u64)q * p.maxneg : nullptr,
                                        p.maxneg);
    if (threadIdx.x == 0) write_record(p.rec + q, p.pulses[q], w, acc, p.maxneg);
  }
}

__device__ __forceinline__ uint32_t parts_of(uint32_t n) { return n ? (n + kPart - 1) / kPart : 1; }

// the slots of this launch: entries of the split list from first_slot on
__device__ __forceinline__ uint32_t slots_here(const MopParams& p) {
  const uint32_t total = min(*p.list_count, p.count);
  return total > p.first_slot ? min(total - p.first_slot, p.slots) : 0;
}

template <int FMT>
__global__ void __launch_bounds__(kThreads) mop_split(const MopParams p) {
  using T = typename Fmt<FMT>::T;
  __shared__ GroupLds<T> s;
  // part-major: the first parts of all slots come first, so that the parts that exist lie on different workgroups
  const uint32_t slots = slots_here(p), units = slots * kMaxParts;
  for (uint32_t unit = blockIdx.x; unit < units; unit += gridDim.x) {
    const uint32_t slot = unit % slots, part = unit / slots;
    const uint32_t q = p.list[p.first_slot + slot];
    const Work w = p.work[q];
    if (part >= parts_of(w.n)) continue;
    const uint32_t lo = part * kPart, hi = min(w.n, lo + kPart);
    const u64 at = (u64)slot * kMaxParts + part;
    const Acc<T> acc = group_range<FMT>(s, p.x, w.elem0, p.ld, w.n, lo, hi, p.part_negs + at * p.maxneg, p.maxneg);
    if (threadIdx.x == 0) reinterpret_cast<Acc<T>*>(p.partial)[at] = acc;
  }
}

template <class T>
__global__ void __launch_bounds__(kThreads) mop_join(const MopParams p) {
  __shared__ uint32_t s_count[kMaxParts];
  const uint32_t slots = slots_here(p);
  for (uint32_t slot = blockIdx.x; slot < slots; slot += gridDim.x) {
    const uint32_t q = p.list[p.first_slot + slot];
    const Work w = p.work[q];
    const uint32_t parts = parts_of(w.n);
    const Acc<T>* partial = reinterpret_cast<const Acc<T>*>(p.partial) + (u64)slot * kMaxParts;
    if (threadIdx.x < parts) s_count[threadIdx.x] = min(partial[threadIdx.x].negs, p.maxneg);
    __syncthreads();
    if (threadIdx.x == 0) {
      Acc<T> all = partial[0];
      for (uint32_t k = 1; k < parts; ++k) merge(all, partial[k]);
      write_record(p.rec + q, p.pulses[q], w, all, p.maxneg);
    }
    if (p.negs && threadIdx.x < p.maxneg) {
      uint32_t v = kNone, before = 0;
      for (uint32_t k = 0; k < parts && before <= threadIdx.x; ++k) {
        if (threadIdx.x < before + s_count[k])
          v = p.part_negs[((u64)slot * kMaxParts + k) * p.maxneg + (threadIdx.x - before)];
        before += s_count[k];
      }
      p.negs[(u64)q * p.maxneg + threadIdx.x] = v;
    }
    __syncthreads();  // s_count is written again
  }
}

// ---------------------------------------------------------------------------------
// host: checks and plan

// the carving of a handle's scratch: fixed, for slices of kSlice pulses
struct Scratch {
  Work* work;
  uint32_t* glist;
  uint32_t* slist;
  uint32_t* ctl;                // the two lists' counts
  Acc<double>* partial;
  uint32_t* part_negs;
  pfb_mop_pulse* pulses;        // a host list's slice, its records and negatives
  pfb_mop_record* rec;
  uint32_t* negs;
  size_t bytes;
  Scratch(char* base, uint32_t maxneg) {
    Carver c{base};
    work = c.array<Work>(kSlice);
    glist = c.array<uint32_t>(kSlice);
    slist = c.array<uint32_t>(kSlice);
    ctl = c.array<uint32_t>(2);
    partial = c.array<Acc<double>>((size_t)kSlots * kMaxParts);
    part_negs = c.array<uint32_t>((size_t)kSlots * kMaxParts * maxneg);
    pulses = c.array<pfb_mop_pulse>(kSlice);
    rec = c.array<pfb_mop_record>(kSlice);
    negs = c.array<uint32_t>((size_t)kSlice * maxneg);
    bytes = c.bytes();
  }
};

// Everything pfb_mop_describe and pfb_mop_create check before the device, in the order the header states
int mop_check(const pfb_mop_config* cfg) {
  if (!cfg || cfg->struct_size != sizeof(pfb_mop_config)) return PFB_ERR_BAD_ARG;
  if (cfg->max_negatives > kMaxNegs) return PFB_ERR_BAD_ARG;
  if (cfg->trim_samples > kMaxTrim) return PFB_ERR_BAD_ARG;
  if (cfg->sample_format > PFB_FMT_CF32) return PFB_ERR_BAD_FORMAT;
  if (cfg->sample_format == PFB_FMT_INT8_IQ && (cfg->bit_width < 1 || cfg->bit_width > 8)) return PFB_ERR_BAD_FORMAT;
  if (cfg->sample_format == PFB_FMT_INT16_IQ && (cfg->bit_width < 1 || cfg->bit_width > 16)) return PFB_ERR_BAD_FORMAT;
  return PFB_OK;
}

}  // namespace

struct pfb_mop_handle {
  int device = 0;
  int fmt = 0, bps = 0;
  uint32_t trim = 0, maxneg = 0;
  int forced = kAuto;
  uint32_t grid_cap = kGridCap;
  u64 stage_bytes = kStageBytes;
  hipStream_t stream = nullptr;
  hipEvent_t ev_switch = nullptr;
  char* d_scratch = nullptr;
  char* h_stage = nullptr;  // page-locked: a batch's windows
  char* d_stage = nullptr;
  size_t stage_cap = 0;
  std::string last_kernel;
};

namespace {

void free_mop(pfb_mop_handle* h) {
  if (!h) return;
  DeviceGuard g(h->device);
  (void)hipFree(h->d_scratch);
  (void)hipFree(h->d_stage);
  (void)hipHostFree(h->h_stage);
  if (h->ev_switch) (void)hipEventDestroy(h->ev_switch);
  delete h;
}

struct Names {  // what a call launched, each name once, in the tiers' order
  bool ran[4] = {false, false, false, false};
  std::string joined() const {
    static const char* const name[4] = {"mop_wave", "mop_group", "mop_split", "mop_join"};
    std::string s;
    for (int k = 0; k < 4; ++k)
      if (ran[k]) s += (s.empty() ? "" : "+") + std::string(name[k]);
    return s;
  }
};

template <int FMT>
void launch_tier(int tier, dim3 grid, hipStream_t stream, const MopParams& p) {
  using T = typename Fmt<FMT>::T;
  const dim3 block(kThreads);
  if (tier == kWave) hipLaunchKernelGGL(mop_wave<FMT>, grid, block, 0, stream, p);
  else if (tier == kGroup) hipLaunchKernelGGL(mop_group<FMT>, grid, block, 0, stream, p);
  else if (tier == kSplit) hipLaunchKernelGGL(mop_split<FMT>, grid, block, 0, stream, p);
  else hipLaunchKernelGGL(mop_join<T>, grid, block, 0, stream, p);
}

void launch(const pfb_mop_handle* h, int tier, uint32_t blocks, const MopParams& p) {
  const dim3 grid(std::max(1u, std::min(blocks, h->grid_cap)));
  if (h->fmt == PFB_FMT_INT8_IQ) launch_tier<PFB_FMT_INT8_IQ>(tier, grid, h->stream, p);
  else if (h->fmt == PFB_FMT_INT16_IQ) launch_tier<PFB_FMT_INT16_IQ>(tier, grid, h->stream, p);
  else launch_tier<PFB_FMT_CF32>(tier, grid, h->stream, p);
}

struct Series {  // where the kernels read: the caller's device series, or a batch of packed windows
  const void* d_x;
  u64 num_samples, ld, base;
};

// One round of launches over `count` <= kSlice pulses.  d_pulses: the pulses the records echo; geometry: derive the
// work from them (the host route has uploaded it instead).  may_wait: the call is synchronous and reads the lists'
// counts; without it every tier that could have work is launched and the long pulses stay on mop_group.
int run_slice(pfb_mop_handle* h, const Series& sx, const pfb_mop_pulse* d_pulses, uint32_t count, bool geometry,
              pfb_mop_record* d_rec, uint32_t* d_negs, bool may_wait, Names* names) {
  const Scratch scr(h->d_scratch, h->maxneg);
  uint32_t* ctl = scr.ctl;
  PrepParams pp{};
  pp.pulses = geometry ? d_pulses : nullptr;
  pp.work = scr.work;
  pp.count = count;
  pp.trim = h->trim;
  pp.num_samples = sx.num_samples;
  pp.ld = sx.ld;
  pp.base = sx.base;
  pp.tiers = Tiers{h->forced, kGroupMin, may_wait ? kSplitMin : 0xffffffffu};
  pp.glist = scr.glist;
  pp.slist = scr.slist;
  pp.ctl = ctl;
  HIP_TRY(hipMemsetAsync(ctl, 0, 8, h->stream));
  hipLaunchKernelGGL(mop_prep, dim3((count + kThreads - 1) / kThreads), dim3(kThreads), 0, h->stream, pp);
  HIP_TRY(hipGetLastError());
  uint32_t groups = count, splits = 0;  // bounds when the counts are not read
  bool waves = true;
  if (h->forced != kAuto) {
    waves = h->forced == kWave;
    groups = h->forced == kGroup ? count : 0;
    splits = h->forced == kSplit ? count : 0;
  } else if (may_wait) {
    uint32_t got[2] = {0, 0};
    HIP_TRY(hipMemcpyAsync(got, ctl, 8, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    groups = got[0];
    splits = got[1];
    waves = groups + splits < count;
  }
  MopParams p{};
  p.x = sx.d_x;
  p.ld = sx.ld;
  p.work = pp.work;
  p.pulses = d_pulses;
  p.rec = d_rec;
  p.negs = h->maxneg ? d_negs : nullptr;
  p.count = count;
  p.maxneg = h->maxneg;
  p.tiers = pp.tiers;
  p.partial = scr.partial;
  p.part_negs = scr.part_negs;
  if (waves) {
    launch(h, kWave, (count + kWaves - 1) / kWaves, p);
    names->ran[0] = true;
  }
  if (groups) {
    p.list = pp.glist;
    p.list_count = ctl;
    launch(h, kGroup, groups, p);
    names->ran[1] = true;
  }
  p.list = pp.slist;
  p.list_count = ctl + 1;
  for (uint32_t first = 0; first < splits; first += kSlots) {  // the partial slots are reused: the stream keeps the order
    p.first_slot = first;
    p.slots = kSlots;
    const uint32_t here = std::min(splits - first, kSlots);
    launch(h, kSplit, here * kMaxParts, p);
    launch(h, kSplit + 1, here, p);
    names->ran[2] = names->ran[3] = true;
  }
  HIP_TRY(hipGetLastError());
  return PFB_OK;
}

// what both measuring calls check before the device is touched, in the order the header states
int check_call(const pfb_mop_handle* h, const void* x, uint64_t num_samples, uint64_t ld, uint32_t mem,
               const pfb_mop_pulse* pulses, uint64_t num_pulses, uint32_t pulses_mem, const pfb_mop_record* rec_out,
               const uint32_t* negs_out) {
  if (!h || mem > PFB_MEM_DEVICE || pulses_mem > PFB_MEM_DEVICE) return PFB_ERR_BAD_ARG;
  if (ld == 0 || (h->fmt != PFB_FMT_CF32 && ld != 1)) return PFB_ERR_BAD_ARG;
  if (num_pulses > kMaxPulses) return PFB_ERR_BAD_ARG;
  if (num_samples > (1ull << 63) / ld) return PFB_ERR_BAD_ARG;
  if ((num_samples > 0 && !x) || (num_pulses > 0 && (!pulses || !rec_out))) return PFB_ERR_BAD_ARG;
  if (mem == PFB_MEM_DEVICE && reinterpret_cast<uintptr_t>(x) % (uintptr_t)h->bps) return PFB_ERR_BAD_ARG;
  if (pulses_mem == PFB_MEM_DEVICE && (reinterpret_cast<uintptr_t>(pulses) % 8 || reinterpret_cast<uintptr_t>(rec_out) % 8 ||
                                       reinterpret_cast<uintptr_t>(negs_out) % 4))
    return PFB_ERR_BAD_ARG;
  return PFB_OK;
}

// records and negatives of a slice from the scratch to the caller's host arrays
int copy_back(pfb_mop_handle* h, const Scratch& scr, uint64_t first, uint32_t count, pfb_mop_record* rec_out,
              uint32_t* negs_out) {
  HIP_TRY(hipMemcpyAsync(rec_out + first, scr.rec, (size_t)count * sizeof(pfb_mop_record), hipMemcpyDeviceToHost, h->stream));
  if (negs_out && h->maxneg)
    HIP_TRY(hipMemcpyAsync(negs_out + first * h->maxneg, scr.negs, (size_t)count * h->maxneg * 4,
                           hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(hipStreamSynchronize(h->stream));
  return PFB_OK;
}

// x on the device: slices of the list, a host list through the scratch
int measure_device(pfb_mop_handle* h, const Series& sx, const pfb_mop_pulse* pulses, uint64_t num_pulses,
                   uint32_t pulses_mem, pfb_mop_record* rec_out, uint32_t* negs_out, bool may_wait, Names* names) {
  const Scratch scr(h->d_scratch, h->maxneg);
  for (uint64_t first = 0; first < num_pulses; first += kSlice) {
    const uint32_t count = (uint32_t)std::min<uint64_t>(kSlice, num_pulses - first);
    int rc;
    if (pulses_mem == PFB_MEM_HOST) {
      pfb_mop_pulse* d_pulses = scr.pulses;
      HIP_TRY(hipMemcpyAsync(d_pulses, pulses + first, (size_t)count * sizeof(pfb_mop_pulse), hipMemcpyHostToDevice,
                             h->stream));
      rc = run_slice(h, sx, d_pulses, count, true, scr.rec, scr.negs, may_wait, names);
      if (rc == PFB_OK) rc = copy_back(h, scr, first, count, rec_out, negs_out);
    } else {
      rc = run_slice(h, sx, pulses + first, count, true, rec_out + first, negs_out ? negs_out + first * h->maxneg : nullptr,
                     may_wait, names);
    }
    if (rc != PFB_OK) return rc;
  }
  return PFB_OK;
}

int ensure_stage(pfb_mop_handle* h, size_t bytes) {
  if (bytes <= h->stage_cap) return PFB_OK;
  (void)hipFree(h->d_stage);
  (void)hipHostFree(h->h_stage);
  h->d_stage = h->h_stage = nullptr;
  h->stage_cap = 0;
  HIP_TRY(hipHostMalloc(reinterpret_cast<void**>(&h->h_stage), bytes, hipHostMallocDefault));
  HIP_TRY(hipMalloc(reinterpret_cast<void**>(&h->d_stage), bytes));
  h->stage_cap = bytes;
  return PFB_OK;
}

// x on the host: the windows of a batch of whole pulses, packed back to back, are all that is uploaded
int measure_host(pfb_mop_handle* h, const char* x, const Series& sx, const pfb_mop_pulse* pulses, uint64_t num_pulses,
                 uint32_t pulses_mem, pfb_mop_record* rec_out, uint32_t* negs_out, Names* names) {
  const Scratch scr(h->d_scratch, h->maxneg);
  std::vector<pfb_mop_pulse> copy;
  const pfb_mop_pulse* list = pulses;  // on the host
  if (pulses_mem == PFB_MEM_DEVICE) {
    copy.resize(num_pulses);
    HIP_TRY(hipMemcpyAsync(copy.data(), pulses, num_pulses * sizeof(pfb_mop_pulse), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    list = copy.data();
  }
  const size_t bps = (size_t)h->bps;
  std::vector<Work> work;
  for (uint64_t first = 0; first < num_pulses;) {
    // the batch: pulses while their windows fit the chunk, one at least
    work.clear();
    size_t bytes = 0;
    uint64_t end = first;
    while (end < num_pulses && end - first < kSlice) {
      Work w = geometry(list[end], sx.num_samples, sx.ld, sx.base, h->trim);
      const size_t need = (size_t)w.n * bps;
      if (end > first && bytes + need > h->stage_bytes) break;
      work.push_back(w);
      bytes += need;
      ++end;
    }
    const uint32_t count = (uint32_t)(end - first);
    int rc = ensure_stage(h, std::max<size_t>(bytes, 256));
    if (rc != PFB_OK) return rc;
    size_t at = 0;
    for (Work& w : work) {
      const char* src = x + (size_t)w.elem0 * bps;
      if (sx.ld == 1) {
        std::memcpy(h->h_stage + at, src, (size_t)w.n * bps);
      } else {
        for (uint32_t i = 0; i < w.n; ++i) std::memcpy(h->h_stage + at + i * bps, src + (size_t)i * sx.ld * bps, bps);
      }
      w.elem0 = at / bps;
      at += (size_t)w.n * bps;
    }
    if (bytes) HIP_TRY(hipMemcpyAsync(h->d_stage, h->h_stage, bytes, hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipMemcpyAsync(scr.work, work.data(), (size_t)count * sizeof(Work), hipMemcpyHostToDevice, h->stream));
    const Series packed{h->d_stage, bytes / bps, 1, 0};
    if (pulses_mem == PFB_MEM_HOST) {
      pfb_mop_pulse* d_pulses = scr.pulses;
      HIP_TRY(hipMemcpyAsync(d_pulses, list + first, (size_t)count * sizeof(pfb_mop_pulse), hipMemcpyHostToDevice,
                             h->stream));
      rc = run_slice(h, packed, d_pulses, count, false, scr.rec, scr.negs, true, names);
      if (rc == PFB_OK) rc = copy_back(h, scr, first, count, rec_out, negs_out);
    } else {
      rc = run_slice(h, packed, pulses + first, count, false, rec_out + first,
                     negs_out ? negs_out + first * h->maxneg : nullptr, true, names);
      if (rc == PFB_OK) HIP_TRY(hipStreamSynchronize(h->stream));  // the staging is packed again
    }
    if (rc != PFB_OK) return rc;
    first = end;
  }
  return PFB_OK;
}

}  // namespace

extern "C" int pfb_mop_describe(const pfb_mop_config* cfg, pfb_mop_plan* plan_out) {
  return pfb::abi_guard([&]() -> int {
    if (!plan_out) return PFB_ERR_BAD_ARG;
    const int rc = mop_check(cfg);
    if (rc != PFB_OK) return rc;
    pfb_mop_plan plan{};
    plan.scratch_bytes = Scratch(nullptr, cfg->max_negatives).bytes;
    plan.group_min = kGroupMin;
    plan.split_min = kSplitMin;
    plan.part_samples = kPart;
    plan.grid_cap = kGridCap;
    plan.threads = kThreads;
    plan.slice_pulses = kSlice;
    plan.split_slots = kSlots;
    plan.stage_bytes = (uint32_t)kStageBytes;
    std::snprintf(plan.wave_kernel, sizeof(plan.wave_kernel), "%s", "mop_wave");
    std::snprintf(plan.group_kernel, sizeof(plan.group_kernel), "%s", "mop_group");
    std::snprintf(plan.split_kernel, sizeof(plan.split_kernel), "%s", "mop_split");
    std::snprintf(plan.join_kernel, sizeof(plan.join_kernel), "%s", "mop_join");
    *plan_out = plan;
    return PFB_OK;
  });
}

extern "C" int pfb_mop_create(const pfb_mop_config* cfg, pfb_mop_handle** out) {
  return pfb::abi_guard([&]() -> int {
    if (!out) return PFB_ERR_BAD_ARG;
    *out = nullptr;
    int rc = mop_check(cfg);
    if (rc != PFB_OK) return rc;
    int dev = 0;
    rc = pfb::resolve_device(cfg->device_id, &dev);
    if (rc != PFB_OK) return rc;
    pfb_mop_handle* h = new pfb_mop_handle();
    h->device = dev;
    h->fmt = (int)cfg->sample_format;
    h->bps = bytes_per_sample(h->fmt);
    h->trim = cfg->trim_samples;
    h->maxneg = cfg->max_negatives;
    DeviceGuard g(dev);
    const hipError_t e = hipMalloc(reinterpret_cast<void**>(&h->d_scratch), Scratch(nullptr, h->maxneg).bytes);
    if (e != hipSuccess) {
      free_mop(h);
      return pfb::hip_fail(e, "hipMalloc(scratch)");
    }
    *out = h;
    return PFB_OK;
  });
}

extern "C" int pfb_mop_destroy(pfb_mop_handle* h) {
  return pfb::abi_guard([&]() -> int {
    if (!h) return PFB_ERR_BAD_ARG;
    free_mop(h);
    return PFB_OK;
  });
}

extern "C" int pfb_mop_set_stream(pfb_mop_handle* h, void* hip_stream) {
  return pfb::abi_guard([&]() -> int {
    if (!h) return PFB_ERR_BAD_ARG;
    return pfb::switch_stream(h->device, &h->stream, &h->ev_switch, static_cast<hipStream_t>(hip_stream));
  });
}

extern "C" int pfb_mop_sync(pfb_mop_handle* h) {
  return pfb::abi_guard([&]() -> int {
    if (!h) return PFB_ERR_BAD_ARG;
    DeviceGuard g(h->device);
    HIP_TRY(hipStreamSynchronize(h->stream));
    return PFB_OK;
  });
}

extern "C" int pfb_mop_get_device(const pfb_mop_handle* h, int* device_id) {
  return pfb::abi_guard([&]() -> int {
    if (!h || !device_id) return PFB_ERR_BAD_ARG;
    *device_id = h->device;
    return PFB_OK;
  });
}

extern "C" int pfb_mop_set_tier(pfb_mop_handle* h, int tier, uint32_t grid_cap, uint64_t stage_bytes) {
  return pfb::abi_guard([&]() -> int {
    if (!h || tier < kAuto || tier > kSplit || grid_cap > 65536) return PFB_ERR_BAD_ARG;
    h->forced = tier;
    h->grid_cap = grid_cap ? grid_cap : kGridCap;
    h->stage_bytes = stage_bytes ? stage_bytes : kStageBytes;
    return PFB_OK;
  });
}

extern "C" int pfb_mop_measure(pfb_mop_handle* h, const void* x, uint64_t num_samples, uint64_t ld, uint64_t base_index,
                               uint32_t mem, const pfb_mop_pulse* pulses, uint64_t num_pulses, uint32_t pulses_mem,
                               pfb_mop_record* rec_out, uint32_t* negs_out) {
  return pfb::abi_guard([&]() -> int {
    int rc = check_call(h, x, num_samples, ld, mem, pulses, num_pulses, pulses_mem, rec_out, negs_out);
    if (rc != PFB_OK) return rc;
    h->last_kernel.clear();
    if (num_pulses == 0) return PFB_OK;
    DeviceGuard g(h->device);
    Names names;
    const Series sx{x, num_samples, ld, base_index};
    if (mem == PFB_MEM_DEVICE)
      rc = measure_device(h, sx, pulses, num_pulses, pulses_mem, rec_out, negs_out, true, &names);
    else
      rc = measure_host(h, static_cast<const char*>(x), sx, pulses, num_pulses, pulses_mem, rec_out, negs_out, &names);
    if (rc != PFB_OK) {
      (void)hipStreamSynchronize(h->stream);  // nothing touches the caller's buffers any more
      return rc;
    }
    HIP_TRY(hipStreamSynchronize(h->stream));
    h->last_kernel = names.joined();
    return PFB_OK;
  });
}

extern "C" int pfb_mop_measure_async(pfb_mop_handle* h, const void* x, uint64_t num_samples, uint64_t ld,
                                     uint64_t base_index, const pfb_mop_pulse* pulses, uint64_t num_pulses,
                                     pfb_mop_record* rec_out, uint32_t* negs_out) {
  return pfb::abi_guard([&]() -> int {
    int rc = check_call(h, x, num_samples, ld, PFB_MEM_DEVICE, pulses, num_pulses, PFB_MEM_DEVICE, rec_out, negs_out);
    if (rc != PFB_OK) return rc;
    h->last_kernel.clear();
    if (num_pulses == 0) return PFB_OK;
    DeviceGuard g(h->device);
    Names names;
    rc = measure_device(h, Series{x, num_samples, ld, base_index}, pulses, num_pulses, PFB_MEM_DEVICE, rec_out, negs_out,
                        false, &names);
    if (rc != PFB_OK) return rc;
    h->last_kernel = names.joined();
    return PFB_OK;
  });
}

extern "C" const char* pfb_mop_last_kernel(const pfb_mop_handle* h) { return h ? h->last_kernel.c_str() : ""; }

extern "C" int pfb_mop_figures(const pfb_mop_record* records, uint64_t n, double fs, pfb_mop_figure* out) {
  return pfb::abi_guard([&]() -> int {
    if ((n > 0 && (!records || !out)) || !std::isfinite(fs) || fs <= 0) return PFB_ERR_BAD_ARG;
    const double two_pi = 6.283185307179586476925286766559;
    for (uint64_t k = 0; k < n; ++k) {
      const pfb_mop_record& r = records[k];
      pfb_mop_figure f{};
      const uint32_t L = r.n ? (r.n - 1) / 2 : 0;
      f.freq_hz = std::atan2(r.s1_im, r.s1_re) / two_pi * fs;
      f.rate_hz_per_s = L ? std::atan2(r.s2_im, r.s2_re) / (two_pi * (double)L) * fs * fs : 0.0;
      f.extent_hz = r.n ? f.rate_hz_per_s * (double)(r.n - 1) / fs : 0.0;
      f.mean_power = r.n ? r.energy / (double)r.n : 0.0;
      f.flips = (double)r.neg_count / 2.0;
      if (r.n < 3 || (r.flags & PFB_MOP_OUTSIDE))
        f.kind = PFB_MOP_KIND_NOT_MEASURABLE;
      else
        f.kind = (std::fabs(f.extent_hz) >= fs / (double)r.n ? 1u : 0u) | (r.neg_count >= 2 ? 2u : 0u);
      out[k] = f;
    }
    return PFB_OK;
  });
}

extern "C" int pfb_mop_pulses_from_pdw(const pfb_pdw* pdws, uint64_t n, double series_rate, double t0,
                                       pfb_mop_pulse* pulses_out) {
  return pfb::abi_guard([&]() -> int {
    if ((n > 0 && (!pdws || !pulses_out)) || n > (1ull << 31)) return PFB_ERR_BAD_ARG;
    if (!std::isfinite(series_rate) || series_rate <= 0 || !std::isfinite(t0)) return PFB_ERR_BAD_ARG;
    std::vector<pfb_mop_pulse> made(n);
    for (uint64_t i = 0; i < n; ++i) {
      // to nearest, ties to even: llrint without its range trouble; the scripts' toa is 1-based
      const double s = std::rint((pdws[i].toa - t0) * series_rate) - 1.0;
      const double len = std::rint(pdws[i].pw * series_rate);
      if (!std::isfinite(s) || s < 0 || s >= 4611686018427387904.0) return PFB_ERR_BAD_ARG;
      if (!std::isfinite(len) || len < 0 || len > 4294967295.0 || pdws[i].bin < 0) return PFB_ERR_BAD_ARG;
      made[i].start = (uint64_t)s;
      made[i].length = (uint32_t)len;
      made[i].column = (uint32_t)pdws[i].bin;
    }
    if (n) std::memcpy(pulses_out, made.data(), n * sizeof(pfb_mop_pulse));
    return PFB_OK;
  });
}
