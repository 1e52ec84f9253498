// pfb_waterfall.hip -- time-binned waterfalls of channelizer and STFT output (pfb_wf_* in include/pfb_channelizer.h,
// where the arithmetic is defined): per (bin of B rows, column) the largest, mean and smallest power and the row of the
// peak -- the arithmetic under the reference's surf / mesh pictures (matlab/channelizer_example.m:56-71,
// generate_channelized_training_iq.m:100-108, spectrogram_my_iq.m:114-115) as one read of the matrix.
//
// A segmented reduction whose read streams.  The call's rows are cut at every bin boundary and at every multiple of a
// row tile from a bin's start (pfb_trace.hip cuts its samples the same way), so each segment lies in one bin and the
// grid follows from (rows, B, rows the open bin already holds, W) alone.
//   PFB_WF_ROWS     a row is contiguous: lanes map to 16-byte slots of a row (2 complex64 or 4 float32 columns; a slot
//                   that a row's edge cuts is read element by element), rows stack across the rest of the wave and the
//                   workgroup.  A group of G = 1 .. 256 lanes (a power of two) spans a row:
//                     fewer than 64 slots   64 / G rows per wave-wide load, one contiguous stretch when ld == W
//                     64 .. 256 slots       whole waves per row
//                     more                  256 slots per workgroup, the rest in gridDim.y column tiles
//                   Rows whose pitch is no multiple of 16 bytes would change a lane's columns from row to row: they
//                   take the same kernel with one-element slots.  Bins shorter than the workgroup's row count share
//                   the workgroup (`span` threads per segment).
//   PFB_WF_COLUMNS  every (column, segment) is one contiguous run: a group of 1 .. 256 lanes per run, scalar head,
//                   16-byte body, scalar tail (the trace unit's segment reduction, over a second dimension).
// Lanes that hold the same column meet by xor shuffles inside a wave and through LDS across waves; one lane per column
// writes the 16-byte cell as one vector store.  Bins longer than the tile: every segment writes a partial per column to
// the handle's scratch and wf_fold_kernel combines a bin's partials in a fixed order.  The bin a call leaves open lives
// on the device as W partials (two sets, written in turn: the workgroup that reads the old one and the one that writes
// the new one may differ); the host keeps only the row position.  Everything combined is associative and commutative
// -- min, the lexicographic (largest power, lowest row) -- or a double sum in the grid's fixed order.  No atomics.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <new>
#include <vector>

#include "pfb_common.h"
#include "pfb_host.h"

namespace {

constexpr int kThreads = 256;
constexpr uint32_t kMaxWidth = 65536;
constexpr uint32_t kMaxBin = 1u << 24;
// PFB_WF_ROWS: rows per segment = clamp(kTileElems / W, kMinTileRows, kMaxTileRows) (sdr_channelizer_amd/waterfall.py:
// row_tile); PFB_WF_COLUMNS: kColTile elements of a column
constexpr uint32_t kTileElems = 1u << 18, kMinTileRows = 64, kMaxTileRows = 4096;
constexpr uint32_t kColTile = 4096;
constexpr uint32_t kLaneElems = 16;   // PFB_WF_COLUMNS: a lane takes about this many elements of a run
constexpr uint32_t kFoldCols = 32, kFoldLanes = kThreads / kFoldCols;  // wf_fold_kernel: columns x segment lanes
constexpr unsigned kMaxGrid = 1u << 20;
constexpr uint32_t kNone = 0xFFFFFFFFu;
constexpr uint64_t kStageBytes = (uint64_t)64 << 20;  // per side of the host staging
constexpr uint64_t kMaxRows = (uint64_t)1 << 48;

static_assert(sizeof(pfb_wf_cell) == 16, "the cell of include/pfb_channelizer.h");

// A (bin, column)'s figures over some of its rows, as they travel between kernels and calls.  The selections stay
// doubles until the cell is written: the first-row rule is defined on the double power, and two different doubles may
// round to one float.  row: offset inside the bin, kNone before the first row (count == 0).
struct alignas(16) Part {
  double pmax, pmin, sum;
  uint32_t row, count;
};
static_assert(sizeof(Part) == 32, "two 16-byte stores");

__host__ __device__ inline double dinf() {
  const uint64_t b = 0x7FF0000000000000ull;
  double d;
  memcpy(&d, &b, 8);
  return d;
}

__host__ __device__ inline Part empty_part() { return Part{-dinf(), dinf(), 0.0, kNone, 0u}; }

__host__ __device__ inline void merge_part(Part& a, const Part& b) {  // an empty side never wins a selection
  a.sum += b.sum;
  a.pmin = b.pmin < a.pmin ? b.pmin : a.pmin;
  if (b.pmax > a.pmax || (b.pmax == a.pmax && b.row < a.row)) {
    a.pmax = b.pmax;
    a.row = b.row;
  }
  a.count += b.count;
}

// The cell of a (bin, column) whose rows are all in `p`; on the device for the bins a call completes and on the host
// for the bin pfb_wf_flush returns: IEEE conversions and one division give the same bits on both.
__host__ __device__ inline pfb_wf_cell finish_cell(const Part& p) {
  pfb_wf_cell c;
  c.power_max = (float)p.pmax;
  c.power_mean = (float)(p.sum / (double)p.count);
  c.power_min = (float)p.pmin;
  c.peak_row = p.row;
  return c;
}

template <int KIND> struct Elem { using type = float; };
template <> struct Elem<PFB_WF_COMPLEX> { using type = float2; };

template <int KIND>
__device__ __forceinline__ double power_of(typename Elem<KIND>::type v) {
  if constexpr (KIND == PFB_WF_COMPLEX)
    return (double)v.x * (double)v.x + (double)v.y * (double)v.y;  // exact products: contraction changes nothing
  else if constexpr (KIND == PFB_WF_MAGNITUDE)
    return (double)v * (double)v;
  else
    return (double)v;
}

// What one lane gathers for one column.  idx: the row's offset from the start of the lane's segment, kNone before the
// first; a lane visits its rows in rising order, so the strict comparison keeps the first of equal powers.
struct Acc {
  double pmin, pmax, sum;
  uint32_t idx;
  static __device__ __forceinline__ Acc empty() { return Acc{dinf(), -dinf(), 0.0, kNone}; }
  __device__ __forceinline__ void add(double p, uint32_t off) {
    sum += p;
    pmin = p < pmin ? p : pmin;
    if (p > pmax || idx == kNone) {
      pmax = p;
      idx = off;
    }
  }
  __device__ __forceinline__ void merge(const Acc& b) {  // an empty b (-inf, kNone) never wins
    sum += b.sum;
    pmin = b.pmin < pmin ? b.pmin : pmin;
    if (b.pmax > pmax || (b.pmax == pmax && b.idx < idx)) {
      pmax = b.pmax;
      idx = b.idx;
    }
  }
  __device__ __forceinline__ Acc lane_xor(int mask) const {
    return Acc{__shfl_xor(pmin, mask), __shfl_xor(pmax, mask), __shfl_xor(sum, mask), __shfl_xor(idx, mask)};
  }
};

// Kernel-side view of one call.  "Grid position" g counts rows from the first row of the bin that was open when the
// call began: call row j sits at g = open + j, in local bin g / B at offset g % B.
struct WfParams {
  const void* x;
  uint64_t n;            // rows of this call (> 0)
  uint64_t ld;           // elements between rows (PFB_WF_ROWS) or columns (PFB_WF_COLUMNS)
  uint64_t bins;         // local bins the call touches
  uint64_t segs;         // segments of the call
  uint32_t W, B;
  uint32_t open;         // rows of local bin 0 that earlier calls took (< B); they are in carry_in[0 .. W)
  uint32_t tile;         // rows per segment
  uint32_t seg_per_bin;  // ceil(B / tile)
  uint32_t seg0;         // index inside local bin 0 of the call's first segment: open / tile
  uint32_t G;            // wf_rows_kernel: lanes across a row (a power of two, 256 with column tiles)
  uint32_t span;         // threads per segment: G .. 256 (rows), 1 .. 256 (columns), a power of two
  uint32_t slots;        // wf_rows_kernel: slots of a row
  uint32_t head;         // wf_rows_kernel: elements by which a row's first column lies behind a 16-byte boundary
  const Part* carry_in;
  Part* carry_out;
  Part* parts;           // [segment][column] when seg_per_bin > 1
  pfb_wf_cell* out;      // [completed local bin][column]
};

struct Seg {
  uint64_t b;    // local bin
  uint64_t j0;   // first row of the call in the segment
  uint32_t o0;   // offset inside the bin of that row
  uint32_t len;  // rows: 1 .. tile (0: no such segment)
};

__device__ __forceinline__ Seg segment_of(const WfParams& p, uint64_t q) {
  const uint64_t qq = q + p.seg0, b = qq / p.seg_per_bin, s = qq % p.seg_per_bin;
  const uint64_t end = p.open + p.n;
  const uint64_t g0 = std::max<uint64_t>(b * p.B + s * p.tile, p.open);
  const uint64_t g1 = std::min<uint64_t>(b * p.B + std::min<uint64_t>((s + 1) * (uint64_t)p.tile, p.B), end);
  return Seg{b, g0 - p.open, (uint32_t)(g0 - b * p.B), (uint32_t)(g1 - g0)};
}

__device__ __forceinline__ void store_cell(pfb_wf_cell* dst, const pfb_wf_cell& c) {  // dst is 16-byte aligned
  *reinterpret_cast<uint4*>(dst) =
      make_uint4(__float_as_uint(c.power_max), __float_as_uint(c.power_mean), __float_as_uint(c.power_min), c.peak_row);
}

// one lane per (bin, column): the column's share of this call is in `mine`
__device__ __forceinline__ void close_or_carry(const WfParams& p, uint64_t b, uint32_t col, Part mine) {
  if (b == 0 && p.open > 0) {
    Part all = p.carry_in[col];
    merge_part(all, mine);
    mine = all;
  }
  if ((b + 1) * p.B <= p.open + p.n)
    store_cell(p.out + b * p.W + col, finish_cell(mine));
  else
    p.carry_out[col] = mine;
}

__device__ __forceinline__ void emit(const WfParams& p, uint64_t q, const Seg& sg, uint32_t col, const Acc& a) {
  const Part mine{a.pmax, a.pmin, a.sum, a.idx == kNone ? kNone : sg.o0 + a.idx, sg.len};
  if (p.seg_per_bin == 1)
    close_or_carry(p, sg.b, col, mine);
  else
    p.parts[q * p.W + col] = mine;
}

// The lanes of one segment that hold the same columns meet: `span` consecutive threads, of which each run of G holds a
// row's slots.  Inside a wave by xor shuffles; across waves through LDS, merged by the segment's first G threads in
// rising thread order.  Every thread of the workgroup calls it.
template <int NA>
struct Meet {
  double pmin[NA][kThreads], pmax[NA][kThreads], sum[NA][kThreads];
  uint32_t idx[NA][kThreads];
  __device__ __forceinline__ void run(Acc (&a)[NA], uint32_t G, uint32_t span) {
    const uint32_t t = threadIdx.x;
    const uint32_t U = std::max<uint32_t>(G, std::min<uint32_t>(64, span));  // threads one shuffle stage covers
    for (uint32_t m = G; m < U; m <<= 1) {
#pragma unroll
      for (int k = 0; k < NA; ++k) a[k].merge(a[k].lane_xor((int)m));
    }
    if (span > U) {  // the same in every thread of the workgroup
      __syncthreads();  // the previous round's readers are done
#pragma unroll
      for (int k = 0; k < NA; ++k) {
        pmin[k][t] = a[k].pmin;
        pmax[k][t] = a[k].pmax;
        sum[k][t] = a[k].sum;
        idx[k][t] = a[k].idx;
      }
      __syncthreads();
      if (t % span < G) {
        for (uint32_t o = t + U; o < t - t % span + span; o += U) {
#pragma unroll
          for (int k = 0; k < NA; ++k) a[k].merge(Acc{pmin[k][o], pmax[k][o], sum[k][o], idx[k][o]});
        }
      }
    }
  }
};

// PFB_WF_ROWS.  S columns per slot: 16 bytes' worth, or 1.  Slot q of a row holds columns q S - head .. q S - head + S-1.
template <int KIND, int S>
__global__ __launch_bounds__(kThreads) void wf_rows_kernel(const WfParams p) {
  using E = typename Elem<KIND>::type;
  struct alignas(sizeof(E) * S) Vec { E w[S]; };
  __shared__ Meet<S> meet;
  const E* x = static_cast<const E*>(p.x);
  const uint32_t t = threadIdx.x, tt = t % p.span, part = t / p.span, per_block = kThreads / p.span;
  const uint32_t r = tt / p.G, step = p.span / p.G;
  const uint32_t q = tt % p.G + blockIdx.y * p.G;
  const int64_t c0 = (int64_t)q * S - (int64_t)p.head;  // the slot's first column
  const bool on = q < p.slots;
  const bool whole = on && c0 >= 0 && c0 + S <= (int64_t)p.W;
  // the loop's bounds are the same for every thread of the workgroup: all of them reach the barriers of meet.run
  for (uint64_t s0 = (uint64_t)blockIdx.x * per_block; s0 < p.segs; s0 += (uint64_t)gridDim.x * per_block) {
    const uint64_t sq = s0 + part;
    Seg sg{0, 0, 0, 0};
    if (sq < p.segs) sg = segment_of(p, sq);
    Acc acc[S];
#pragma unroll
    for (int k = 0; k < S; ++k) acc[k] = Acc::empty();
    if (whole) {
      const E* base = x + sg.j0 * p.ld + c0;
      uint32_t i = r;
      for (; i + 3 * step < sg.len; i += 4 * step) {  // four loads in flight
        Vec v[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) v[u] = *reinterpret_cast<const Vec*>(base + (uint64_t)(i + u * step) * p.ld);
#pragma unroll
        for (int u = 0; u < 4; ++u) {
#pragma unroll
          for (int k = 0; k < S; ++k) acc[k].add(power_of<KIND>(v[u].w[k]), i + u * step);
        }
      }
      for (; i < sg.len; i += step) {
        const Vec v = *reinterpret_cast<const Vec*>(base + (uint64_t)i * p.ld);
#pragma unroll
        for (int k = 0; k < S; ++k) acc[k].add(power_of<KIND>(v.w[k]), i);
      }
    } else if (on) {  // a slot that the row's first or last column cuts: its columns one by one
      for (uint32_t i = r; i < sg.len; i += step) {
        const E* row = x + (sg.j0 + i) * p.ld;
#pragma unroll
        for (int k = 0; k < S; ++k) {
          const int64_t c = c0 + k;
          if (c >= 0 && c < (int64_t)p.W) acc[k].add(power_of<KIND>(row[c]), i);
        }
      }
    }
    meet.run(acc, p.G, p.span);
    if (tt < p.G && on && sg.len > 0) {
#pragma unroll
      for (int k = 0; k < S; ++k) {
        const int64_t c = c0 + k;
        if (c >= 0 && c < (int64_t)p.W) emit(p, sq, sg, (uint32_t)c, acc[k]);
      }
    }
  }
}

// PFB_WF_COLUMNS.  Item = (column, segment), the segments of a column next to each other so that the groups of a wave
// read one stretch; `span` lanes per item: the elements before the first 16-byte boundary and behind the last whole
// vector one by one, the body by 16-byte loads.
template <int KIND>
__global__ __launch_bounds__(kThreads) void wf_cols_kernel(const WfParams p) {
  using E = typename Elem<KIND>::type;
  constexpr uint32_t S = 16 / (uint32_t)sizeof(E);
  struct alignas(16) Vec { E w[S]; };
  __shared__ Meet<1> meet;
  const E* x = static_cast<const E*>(p.x);
  const uint32_t t = threadIdx.x, r = t % p.span, per_block = kThreads / p.span;
  const uint64_t items = p.segs * p.W;
  for (uint64_t i0 = (uint64_t)blockIdx.x * per_block; i0 < items; i0 += (uint64_t)gridDim.x * per_block) {
    const uint64_t item = i0 + t / p.span;
    Seg sg{0, 0, 0, 0};
    uint32_t col = 0;
    uint64_t sq = 0;
    Acc acc[1] = {Acc::empty()};
    if (item < items) {
      col = (uint32_t)(item / p.segs);
      sq = item % p.segs;
      sg = segment_of(p, sq);
      const E* run = x + (uint64_t)col * p.ld + sg.j0;
      const uint32_t to_boundary = (uint32_t)(((16 - reinterpret_cast<uintptr_t>(run) % 16) % 16) / sizeof(E));
      const uint32_t head = to_boundary < sg.len ? to_boundary : sg.len;
      const uint32_t nvec = (sg.len - head) / S, tail0 = head + nvec * S;
      for (uint32_t o = r; o < head; o += p.span) acc[0].add(power_of<KIND>(run[o]), o);
      for (uint32_t v = r; v < nvec; v += p.span) {
        const uint32_t o = head + v * S;
        const Vec vec = *reinterpret_cast<const Vec*>(run + o);
#pragma unroll
        for (uint32_t e = 0; e < S; ++e) acc[0].add(power_of<KIND>(vec.w[e]), o + e);
      }
      for (uint32_t o = tail0 + r; o < sg.len; o += p.span) acc[0].add(power_of<KIND>(run[o]), o);
    }
    meet.run(acc, 1, p.span);
    if (r == 0 && item < items) emit(p, sq, sg, col, acc[0]);
  }
}

// Bins longer than the tile: kFoldLanes lanes per (bin, column) fold the bin's partials of this call, lane j those of
// segments j, j + kFoldLanes, ...; the lanes meet through LDS in rising order.  grid: (column tiles, bins).
__global__ __launch_bounds__(kThreads) void wf_fold_kernel(const WfParams p) {
  __shared__ Part s_part[kThreads];
  const uint32_t t = threadIdx.x, j = t / kFoldCols;
  const uint32_t col = blockIdx.x * kFoldCols + t % kFoldCols;
  for (uint64_t b = blockIdx.y; b < p.bins; b += gridDim.y) {
    const uint64_t lo = std::max<uint64_t>(b * p.seg_per_bin, p.seg0) - p.seg0;
    const uint64_t hi = std::min<uint64_t>((b + 1) * (uint64_t)p.seg_per_bin - p.seg0, p.segs);
    Part a = empty_part();
    if (col < p.W)
      for (uint64_t q = lo + j; q < hi; q += kFoldLanes) merge_part(a, p.parts[q * p.W + col]);
    __syncthreads();  // the previous bin's readers are done
    s_part[t] = a;
    __syncthreads();
    if (j == 0 && col < p.W) {
      for (uint32_t jj = 1; jj < kFoldLanes; ++jj) merge_part(a, s_part[jj * kFoldCols + t]);
      close_or_carry(p, b, col, a);
    }
  }
}

uint32_t pow2_ceil(uint64_t v) {
  uint32_t r = 1;
  while (r < v) r <<= 1;
  return r;
}

}  // namespace

struct pfb_wf_handle {
  uint32_t W = 1, B = 1;
  int element = 0, layout = 0;
  int device = 0;
  int elem_bytes = 4;
  uint32_t tile = 1;        // rows per segment
  uint64_t pos = 0;         // rows since create / reset: the index of the next one
  uint64_t grid0 = 0;       // where the bin grid starts: 0, or the position of the last flush
  Part* d_carry = nullptr;  // two sets of W; [cur] holds the open bin when (pos - grid0) % B > 0
  int cur = 0;
  Part* d_parts = nullptr;  // segment partials of the call in flight (grow-only)
  uint64_t parts_cap = 0;
  hipStream_t stream = nullptr;
  hipEvent_t ev_switch = nullptr;
  pfb::HostStage stage;     // host path
};

namespace {

void free_wf(pfb_wf_handle* h) {
  if (!h) return;
  pfb::DeviceGuard g(h->device);
  (void)hipFree(h->d_carry);
  (void)hipFree(h->d_parts);
  h->stage.release();
  if (h->ev_switch) (void)hipEventDestroy(h->ev_switch);
  delete h;
}

int check_config(const pfb_wf_config* cfg) {
  if (!cfg || cfg->struct_size != sizeof(pfb_wf_config)) return PFB_ERR_BAD_ARG;
  if (cfg->width < 1 || cfg->width > kMaxWidth || cfg->bin_rows < 1 || cfg->bin_rows > kMaxBin) return PFB_ERR_BAD_ARG;
  if (cfg->element > PFB_WF_POWER || cfg->layout > PFB_WF_COLUMNS || cfg->flags != 0) return PFB_ERR_BAD_ARG;
  return PFB_OK;
}

int create_wf(const pfb_wf_config* cfg, pfb_wf_handle** out) {
  int rc = check_config(cfg);
  if (rc != PFB_OK) return rc;
  int dev = 0;
  rc = pfb::resolve_device(cfg->device_id, &dev);
  if (rc != PFB_OK) return rc;
  pfb_wf_handle* h = new pfb_wf_handle();
  h->W = cfg->width;
  h->B = cfg->bin_rows;
  h->element = (int)cfg->element;
  h->layout = (int)cfg->layout;
  h->device = dev;
  h->elem_bytes = h->element == PFB_WF_COMPLEX ? 8 : 4;
  h->tile = h->layout == PFB_WF_COLUMNS
                ? kColTile
                : std::min(std::max(kTileElems / h->W, kMinTileRows), kMaxTileRows);
  pfb::DeviceGuard g(dev);
  const size_t carry_bytes = 2 * (size_t)h->W * sizeof(Part);
  hipError_t e = hipMalloc((void**)&h->d_carry, carry_bytes);
  if (e == hipSuccess) e = hipMemset(h->d_carry, 0, carry_bytes);
  if (e != hipSuccess) {
    rc = pfb::hip_fail(e, "pfb_wf_create allocation");
    free_wf(h);
    return rc;
  }
  *out = h;
  return PFB_OK;
}

uint64_t open_rows(const pfb_wf_handle* h) { return (h->pos - h->grid0) % h->B; }
uint64_t bins_for(const pfb_wf_handle* h, uint64_t n) { return (open_rows(h) + n) / h->B; }

template <int KIND>
void launch_rows(bool vec, dim3 grid, hipStream_t s, const WfParams& p) {
  constexpr int S = 16 / (int)sizeof(typename Elem<KIND>::type);
  if (vec)
    hipLaunchKernelGGL((wf_rows_kernel<KIND, S>), grid, dim3(kThreads), 0, s, p);
  else
    hipLaunchKernelGGL((wf_rows_kernel<KIND, 1>), grid, dim3(kThreads), 0, s, p);
}

// the kernels of one call and the position update, on the handle's stream; bins_for(n) * W cells land at d_out.
// ld: the resolved pitch (>= W for rows, >= n for columns)
int wf_enqueue(pfb_wf_handle* h, const void* d_x, uint64_t n, uint64_t ld, pfb_wf_cell* d_out) {
  if (n == 0) return PFB_OK;
  const uint64_t B = h->B, T = h->tile;
  WfParams p{};
  p.x = d_x;
  p.n = n;
  p.ld = ld;
  p.W = h->W;
  p.B = h->B;
  p.open = (uint32_t)open_rows(h);
  p.bins = (p.open + n + B - 1) / B;
  p.tile = h->tile;
  p.seg_per_bin = (uint32_t)((B + T - 1) / T);
  p.seg0 = (uint32_t)(p.open / T);
  const uint64_t last = p.open + n - 1;
  p.segs = (last / B) * p.seg_per_bin + (last % B) / T + 1 - p.seg0;
  p.carry_in = h->d_carry + (size_t)h->cur * h->W;
  p.carry_out = h->d_carry + (size_t)(h->cur ^ 1) * h->W;
  p.out = d_out;
  if (p.seg_per_bin > 1) {
    const uint64_t need = p.segs * h->W;
    if (need > h->parts_cap) {  // frees only after the device has drained: earlier calls are done with the old one
      (void)hipFree(h->d_parts);
      h->d_parts = nullptr;
      h->parts_cap = 0;
      HIP_TRY(hipMalloc((void**)&h->d_parts, need * sizeof(Part)));
      h->parts_cap = need;
    }
    p.parts = h->d_parts;
  }
  const uint64_t longest = std::min<uint64_t>(B, T);  // rows of the longest segment
  if (h->layout == PFB_WF_ROWS) {
    // 16-byte slots need every row to start at the same offset from a 16-byte boundary
    const bool vec = ((ld * (uint64_t)h->elem_bytes) % 16) == 0;
    const uint32_t S = vec ? 16u / (uint32_t)h->elem_bytes : 1u;
    p.head = vec ? (uint32_t)((reinterpret_cast<uintptr_t>(d_x) % 16) / (uintptr_t)h->elem_bytes) : 0u;
    p.slots = (p.W + p.head + S - 1) / S;
    p.G = std::min<uint32_t>(pow2_ceil(p.slots), kThreads);
    p.span = std::max<uint32_t>(p.G, std::min<uint32_t>(kThreads, p.G * pow2_ceil(longest)));
    const uint64_t per_block = kThreads / p.span, want = (p.segs + per_block - 1) / per_block;
    const dim3 grid((unsigned)std::min<uint64_t>(want, kMaxGrid), (p.slots + p.G - 1) / p.G);
    if (h->element == PFB_WF_COMPLEX)
      launch_rows<PFB_WF_COMPLEX>(vec, grid, h->stream, p);
    else if (h->element == PFB_WF_MAGNITUDE)
      launch_rows<PFB_WF_MAGNITUDE>(vec, grid, h->stream, p);
    else
      launch_rows<PFB_WF_POWER>(vec, grid, h->stream, p);
  } else {
    p.G = 1;
    p.span = std::min<uint32_t>(kThreads, pow2_ceil((longest + kLaneElems - 1) / kLaneElems));
    const uint64_t per_block = kThreads / p.span, want = (p.segs * h->W + per_block - 1) / per_block;
    const dim3 grid((unsigned)std::min<uint64_t>(want, kMaxGrid));
    if (h->element == PFB_WF_COMPLEX)
      hipLaunchKernelGGL(wf_cols_kernel<PFB_WF_COMPLEX>, grid, dim3(kThreads), 0, h->stream, p);
    else if (h->element == PFB_WF_MAGNITUDE)
      hipLaunchKernelGGL(wf_cols_kernel<PFB_WF_MAGNITUDE>, grid, dim3(kThreads), 0, h->stream, p);
    else
      hipLaunchKernelGGL(wf_cols_kernel<PFB_WF_POWER>, grid, dim3(kThreads), 0, h->stream, p);
  }
  HIP_TRY(hipGetLastError());
  if (p.seg_per_bin > 1) {
    const dim3 fgrid((h->W + kFoldCols - 1) / kFoldCols, (unsigned)std::min<uint64_t>(p.bins, 32768));
    hipLaunchKernelGGL(wf_fold_kernel, fgrid, dim3(kThreads), 0, h->stream, p);
    HIP_TRY(hipGetLastError());
  }
  h->pos += n;
  if (open_rows(h) > 0) h->cur ^= 1;  // the call wrote the other carry set
  return PFB_OK;
}

// what every process call checks before the device is touched; *ld = the resolved pitch, *f = the bins completed
int check_process(const pfb_wf_handle* h, const void* x, uint64_t n, uint64_t* ld, const void* out, uint64_t cap,
                  uint64_t* bins_out, bool device, uint64_t* f) {
  if (!h || (n > 0 && !x) || n > kMaxRows || h->pos + n < h->pos) return PFB_ERR_BAD_ARG;
  const uint64_t dense = h->layout == PFB_WF_ROWS ? h->W : n;
  if (*ld == 0) *ld = dense;
  if (*ld < dense || *ld > kMaxRows) return PFB_ERR_BAD_ARG;
  if (!device && h->layout != PFB_WF_ROWS) return PFB_ERR_BAD_ARG;
  *f = bins_for(h, n);
  if (bins_out) *bins_out = *f;
  if (*f > cap) return PFB_ERR_CAPACITY;
  if (*f > 0 && !out) return PFB_ERR_BAD_ARG;
  if ((device && reinterpret_cast<uintptr_t>(x) % (uintptr_t)h->elem_bytes) || reinterpret_cast<uintptr_t>(out) % 16)
    return PFB_ERR_BAD_ARG;
  return PFB_OK;
}

// n host rows of pitch `pitch` elements through the staged pipeline: a "sample" is one row of `pitch` elements, a
// "frame" one bin of W cells, a step at most 64 MiB on either side
int stage_rows(pfb_wf_handle* h, const void* x, uint64_t n, uint64_t pitch, pfb_wf_cell* out) {
  if (n == 0) return PFB_OK;
  const uint64_t row_bytes = pitch * (uint64_t)h->elem_bytes, bin_bytes = (uint64_t)h->W * sizeof(pfb_wf_cell);
  uint64_t chunk = std::max<uint64_t>(kStageBytes / row_bytes, 1);
  chunk = std::min<uint64_t>(chunk, std::max<uint64_t>(kStageBytes / bin_bytes, 1) * h->B);
  const pfb::StageSteps steps{
      chunk, (h->B - 1 + chunk) / h->B, (size_t)row_bytes, (size_t)bin_bytes,
      [h](uint64_t m) { return bins_for(h, m); },
      [h, pitch](const void* d_in, uint64_t m, void* d_out, uint64_t, int64_t, int64_t) {
        return wf_enqueue(h, d_in, m, pitch, static_cast<pfb_wf_cell*>(d_out));
      }};
  return pfb::stage_host(h->stage, h->stream, steps, x, n, pfb::StageOut{out});
}

// Host rows.  With ld > W the last row ends W elements in: it is staged on its own, so that nothing behind the
// caller's last element is read.
int process_host(pfb_wf_handle* h, const void* x, uint64_t n, uint64_t ld, pfb_wf_cell* out) {
  if (n == 0) return PFB_OK;
  if (ld == h->W) return stage_rows(h, x, n, ld, out);
  const uint64_t f = bins_for(h, n - 1);
  const int rc = stage_rows(h, x, n - 1, ld, out);
  if (rc != PFB_OK) return rc;
  const char* last = static_cast<const char*>(x) + (n - 1) * ld * (uint64_t)h->elem_bytes;
  return stage_rows(h, last, 1, h->W, out + f * h->W);
}

int flush_wf(pfb_wf_handle* h, pfb_wf_cell* out_host, uint32_t* rows_in_bin) {
  const uint64_t open = open_rows(h);
  *rows_in_bin = (uint32_t)open;
  if (open > 0) {
    pfb::DeviceGuard g(h->device);
    std::vector<Part> parts(h->W);
    HIP_TRY(hipMemcpyAsync(parts.data(), h->d_carry + (size_t)h->cur * h->W, (size_t)h->W * sizeof(Part),
                           hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    for (uint32_t k = 0; k < h->W; ++k) out_host[k] = finish_cell(parts[k]);
  }
  h->grid0 = h->pos;  // the next row starts a bin
  return PFB_OK;
}

// One record through a producer (the channelizer or the STFT) and the reduction, chunk by chunk on one stream.
// frames_for(n) and process_async(d_in, n, d_out, cap, &frames) are the producer's; `src` describes its output.
template <class FramesFor, class ProcessAsync>
int record_to_cells(const pfb::OutputDesc& src, pfb::Record& rec, uint32_t max_bins, uint64_t chunk_samples,
                    pfb_wf_cell* out, uint64_t capacity_bins, uint64_t* bins_out, uint32_t* bin_rows_out,
                    FramesFor frames_for, ProcessAsync process_async) {
  const uint64_t n = rec.info.packet.numSamples;
  uint64_t frames = 0;
  int rc = frames_for(n, &frames);
  if (rc != PFB_OK) return rc;
  pfb_wf_config cfg{};
  cfg.struct_size = sizeof(cfg);
  cfg.width = src.width;
  cfg.element = src.element;
  cfg.layout = src.layout;
  cfg.device_id = src.device;
  rc = pfb_wf_choose_bin(frames, max_bins, &cfg.bin_rows);
  if (rc != PFB_OK) return rc;
  *bin_rows_out = cfg.bin_rows;
  const uint64_t need = (frames + cfg.bin_rows - 1) / cfg.bin_rows;  // the final partial bin included
  *bins_out = need;
  if (need > capacity_bins) return PFB_ERR_CAPACITY;
  if (need == 0) return PFB_OK;
  pfb_wf_handle* h = nullptr;
  rc = create_wf(&cfg, &h);
  if (rc != PFB_OK) return rc;
  h->stream = src.stream;
  pfb::DeviceGuard g(src.device);
  const uint64_t chunk = std::min<uint64_t>(chunk_samples ? chunk_samples : (uint64_t)1 << 24, std::max<uint64_t>(n, 1));
  // the most frames one chunk can complete: what the chunk and the longest carry give a producer that carries nothing
  uint64_t chunk_frames = 0;
  rc = frames_for(chunk + src.carry_max, &chunk_frames);
  chunk_frames = std::max<uint64_t>(chunk_frames, 1);
  const size_t elem = src.element == PFB_WF_COMPLEX ? 8 : 4;
  void *d_in = nullptr, *d_mat = nullptr;
  pfb_wf_cell* d_cells = nullptr;
  hipError_t e = hipMalloc(&d_in, chunk * (size_t)src.bps);
  if (e == hipSuccess) e = hipMalloc(&d_mat, chunk_frames * src.width * elem);
  if (e == hipSuccess) e = hipMalloc((void**)&d_cells, need * src.width * sizeof(pfb_wf_cell));
  if (e != hipSuccess) rc = pfb::hip_fail(e, "pfb_wf_from_iq_file allocation");
  uint64_t done = 0;
  if (rc == PFB_OK) {
    rc = rec.read(chunk, [&](const char* buf, uint64_t, uint64_t m) {
      HIP_TRY(hipMemcpyAsync(d_in, buf, m * (size_t)src.bps, hipMemcpyHostToDevice, src.stream));
      uint64_t f = 0;
      int r = process_async(d_in, m, d_mat, chunk_frames, &f);
      if (r != PFB_OK) return r;
      // channel-major: the producer's column stride is the frames of its call
      const uint64_t b = bins_for(h, f);
      r = wf_enqueue(h, d_mat, f, src.layout == PFB_WF_COLUMNS ? f : src.width, d_cells + done * src.width);
      if (r != PFB_OK) return r;
      done += b;
      HIP_TRY(hipStreamSynchronize(src.stream));  // `buf`, d_in and d_mat are free for the next chunk
      return (int)PFB_OK;
    });
  }
  if (rc == PFB_OK && done > 0) {
    e = hipMemcpy(out, d_cells, done * src.width * sizeof(pfb_wf_cell), hipMemcpyDeviceToHost);
    if (e != hipSuccess) rc = pfb::hip_fail(e, "pfb_wf_from_iq_file copy-out");
  }
  if (rc == PFB_OK && done < need) {
    uint32_t have = 0;
    rc = flush_wf(h, out + done * src.width, &have);
    done += have > 0;
  }
  *bins_out = done;
  (void)hipFree(d_in);
  (void)hipFree(d_mat);
  (void)hipFree(d_cells);
  free_wf(h);
  return rc;
}

}  // namespace

extern "C" int pfb_wf_create(const pfb_wf_config* cfg, pfb_wf_handle** out) {
  return pfb::abi_guard([&]() -> int {
    if (!out) return PFB_ERR_BAD_ARG;
    *out = nullptr;
    return create_wf(cfg, out);
  });
}

extern "C" int pfb_wf_destroy(pfb_wf_handle* h) {
  return pfb::abi_guard([&]() -> int {
    if (!h) return PFB_ERR_BAD_ARG;
    free_wf(h);
    return PFB_OK;
  });
}

extern "C" int pfb_wf_reset(pfb_wf_handle* h) {
  return pfb::abi_guard([&]() -> int {
    if (!h) return PFB_ERR_BAD_ARG;
    h->pos = h->grid0 = 0;  // no open bin: the carry set is never read again
    return PFB_OK;
  });
}

extern "C" int pfb_wf_set_stream(pfb_wf_handle* h, void* hip_stream) {
  return pfb::abi_guard([&]() -> int {
    if (!h) return PFB_ERR_BAD_ARG;
    return pfb::switch_stream(h->device, &h->stream, &h->ev_switch, static_cast<hipStream_t>(hip_stream));
  });
}

extern "C" int pfb_wf_sync(pfb_wf_handle* h) {
  return pfb::abi_guard([&]() -> int {
    if (!h) return PFB_ERR_BAD_ARG;
    pfb::DeviceGuard g(h->device);
    HIP_TRY(hipStreamSynchronize(h->stream));
    return PFB_OK;
  });
}

extern "C" int pfb_wf_get_device(const pfb_wf_handle* h, int* device_id) {
  return pfb::abi_guard([&]() -> int {
    if (!h || !device_id) return PFB_ERR_BAD_ARG;
    *device_id = h->device;
    return PFB_OK;
  });
}

extern "C" int pfb_wf_bins_for(const pfb_wf_handle* h, uint64_t rows, uint64_t* bins_out) {
  return pfb::abi_guard([&]() -> int {
    if (!h || !bins_out || rows > kMaxRows) return PFB_ERR_BAD_ARG;
    *bins_out = bins_for(h, rows);
    return PFB_OK;
  });
}

extern "C" int pfb_wf_process_async(pfb_wf_handle* h, const void* d_x, uint64_t rows, uint64_t ld, pfb_wf_cell* d_out,
                                    uint64_t capacity_bins, uint64_t* bins_out) {
  return pfb::abi_guard([&]() -> int {
    uint64_t f = 0;
    const int rc = check_process(h, d_x, rows, &ld, d_out, capacity_bins, bins_out, true, &f);
    if (rc != PFB_OK) return rc;
    pfb::DeviceGuard g(h->device);
    return wf_enqueue(h, d_x, rows, ld, d_out);
  });
}

extern "C" int pfb_wf_process(pfb_wf_handle* h, const void* x, uint64_t rows, uint64_t ld, pfb_wf_cell* out,
                              uint64_t capacity_bins, uint64_t* bins_out, uint32_t mem) {
  return pfb::abi_guard([&]() -> int {
    if (mem > PFB_MEM_DEVICE) return PFB_ERR_BAD_ARG;
    uint64_t f = 0;
    int rc = check_process(h, x, rows, &ld, out, capacity_bins, bins_out, mem == PFB_MEM_DEVICE, &f);
    if (rc != PFB_OK) return rc;
    pfb::DeviceGuard g(h->device);
    if (mem == PFB_MEM_HOST) return process_host(h, x, rows, ld, out);
    rc = wf_enqueue(h, x, rows, ld, out);
    if (rc != PFB_OK) return rc;
    HIP_TRY(hipStreamSynchronize(h->stream));
    return PFB_OK;
  });
}

extern "C" int pfb_wf_flush(pfb_wf_handle* h, pfb_wf_cell* out_host, uint32_t* rows_in_bin) {
  return pfb::abi_guard([&]() -> int {
    if (!h || !out_host || !rows_in_bin) return PFB_ERR_BAD_ARG;
    return flush_wf(h, out_host, rows_in_bin);
  });
}

extern "C" int pfb_wf_choose_bin(uint64_t rows, uint32_t max_bins, uint32_t* bin_rows) {
  return pfb::abi_guard([&]() -> int {
    if (!bin_rows || max_bins == 0) return PFB_ERR_BAD_ARG;
    const uint64_t b = std::max<uint64_t>(1, rows / max_bins + (rows % max_bins != 0));
    if (b > kMaxBin) return PFB_ERR_BAD_ARG;
    *bin_rows = (uint32_t)b;
    return PFB_OK;
  });
}

extern "C" int pfb_wf_from_channelizer_iq_file(pfb_handle* ch, const char* path, uint32_t max_bins,
                                               uint64_t chunk_samples, pfb_wf_cell* out, uint64_t capacity_bins,
                                               uint64_t* bins_out, uint32_t* bin_rows_out, pfb_iq_info* info_out) {
  return pfb::abi_guard([&]() -> int {
    if (!ch || !path || !bins_out || !bin_rows_out || max_bins == 0 || (capacity_bins > 0 && !out) ||
        reinterpret_cast<uintptr_t>(out) % 16)
      return PFB_ERR_BAD_ARG;
    const pfb::OutputDesc src = pfb::describe_output(ch);
    pfb::Record rec;
    int rc = rec.open(path, src.fmt, src.bit_width);
    if (info_out) *info_out = rec.info;
    if (rc != PFB_OK) return rc;
    rc = pfb_reset(ch);
    if (rc != PFB_OK) return rc;
    return record_to_cells(
        src, rec, max_bins, chunk_samples, out, capacity_bins, bins_out, bin_rows_out,
        [ch](uint64_t n, uint64_t* f) { return pfb_frames_for(ch, n, f); },
        [ch](const void* d_in, uint64_t m, void* d_out, uint64_t cap, uint64_t* f) {
          return pfb_process_async(ch, d_in, m, d_out, cap, f);
        });
  });
}

extern "C" int pfb_wf_from_stft_iq_file(pfb_stft_handle* st, const char* path, uint32_t max_bins, uint64_t chunk_samples,
                                        pfb_wf_cell* out, uint64_t capacity_bins, uint64_t* bins_out,
                                        uint32_t* bin_rows_out, pfb_iq_info* info_out) {
  return pfb::abi_guard([&]() -> int {
    if (!st || !path || !bins_out || !bin_rows_out || max_bins == 0 || (capacity_bins > 0 && !out) ||
        reinterpret_cast<uintptr_t>(out) % 16)
      return PFB_ERR_BAD_ARG;
    const pfb::OutputDesc src = pfb::describe_output(st);
    if (!src.reducible) return PFB_ERR_BAD_ARG;  // averaging dB is not averaging power
    pfb::Record rec;
    int rc = rec.open(path, src.fmt, src.bit_width);
    if (info_out) *info_out = rec.info;
    if (rc != PFB_OK) return rc;
    rc = pfb_stft_reset(st);
    if (rc != PFB_OK) return rc;
    return record_to_cells(
        src, rec, max_bins, chunk_samples, out, capacity_bins, bins_out, bin_rows_out,
        [st](uint64_t n, uint64_t* f) { return pfb_stft_frames_for(st, n, f); },
        [st](const void* d_in, uint64_t m, void* d_out, uint64_t cap, uint64_t* f) {
          return pfb_stft_process_async(st, d_in, m, d_out, cap, f);
        });
  });
}
