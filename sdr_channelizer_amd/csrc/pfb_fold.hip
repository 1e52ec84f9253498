// pfb_fold.hip -- PRI search by epoch folding (pfb_fold_* in include/pfb_channelizer.h, where the arithmetic is
// defined): a float32 power stream added into one profile of floor(L / C) phase bins per candidate period L, and one
// score record per candidate, kernels and host side.
//   fold_direct<CW>   one work item per (candidate, bin), found through the prefix table of the candidates' bin counts.
//                     For a step that brings cells [s, s+n) a lane loads its accumulator, walks the periods the step
//                     touches in order, adds its bin's cells in ascending index and stores the accumulator back: the
//                     definition's order, so any cutting of the stream gives the same bits.  Only the first and the
//                     last period of a step are clamped to the step.  Consecutive lanes read consecutive C-cell groups.
//                     The adds of one bin depend on each other, the loads do not: CW = 1 .. 4 (C known at compile time)
//                     loads a batch of periods, up to 32 cells, before the adds that use them; CW = 0 (any C) loads a
//                     period's cells in groups of 16.
//   fold_tile<C>      C = 8, 16, 32, 64, where a lane's C cells are a private run and fold_direct's loads scatter: one
//                     wave per (candidate, 64 adjacent bins) stages the bins' contiguous stretch of P = 64 / C periods
//                     in LDS with coalesced loads, one padded row per bin, and every lane adds its row in the same
//                     order; 3 to 5 times faster there, the same bytes.  The library runs it
//                     for those C; pfb_fold_set_tier (pfb_channelizer_dev.h) switches a handle for tests and meter.
//   fold_score        one workgroup per candidate: counts by the closed form, means in float64, the peak by a reduction
//                     over (mean, bin) whose order is the definition's (larger mean, then lower bin: independent of the
//                     reduction's shape), the two float64 sums by a fixed butterfly.
// No atomics: every profile element and every record has one writer.  Every candidate re-reads the whole step, 64 MiB at
// most, which the 256 MiB last-level cache holds: that is why a step is 2^24 cells.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <new>
#include <vector>

#include "pfb_common.h"
#include "pfb_host.h"

namespace {

using namespace pfb;

constexpr uint64_t kStepCells = (uint64_t)1 << 24;  // cells per kernel launch, and per staging step of a host buffer
constexpr uint64_t kMaxProfileBytes = (uint64_t)64 << 20;
constexpr uint32_t kMaxPeriod = 1u << 24, kMaxBins = 1u << 16, kMaxPeriods = 4096, kMaxBinCells = 64;
constexpr uint64_t kMaxIndex = (uint64_t)1 << 62;
constexpr unsigned kMaxGrid = 1u << 16;

struct FoldParams {
  const float* x;             // the step's cells: x[0] is global cell s
  float* F;                   // the profiles, candidate after candidate
  const uint32_t* periods;    // [NC]
  const uint32_t* prefix;     // [NC + 1]: bins before candidate c
  const uint32_t* tile_prefix;  // [NC + 1]: tiles of 64 bins before candidate c (fold_tile)
  unsigned long long s;       // global index of x[0]
  int n;                      // cells of the step, 1 .. 2^24
  int NC, C, total_bins;
};

struct ScoreParams {
  const float* F;
  const uint32_t* periods;
  const uint32_t* prefix;
  pfb_fold_score* out;
  unsigned long long N;
  int C;
};

// the candidate that owns global bin g: the last c with prefix[c] <= g
__device__ __forceinline__ int owner(const uint32_t* prefix, int NC, uint32_t g) {
  int lo = 0, hi = NC;  // prefix[lo] <= g < prefix[hi]
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (prefix[mid] <= g) lo = mid; else hi = mid;
  }
  return lo;
}

// cells [lo, hi) of the step, in order, 16 loads ahead of their adds
__device__ __forceinline__ float add_run(float acc, const float* x, int lo, int hi) {
  for (int k = lo; k < hi; k += 16) {
    float v[16];
#pragma unroll
    for (int u = 0; u < 16; ++u)
      if (k + u < hi) v[u] = x[k + u];
#pragma unroll
    for (int u = 0; u < 16; ++u)
      if (k + u < hi) acc += v[u];
  }
  return acc;
}

template <int CW>
__global__ void __launch_bounds__(256) fold_direct(const FoldParams p) {
  const int C = CW ? CW : p.C;
  const int n = p.n;
  const uint32_t stride = gridDim.x * blockDim.x;
  for (uint32_t g = blockIdx.x * blockDim.x + threadIdx.x; g < (uint32_t)p.total_bins; g += stride) {
    const int c = owner(p.prefix, p.NC, g);
    const int L = (int)p.periods[c];
    const int j = (int)(g - p.prefix[c]), NB = (int)(p.prefix[c + 1] - p.prefix[c]);
    const int a = j * C;
    const int w = j == NB - 1 ? L - a : C;  // the last bin takes the L mod C cells left over
    const int r = (int)(p.s % (unsigned long long)L);
    const int T = (int)(((long long)r + n + L - 1) / L);  // periods the step touches
    // period t of the step begins at step-local cell t L - r; this bin's cells there are [t L - r + a, .. + w)
    long long at = (long long)a - r;
    float acc = p.F[g];
    acc = add_run(acc, p.x, (int)max(at, 0ll), (int)min(at + w, (long long)n));  // the first period, clamped
    int t = 1;
    at += L;
    if constexpr (CW > 0) {
      if (w == CW) {  // whole periods, a batch of them loaded before the adds
        constexpr int P = CW == 1 ? 32 : CW == 2 ? 16 : 8;
        for (; t + P <= T - 1; t += P, at += (long long)P * L) {
          float v[P][CW];
#pragma unroll
          for (int q = 0; q < P; ++q)
#pragma unroll
            for (int k = 0; k < CW; ++k) v[q][k] = p.x[at + (long long)q * L + k];
#pragma unroll
          for (int q = 0; q < P; ++q)
#pragma unroll
            for (int k = 0; k < CW; ++k) acc += v[q][k];
        }
      }
    }
    for (; t < T - 1; ++t, at += L) acc = add_run(acc, p.x, (int)at, (int)at + w);  // whole periods: nothing to clamp
    if (T > 1) acc = add_run(acc, p.x, (int)at, (int)min(at + w, (long long)n));     // the last period, clamped
    p.F[g] = acc;
  }
}

// fold_tile<C>: one wave per (candidate, 64 adjacent bins).  The bins' cells of one period are one contiguous stretch
// of the step, 64 C cells (up to C - 1 more when the tile holds the widened last bin): the wave loads the stretches of P
// periods with consecutive lanes on consecutive cells, lays them out in LDS one row per bin, rows C + 1 floats apart so
// that the lanes' walk down their rows meets no bank twice, and every lane adds its row in ascending index.  The next
// batch's loads are issued before the adds of this one.  The first and the last period of a step, and the periods that
// do not fill a batch, are added from global memory as fold_direct adds them: per bin the same cells in the same order.
template <int C>
struct TileShape {
  static constexpr int P = C >= 64 ? 1 : 64 / C;        // periods per batch: about 64 loads per lane in flight
  static constexpr int V = C + 1;                       // loads per lane and period: ceil((64 C + C - 1) / 64)
  static constexpr int Row = 64 * (C + 1) + C;          // floats of one period in LDS
};

template <int C>
__global__ void __launch_bounds__(64) fold_tile(const FoldParams p) {
  using S = TileShape<C>;
  constexpr int P = S::P, V = S::V;
  __shared__ float sh[P * S::Row];
  const int lane = threadIdx.x;
  const int c = owner(p.tile_prefix, p.NC, blockIdx.x);
  const int L = (int)p.periods[c];
  const int NB = (int)(p.prefix[c + 1] - p.prefix[c]);
  const int j0 = (int)(blockIdx.x - p.tile_prefix[c]) * 64;
  const int nb = min(64, NB - j0);                      // bins of this tile
  const bool tail = j0 + nb == NB;                      // it holds the last bin
  const int W = tail ? L - j0 * C : 64 * C;             // cells of the tile in one period
  const int j = j0 + lane;
  const bool live = lane < nb;
  const int a = j * C;
  const int w = !live ? 0 : (j == NB - 1 ? L - a : C);
  const int n = p.n;
  const int r = (int)(p.s % (unsigned long long)L);
  const int T = (int)(((long long)r + n + L - 1) / L);
  long long at = (long long)a - r;                      // this bin's first cell in period 0, step-local
  long long tile_at = (long long)j0 * C - r + L;        // the tile's first cell in period 1
  float acc = live ? p.F[p.prefix[c] + j] : 0.f;
  if (live) acc = add_run(acc, p.x, (int)max(at, 0ll), (int)min(at + w, (long long)n));
  int t = 1;
  at += L;
  float v[P][V];
  auto load = [&](long long from) {                     // the stretches of periods from, from + L, ...: whole periods
#pragma unroll
    for (int q = 0; q < P; ++q)
#pragma unroll
      for (int k = 0; k < V; ++k) {
        const int e = lane + 64 * k;
        if (e < W) v[q][k] = p.x[from + (long long)q * L + e];
      }
  };
  if (t + P <= T - 1) load(tile_at);
  for (; t + P <= T - 1; t += P, at += (long long)P * L) {
    __syncthreads();                                    // the rows of the batch before are read
#pragma unroll
    for (int q = 0; q < P; ++q)
#pragma unroll
      for (int k = 0; k < V; ++k) {
        const int e = lane + 64 * k;
        if (e < W) sh[q * S::Row + e + min(e / C, nb - 1)] = v[q][k];   // row e / C, the last row takes what is left
      }
    __syncthreads();
    tile_at += (long long)P * L;
    if (t + 2 * P <= T - 1) load(tile_at);              // in flight under the adds
    if (live) {
#pragma unroll
      for (int q = 0; q < P; ++q) {
        const float* row = sh + q * S::Row + lane * (C + 1);
#pragma unroll
        for (int k = 0; k < C; ++k) acc += row[k];
        for (int k = C; k < w; ++k) acc += row[k];      // the widened last bin
      }
    }
  }
  if (live) {
    for (; t < T - 1; ++t, at += L) acc = add_run(acc, p.x, (int)at, (int)at + w);
    if (T > 1) acc = add_run(acc, p.x, (int)at, (int)min(at + w, (long long)n));
    p.F[p.prefix[c] + j] = acc;
  }
}

struct Peak {
  double m;
  uint32_t j;  // 0xffffffff: none
};
__device__ __forceinline__ bool peak_beats(const Peak& a, const Peak& b) {  // a before b: larger mean, then lower bin
  if (a.j == 0xffffffffu) return false;
  if (b.j == 0xffffffffu) return true;
  return a.m > b.m || (a.m == b.m && a.j < b.j);
}

__device__ __forceinline__ unsigned long long bin_count(unsigned long long N, uint32_t L, uint32_t C, uint32_t NB, uint32_t j) {
  const unsigned long long a = (unsigned long long)j * C, b = j == NB - 1 ? L : a + C;
  const unsigned long long q = N / L, rem = N % L;
  const unsigned long long part = rem <= a ? 0 : (rem >= b ? b - a : rem - a);
  return q * (b - a) + part;
}

__global__ void __launch_bounds__(256) fold_score(const ScoreParams p) {
  __shared__ double sh_m[4], sh_s[4], sh_q[4];
  __shared__ uint32_t sh_j[4];
  const int c = blockIdx.x;
  const uint32_t L = p.periods[c], C = (uint32_t)p.C;
  const uint32_t NB = p.prefix[c + 1] - p.prefix[c];
  const float* F = p.F + p.prefix[c];
  const unsigned long long N = p.N;
  const unsigned long long need = (N + C - 1) / C;
  const uint32_t used = need < NB ? (uint32_t)need : NB;
  // a NaN never displaces anything, so a thread's best skips them; a NaN in bin 0 stays, which the end looks at
  Peak best{0.0, 0xffffffffu};
  double s = 0.0, q = 0.0;
  for (uint32_t j = threadIdx.x; j < used; j += blockDim.x) {
    const double m = (double)F[j] / (double)bin_count(N, L, C, NB, j);
    s += m;
    q += m * m;
    const Peak x{m, j};
    if (m == m && peak_beats(x, best)) best = x;
  }
  for (int d = 32; d >= 1; d >>= 1) {
    const Peak o{__shfl_xor(best.m, d, 64), __shfl_xor(best.j, d, 64)};
    if (peak_beats(o, best)) best = o;
    s += __shfl_xor(s, d, 64);
    q += __shfl_xor(q, d, 64);
  }
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  if (lane == 0) {
    sh_m[wv] = best.m;
    sh_j[wv] = best.j;
    sh_s[wv] = s;
    sh_q[wv] = q;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int k = 1; k < 4; ++k) {
      const Peak o{sh_m[k], sh_j[k]};
      if (peak_beats(o, best)) best = o;
    }
    pfb_fold_score rec;
    rec.period = L;
    rec.num_bins = NB;
    rec.bins_used = used;
    rec.peak_bin = rec.peak_cells = rec.reserved = 0;
    rec.peak_sum = rec.peak_mean = 0.f;
    rec.sum_means = rec.sum_sq_means = 0.0;
    rec.cells = N;
    if (used > 0) {
      const double m0 = (double)F[0] / (double)bin_count(N, L, C, NB, 0);
      const uint32_t pj = (m0 != m0 || best.j == 0xffffffffu) ? 0u : best.j;  // only NaNs after a first: bin 0 stays
      const unsigned long long cnt = bin_count(N, L, C, NB, pj);
      rec.peak_bin = pj;
      rec.peak_cells = (uint32_t)cnt;
      rec.peak_sum = F[pj];
      rec.peak_mean = (float)((double)F[pj] / (double)cnt);
      rec.sum_means = (sh_s[0] + sh_s[1]) + (sh_s[2] + sh_s[3]);
      rec.sum_sq_means = (sh_q[0] + sh_q[1]) + (sh_q[2] + sh_q[3]);
    }
    p.out[c] = rec;
  }
}

// ---------------------------------------------------------------------------------
// host: checks and plan

enum { kTierAuto = 0, kTierDirect = 1, kTierTile = 2 };  // pfb_fold_set_tier (pfb_channelizer_dev.h)

bool tile_able(uint32_t C) { return C == 8 || C == 16 || C == 32 || C == 64; }

// fold_tile wherever it exists: it was measured to win there; kTierDirect is for tests and meter
bool runs_tile(uint32_t C, int tier) { return tile_able(C) && tier != kTierDirect; }

const char* fold_tier(uint32_t C, int tier = kTierAuto) {
  if (runs_tile(C, tier)) {
    switch (C) {
      case 8: return "pfb_fold_tile<8>";
      case 16: return "pfb_fold_tile<16>";
      case 32: return "pfb_fold_tile<32>";
      default: return "pfb_fold_tile<64>";
    }
  }
  switch (C) {
    case 1: return "pfb_fold_direct<1>";
    case 2: return "pfb_fold_direct<2>";
    case 3: return "pfb_fold_direct<3>";
    case 4: return "pfb_fold_direct<4>";
    default: return "pfb_fold_direct<n>";
  }
}

// Everything pfb_fold_describe and pfb_fold_create check before the device, in the order the header states
int fold_check(const pfb_fold_config* cfg, pfb_fold_plan* plan) {
  if (!cfg || !plan || cfg->struct_size != sizeof(pfb_fold_config) || !cfg->periods) return PFB_ERR_BAD_ARG;
  const uint32_t C = cfg->bin_cells;
  if (C < 1 || C > kMaxBinCells) return PFB_ERR_BAD_ARG;
  if (cfg->num_periods < 1 || cfg->num_periods > kMaxPeriods) return PFB_ERR_BAD_ARG;
  uint64_t total = 0;
  uint32_t most = 0;
  for (uint32_t c = 0; c < cfg->num_periods; ++c) {
    const uint32_t L = cfg->periods[c];
    if (L < C || L > kMaxPeriod || L / C > kMaxBins) return PFB_ERR_BAD_ARG;
    total += L / C;
    most = std::max(most, L / C);
  }
  if (cfg->flags != 0) return PFB_ERR_BAD_ARG;
  if (total * sizeof(float) > kMaxProfileBytes) return PFB_ERR_UNSUPPORTED;
  plan->profile_bytes = total * sizeof(float);
  plan->total_bins = total;
  plan->max_bins = most;
  std::memset(plan->kernel, 0, sizeof(plan->kernel));
  std::snprintf(plan->kernel, sizeof(plan->kernel), "%s", fold_tier(C));
  return PFB_OK;
}

uint64_t host_count(uint64_t N, uint32_t L, uint32_t C, uint32_t NB, uint32_t j) {
  const uint64_t a = (uint64_t)j * C, b = j == NB - 1 ? L : a + C;
  const uint64_t rem = N % L;
  return (N / L) * (b - a) + (rem <= a ? 0 : std::min(rem, b) - a);
}

}  // namespace

struct pfb_fold_handle {
  int device = 0;
  uint32_t C = 0, NC = 0;
  uint64_t total_bins = 0;
  std::vector<uint32_t> periods, prefix, tile_prefix;  // prefix[NC + 1], tile_prefix[NC + 1]
  int tier = 0;                // pfb_fold_set_tier
  hipStream_t stream = nullptr;
  hipEvent_t ev_switch = nullptr;
  uint64_t n = 0;              // cells taken
  float* d_F = nullptr;        // the profiles
  float* d_backup = nullptr;   // their state before the pfb_fold_process call that runs
  uint32_t* d_tables = nullptr;  // periods[NC], prefix[NC + 1], tile_prefix[NC + 1]
  pfb_fold_score* d_scores = nullptr;
  float* d_stage = nullptr;    // host cells on their way in
  size_t stage_cells = 0;
  const char* last_kernel = "";
};

namespace {

void free_fold(pfb_fold_handle* h) {
  if (!h) return;
  DeviceGuard g(h->device);
  (void)hipFree(h->d_F);
  (void)hipFree(h->d_backup);
  (void)hipFree(h->d_tables);
  (void)hipFree(h->d_scores);
  (void)hipFree(h->d_stage);
  if (h->ev_switch) (void)hipEventDestroy(h->ev_switch);
  delete h;
}

hipError_t allocate_fold(pfb_fold_handle* h) {
  const size_t bytes = (size_t)h->total_bins * sizeof(float);
  hipError_t e = hipSuccess;
  auto alloc = [&e](auto** p, size_t b) {
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(p), b);
  };
  alloc(&h->d_F, bytes);
  alloc(&h->d_backup, bytes);
  alloc(&h->d_tables, (3 * (size_t)h->NC + 2) * sizeof(uint32_t));
  alloc(&h->d_scores, (size_t)h->NC * sizeof(pfb_fold_score));
  if (e == hipSuccess) e = hipMemset(h->d_F, 0, bytes);
  if (e == hipSuccess) e = hipMemcpy(h->d_tables, h->periods.data(), h->NC * sizeof(uint32_t), hipMemcpyHostToDevice);
  if (e == hipSuccess)
    e = hipMemcpy(h->d_tables + h->NC, h->prefix.data(), ((size_t)h->NC + 1) * sizeof(uint32_t), hipMemcpyHostToDevice);
  if (e == hipSuccess)
    e = hipMemcpy(h->d_tables + 2 * (size_t)h->NC + 1, h->tile_prefix.data(), ((size_t)h->NC + 1) * sizeof(uint32_t),
                  hipMemcpyHostToDevice);
  return e;
}

int create_fold(const pfb_fold_config* cfg, pfb_fold_handle** out) {
  pfb_fold_plan plan{};
  int rc = fold_check(cfg, &plan);
  if (rc != PFB_OK) return rc;
  int dev = 0;
  rc = pfb::resolve_device(cfg->device_id, &dev);
  if (rc != PFB_OK) return rc;
  pfb_fold_handle* h = new pfb_fold_handle();
  h->device = dev;
  h->C = cfg->bin_cells;
  h->NC = cfg->num_periods;
  h->total_bins = plan.total_bins;
  h->periods.assign(cfg->periods, cfg->periods + cfg->num_periods);
  h->prefix.resize((size_t)h->NC + 1);
  h->prefix[0] = 0;
  h->tile_prefix.resize((size_t)h->NC + 1);
  h->tile_prefix[0] = 0;
  for (uint32_t c = 0; c < h->NC; ++c) {
    h->prefix[c + 1] = h->prefix[c] + h->periods[c] / h->C;
    h->tile_prefix[c + 1] = h->tile_prefix[c] + (h->periods[c] / h->C + 63) / 64;
  }
  DeviceGuard g(dev);
  const hipError_t e = allocate_fold(h);
  if (e != hipSuccess) {
    rc = pfb::hip_fail(e, "pfb_fold_create allocation");
    free_fold(h);
    return rc;
  }
  *out = h;
  return PFB_OK;
}

// One step: m <= 2^24 device cells, queued on the handle's stream; the index advances
int fold_step(pfb_fold_handle* h, const float* d_cells, uint64_t m) {
  FoldParams p{};
  p.x = d_cells;
  p.F = h->d_F;
  p.periods = h->d_tables;
  p.prefix = h->d_tables + h->NC;
  p.tile_prefix = h->d_tables + 2 * (size_t)h->NC + 1;
  p.s = h->n;
  p.n = (int)m;
  p.NC = (int)h->NC;
  p.C = (int)h->C;
  p.total_bins = (int)h->total_bins;
  const dim3 grid((unsigned)std::min<uint64_t>((h->total_bins + 255) / 256, kMaxGrid)), block(256);
  const dim3 tiles(h->tile_prefix[h->NC]), wave(64);
  if (runs_tile(h->C, h->tier)) {
    switch (h->C) {
      case 8: hipLaunchKernelGGL(fold_tile<8>, tiles, wave, 0, h->stream, p); break;
      case 16: hipLaunchKernelGGL(fold_tile<16>, tiles, wave, 0, h->stream, p); break;
      case 32: hipLaunchKernelGGL(fold_tile<32>, tiles, wave, 0, h->stream, p); break;
      default: hipLaunchKernelGGL(fold_tile<64>, tiles, wave, 0, h->stream, p); break;
    }
  } else switch (h->C) {
    case 1: hipLaunchKernelGGL(fold_direct<1>, grid, block, 0, h->stream, p); break;
    case 2: hipLaunchKernelGGL(fold_direct<2>, grid, block, 0, h->stream, p); break;
    case 3: hipLaunchKernelGGL(fold_direct<3>, grid, block, 0, h->stream, p); break;
    case 4: hipLaunchKernelGGL(fold_direct<4>, grid, block, 0, h->stream, p); break;
    default: hipLaunchKernelGGL(fold_direct<0>, grid, block, 0, h->stream, p); break;
  }
  HIP_TRY(hipGetLastError());
  h->last_kernel = fold_tier(h->C, h->tier);
  h->n += m;
  return PFB_OK;
}

int fold_enqueue(pfb_fold_handle* h, const float* d_cells, uint64_t n) {
  for (uint64_t done = 0; done < n;) {
    const uint64_t m = std::min(kStepCells, n - done);
    const int rc = fold_step(h, d_cells + done, m);
    if (rc != PFB_OK) return rc;
    done += m;
  }
  return PFB_OK;
}

// what every process call checks before the device is touched
int fold_check_call(const pfb_fold_handle* h, const float* cells, uint64_t n, bool device) {
  if (!h || (n > 0 && !cells)) return PFB_ERR_BAD_ARG;
  if (device && (reinterpret_cast<uintptr_t>(cells) % sizeof(float))) return PFB_ERR_BAD_ARG;
  if (n > kMaxIndex || h->n + n > kMaxIndex) return PFB_ERR_BAD_ARG;
  return PFB_OK;
}

// pfb_fold_process: the steps, and profiles and index back where they were when one of them fails
int fold_sync_call(pfb_fold_handle* h, const float* cells, uint64_t n, bool host) {
  DeviceGuard g(h->device);
  if (n == 0) {
    HIP_TRY(hipStreamSynchronize(h->stream));
    return PFB_OK;
  }
  const size_t bytes = (size_t)h->total_bins * sizeof(float);
  const uint64_t n0 = h->n;
  if (host && h->stage_cells < std::min(n, kStepCells)) {
    (void)hipFree(h->d_stage);
    h->d_stage = nullptr;
    h->stage_cells = 0;
    HIP_TRY(hipMalloc(reinterpret_cast<void**>(&h->d_stage), (size_t)std::min(n, kStepCells) * sizeof(float)));
    h->stage_cells = (size_t)std::min(n, kStepCells);
  }
  HIP_TRY(hipMemcpyAsync(h->d_backup, h->d_F, bytes, hipMemcpyDeviceToDevice, h->stream));
  auto fail = [&](int code) {  // from here on every failure puts the state back before the call returns
    (void)hipStreamSynchronize(h->stream);
    (void)hipMemcpyAsync(h->d_F, h->d_backup, bytes, hipMemcpyDeviceToDevice, h->stream);
    (void)hipStreamSynchronize(h->stream);
    h->n = n0;
    return code;
  };
  int rc = PFB_OK;
  if (!host) {
    rc = fold_enqueue(h, cells, n);
    if (rc != PFB_OK) return fail(rc);
  } else {
    for (uint64_t done = 0; done < n;) {
      const uint64_t m = std::min(kStepCells, n - done);
      hipError_t e = hipMemcpyAsync(h->d_stage, cells + done, m * sizeof(float), hipMemcpyHostToDevice, h->stream);
      if (e != hipSuccess) return fail(pfb::hip_fail(e, "pfb_fold_process staging"));
      rc = fold_step(h, h->d_stage, m);
      if (rc != PFB_OK) return fail(rc);
      e = hipStreamSynchronize(h->stream);  // the one staging buffer is free again
      if (e != hipSuccess) return fail(pfb::hip_fail(e, "pfb_fold_process"));
      done += m;
    }
  }
  const hipError_t e = hipStreamSynchronize(h->stream);
  if (e != hipSuccess) return fail(pfb::hip_fail(e, "pfb_fold_process"));
  return PFB_OK;
}

}  // namespace

extern "C" int pfb_fold_describe(const pfb_fold_config* cfg, pfb_fold_plan* plan_out) {
  return pfb::abi_guard([&]() -> int {
    pfb_fold_plan plan{};
    const int rc = fold_check(cfg, plan_out ? &plan : nullptr);
    if (rc == PFB_OK) *plan_out = plan;
    return rc;
  });
}

extern "C" int pfb_fold_counts(const pfb_fold_config* cfg, uint32_t candidate, uint64_t num_cells, uint64_t* counts_out) {
  return pfb::abi_guard([&]() -> int {
    pfb_fold_plan plan{};
    const int rc = fold_check(cfg, &plan);
    if (rc != PFB_OK) return rc;
    if (!counts_out || candidate >= cfg->num_periods || num_cells > kMaxIndex) return PFB_ERR_BAD_ARG;
    const uint32_t L = cfg->periods[candidate], C = cfg->bin_cells, NB = L / C;
    for (uint32_t j = 0; j < NB; ++j) counts_out[j] = host_count(num_cells, L, C, NB, j);
    return PFB_OK;
  });
}

extern "C" int pfb_fold_create(const pfb_fold_config* cfg, pfb_fold_handle** out) {
  return pfb::abi_guard([&]() -> int {
    if (!out) return PFB_ERR_BAD_ARG;
    *out = nullptr;
    return create_fold(cfg, out);
  });
}

extern "C" int pfb_fold_destroy(pfb_fold_handle* h) {
  return pfb::abi_guard([&]() -> int {
    if (!h) return PFB_ERR_BAD_ARG;
    free_fold(h);
    return PFB_OK;
  });
}

extern "C" int pfb_fold_reset(pfb_fold_handle* h) {
  return pfb::abi_guard([&]() -> int {
    if (!h) return PFB_ERR_BAD_ARG;
    DeviceGuard g(h->device);
    HIP_TRY(hipMemsetAsync(h->d_F, 0, (size_t)h->total_bins * sizeof(float), h->stream));
    h->n = 0;
    return PFB_OK;
  });
}

extern "C" int pfb_fold_set_stream(pfb_fold_handle* h, void* hip_stream) {
  return pfb::abi_guard([&]() -> int {
    if (!h) return PFB_ERR_BAD_ARG;
    return pfb::switch_stream(h->device, &h->stream, &h->ev_switch, static_cast<hipStream_t>(hip_stream));
  });
}

extern "C" int pfb_fold_sync(pfb_fold_handle* h) {
  return pfb::abi_guard([&]() -> int {
    if (!h) return PFB_ERR_BAD_ARG;
    DeviceGuard g(h->device);
    HIP_TRY(hipStreamSynchronize(h->stream));
    return PFB_OK;
  });
}

extern "C" int pfb_fold_get_device(const pfb_fold_handle* h, int* device_id) {
  return pfb::abi_guard([&]() -> int {
    if (!h || !device_id) return PFB_ERR_BAD_ARG;
    *device_id = h->device;
    return PFB_OK;
  });
}

extern "C" int pfb_fold_next_index(const pfb_fold_handle* h, uint64_t* index_out) {
  return pfb::abi_guard([&]() -> int {
    if (!h || !index_out) return PFB_ERR_BAD_ARG;
    *index_out = h->n;
    return PFB_OK;
  });
}

extern "C" int pfb_fold_set_tier(pfb_fold_handle* h, int tier) {
  return pfb::abi_guard([&]() -> int {
    if (!h || tier < kTierAuto || tier > kTierTile) return PFB_ERR_BAD_ARG;
    if (tier == kTierTile && !tile_able(h->C)) return PFB_ERR_UNSUPPORTED;
    h->tier = tier;
    return PFB_OK;
  });
}

extern "C" int pfb_fold_process(pfb_fold_handle* h, const float* cells, uint64_t num_cells, uint32_t mem) {
  return pfb::abi_guard([&]() -> int {
    if (mem > PFB_MEM_DEVICE) return PFB_ERR_BAD_ARG;
    const int rc = fold_check_call(h, cells, num_cells, mem == PFB_MEM_DEVICE);
    if (rc != PFB_OK) return rc;
    return fold_sync_call(h, cells, num_cells, mem == PFB_MEM_HOST);
  });
}

extern "C" int pfb_fold_process_async(pfb_fold_handle* h, const float* d_cells, uint64_t num_cells) {
  return pfb::abi_guard([&]() -> int {
    const int rc = fold_check_call(h, d_cells, num_cells, true);
    if (rc != PFB_OK) return rc;
    DeviceGuard g(h->device);
    return fold_enqueue(h, d_cells, num_cells);
  });
}

extern "C" int pfb_fold_scores(pfb_fold_handle* h, pfb_fold_score* out, uint64_t capacity, uint32_t mem) {
  return pfb::abi_guard([&]() -> int {
    if (mem > PFB_MEM_DEVICE || !h || !out) return PFB_ERR_BAD_ARG;
    if (mem == PFB_MEM_DEVICE && reinterpret_cast<uintptr_t>(out) % 8) return PFB_ERR_BAD_ARG;
    if (capacity < h->NC) return PFB_ERR_CAPACITY;
    DeviceGuard g(h->device);
    ScoreParams p{};
    p.F = h->d_F;
    p.periods = h->d_tables;
    p.prefix = h->d_tables + h->NC;
    p.out = mem == PFB_MEM_DEVICE ? out : h->d_scores;
    p.N = h->n;
    p.C = (int)h->C;
    hipLaunchKernelGGL(fold_score, dim3(h->NC), dim3(256), 0, h->stream, p);
    HIP_TRY(hipGetLastError());
    if (mem == PFB_MEM_HOST)
      HIP_TRY(hipMemcpyAsync(out, h->d_scores, (size_t)h->NC * sizeof(pfb_fold_score), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    return PFB_OK;
  });
}

extern "C" int pfb_fold_profile(pfb_fold_handle* h, uint32_t candidate, float* out, uint64_t capacity_bins, uint32_t mem) {
  return pfb::abi_guard([&]() -> int {
    if (mem > PFB_MEM_DEVICE || !h || !out || candidate >= h->NC) return PFB_ERR_BAD_ARG;
    if (mem == PFB_MEM_DEVICE && reinterpret_cast<uintptr_t>(out) % sizeof(float)) return PFB_ERR_BAD_ARG;
    const uint32_t NB = h->prefix[candidate + 1] - h->prefix[candidate];
    if (capacity_bins < NB) return PFB_ERR_CAPACITY;
    DeviceGuard g(h->device);
    HIP_TRY(hipMemcpyAsync(out, h->d_F + h->prefix[candidate], (size_t)NB * sizeof(float),
                           mem == PFB_MEM_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    return PFB_OK;
  });
}

extern "C" const char* pfb_fold_last_kernel(const pfb_fold_handle* h) { return h ? h->last_kernel : ""; }
