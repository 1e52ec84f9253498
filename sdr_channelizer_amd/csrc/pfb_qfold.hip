// pfb_qfold.hip -- fractional-PRI search and regridder (pfb_qfold_* and pfb_regrid_* in include/pfb_channelizer.h, where
// the arithmetic is defined): pfb_fold.hip's folder at periods Pq given in 2^-32 samples, and a gather that lays the
// windows of such a train onto an integer grid.  The structure is pfb_fold.hip's; only where a period begins changes.
//   The position of a candidate in the stream is three numbers (QState): m, the period the next cell lies in, Al, the
//   low 32 bits of m Pf, and back, the cells of period m already taken.  From them the start of period m + t relative to
//   period m's is random access in 64 bits:  off(t) = t Pi + ceil((Al + t Pf) / 2^32) - (Al > 0).  Only the three numbers
//   themselves need more than 64 bits, once: pfb_qfold_set_index computes them on the host in 128-bit arithmetic, and
//   qfold_advance, one lane per candidate queued behind every step, moves them on by the step's cells with a 64-bit
//   division ((back + n) 2^32 < 2^58).  So pfb_qfold_process_async never waits for the device and uploads nothing.
//   Consecutive periods are walked without the multiply (Walker): the fraction's low word takes Pf and its carry is the
//   period's extra cell.  Computing off(t) afresh for every period cost the batched kernels up to a factor of two.
//   qfold_direct<CW>  fold_direct: one lane per (candidate, bin).  CW = 1 .. 4 loads a batch of whole periods before the
//                     dependent adds; the widened last bin joins the batch when it is CW cells in a short period, and
//                     takes its one extra cell of a long period under a flag.  CW = 0 for any C.
//   qfold_tile<C>     fold_tile, C = 8, 16, 32, 64: one wave per (candidate, 64 adjacent bins), the stretches of P = 64 / C
//                     periods staged in LDS, rows C + 1 floats apart.  A stretch begins at off(t) + j0 C, and the tail
//                     tile's is one cell longer in a long period.
//   qfold_score       fold_score with counts from the state now and the state at the start index, over the used bins.
//   regrid_copy       one lane per output element, consecutive lanes on consecutive t: within a row a wave's loads and
//                     stores are runs.  Rows start at element alignment only (4 or 8 bytes) and source and destination
//                     are misaligned against each other differently in every row, so accesses are one element wide.
// No atomics: every profile element, state and record has one writer.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <new>
#include <vector>

#include "pfb_channelizer_dev.h"
#include "pfb_common.h"
#include "pfb_host.h"

namespace {

using namespace pfb;

constexpr uint64_t kStepCells = (uint64_t)1 << 24;  // cells per kernel launch, and per staging step of a host buffer
constexpr uint64_t kMaxProfileBytes = (uint64_t)64 << 20;
constexpr uint32_t kMaxPeriod = 1u << 24, kMaxBins = 1u << 16, kMaxPeriods = 4096, kMaxBinCells = 64;
constexpr uint64_t kMaxPeriodQ = (uint64_t)kMaxPeriod << 32;
constexpr uint64_t kMaxIndex = (uint64_t)1 << 62;
constexpr unsigned kMaxGrid = 1u << 16;

struct QState {            // where the next cell lies under one candidate
  unsigned long long m;    // its period
  uint32_t Al;             // (m Pf) mod 2^32
  uint32_t back;           // cells of period m before it: N - start(m), less than the period's length
};

struct QFoldParams {
  const float* x;                    // the step's cells: x[0] is global cell N
  float* F;                          // the profiles, candidate after candidate
  const unsigned long long* pq;      // [NC]
  const uint32_t* prefix;            // [NC + 1]: bins before candidate c
  const uint32_t* tile_prefix;       // [NC + 1]: tiles of 64 bins before candidate c (qfold_tile)
  const QState* st;                  // [NC]: the state at x[0]
  int n;                             // cells of the step, 1 .. 2^24
  int NC, C, total_bins;
};

struct QScoreParams {
  const float* F;
  const unsigned long long* pq;
  const uint32_t* prefix;
  const QState* st;    // at N
  const QState* st0;   // at N0
  pfb_qfold_score* out;
  unsigned long long N, N0;
  int C;
};

// the candidate that owns global bin g: the last c with prefix[c] <= g
__device__ __forceinline__ int owner(const uint32_t* prefix, int NC, uint32_t g) {
  int lo = 0, hi = NC;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (prefix[mid] <= g) lo = mid; else hi = mid;
  }
  return lo;
}

// start(m + t) - start(m) for a period m with (m Pf) mod 2^32 = Al; t < 2^27
__host__ __device__ __forceinline__ long long qoff(uint32_t Pi, uint32_t Pf, uint32_t Al, unsigned long long t) {
  return (long long)(t * Pi + ((Al + t * Pf + 0xffffffffull) >> 32)) - (Al > 0 ? 1 : 0);
}

// the largest t with start(m + t) <= start(m) + rel; rel < 2^26
__host__ __device__ __forceinline__ unsigned long long qperiods(unsigned long long Pq, uint32_t Al, unsigned long long rel) {
  return ((rel << 32) + (uint32_t)(0u - Al)) / Pq;
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

// off(t) for consecutive t: one 64-bit multiply seats it, then every period is an add with carry.  With
// u(t) = Al + t Pf + 2^32 - 1, off(t) = t Pi + (u(t) >> 32) - (Al > 0), and u(t + 1) = u(t) + Pf: period t is one cell
// longer than Pi exactly when the low word of u overflows.
struct Walker {
  long long off;  // off(t)
  uint32_t lo;    // the low word of u(t)
  __device__ __forceinline__ Walker(uint32_t Pi, uint32_t Pf, uint32_t Al, unsigned long long t) {
    const unsigned long long u = Al + t * Pf + 0xffffffffull;
    off = (long long)(t * Pi + (u >> 32)) - (Al > 0 ? 1 : 0);
    lo = (uint32_t)u;
  }
  // the length of period t; moves on to t + 1
  __device__ __forceinline__ int next(uint32_t Pi, uint32_t Pf) {
    const uint32_t s = lo + Pf;
    const int len = (int)Pi + (s < lo ? 1 : 0);
    lo = s;
    off += len;
    return len;
  }
};

struct Lane {  // one bin of one candidate inside a step
  uint32_t Pi, Pf, Al;
  long long back;
  int a, C, n;
  bool last;
  // the bin's cells of the period that begins at off (relative to the state's period) and is len cells long, clamped to
  // the step
  __device__ __forceinline__ float period(float acc, const float* x, long long off, int len) const {
    const int w = last ? len - a : C;
    const long long lo = off - back + a;
    return add_run(acc, x, (int)max(lo, 0ll), (int)min(lo + w, (long long)n));
  }
  // periods t .. T - 1, one after the other
  __device__ __forceinline__ float periods(float acc, const float* x, int t, int T) const {
    Walker w(Pi, Pf, Al, (unsigned long long)t);
    for (; t < T; ++t) {
      const long long off = w.off;
      acc = period(acc, x, off, w.next(Pi, Pf));
    }
    return acc;
  }
};

template <int CW>
__global__ void __launch_bounds__(256) qfold_direct(const QFoldParams p) {
  const int C = CW ? CW : p.C;
  const uint32_t stride = gridDim.x * blockDim.x;
  for (uint32_t g = blockIdx.x * blockDim.x + threadIdx.x; g < (uint32_t)p.total_bins; g += stride) {
    const int c = owner(p.prefix, p.NC, g);
    const unsigned long long Pq = p.pq[c];
    const QState st = p.st[c];
    const int j = (int)(g - p.prefix[c]), NB = (int)(p.prefix[c + 1] - p.prefix[c]);
    Lane ln{(uint32_t)(Pq >> 32), (uint32_t)Pq, st.Al, (long long)st.back, j * C, C, p.n, j == NB - 1};
    const int T = (int)qperiods(Pq, st.Al, (unsigned long long)(ln.back + p.n - 1)) + 1;  // periods the step touches
    float acc = p.F[g];
    acc = ln.periods(acc, p.x, 0, 1);
    int t = 1;
    if constexpr (CW > 0) {
      if (!ln.last || (int)ln.Pi - ln.a == CW) {  // whole periods, a batch of them loaded before the adds
        constexpr int P = CW == 1 ? 32 : CW == 2 ? 16 : 8;
        Walker w(ln.Pi, ln.Pf, ln.Al, 1);
        for (; t + P <= T - 1; t += P) {
          float v[P][CW], ex[P];
          bool lg[P];
#pragma unroll
          for (int q = 0; q < P; ++q) {
            const float* at = p.x + (w.off - ln.back + ln.a);
            lg[q] = w.next(ln.Pi, ln.Pf) > (int)ln.Pi && ln.last;  // a long period gives the last bin one cell more
#pragma unroll
            for (int k = 0; k < CW; ++k) v[q][k] = at[k];
            if (lg[q]) ex[q] = at[CW];
          }
#pragma unroll
          for (int q = 0; q < P; ++q) {
#pragma unroll
            for (int k = 0; k < CW; ++k) acc += v[q][k];
            if (lg[q]) acc += ex[q];
          }
        }
      }
    }
    acc = ln.periods(acc, p.x, t, T);
    p.F[g] = acc;
  }
}

template <int C>
struct TileShape {
  static constexpr int P = C >= 64 ? 1 : 64 / C;        // periods per batch: about 64 loads per lane in flight
  static constexpr int V = C + 1;                       // loads per lane and period: ceil((64 C + C) / 64)
  static constexpr int Row = 64 * (C + 1) + C;          // floats of one period in LDS: 64 rows of C + 1, the last up to 2 C
};

template <int C>
__global__ void __launch_bounds__(64) qfold_tile(const QFoldParams p) {
  using S = TileShape<C>;
  constexpr int P = S::P, V = S::V;
  __shared__ float sh[P * S::Row];
  const int lane = threadIdx.x;
  const int c = owner(p.tile_prefix, p.NC, blockIdx.x);
  const unsigned long long Pq = p.pq[c];
  const QState st = p.st[c];
  const uint32_t Pi = (uint32_t)(Pq >> 32), Pf = (uint32_t)Pq, Al = st.Al;
  const long long back = (long long)st.back;
  const int NB = (int)(p.prefix[c + 1] - p.prefix[c]);
  const int j0 = (int)(blockIdx.x - p.tile_prefix[c]) * 64;
  const int nb = min(64, NB - j0);                      // bins of this tile
  const bool tail = j0 + nb == NB;                      // it holds the last bin
  const int W0 = tail ? (int)Pi - j0 * C : 64 * C;      // cells of the tile in a short period
  const int j = j0 + lane;
  const bool live = lane < nb;
  Lane ln{Pi, Pf, Al, back, j * C, C, p.n, live && j == NB - 1};
  const int T = (int)qperiods(Pq, Al, (unsigned long long)(back + p.n - 1)) + 1;
  float acc = live ? p.F[p.prefix[c] + j] : 0.f;
  if (live) acc = ln.periods(acc, p.x, 0, 1);
  int t = 1;
  float v[P][V];
  Walker w(Pi, Pf, Al, 1);                              // at the next period to load
  // the stretches of the next P whole periods; bit q of the result: period q of them is a long one and this the tail tile
  auto load = [&]() -> unsigned {
    unsigned mask = 0;
#pragma unroll
    for (int q = 0; q < P; ++q) {
      const float* from = p.x + (w.off - back + (long long)j0 * C);
      const bool lg = w.next(Pi, Pf) > (int)Pi && tail;
      const int Wq = W0 + (lg ? 1 : 0);
#pragma unroll
      for (int k = 0; k < V; ++k) {
        const int e = lane + 64 * k;
        if (e < Wq) v[q][k] = from[e];
      }
      mask |= (lg ? 1u : 0u) << q;
    }
    return mask;
  };
  unsigned next_mask = 0;
  if (t + P <= T - 1) next_mask = load();
  for (; t + P <= T - 1; t += P) {
    const unsigned mask = next_mask;
    __syncthreads();                                    // the rows of the batch before are read
#pragma unroll
    for (int q = 0; q < P; ++q) {
      const int Wq = W0 + (int)((mask >> q) & 1u);
#pragma unroll
      for (int k = 0; k < V; ++k) {
        const int e = lane + 64 * k;
        if (e < Wq) sh[q * S::Row + e + min(e / C, nb - 1)] = v[q][k];   // row e / C, the last row takes what is left
      }
    }
    __syncthreads();
    if (t + 2 * P <= T - 1) next_mask = load();         // in flight under the adds
    if (live) {
#pragma unroll
      for (int q = 0; q < P; ++q) {
        const float* row = sh + q * S::Row + lane * (C + 1);
#pragma unroll
        for (int k = 0; k < C; ++k) acc += row[k];
        const int wd = ln.last ? (int)Pi - ln.a + (int)((mask >> q) & 1u) : C;
        for (int k = C; k < wd; ++k) acc += row[k];     // the widened last bin
      }
    }
  }
  if (live) {
    acc = ln.periods(acc, p.x, t, T);
    p.F[p.prefix[c] + j] = acc;
  }
}

// the states moved on by the n cells of the step before: one lane per candidate
__global__ void __launch_bounds__(256) qfold_advance(QState* st, const unsigned long long* pq, int NC, int n) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= NC) return;
  const unsigned long long Pq = pq[c];
  const uint32_t Pi = (uint32_t)(Pq >> 32), Pf = (uint32_t)Pq;
  const QState s = st[c];
  const unsigned long long rel = (unsigned long long)s.back + (unsigned long long)n;
  const unsigned long long t = qperiods(Pq, s.Al, rel);
  QState o;
  o.m = s.m + t;
  o.Al = (uint32_t)(s.Al + t * Pf);
  o.back = (uint32_t)(rel - (unsigned long long)qoff(Pi, Pf, s.Al, t));
  st[c] = o;
}

struct Peak {
  double m;
  uint32_t j;  // 0xffffffff: none
};
__host__ __device__ __forceinline__ bool peak_beats(const Peak& a, const Peak& b) {  // a before b: larger mean, then lower bin
  if (a.j == 0xffffffffu) return false;
  if (b.j == 0xffffffffu) return true;
  return a.m > b.m || (a.m == b.m && a.j < b.j);
}

// n_j(N) from the state at N
__host__ __device__ __forceinline__ unsigned long long qcount(const QState& s, unsigned long long N, uint32_t C, uint32_t NB,
                                                              uint32_t j) {
  if (j < NB - 1) {
    const long long d = (long long)s.back - (long long)j * C;
    return s.m * C + (unsigned long long)(d <= 0 ? 0 : (d >= (long long)C ? (long long)C : d));
  }
  const unsigned long long a = (unsigned long long)(NB - 1) * C;
  return (N - s.back) - s.m * a + (s.back > a ? s.back - a : 0);
}

__global__ void __launch_bounds__(256) qfold_score(const QScoreParams p) {
  __shared__ double sh_m[4], sh_s[4], sh_q[4];
  __shared__ uint32_t sh_j[4], sh_u[4], sh_f[4];
  const int c = blockIdx.x;
  const uint32_t C = (uint32_t)p.C;
  const uint32_t NB = p.prefix[c + 1] - p.prefix[c];
  const float* F = p.F + p.prefix[c];
  const QState s1 = p.st[c], s0 = p.st0[c];
  auto count = [&](uint32_t j) { return qcount(s1, p.N, C, NB, j) - qcount(s0, p.N0, C, NB, j); };
  // a NaN never displaces anything, so a thread's best skips them; a NaN in the first used bin stays: the end looks at it
  Peak best{0.0, 0xffffffffu};
  double s = 0.0, q = 0.0;
  uint32_t used = 0, first = 0xffffffffu;
  for (uint32_t j = threadIdx.x; j < NB; j += blockDim.x) {
    const unsigned long long n = count(j);
    if (n == 0) continue;
    ++used;
    first = min(first, j);
    const double m = (double)F[j] / (double)n;
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
    used += __shfl_xor(used, d, 64);
    first = min(first, (uint32_t)__shfl_xor(first, d, 64));
  }
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  if (lane == 0) {
    sh_m[wv] = best.m;
    sh_j[wv] = best.j;
    sh_s[wv] = s;
    sh_q[wv] = q;
    sh_u[wv] = used;
    sh_f[wv] = first;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int k = 1; k < 4; ++k) {
      const Peak o{sh_m[k], sh_j[k]};
      if (peak_beats(o, best)) best = o;
      first = min(first, sh_f[k]);
    }
    pfb_qfold_score rec;
    rec.period_q32 = p.pq[c];
    rec.num_bins = NB;
    rec.bins_used = (sh_u[0] + sh_u[1]) + (sh_u[2] + sh_u[3]);
    rec.peak_bin = rec.reserved = 0;
    rec.peak_cells = 0;
    rec.peak_sum = rec.peak_mean = 0.f;
    rec.sum_means = rec.sum_sq_means = 0.0;
    rec.cells = p.N - p.N0;
    if (rec.bins_used > 0) {
      const double m0 = (double)F[first] / (double)count(first);
      const uint32_t pj = (m0 != m0 || best.j == 0xffffffffu) ? first : best.j;  // only NaNs after a first: it stays
      const unsigned long long cnt = count(pj);
      rec.peak_bin = pj;
      rec.peak_cells = cnt;
      rec.peak_sum = F[pj];
      rec.peak_mean = (float)((double)F[pj] / (double)cnt);
      rec.sum_means = (sh_s[0] + sh_s[1]) + (sh_s[2] + sh_s[3]);
      rec.sum_sq_means = (sh_q[0] + sh_q[1]) + (sh_q[2] + sh_q[3]);
    }
    p.out[c] = rec;
  }
}

struct RegridParams {
  const void* x;              // the step's input: x[0] is input element s
  void* out;                  // the step's first output element
  unsigned long long* count_out;  // where the call's count goes (the call's first launch only), or null
  unsigned long long total;   // the call's count
  long long base;             // o + start(k0) - s
  uint32_t count;             // output elements of the step
  uint32_t Pi, Pf, Al;        // Al = (k0 Pf) mod 2^32
  uint32_t R, r0;             // the step's first output element is element r0 of row k0
};

template <typename E>
__global__ void __launch_bounds__(256) regrid_copy(const RegridParams p) {
  if (p.count_out && blockIdx.x == 0 && threadIdx.x == 0) *p.count_out = p.total;
  const E* x = static_cast<const E*>(p.x);
  E* out = static_cast<E*>(p.out);
  const uint32_t stride = gridDim.x * blockDim.x;
  for (uint32_t u = blockIdx.x * blockDim.x + threadIdx.x; u < p.count; u += stride) {
    const uint32_t q = p.r0 + u;
    const uint32_t dk = q / p.R, r = q - dk * p.R;
    out[u] = x[p.base + qoff(p.Pi, p.Pf, p.Al, dk) + r];
  }
}

// ---------------------------------------------------------------------------------
// host: 128-bit arithmetic, checks and plan

using u128 = unsigned __int128;

QState state_at(uint64_t N, uint64_t Pq) {  // m(N), (m Pf) mod 2^32, N - start(m)
  const uint64_t Pi = Pq >> 32, Pf = Pq & 0xffffffffull;
  const uint64_t m = (uint64_t)(((u128)N << 32) / Pq);
  const u128 A = (u128)m * Pf;
  const uint64_t start = (uint64_t)((u128)m * Pi + ((A + 0xffffffffull) >> 32));
  return QState{m, (uint32_t)(uint64_t)A, (uint32_t)(N - start)};
}

uint64_t start_of(uint64_t m, uint64_t Pq) { return (uint64_t)(((u128)m * Pq + 0xffffffffull) >> 32); }

enum { kTierAuto = 0, kTierDirect = 1, kTierTile = 2 };  // pfb_qfold_set_tier (pfb_channelizer_dev.h)

bool tile_able(uint32_t C) { return C == 8 || C == 16 || C == 32 || C == 64; }

// qfold_tile wherever it exists: measured to win there as fold_tile does
bool runs_tile(uint32_t C, int tier) { return tile_able(C) && tier != kTierDirect; }

const char* qfold_tier(uint32_t C, int tier = kTierAuto) {
  if (runs_tile(C, tier)) {
    switch (C) {
      case 8: return "pfb_qfold_tile<8>";
      case 16: return "pfb_qfold_tile<16>";
      case 32: return "pfb_qfold_tile<32>";
      default: return "pfb_qfold_tile<64>";
    }
  }
  switch (C) {
    case 1: return "pfb_qfold_direct<1>";
    case 2: return "pfb_qfold_direct<2>";
    case 3: return "pfb_qfold_direct<3>";
    case 4: return "pfb_qfold_direct<4>";
    default: return "pfb_qfold_direct<n>";
  }
}

// Everything pfb_qfold_describe and pfb_qfold_create check before the device, in the order the header states
int qfold_check(const pfb_qfold_config* cfg, pfb_qfold_plan* plan) {
  if (!cfg || !plan || cfg->struct_size != sizeof(pfb_qfold_config) || !cfg->periods_q32) return PFB_ERR_BAD_ARG;
  const uint32_t C = cfg->bin_cells;
  if (C < 1 || C > kMaxBinCells) return PFB_ERR_BAD_ARG;
  if (cfg->num_periods < 1 || cfg->num_periods > kMaxPeriods) return PFB_ERR_BAD_ARG;
  uint64_t total = 0;
  uint32_t most = 0;
  for (uint32_t c = 0; c < cfg->num_periods; ++c) {
    const uint64_t Pq = cfg->periods_q32[c];
    const uint32_t Pi = (uint32_t)(Pq >> 32);
    if (Pq > kMaxPeriodQ || Pi < C || Pi / C > kMaxBins) return PFB_ERR_BAD_ARG;
    total += Pi / C;
    most = std::max(most, Pi / C);
  }
  if (cfg->flags != 0) return PFB_ERR_BAD_ARG;
  if (total * sizeof(float) > kMaxProfileBytes) return PFB_ERR_UNSUPPORTED;
  plan->profile_bytes = total * sizeof(float);
  plan->total_bins = total;
  plan->max_bins = most;
  std::memset(plan->kernel, 0, sizeof(plan->kernel));
  std::snprintf(plan->kernel, sizeof(plan->kernel), "%s", qfold_tier(C));
  return PFB_OK;
}

}  // namespace

struct pfb_qfold_handle {
  int device = 0;
  uint32_t C = 0, NC = 0;
  uint64_t total_bins = 0;
  std::vector<uint64_t> periods;
  std::vector<uint32_t> prefix, tile_prefix;  // [NC + 1] each
  int tier = 0;                  // pfb_qfold_set_tier
  uint64_t step = kStepCells;
  hipStream_t stream = nullptr;
  hipEvent_t ev_switch = nullptr;
  uint64_t n0 = 0, n = 0;        // the start index, the index of the next cell
  float* d_F = nullptr;          // the profiles
  float* d_backup = nullptr;     // their state before the pfb_qfold_process call that runs
  unsigned long long* d_pq = nullptr;
  uint32_t* d_tables = nullptr;  // prefix[NC + 1], tile_prefix[NC + 1]
  QState* d_state = nullptr;     // [3 NC]: at N, at N0, and the first as it was before the pfb_qfold_process call that runs
  pfb_qfold_score* d_scores = nullptr;
  float* d_stage = nullptr;      // host cells on their way in
  size_t stage_cells = 0;
  const char* last_kernel = "";
};

struct pfb_regrid_handle {
  int device = 0;
  uint64_t Pq = 0, origin = 0;
  uint32_t R = 0, elem = 0;
  hipStream_t stream = nullptr;
  hipEvent_t ev_switch = nullptr;
  uint64_t n = 0;                // index of the next input element
  void* d_in = nullptr;          // the host route's staging
  void* d_out = nullptr;
  size_t in_elems = 0, out_elems = 0;
};

namespace {

void free_qfold(pfb_qfold_handle* h) {
  if (!h) return;
  DeviceGuard g(h->device);
  (void)hipFree(h->d_F);
  (void)hipFree(h->d_backup);
  (void)hipFree(h->d_pq);
  (void)hipFree(h->d_tables);
  (void)hipFree(h->d_state);
  (void)hipFree(h->d_scores);
  (void)hipFree(h->d_stage);
  if (h->ev_switch) (void)hipEventDestroy(h->ev_switch);
  delete h;
}

// profiles to +0 and both states to those of cell N0: waits for the stream, before and after
hipError_t seek_qfold(pfb_qfold_handle* h, uint64_t N0) {
  std::vector<QState> st(2 * (size_t)h->NC);
  for (uint32_t c = 0; c < h->NC; ++c) st[c] = st[h->NC + c] = state_at(N0, h->periods[c]);
  hipError_t e = hipStreamSynchronize(h->stream);
  if (e == hipSuccess) e = hipMemsetAsync(h->d_F, 0, (size_t)h->total_bins * sizeof(float), h->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(h->d_state, st.data(), st.size() * sizeof(QState), hipMemcpyHostToDevice, h->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
  if (e == hipSuccess) h->n0 = h->n = N0;
  return e;
}

hipError_t allocate_qfold(pfb_qfold_handle* h) {
  const size_t bytes = (size_t)h->total_bins * sizeof(float);
  const size_t NC = h->NC;
  hipError_t e = hipSuccess;
  auto alloc = [&e](auto** p, size_t b) {
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(p), b);
  };
  alloc(&h->d_F, bytes);
  alloc(&h->d_backup, bytes);
  alloc(&h->d_pq, NC * sizeof(uint64_t));
  alloc(&h->d_tables, (2 * NC + 2) * sizeof(uint32_t));
  alloc(&h->d_state, 3 * NC * sizeof(QState));
  alloc(&h->d_scores, NC * sizeof(pfb_qfold_score));
  if (e == hipSuccess) e = hipMemcpy(h->d_pq, h->periods.data(), NC * sizeof(uint64_t), hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(h->d_tables, h->prefix.data(), (NC + 1) * sizeof(uint32_t), hipMemcpyHostToDevice);
  if (e == hipSuccess)
    e = hipMemcpy(h->d_tables + NC + 1, h->tile_prefix.data(), (NC + 1) * sizeof(uint32_t), hipMemcpyHostToDevice);
  if (e == hipSuccess) e = seek_qfold(h, 0);
  return e;
}

int create_qfold(const pfb_qfold_config* cfg, pfb_qfold_handle** out) {
  pfb_qfold_plan plan{};
  int rc = qfold_check(cfg, &plan);
  if (rc != PFB_OK) return rc;
  int dev = 0;
  rc = pfb::resolve_device(cfg->device_id, &dev);
  if (rc != PFB_OK) return rc;
  pfb_qfold_handle* h = new pfb_qfold_handle();
  h->device = dev;
  h->C = cfg->bin_cells;
  h->NC = cfg->num_periods;
  h->total_bins = plan.total_bins;
  h->periods.assign(cfg->periods_q32, cfg->periods_q32 + cfg->num_periods);
  h->prefix.resize((size_t)h->NC + 1);
  h->prefix[0] = 0;
  h->tile_prefix.resize((size_t)h->NC + 1);
  h->tile_prefix[0] = 0;
  for (uint32_t c = 0; c < h->NC; ++c) {
    const uint32_t NB = (uint32_t)(h->periods[c] >> 32) / h->C;
    h->prefix[c + 1] = h->prefix[c] + NB;
    h->tile_prefix[c + 1] = h->tile_prefix[c] + (NB + 63) / 64;
  }
  DeviceGuard g(dev);
  const hipError_t e = allocate_qfold(h);
  if (e != hipSuccess) {
    rc = pfb::hip_fail(e, "pfb_qfold_create allocation");
    free_qfold(h);
    return rc;
  }
  *out = h;
  return PFB_OK;
}

// One step: m <= step device cells and the states' advance behind them, queued on the handle's stream
int qfold_step(pfb_qfold_handle* h, const float* d_cells, uint64_t m) {
  QFoldParams p{};
  p.x = d_cells;
  p.F = h->d_F;
  p.pq = h->d_pq;
  p.prefix = h->d_tables;
  p.tile_prefix = h->d_tables + h->NC + 1;
  p.st = h->d_state;
  p.n = (int)m;
  p.NC = (int)h->NC;
  p.C = (int)h->C;
  p.total_bins = (int)h->total_bins;
  const dim3 grid((unsigned)std::min<uint64_t>((h->total_bins + 255) / 256, kMaxGrid)), block(256);
  const dim3 tiles(h->tile_prefix[h->NC]), wave(64);
  if (runs_tile(h->C, h->tier)) {
    switch (h->C) {
      case 8: hipLaunchKernelGGL(qfold_tile<8>, tiles, wave, 0, h->stream, p); break;
      case 16: hipLaunchKernelGGL(qfold_tile<16>, tiles, wave, 0, h->stream, p); break;
      case 32: hipLaunchKernelGGL(qfold_tile<32>, tiles, wave, 0, h->stream, p); break;
      default: hipLaunchKernelGGL(qfold_tile<64>, tiles, wave, 0, h->stream, p); break;
    }
  } else switch (h->C) {
    case 1: hipLaunchKernelGGL(qfold_direct<1>, grid, block, 0, h->stream, p); break;
    case 2: hipLaunchKernelGGL(qfold_direct<2>, grid, block, 0, h->stream, p); break;
    case 3: hipLaunchKernelGGL(qfold_direct<3>, grid, block, 0, h->stream, p); break;
    case 4: hipLaunchKernelGGL(qfold_direct<4>, grid, block, 0, h->stream, p); break;
    default: hipLaunchKernelGGL(qfold_direct<0>, grid, block, 0, h->stream, p); break;
  }
  HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(qfold_advance, dim3((h->NC + 255) / 256), block, 0, h->stream, h->d_state, h->d_pq, (int)h->NC, (int)m);
  HIP_TRY(hipGetLastError());
  h->last_kernel = qfold_tier(h->C, h->tier);
  h->n += m;
  return PFB_OK;
}

int qfold_enqueue(pfb_qfold_handle* h, const float* d_cells, uint64_t n) {
  for (uint64_t done = 0; done < n;) {
    const uint64_t m = std::min(h->step, n - done);
    const int rc = qfold_step(h, d_cells + done, m);
    if (rc != PFB_OK) return rc;
    done += m;
  }
  return PFB_OK;
}

// what every process call checks before the device is touched
int qfold_check_call(const pfb_qfold_handle* h, const float* cells, uint64_t n, bool device) {
  if (!h || (n > 0 && !cells)) return PFB_ERR_BAD_ARG;
  if (device && (reinterpret_cast<uintptr_t>(cells) % sizeof(float))) return PFB_ERR_BAD_ARG;
  if (n > kMaxIndex || h->n + n > kMaxIndex) return PFB_ERR_BAD_ARG;
  return PFB_OK;
}

// pfb_qfold_process: the steps, and profiles, states and index back where they were when one of them fails
int qfold_sync_call(pfb_qfold_handle* h, const float* cells, uint64_t n, bool host) {
  DeviceGuard g(h->device);
  if (n == 0) {
    HIP_TRY(hipStreamSynchronize(h->stream));
    return PFB_OK;
  }
  const size_t bytes = (size_t)h->total_bins * sizeof(float), sbytes = (size_t)h->NC * sizeof(QState);
  const uint64_t n0 = h->n;
  if (host && h->stage_cells < std::min(n, h->step)) {
    (void)hipFree(h->d_stage);
    h->d_stage = nullptr;
    h->stage_cells = 0;
    HIP_TRY(hipMalloc(reinterpret_cast<void**>(&h->d_stage), (size_t)std::min(n, h->step) * sizeof(float)));
    h->stage_cells = (size_t)std::min(n, h->step);
  }
  QState* keep = h->d_state + 2 * (size_t)h->NC;
  HIP_TRY(hipMemcpyAsync(h->d_backup, h->d_F, bytes, hipMemcpyDeviceToDevice, h->stream));
  HIP_TRY(hipMemcpyAsync(keep, h->d_state, sbytes, hipMemcpyDeviceToDevice, h->stream));
  auto fail = [&](int code) {  // from here on every failure puts the state back before the call returns
    (void)hipStreamSynchronize(h->stream);
    (void)hipMemcpyAsync(h->d_F, h->d_backup, bytes, hipMemcpyDeviceToDevice, h->stream);
    (void)hipMemcpyAsync(h->d_state, keep, sbytes, hipMemcpyDeviceToDevice, h->stream);
    (void)hipStreamSynchronize(h->stream);
    h->n = n0;
    return code;
  };
  int rc = PFB_OK;
  if (!host) {
    rc = qfold_enqueue(h, cells, n);
    if (rc != PFB_OK) return fail(rc);
  } else {
    for (uint64_t done = 0; done < n;) {
      const uint64_t m = std::min(h->step, n - done);
      hipError_t e = hipMemcpyAsync(h->d_stage, cells + done, m * sizeof(float), hipMemcpyHostToDevice, h->stream);
      if (e != hipSuccess) return fail(pfb::hip_fail(e, "pfb_qfold_process staging"));
      rc = qfold_step(h, h->d_stage, m);
      if (rc != PFB_OK) return fail(rc);
      e = hipStreamSynchronize(h->stream);  // the one staging buffer is free again
      if (e != hipSuccess) return fail(pfb::hip_fail(e, "pfb_qfold_process"));
      done += m;
    }
  }
  const hipError_t e = hipStreamSynchronize(h->stream);
  if (e != hipSuccess) return fail(pfb::hip_fail(e, "pfb_qfold_process"));
  return PFB_OK;
}

// ---- regrid ------------------------------------------------------------------------

int regrid_check(const pfb_regrid_config* cfg) {
  if (!cfg || cfg->struct_size != sizeof(pfb_regrid_config)) return PFB_ERR_BAD_ARG;
  const uint64_t Pi = cfg->period_q32 >> 32;
  if (Pi < 1 || cfg->period_q32 > kMaxPeriodQ) return PFB_ERR_BAD_ARG;
  if (cfg->origin > kMaxIndex) return PFB_ERR_BAD_ARG;
  if (cfg->row_samples < 1 || cfg->row_samples > Pi) return PFB_ERR_BAD_ARG;
  if (cfg->elem_bytes != 4 && cfg->elem_bytes != 8) return PFB_ERR_BAD_ARG;
  if (cfg->flags != 0) return PFB_ERR_BAD_ARG;
  return PFB_OK;
}

// the output elements whose source lies before input element X
uint64_t regrid_before(const pfb_regrid_handle* h, uint64_t X) {
  if (X <= h->origin) return 0;
  const uint64_t y = X - h->origin;
  const uint64_t k = (uint64_t)(((u128)(y - 1) << 32) / h->Pq);  // the last row begun
  return k * h->R + std::min<uint64_t>(y - start_of(k, h->Pq), h->R);
}

void free_regrid(pfb_regrid_handle* h) {
  if (!h) return;
  DeviceGuard g(h->device);
  (void)hipFree(h->d_in);
  (void)hipFree(h->d_out);
  if (h->ev_switch) (void)hipEventDestroy(h->ev_switch);
  delete h;
}

constexpr uint64_t kRegridStep = (uint64_t)1 << 24;  // input elements per launch and per staging step

// One step: input [s, s + m) at d_x, its outputs t0 .. t0 + cnt - 1 to d_out; the call's count on the first launch
int regrid_step(pfb_regrid_handle* h, const void* d_x, uint64_t s, uint64_t t0, uint64_t cnt, void* d_out,
                uint64_t* d_count, uint64_t total) {
  if (cnt == 0 && !d_count) return PFB_OK;
  RegridParams p{};
  p.x = d_x;
  p.out = d_out;
  p.count_out = reinterpret_cast<unsigned long long*>(d_count);
  p.total = total;
  const uint64_t k0 = t0 / h->R;
  p.r0 = (uint32_t)(t0 % h->R);
  p.R = h->R;
  p.Pi = (uint32_t)(h->Pq >> 32);
  p.Pf = (uint32_t)h->Pq;
  p.Al = (uint32_t)(uint64_t)((u128)k0 * p.Pf);
  p.base = (long long)(h->origin + start_of(k0, h->Pq)) - (long long)s;
  p.count = (uint32_t)cnt;
  const dim3 grid((unsigned)std::max<uint64_t>(1, std::min<uint64_t>((cnt + 255) / 256, kMaxGrid))), block(256);
  if (h->elem == 8) hipLaunchKernelGGL(regrid_copy<unsigned long long>, grid, block, 0, h->stream, p);
  else hipLaunchKernelGGL(regrid_copy<uint32_t>, grid, block, 0, h->stream, p);
  HIP_TRY(hipGetLastError());
  return PFB_OK;
}

int regrid_enqueue(pfb_regrid_handle* h, const char* d_x, uint64_t n, char* d_out, uint64_t* d_count, uint64_t total) {
  const uint64_t s0 = h->n, t00 = regrid_before(h, s0);
  if (n == 0 && d_count) return regrid_step(h, d_x, s0, t00, 0, d_out, d_count, total);
  for (uint64_t done = 0; done < n;) {
    const uint64_t m = std::min(kRegridStep, n - done);
    const uint64_t t0 = regrid_before(h, s0 + done), t1 = regrid_before(h, s0 + done + m);
    const int rc = regrid_step(h, d_x + done * h->elem, s0 + done, t0, t1 - t0, d_out + (t0 - t00) * h->elem,
                               done == 0 ? d_count : nullptr, total);
    if (rc != PFB_OK) return rc;
    done += m;
  }
  return PFB_OK;
}

int regrid_check_call(const pfb_regrid_handle* h, const void* x, uint64_t n, const void* out, uint64_t* count, bool device) {
  if (!h || !count || (n > 0 && !x)) return PFB_ERR_BAD_ARG;
  if (device && (reinterpret_cast<uintptr_t>(x) % h->elem || reinterpret_cast<uintptr_t>(out) % h->elem)) return PFB_ERR_BAD_ARG;
  if (n > kMaxIndex || h->n + n > kMaxIndex) return PFB_ERR_BAD_ARG;
  return PFB_OK;
}

int regrid_sync_call(pfb_regrid_handle* h, const char* x, uint64_t n, char* out, uint64_t capacity, uint64_t* count_out,
                     bool host) {
  const uint64_t t00 = regrid_before(h, h->n), total = regrid_before(h, h->n + n) - t00;
  *count_out = total;
  if (capacity < total) return PFB_ERR_CAPACITY;
  if (total > 0 && !out) return PFB_ERR_BAD_ARG;
  DeviceGuard g(h->device);
  if (!host) {
    const int rc = regrid_enqueue(h, x, n, out, nullptr, total);
    if (rc != PFB_OK) return rc;
  } else {
    const uint64_t s0 = h->n;
    for (uint64_t done = 0; done < n;) {
      const uint64_t m = std::min(kRegridStep, n - done);
      const uint64_t t0 = regrid_before(h, s0 + done), cnt = regrid_before(h, s0 + done + m) - t0;
      if (cnt > 0) {
        if (h->in_elems < m) {
          (void)hipFree(h->d_in);
          h->d_in = nullptr;
          h->in_elems = 0;
          HIP_TRY(hipMalloc(&h->d_in, (size_t)m * h->elem));
          h->in_elems = (size_t)m;
        }
        if (h->out_elems < cnt) {
          (void)hipFree(h->d_out);
          h->d_out = nullptr;
          h->out_elems = 0;
          HIP_TRY(hipMalloc(&h->d_out, (size_t)cnt * h->elem));
          h->out_elems = (size_t)cnt;
        }
        HIP_TRY(hipMemcpyAsync(h->d_in, x + done * h->elem, (size_t)m * h->elem, hipMemcpyHostToDevice, h->stream));
        const int rc = regrid_step(h, h->d_in, s0 + done, t0, cnt, h->d_out, nullptr, total);
        if (rc != PFB_OK) return rc;
        HIP_TRY(hipMemcpyAsync(out + (t0 - t00) * h->elem, h->d_out, (size_t)cnt * h->elem, hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(hipStreamSynchronize(h->stream));  // the staging buffers are free again
      }
      done += m;
    }
  }
  HIP_TRY(hipStreamSynchronize(h->stream));
  h->n += n;
  return PFB_OK;
}

}  // namespace

extern "C" int pfb_qfold_describe(const pfb_qfold_config* cfg, pfb_qfold_plan* plan_out) {
  return pfb::abi_guard([&]() -> int {
    pfb_qfold_plan plan{};
    const int rc = qfold_check(cfg, plan_out ? &plan : nullptr);
    if (rc == PFB_OK) *plan_out = plan;
    return rc;
  });
}

extern "C" int pfb_qfold_counts(const pfb_qfold_config* cfg, uint32_t candidate, uint64_t first_cell, uint64_t num_cells,
                                uint64_t* counts_out) {
  return pfb::abi_guard([&]() -> int {
    pfb_qfold_plan plan{};
    const int rc = qfold_check(cfg, &plan);
    if (rc != PFB_OK) return rc;
    if (!counts_out || candidate >= cfg->num_periods || first_cell > num_cells || num_cells > kMaxIndex) return PFB_ERR_BAD_ARG;
    const uint64_t Pq = cfg->periods_q32[candidate];
    const uint32_t C = cfg->bin_cells, NB = (uint32_t)(Pq >> 32) / C;
    const QState s1 = state_at(num_cells, Pq), s0 = state_at(first_cell, Pq);
    for (uint32_t j = 0; j < NB; ++j) counts_out[j] = qcount(s1, num_cells, C, NB, j) - qcount(s0, first_cell, C, NB, j);
    return PFB_OK;
  });
}

extern "C" int pfb_qfold_create(const pfb_qfold_config* cfg, pfb_qfold_handle** out) {
  return pfb::abi_guard([&]() -> int {
    if (!out) return PFB_ERR_BAD_ARG;
    *out = nullptr;
    return create_qfold(cfg, out);
  });
}

extern "C" int pfb_qfold_destroy(pfb_qfold_handle* h) {
  return pfb::abi_guard([&]() -> int {
    if (!h) return PFB_ERR_BAD_ARG;
    free_qfold(h);
    return PFB_OK;
  });
}

extern "C" int pfb_qfold_reset(pfb_qfold_handle* h) {
  return pfb::abi_guard([&]() -> int {
    if (!h) return PFB_ERR_BAD_ARG;
    DeviceGuard g(h->device);
    HIP_TRY(seek_qfold(h, 0));
    return PFB_OK;
  });
}

extern "C" int pfb_qfold_set_index(pfb_qfold_handle* h, uint64_t next_cell) {
  return pfb::abi_guard([&]() -> int {
    if (!h || next_cell > kMaxIndex) return PFB_ERR_BAD_ARG;
    DeviceGuard g(h->device);
    HIP_TRY(seek_qfold(h, next_cell));
    return PFB_OK;
  });
}

extern "C" int pfb_qfold_set_stream(pfb_qfold_handle* h, void* hip_stream) {
  return pfb::abi_guard([&]() -> int {
    if (!h) return PFB_ERR_BAD_ARG;
    return pfb::switch_stream(h->device, &h->stream, &h->ev_switch, static_cast<hipStream_t>(hip_stream));
  });
}

extern "C" int pfb_qfold_sync(pfb_qfold_handle* h) {
  return pfb::abi_guard([&]() -> int {
    if (!h) return PFB_ERR_BAD_ARG;
    DeviceGuard g(h->device);
    HIP_TRY(hipStreamSynchronize(h->stream));
    return PFB_OK;
  });
}

extern "C" int pfb_qfold_get_device(const pfb_qfold_handle* h, int* device_id) {
  return pfb::abi_guard([&]() -> int {
    if (!h || !device_id) return PFB_ERR_BAD_ARG;
    *device_id = h->device;
    return PFB_OK;
  });
}

extern "C" int pfb_qfold_next_index(const pfb_qfold_handle* h, uint64_t* index_out) {
  return pfb::abi_guard([&]() -> int {
    if (!h || !index_out) return PFB_ERR_BAD_ARG;
    *index_out = h->n;
    return PFB_OK;
  });
}

extern "C" int pfb_qfold_set_tier(pfb_qfold_handle* h, int tier, uint64_t step_cells) {
  return pfb::abi_guard([&]() -> int {
    if (!h || tier < kTierAuto || tier > kTierTile || step_cells > kStepCells) return PFB_ERR_BAD_ARG;
    if (tier == kTierTile && !tile_able(h->C)) return PFB_ERR_UNSUPPORTED;
    h->tier = tier;
    h->step = step_cells ? step_cells : kStepCells;
    return PFB_OK;
  });
}

extern "C" int pfb_qfold_process(pfb_qfold_handle* h, const float* cells, uint64_t num_cells, uint32_t mem) {
  return pfb::abi_guard([&]() -> int {
    if (mem > PFB_MEM_DEVICE) return PFB_ERR_BAD_ARG;
    const int rc = qfold_check_call(h, cells, num_cells, mem == PFB_MEM_DEVICE);
    if (rc != PFB_OK) return rc;
    return qfold_sync_call(h, cells, num_cells, mem == PFB_MEM_HOST);
  });
}

extern "C" int pfb_qfold_process_async(pfb_qfold_handle* h, const float* d_cells, uint64_t num_cells) {
  return pfb::abi_guard([&]() -> int {
    const int rc = qfold_check_call(h, d_cells, num_cells, true);
    if (rc != PFB_OK) return rc;
    DeviceGuard g(h->device);
    return qfold_enqueue(h, d_cells, num_cells);
  });
}

extern "C" int pfb_qfold_scores(pfb_qfold_handle* h, pfb_qfold_score* out, uint64_t capacity, uint32_t mem) {
  return pfb::abi_guard([&]() -> int {
    if (mem > PFB_MEM_DEVICE || !h || !out) return PFB_ERR_BAD_ARG;
    if (mem == PFB_MEM_DEVICE && reinterpret_cast<uintptr_t>(out) % 8) return PFB_ERR_BAD_ARG;
    if (capacity < h->NC) return PFB_ERR_CAPACITY;
    DeviceGuard g(h->device);
    QScoreParams p{};
    p.F = h->d_F;
    p.pq = h->d_pq;
    p.prefix = h->d_tables;
    p.st = h->d_state;
    p.st0 = h->d_state + h->NC;
    p.out = mem == PFB_MEM_DEVICE ? out : h->d_scores;
    p.N = h->n;
    p.N0 = h->n0;
    p.C = (int)h->C;
    hipLaunchKernelGGL(qfold_score, dim3(h->NC), dim3(256), 0, h->stream, p);
    HIP_TRY(hipGetLastError());
    if (mem == PFB_MEM_HOST)
      HIP_TRY(hipMemcpyAsync(out, h->d_scores, (size_t)h->NC * sizeof(pfb_qfold_score), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    return PFB_OK;
  });
}

extern "C" int pfb_qfold_profile(pfb_qfold_handle* h, uint32_t candidate, float* out, uint64_t capacity_bins, uint32_t mem) {
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

extern "C" const char* pfb_qfold_last_kernel(const pfb_qfold_handle* h) { return h ? h->last_kernel : ""; }

extern "C" int pfb_regrid_create(const pfb_regrid_config* cfg, pfb_regrid_handle** out) {
  return pfb::abi_guard([&]() -> int {
    if (!out) return PFB_ERR_BAD_ARG;
    *out = nullptr;
    int rc = regrid_check(cfg);
    if (rc != PFB_OK) return rc;
    int dev = 0;
    rc = pfb::resolve_device(cfg->device_id, &dev);
    if (rc != PFB_OK) return rc;
    pfb_regrid_handle* h = new pfb_regrid_handle();
    h->device = dev;
    h->Pq = cfg->period_q32;
    h->origin = cfg->origin;
    h->R = cfg->row_samples;
    h->elem = cfg->elem_bytes;
    *out = h;
    return PFB_OK;
  });
}

extern "C" int pfb_regrid_destroy(pfb_regrid_handle* h) {
  return pfb::abi_guard([&]() -> int {
    if (!h) return PFB_ERR_BAD_ARG;
    free_regrid(h);
    return PFB_OK;
  });
}

extern "C" int pfb_regrid_reset(pfb_regrid_handle* h) {
  return pfb::abi_guard([&]() -> int {
    if (!h) return PFB_ERR_BAD_ARG;
    h->n = 0;
    return PFB_OK;
  });
}

extern "C" int pfb_regrid_set_index(pfb_regrid_handle* h, uint64_t next_input) {
  return pfb::abi_guard([&]() -> int {
    if (!h || next_input > kMaxIndex) return PFB_ERR_BAD_ARG;
    h->n = next_input;
    return PFB_OK;
  });
}

extern "C" int pfb_regrid_set_stream(pfb_regrid_handle* h, void* hip_stream) {
  return pfb::abi_guard([&]() -> int {
    if (!h) return PFB_ERR_BAD_ARG;
    return pfb::switch_stream(h->device, &h->stream, &h->ev_switch, static_cast<hipStream_t>(hip_stream));
  });
}

extern "C" int pfb_regrid_sync(pfb_regrid_handle* h) {
  return pfb::abi_guard([&]() -> int {
    if (!h) return PFB_ERR_BAD_ARG;
    DeviceGuard g(h->device);
    HIP_TRY(hipStreamSynchronize(h->stream));
    return PFB_OK;
  });
}

extern "C" int pfb_regrid_get_device(const pfb_regrid_handle* h, int* device_id) {
  return pfb::abi_guard([&]() -> int {
    if (!h || !device_id) return PFB_ERR_BAD_ARG;
    *device_id = h->device;
    return PFB_OK;
  });
}

extern "C" int pfb_regrid_next_index(const pfb_regrid_handle* h, uint64_t* index_out) {
  return pfb::abi_guard([&]() -> int {
    if (!h || !index_out) return PFB_ERR_BAD_ARG;
    *index_out = h->n;
    return PFB_OK;
  });
}

extern "C" int pfb_regrid_outputs_for(const pfb_regrid_handle* h, uint64_t num_inputs, uint64_t* outputs_out) {
  return pfb::abi_guard([&]() -> int {
    if (!h || !outputs_out || num_inputs > kMaxIndex || h->n + num_inputs > kMaxIndex) return PFB_ERR_BAD_ARG;
    *outputs_out = regrid_before(h, h->n + num_inputs) - regrid_before(h, h->n);
    return PFB_OK;
  });
}

extern "C" int pfb_regrid_process(pfb_regrid_handle* h, const void* x, uint64_t num_inputs, void* out,
                                  uint64_t capacity_outputs, uint64_t* outputs_out, uint32_t mem) {
  return pfb::abi_guard([&]() -> int {
    if (mem > PFB_MEM_DEVICE) return PFB_ERR_BAD_ARG;
    const int rc = regrid_check_call(h, x, num_inputs, out, outputs_out, mem == PFB_MEM_DEVICE);
    if (rc != PFB_OK) return rc;
    return regrid_sync_call(h, static_cast<const char*>(x), num_inputs, static_cast<char*>(out), capacity_outputs,
                            outputs_out, mem == PFB_MEM_HOST);
  });
}

extern "C" int pfb_regrid_process_async(pfb_regrid_handle* h, const void* d_x, uint64_t num_inputs, void* d_out,
                                        uint64_t capacity_outputs, uint64_t* d_outputs_out) {
  return pfb::abi_guard([&]() -> int {
    const int rc = regrid_check_call(h, d_x, num_inputs, d_out, d_outputs_out, true);
    if (rc != PFB_OK) return rc;
    if (reinterpret_cast<uintptr_t>(d_outputs_out) % 8) return PFB_ERR_BAD_ARG;
    const uint64_t total = regrid_before(h, h->n + num_inputs) - regrid_before(h, h->n);
    if (capacity_outputs < total) return PFB_ERR_CAPACITY;
    if (total > 0 && !d_out) return PFB_ERR_BAD_ARG;
    DeviceGuard g(h->device);
    const int rc2 = regrid_enqueue(h, static_cast<const char*>(d_x), num_inputs, static_cast<char*>(d_out), d_outputs_out, total);
    if (rc2 != PFB_OK) return rc2;
    h->n += num_inputs;
    return PFB_OK;
  });
}

extern "C" int pfb_regrid_doppler_frequencies(uint64_t period_q32, uint32_t doppler_length, int centered, double fs,
                                              double* out) {
  return pfb::abi_guard([&]() -> int {
    if (!out || (period_q32 >> 32) < 1 || period_q32 > kMaxPeriodQ) return PFB_ERR_BAD_ARG;
    if (doppler_length < 1 || doppler_length > 65536 || !std::isfinite(fs)) return PFB_ERR_BAD_ARG;
    const double period = (double)period_q32 / 4294967296.0;
    const int ND = (int)doppler_length;
    for (int i = 0; i < ND; ++i) {
      const int d = centered ? i - ND / 2 : i;
      out[i] = (double)d * fs / ((double)ND * period);
    }
    return PFB_OK;
  });
}
