// pfb_oscfar.hip -- an ordered-statistic CFAR detector over range-Doppler maps (pfb_oscfar_* in
// include/pfb_channelizer.h, where the arithmetic is defined): per-cell rank counts, the select of an over cell's
// noise, the peak box, and the checks of a config.  Geometry, records, stats and the call semantics are pfb_rdcfar_*'s:
// the steps, the passes behind the cells kernel and the handle's state are pfb_rdmap.hpp's, shared with pfb_rdcfar.hip.
//   oscfar_cells<LDS>   one workgroup per (map, band of tile_rows rows, tile of 256 gates), a lane per gate: stages the
//                       float32 block with its halo of max(Wd, Pd) rows (wrapped) and Gr+Tr gates (clipped) in LDS,
//                       consecutive lanes loading consecutive gates.  Every lane then DECIDES its cell by counting the
//                       training values with alpha * x < p: over iff the count reaches k' (the header proves that
//                       equal to p > alpha * x_(k')).  The wave walks the training cells in chunks of 8 gates and
//                       leaves as soon as every lane's count has reached k' or can no longer reach it -- the order of
//                       the visit is free, and a noise cell under a high rank is settled after about n - k' values.
//                       Only an over cell SELECTS its noise: a bitwise search, most significant bit first, on an
//                       order-preserving 32-bit key (NaN last, -0 = +0), 32 counting passes, the 64 lanes of the wave
//                       each counting a share of that cell's training values; then its lane walks its peak box.  A
//                       ballot per wave gives one 64-gate word of detections and one over count: one writer each.
//                       The noise of a detection is kept in a side array at the cell's place.
//                       LDS = false, when not even one row's block with its halo fits the LDS budget (Gr + Tr in the
//                       hundreds with Wd or Pd > 0): the same code reads P from the maps through the caches.
// Cost: a cell reads at most n float32 of LDS (a wave as many as its slowest lane); an over cell costs its wave
// 32 ceil(n / 64) more per lane and its own lane the peak box: slow only for maps that are all detections.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>

#include "pfb_rdmap.hpp"

namespace {

constexpr uint32_t kMaxTraining = 4096;  // N at most
constexpr int kMaxBand = 16;             // rows of a band at most
constexpr int kChunk = 8;                // gates a lane counts between two looks at the rest of its wave

struct OsParams : MapParams {
  int rank, N;
  int band_rows, halo_rows, width;
  float alpha, min_power;
};
static_assert(sizeof(OsParams) == 176, "the kernels' parameter layout");

// The order of float32 `<` as unsigned integers: a NaN after every number, -0 and +0 the same key.
__device__ __forceinline__ uint32_t key_of(float x) {
  if (x != x) return 0xffffffffu;
  if (x == 0.f) return 0x80000000u;
  const uint32_t u = __float_as_uint(x);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

__device__ __forceinline__ float value_of(uint32_t key) {  // of a number's key; a zero comes back as +0.0
  return __uint_as_float((key & 0x80000000u) ? (key & 0x7fffffffu) : ~key);
}

template <bool LDS>
__global__ void __launch_bounds__(kTileGates) oscfar_cells(const OsParams p) {
  extern __shared__ float Ps[];  // [band_rows + 2 halo_rows][width]
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int W = p.width, H = p.halo_rows, GT = p.Gr + p.Tr;
  const long long units = (long long)p.num_maps * p.NB * p.NT;
  for (long long u = blockIdx.x; u < units; u += gridDim.x) {
    const int t = (int)(u % p.NT);
    const int b = (int)((u / p.NT) % p.NB);
    const int m = (int)(u / ((long long)p.NT * p.NB));
    const int d0 = b * p.band_rows, nb = min(p.band_rows, p.ND - d0);
    const int g0 = t * kTileGates, e0 = g0 - GT;  // the block's first gate, its halo's
    const float* map = p.maps + (size_t)m * p.ND * p.pitch;
    // P(i, x): row d0 - H + i (wrapped), gate e0 + x; only gates 0 .. R-1 are ever asked for
    auto P = [&](int i, int x) -> float {
      if constexpr (LDS) return Ps[i * W + x];
      else return map[(size_t)wrap((d0 - H + i) % p.ND, p.ND) * p.pitch + (e0 + x)];
    };
    if constexpr (LDS) {
      for (int i = 0; i < nb + 2 * H; ++i) {
        const float* row = map + (size_t)wrap((d0 - H + i) % p.ND, p.ND) * p.pitch;
        for (int x = tid; x < W; x += kTileGates) {
          const int g = e0 + x;
          Ps[i * W + x] = g >= 0 && g < p.R ? row[g] : 0.f;
        }
      }
      __syncthreads();
    }
    const int r = g0 + tid;
    const int x0 = tid + GT;
    // the cell's training gates as block columns: lead [xl0, xl1), lag [xr0, xr1); the same for every row of the band
    const int xl0 = max(r - GT, 0) - e0, xl1 = r - p.Gr - e0;
    const int xr0 = r + p.Gr + 1 - e0, xr1 = min(r + GT + 1, p.R) - e0;
    const int gates = r < p.R ? max(xl1 - xl0, 0) + max(xr1 - xr0, 0) : 0;
    const int n = gates * (2 * p.Wd + 1);
    const int kk = (p.rank * n + p.N - 1) / p.N;  // k'; 0 only with n = 0
    for (int k = 0; k < nb; ++k) {
      const int d = d0 + k;
      bool over = false, det = false;
      float noise = 0.f;
      const float pw = n > 0 ? P(k + H, x0) : 0.f;
      // The count of training values with alpha * x < p, walked by the whole wave in chunks of kChunk gates: a lane is
      // decided once its count has reached k' or can no longer reach it, and the wave leaves when every lane is.
      int below = 0, left = n;
      bool open = n > 0 && pw > p.min_power;
      for (int seg = 0, segs = 2 * (2 * p.Wd + 1); seg < segs && __any(open); ++seg) {
        const int i = k + H - p.Wd + (seg >> 1);
        const int xs = (seg & 1) ? xr0 : xl0, xe = (seg & 1) ? xr1 : xl1;  // this lane's columns of the segment
        for (int c0 = 0; c0 < p.Tr && __any(open); c0 += kChunk) {
          if (open) {
            const int a = xs + c0, e = min(a + kChunk, xe);
            for (int x = a; x < e; ++x) below += (p.alpha * P(i, x) < pw) ? 1 : 0;
            left -= max(e - a, 0);
            open = below < kk && below + left >= kk;
          }
        }
      }
      over = n > 0 && below >= kk && pw > p.min_power;
      // The select, rare: the wave takes its over cells one after another and finds each one's k'-th smallest key bit by
      // bit, every lane counting its share of that cell's training values (one lane alone would wait out n LDS
      // latencies 32 times over).
      for (unsigned long long pending = __ballot(over); pending; pending &= pending - 1) {
        const int owner = __ffsll((long long)pending) - 1;
        const int sl0 = __shfl(xl0, owner, 64), sl1 = __shfl(xl1, owner, 64);
        const int sr0 = __shfl(xr0, owner, 64), sr1 = __shfl(xr1, owner, 64);
        const int skk = __shfl(kk, owner, 64);
        const int nl = max(sl1 - sl0, 0), ng = nl + max(sr1 - sr0, 0);
        uint32_t key = 0;
        for (int bit = 31; bit >= 0; --bit) {
          const uint32_t probe = key | ((1u << bit) - 1u);  // the largest key with this bit clear
          int le = 0;
          for (int j = -p.Wd; j <= p.Wd; ++j)
            for (int q = lane; q < ng; q += 64)
              le += key_of(P(k + H + j, q < nl ? sl0 + q : sr0 + (q - nl))) <= probe ? 1 : 0;
          for (int o = 32; o; o >>= 1) le += __shfl_xor(le, o, 64);
          if (le < skk) key |= 1u << bit;
        }
        if (lane == owner) noise = value_of(key);  // a number: a NaN in the k'-th place is never over
      }
      if (over) {  // the peak box: rare, one lane walks it
        det = true;
        const int b0 = max(r - p.Gr, 0), b1 = min(r + p.Gr, p.R - 1);
        for (int j = -p.Pd; j <= p.Pd && det; ++j) {
          const int qrow = wrap(d + j, p.ND);
          for (int g = b0; g <= b1; ++g) {
            const float q = P(k + H + j, g - e0);
            if (q > pw || (q == pw && (qrow < d || (qrow == d && g < r)))) {
              det = false;
              break;
            }
          }
        }
      }
      const unsigned long long dets = __ballot(det), overs = __ballot(over);
      const int w = t * (kTileGates / 64) + wv;
      if (lane == 0 && w < p.NWR) {
        const size_t at = ((size_t)m * p.ND + d) * p.NWR + w;
        p.words[at] = dets;
        p.over[at] = (uint32_t)__popcll(overs);
      }
      if (det) p.noise[((size_t)m * p.ND + d) * p.R + r] = noise;
    }
    if constexpr (LDS) __syncthreads();  // the block is read no more: the next unit may overwrite it
  }
}

// ---------------------------------------------------------------------------------
// host: checks and plan

// The band of rows a workgroup takes: the tallest of 16, 8, 4, 2, 1 (no taller than the map needs) whose block with its
// halo fits the LDS budget; when not even one row's does, P stays in memory and no LDS is used.
Tiling tiling_for(const pfb_oscfar_config& c) {
  Tiling t{};
  t.halo_rows = (int)std::max(c.doppler_half_width, c.peak_half_width);
  t.width = kTileGates + 2 * (int)(c.guard_gates + c.train_gates);
  int top = kMaxBand;
  while (top > 1 && top / 2 >= (int)c.rows) top /= 2;
  for (int rows = top; rows >= 1; rows /= 2) {
    const uint64_t bytes = (uint64_t)(rows + 2 * t.halo_rows) * t.width * 4;
    if (bytes <= kLdsBudget) {
      t.band_rows = rows;
      t.lds = true;
      t.lds_bytes = (uint32_t)bytes;
      return t;
    }
  }
  t.band_rows = top;  // the direct tier: a band costs nothing, so the tallest
  t.lds = false;
  t.lds_bytes = 0;
  return t;
}

const char* kernel_name(bool lds) { return lds ? "pfb_oscfar_cells<lds>" : "pfb_oscfar_cells<direct>"; }

// Everything pfb_oscfar_describe and pfb_oscfar_create check before the device, in the order the header states
int oscfar_check(const pfb_oscfar_config* cfg, pfb_oscfar_plan* plan) {
  if (!cfg || !plan || cfg->struct_size != sizeof(pfb_oscfar_config)) return PFB_ERR_BAD_ARG;
  if (cfg->rows < 1 || cfg->rows > 1024) return PFB_ERR_BAD_ARG;
  if (cfg->gates < 1 || cfg->gates > (1u << 20)) return PFB_ERR_BAD_ARG;
  if (cfg->pitch != 0 && cfg->pitch < cfg->gates) return PFB_ERR_BAD_ARG;
  if ((uint64_t)cfg->rows * (cfg->pitch ? cfg->pitch : cfg->gates) > ((uint64_t)1 << 26)) return PFB_ERR_BAD_ARG;
  if (cfg->doppler_half_width > 16 || 2 * cfg->doppler_half_width + 1 > cfg->rows) return PFB_ERR_BAD_ARG;
  if (cfg->guard_gates > 1024) return PFB_ERR_BAD_ARG;
  if (cfg->train_gates < 1 || cfg->train_gates > 256) return PFB_ERR_BAD_ARG;
  if (cfg->peak_half_width > 16 || 2 * cfg->peak_half_width + 1 > cfg->rows) return PFB_ERR_BAD_ARG;
  const uint32_t N = 2 * cfg->train_gates * (2 * cfg->doppler_half_width + 1);
  if (N > kMaxTraining) return PFB_ERR_BAD_ARG;
  if (cfg->rank < 1 || cfg->rank > N) return PFB_ERR_BAD_ARG;
  if (!std::isfinite(cfg->alpha) || !(cfg->alpha > 0.f)) return PFB_ERR_BAD_ARG;
  if (!(cfg->min_power >= 0.f)) return PFB_ERR_BAD_ARG;  // NaN included
  if (cfg->flags != 0) return PFB_ERR_BAD_ARG;
  const Tiling t = tiling_for(*cfg);
  plan->training_cells = N;
  plan->tile_rows = (uint32_t)t.band_rows;
  plan->tile_gates = kTileGates;
  plan->lds_bytes = t.lds_bytes;
  plan->reserved = 0;
  std::memset(plan->kernel, 0, sizeof(plan->kernel));
  std::snprintf(plan->kernel, sizeof(plan->kernel), "%s", kernel_name(t.lds));
  return PFB_OK;
}

// log of the false-alarm probability of rank k of N exponential cells at factor a: -sum log1p(a / (N - i))
double log_pfa(double a, uint64_t N, uint64_t k) {
  double s = 0.0;
  for (uint64_t i = 0; i < k; ++i) s -= std::log1p(a / (double)(N - i));
  return s;
}

}  // namespace

struct pfb_oscfar_handle : MapDetector {
  using Params = OsParams;
  pfb_oscfar_config cfg{};
  // this unit's part of a step (pfb_rdmap.hpp): its own parameters and its cells kernel
  const char* cells(OsParams& p, unsigned units) const {
    p.rank = (int)cfg.rank;
    p.N = (int)(2 * cfg.train_gates * (2 * cfg.doppler_half_width + 1));
    if (tile.lds) hipLaunchKernelGGL(oscfar_cells<true>, dim3(units), dim3(kTileGates), tile.lds_bytes, stream, p);
    else hipLaunchKernelGGL(oscfar_cells<false>, dim3(units), dim3(kTileGates), 0, stream, p);
    return kernel_name(tile.lds);
  }
};

extern "C" int pfb_oscfar_describe(const pfb_oscfar_config* cfg, pfb_oscfar_plan* plan_out) {
  return pfb::abi_guard([&]() -> int {
    pfb_oscfar_plan plan{};
    const int rc = oscfar_check(cfg, plan_out ? &plan : nullptr);
    if (rc == PFB_OK) *plan_out = plan;
    return rc;
  });
}

extern "C" int pfb_oscfar_alpha(double pfa, uint64_t training_cells, uint64_t rank, double* alpha_out) {
  return pfb::abi_guard([&]() -> int {
    if (!alpha_out || !(pfa > 0.0 && pfa < 1.0)) return PFB_ERR_BAD_ARG;
    if (training_cells < 1 || training_cells > ((uint64_t)1 << 20)) return PFB_ERR_BAD_ARG;
    if (rank < 1 || rank > training_cells) return PFB_ERR_BAD_ARG;
    const double want = std::log(pfa);
    double lo = 0.0, hi = 1.0;  // log_pfa falls from 0 without bound: double hi until it is below
    while (log_pfa(hi, training_cells, rank) > want) hi *= 2.0;
    for (int it = 0; it < 200; ++it) {
      const double mid = 0.5 * (lo + hi);
      if (mid <= lo || mid >= hi) break;
      if (log_pfa(mid, training_cells, rank) > want) lo = mid;
      else hi = mid;
    }
    *alpha_out = 0.5 * (lo + hi);
    return PFB_OK;
  });
}

extern "C" int pfb_oscfar_create(const pfb_oscfar_config* cfg, pfb_oscfar_handle** out) {
  return pfb::abi_guard([&]() -> int {
    if (!out) return PFB_ERR_BAD_ARG;
    *out = nullptr;
    pfb_oscfar_plan plan{};
    const int rc = oscfar_check(cfg, &plan);
    return rc != PFB_OK ? rc : create_detector(*cfg, tiling_for(*cfg), "pfb_oscfar_create", out);
  });
}

extern "C" int pfb_oscfar_destroy(pfb_oscfar_handle* h) {
  return pfb::abi_guard([&]() -> int {
    if (!h) return PFB_ERR_BAD_ARG;
    delete h;
    return PFB_OK;
  });
}

extern "C" int pfb_oscfar_reset(pfb_oscfar_handle* h) {
  return pfb::abi_guard([&]() -> int { return reset_detector(h); });
}

extern "C" int pfb_oscfar_set_stream(pfb_oscfar_handle* h, void* hip_stream) {
  return pfb::abi_guard([&]() -> int { return set_detector_stream(h, hip_stream); });
}

extern "C" int pfb_oscfar_sync(pfb_oscfar_handle* h) {
  return pfb::abi_guard([&]() -> int { return sync_detector(h); });
}

extern "C" int pfb_oscfar_get_device(const pfb_oscfar_handle* h, int* device_id) {
  return pfb::abi_guard([&]() -> int { return detector_device(h, device_id); });
}

extern "C" int pfb_oscfar_next_map(const pfb_oscfar_handle* h, uint64_t* map_out) {
  return pfb::abi_guard([&]() -> int { return detector_next_map(h, map_out); });
}

extern "C" int pfb_oscfar_get_stats(pfb_oscfar_handle* h, pfb_rdcfar_stats* stats_out) {
  return pfb::abi_guard([&]() -> int { return detector_stats(h, stats_out); });
}

extern "C" int pfb_oscfar_process(pfb_oscfar_handle* h, const float* maps, uint64_t num_maps, pfb_rdcfar_det* det_out,
                                  uint64_t capacity, uint64_t* count_out, uint32_t mem) {
  return pfb::abi_guard([&]() -> int {
    return sync_call(h, maps, num_maps, det_out, capacity, count_out, mem, "pfb_oscfar_process");
  });
}

extern "C" int pfb_oscfar_process_async(pfb_oscfar_handle* h, const float* d_maps, uint64_t num_maps,
                                        pfb_rdcfar_det* d_det_out, uint64_t capacity, uint64_t* d_count_out) {
  return pfb::abi_guard([&]() -> int { return async_call(h, d_maps, num_maps, d_det_out, capacity, d_count_out); });
}

extern "C" const char* pfb_oscfar_last_kernel(const pfb_oscfar_handle* h) { return h ? h->last_kernel : ""; }
