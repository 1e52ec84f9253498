// pfb_rdcfar.hip -- a 2-D CFAR detector over range-Doppler maps (pfb_rdcfar_* in include/pfb_channelizer.h, where the
// arithmetic is defined): column sums, per-cell training walks, the peak box, and the checks of a config.  The steps,
// the passes that turn the cells kernel's words into ordered records, the handle's state and the call semantics are
// pfb_rdmap.hpp's, shared with pfb_oscfar.hip.  The maps are read where they lie.
//   rdcfar_cells<LDS>   one workgroup per (map, band of tile_rows rows, tile of 256 gates), a lane per gate:
//                       stages the float32 block with its halo of max(Wd, Pd) rows (wrapped) and Gr+Tr gates
//                       (clipped) in LDS, consecutive lanes loading consecutive gates; computes A once per (row, gate)
//                       of the block into LDS (float64, j ascending); then every lane walks its cell's lead and lag
//                       sums over A in ascending gate, decides, and, only when over, walks its peak box.  A ballot per
//                       wave gives one 64-gate word of detections and one over count: one writer each.  The noise of
//                       a detection is kept in a side array at the cell's place (nothing else is written there).
//                       LDS = false, when the block with its halo exceeds the LDS budget (Gr + Tr in the hundreds
//                       with Wd or Pd > 0): the same code reads P from the maps instead; A still goes through LDS.
// Cost: a cell reads 2 Tr float64 of LDS; an over cell's peak box, (2 Pd + 1)(2 Gr + 1) cells, is walked by its one
// lane: correct, and slow only for maps that are all detections.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>

#include "pfb_rdmap.hpp"

namespace {

struct RdParams : MapParams {
  int method;
  int band_rows, halo_rows, width;
  float alpha, min_power;
};
static_assert(sizeof(RdParams) == 168, "the kernels' parameter layout");

template <bool LDS>
__global__ void __launch_bounds__(kTileGates) rdcfar_cells(const RdParams p) {
  extern __shared__ double smem[];
  double* As = smem;                                                             // [band_rows][width]
  float* Ps = reinterpret_cast<float*>(smem + (size_t)p.band_rows * p.width);   // [band_rows + 2 halo_rows][width]
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int W = p.width, H = p.halo_rows, GT = p.Gr + p.Tr;
  const double col = (double)(2 * p.Wd + 1);
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
    for (int k = 0; k < nb; ++k) {
      for (int x = tid; x < W; x += kTileGates) {
        const int g = e0 + x;
        double a = 0.0;
        if (g >= 0 && g < p.R)
          for (int j = -p.Wd; j <= p.Wd; ++j) a += (double)P(k + H + j, x);
        As[k * W + x] = a;
      }
    }
    __syncthreads();
    const int r = g0 + tid;
    const int x0 = tid + GT;
    for (int k = 0; k < nb; ++k) {
      const int d = d0 + k;
      bool over = false, det = false;
      float noise = 0.f;
      if (r < p.R) {
        const int l0 = max(r - GT, 0), l1 = r - p.Gr;            // lead: [l0, l1)
        const int r0 = r + p.Gr + 1, r1 = min(r + GT + 1, p.R);  // lag:  [r0, r1)
        const int nl = max(l1 - l0, 0), nr = max(r1 - r0, 0);
        const double* A = As + k * W - e0;                       // A[g]
        double sum_l = 0.0, sum_r = 0.0;
        for (int g = l0; g < l1; ++g) sum_l += A[g];
        for (int g = r0; g < r1; ++g) sum_r += A[g];
        double mean = std::numeric_limits<double>::quiet_NaN();  // no noise: no comparison with it holds
        if (p.method == PFB_CFAR_CA) {
          if (nl + nr > 0) mean = (sum_l + sum_r) / ((double)(nl + nr) * col);
        } else if (nl > 0 && nr > 0) {
          const double a = sum_l / ((double)nl * col), c = sum_r / ((double)nr * col);
          if (a == a && c == c) mean = p.method == PFB_CFAR_GO ? (a > c ? a : c) : (a < c ? a : c);
        } else if (nl > 0) {
          mean = sum_l / ((double)nl * col);
        } else if (nr > 0) {
          mean = sum_r / ((double)nr * col);
        }
        noise = (float)mean;
        const float pw = P(k + H, x0);
        const float thr = p.alpha * noise;
        over = (pw > thr) && (pw > p.min_power);
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
    __syncthreads();  // the block is read no more: the next unit may overwrite it
  }
}

// ---------------------------------------------------------------------------------
// host: checks and plan

// The band of rows a workgroup takes: the tallest of 8, 4, 2, 1 (no taller than the map needs) whose block, halo and
// column sums fit the LDS budget; when not even one row's does, P stays in memory and only the column sums use LDS.
Tiling tiling_for(const pfb_rdcfar_config& c) {
  Tiling t{};
  t.halo_rows = (int)std::max(c.doppler_half_width, c.peak_half_width);
  t.width = kTileGates + 2 * (int)(c.guard_gates + c.train_gates);
  int top = 8;
  while (top > 1 && top / 2 >= (int)c.rows) top /= 2;
  for (int lds = 1; lds >= 0; --lds)
    for (int rows = top; rows >= 1; rows /= 2) {
      const uint64_t bytes = (uint64_t)rows * t.width * 8 + (lds ? (uint64_t)(rows + 2 * t.halo_rows) * t.width * 4 : 0);
      if (bytes <= kLdsBudget) {
        t.band_rows = rows;
        t.lds = lds != 0;
        t.lds_bytes = (uint32_t)bytes;
        return t;
      }
    }
  return t;  // not reached: one row of column sums is at most 2816 * 8 bytes
}

const char* kernel_name(bool lds) { return lds ? "pfb_rdcfar_cells<lds>" : "pfb_rdcfar_cells<direct>"; }

// Everything pfb_rdcfar_describe and pfb_rdcfar_create check before the device, in the order the header states
int rdcfar_check(const pfb_rdcfar_config* cfg, pfb_rdcfar_plan* plan) {
  if (!cfg || !plan || cfg->struct_size != sizeof(pfb_rdcfar_config)) return PFB_ERR_BAD_ARG;
  if (cfg->rows < 1 || cfg->rows > 1024) return PFB_ERR_BAD_ARG;
  if (cfg->gates < 1 || cfg->gates > (1u << 20)) return PFB_ERR_BAD_ARG;
  if (cfg->pitch != 0 && cfg->pitch < cfg->gates) return PFB_ERR_BAD_ARG;
  if ((uint64_t)cfg->rows * (cfg->pitch ? cfg->pitch : cfg->gates) > ((uint64_t)1 << 26)) return PFB_ERR_BAD_ARG;
  if (cfg->doppler_half_width > 16 || 2 * cfg->doppler_half_width + 1 > cfg->rows) return PFB_ERR_BAD_ARG;
  if (cfg->guard_gates > 1024) return PFB_ERR_BAD_ARG;
  if (cfg->train_gates < 1 || cfg->train_gates > 256) return PFB_ERR_BAD_ARG;
  if (cfg->peak_half_width > 16 || 2 * cfg->peak_half_width + 1 > cfg->rows) return PFB_ERR_BAD_ARG;
  if (cfg->method > PFB_CFAR_SO) return PFB_ERR_BAD_ARG;
  if (!std::isfinite(cfg->alpha) || !(cfg->alpha > 0.f)) return PFB_ERR_BAD_ARG;
  if (!(cfg->min_power >= 0.f)) return PFB_ERR_BAD_ARG;  // NaN included
  if (cfg->flags != 0) return PFB_ERR_BAD_ARG;
  const Tiling t = tiling_for(*cfg);
  plan->training_cells = 2ull * cfg->train_gates * (2 * cfg->doppler_half_width + 1);
  plan->tile_rows = (uint32_t)t.band_rows;
  plan->tile_gates = kTileGates;
  plan->lds_bytes = t.lds_bytes;
  plan->reserved = 0;
  std::memset(plan->kernel, 0, sizeof(plan->kernel));
  std::snprintf(plan->kernel, sizeof(plan->kernel), "%s", kernel_name(t.lds));
  return PFB_OK;
}

}  // namespace

struct pfb_rdcfar_handle : MapDetector {
  using Params = RdParams;
  pfb_rdcfar_config cfg{};
  // this unit's part of a step (pfb_rdmap.hpp): its own parameter and its cells kernel
  const char* cells(RdParams& p, unsigned units) const {
    p.method = (int)cfg.method;
    if (tile.lds) hipLaunchKernelGGL(rdcfar_cells<true>, dim3(units), dim3(kTileGates), tile.lds_bytes, stream, p);
    else hipLaunchKernelGGL(rdcfar_cells<false>, dim3(units), dim3(kTileGates), tile.lds_bytes, stream, p);
    return kernel_name(tile.lds);
  }
};

extern "C" int pfb_rdcfar_describe(const pfb_rdcfar_config* cfg, pfb_rdcfar_plan* plan_out) {
  return pfb::abi_guard([&]() -> int {
    pfb_rdcfar_plan plan{};
    const int rc = rdcfar_check(cfg, plan_out ? &plan : nullptr);
    if (rc == PFB_OK) *plan_out = plan;
    return rc;
  });
}

extern "C" int pfb_rdcfar_create(const pfb_rdcfar_config* cfg, pfb_rdcfar_handle** out) {
  return pfb::abi_guard([&]() -> int {
    if (!out) return PFB_ERR_BAD_ARG;
    *out = nullptr;
    pfb_rdcfar_plan plan{};
    const int rc = rdcfar_check(cfg, &plan);
    return rc != PFB_OK ? rc : create_detector(*cfg, tiling_for(*cfg), "pfb_rdcfar_create", out);
  });
}

extern "C" int pfb_rdcfar_destroy(pfb_rdcfar_handle* h) {
  return pfb::abi_guard([&]() -> int {
    if (!h) return PFB_ERR_BAD_ARG;
    delete h;
    return PFB_OK;
  });
}

extern "C" int pfb_rdcfar_reset(pfb_rdcfar_handle* h) {
  return pfb::abi_guard([&]() -> int { return reset_detector(h); });
}

extern "C" int pfb_rdcfar_set_stream(pfb_rdcfar_handle* h, void* hip_stream) {
  return pfb::abi_guard([&]() -> int { return set_detector_stream(h, hip_stream); });
}

extern "C" int pfb_rdcfar_sync(pfb_rdcfar_handle* h) {
  return pfb::abi_guard([&]() -> int { return sync_detector(h); });
}

extern "C" int pfb_rdcfar_get_device(const pfb_rdcfar_handle* h, int* device_id) {
  return pfb::abi_guard([&]() -> int { return detector_device(h, device_id); });
}

extern "C" int pfb_rdcfar_next_map(const pfb_rdcfar_handle* h, uint64_t* map_out) {
  return pfb::abi_guard([&]() -> int { return detector_next_map(h, map_out); });
}

extern "C" int pfb_rdcfar_get_stats(pfb_rdcfar_handle* h, pfb_rdcfar_stats* stats_out) {
  return pfb::abi_guard([&]() -> int { return detector_stats(h, stats_out); });
}

extern "C" int pfb_rdcfar_process(pfb_rdcfar_handle* h, const float* maps, uint64_t num_maps, pfb_rdcfar_det* det_out,
                                  uint64_t capacity, uint64_t* count_out, uint32_t mem) {
  return pfb::abi_guard([&]() -> int {
    return sync_call(h, maps, num_maps, det_out, capacity, count_out, mem, "pfb_rdcfar_process");
  });
}

extern "C" int pfb_rdcfar_process_async(pfb_rdcfar_handle* h, const float* d_maps, uint64_t num_maps,
                                        pfb_rdcfar_det* d_det_out, uint64_t capacity, uint64_t* d_count_out) {
  return pfb::abi_guard([&]() -> int { return async_call(h, d_maps, num_maps, d_det_out, capacity, d_count_out); });
}

extern "C" int pfb_rdcfar_to_pdw(const pfb_rdcfar_det* dets, uint64_t n, double fs, double fc, double sample_start_time,
                                 uint32_t pri, uint32_t num_pulses, uint64_t origin, uint32_t rows, uint32_t centered,
                                 pfb_pdw* pdw_out) {
  return pfb::abi_guard([&]() -> int {
    if ((n > 0 && (!dets || !pdw_out)) || !std::isfinite(fs) || !(fs > 0.0)) return PFB_ERR_BAD_ARG;
    if (pri == 0 || num_pulses == 0 || rows == 0) return PFB_ERR_BAD_ARG;
    for (uint64_t k = 0; k < n; ++k)
      if (dets[k].row >= rows) return PFB_ERR_BAD_ARG;
    for (uint64_t k = 0; k < n; ++k) {
      const pfb_rdcfar_det& d = dets[k];
      pfb_pdw& w = pdw_out[k];
      const int32_t bin = centered ? (int32_t)d.row - (int32_t)(rows / 2)
                                   : (d.row < (rows + 1) / 2 ? (int32_t)d.row : (int32_t)d.row - (int32_t)rows);
      const double first = (double)origin + (double)d.map * (double)num_pulses * (double)pri + (double)d.gate;
      w.toa = (first + 1.0) / fs + sample_start_time;
      w.pw = 1.0 / fs;
      w.snr = 10.0 * std::log10((double)d.power / (double)d.noise);
      w.mag = std::sqrt((double)d.power);
      w.freq = fc + (double)bin * fs / ((double)rows * (double)pri);
      w.sat = 0;
      w.bin = bin;
    }
    return PFB_OK;
  });
}

extern "C" const char* pfb_rdcfar_last_kernel(const pfb_rdcfar_handle* h) { return h ? h->last_kernel : ""; }
