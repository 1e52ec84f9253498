// pfb_oscfar.hip -- an ordered-statistic CFAR detector over range-Doppler maps (pfb_oscfar_* in
// include/pfb_channelizer.h, where the arithmetic is defined): per-cell rank counts, the select of an over cell's
// noise, the peak box, ordered compaction, kernels and host side.  Geometry, records, stats and the call semantics are
// pfb_rdcfar_*'s (pfb_rdcfar.hip); the count, scan and emit passes are that unit's, restated here so that its code
// objects stay as they are.  A step takes whole maps, at most 2^24 cells and 2^18 words of 64 gates.
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
//   oscfar_tile_counts  per tile of 256 words: its detections and its over cells
//   oscfar_scan         one workgroup: exclusive sum of the tile counts; the call's count and the stats
//   oscfar_emit         per tile of 256 words: a block scan places every word's records, ascending (map, row, gate)
// No atomics: every count is a scan, every record has one writer.  Grids are capped and stride.
// Cost: a cell reads at most n float32 of LDS (a wave as many as its slowest lane); an over cell costs its wave
// 32 ceil(n / 64) more per lane and its own lane the peak box: slow only for maps that are all detections.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <new>

#include "pfb_common.h"
#include "pfb_host.h"

namespace {

using namespace pfb;

constexpr uint64_t kStepCells = (uint64_t)1 << 24;  // cells per step at most, and ...
constexpr uint64_t kStepWords = (uint64_t)1 << 18;  // ... words of 64 gates (one map at least)
constexpr unsigned kMaxGrid = 1u << 16;
constexpr int kTileGates = 256;   // gates per workgroup: a lane each
constexpr int kTileWords = 256;   // words per workgroup of the count and emit passes
constexpr uint32_t kLdsBudget = 64u << 10;
constexpr uint32_t kMaxTraining = 4096;  // N at most
constexpr int kMaxBand = 16;             // rows of a band at most
constexpr int kChunk = 8;                // gates a lane counts between two looks at the rest of its wave

struct DevState {  // the counts that depend on the data
  unsigned long long cells_over, detections, dropped;
  unsigned long long call_count;  // detections of the current call so far
};

struct Tiling {
  int band_rows;  // rows of a band
  int halo_rows;  // max(Wd, Pd)
  int width;      // kTileGates + 2 (Gr + Tr): gates of the staged block
  bool lds;       // P staged in LDS
  uint32_t lds_bytes;
};

struct OsParams {
  const float* maps;   // the step's maps
  float* noise;        // [(m' ND + d) R + r], written at detections only
  unsigned long long* words;  // [(m' ND + d) NWR + w]: detection bits of gates 64 w .. 64 w + 63
  uint32_t* over;      // over cells of the same 64 gates
  int* tile_det;
  int* tile_over;
  unsigned long long* tile_off;
  DevState* st;
  pfb_rdcfar_det* det_out;
  unsigned long long capacity;
  unsigned long long map0;  // m of the step's first map
  long long nwords;
  int ntiles;
  int num_maps;
  int ND, R, pitch, NWR, NT, NB;  // NWR words per row, NT gate tiles per row, NB bands per map
  int Wd, Gr, Tr, Pd, rank, N;
  int band_rows, halo_rows, width;
  float alpha, min_power;
};

// ---------------------------------------------------------------------------------
// block scan over 256 threads (int): exclusive prefix and the total

__device__ int block_sum_excl(int v, int* sh, int& total) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, waves = blockDim.x >> 6;
  int inc = v;
  for (int d = 1; d < 64; d <<= 1) {
    const int o = __shfl_up(inc, d, 64);
    if (lane >= d) inc += o;
  }
  int exc = __shfl_up(inc, 1, 64);
  if (lane == 0) exc = 0;
  __syncthreads();  // sh is free again
  if (lane == 63) sh[wv] = inc;
  __syncthreads();
  int pre = 0;
  total = 0;
  for (int k = 0; k < waves; ++k) {
    if (k < wv) pre += sh[k];
    total += sh[k];
  }
  return pre + exc;
}

// ---------------------------------------------------------------------------------
// kernels

__device__ __forceinline__ int wrap(int d, int ND) {  // d in -ND .. 2 ND - 1
  return d < 0 ? d + ND : d >= ND ? d - ND : d;
}

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

__global__ void __launch_bounds__(256) oscfar_tile_counts(const OsParams p) {
  __shared__ int sh[8];
  for (int t = blockIdx.x; t < p.ntiles; t += gridDim.x) {
    const long long j = (long long)t * kTileWords + threadIdx.x;
    const bool live = j < p.nwords;
    int dets, overs;
    block_sum_excl(live ? __popcll(p.words[j]) : 0, sh, dets);
    block_sum_excl(live ? (int)p.over[j] : 0, sh, overs);
    if (threadIdx.x == 0) {
      p.tile_det[t] = dets;
      p.tile_over[t] = overs;
    }
  }
}

__global__ void __launch_bounds__(256) oscfar_scan(const OsParams p) {
  __shared__ int sh[8];
  DevState& st = *p.st;
  const unsigned long long base = st.call_count;  // every thread reads it before thread 0 writes it (the scans' barriers)
  unsigned long long running = 0, over = 0;
  for (int t0 = 0; t0 < p.ntiles; t0 += blockDim.x) {
    const int t = t0 + threadIdx.x;
    int total, sum;
    const int exc = block_sum_excl(t < p.ntiles ? p.tile_det[t] : 0, sh, total);
    if (t < p.ntiles) p.tile_off[t] = base + running + (unsigned long long)exc;
    running += (unsigned long long)total;
    block_sum_excl(t < p.ntiles ? p.tile_over[t] : 0, sh, sum);
    over += (unsigned long long)sum;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    const unsigned long long after = base + running;
    st.dropped += max(after, p.capacity) - max(base, p.capacity);
    st.detections += running;
    st.cells_over += over;
    st.call_count = after;
  }
}

__global__ void __launch_bounds__(256) oscfar_emit(const OsParams p) {
  __shared__ int sh[8];
  for (int t = blockIdx.x; t < p.ntiles; t += gridDim.x) {
    if (p.tile_det[t] == 0) continue;  // uniform over the workgroup
    const long long j = (long long)t * kTileWords + threadIdx.x;
    unsigned long long w = j < p.nwords ? p.words[j] : 0ull;
    int total;
    unsigned long long pos = p.tile_off[t] + (unsigned long long)block_sum_excl(__popcll(w), sh, total);
    if (!w) continue;
    const long long rowi = j / p.NWR;  // m' ND + d
    const int wi = (int)(j % p.NWR);
    const int d = (int)(rowi % p.ND);
    const unsigned long long m = p.map0 + (unsigned long long)(rowi / p.ND);
    for (; w && pos < p.capacity; w &= w - 1, ++pos) {
      const int r = wi * 64 + __ffsll((long long)w) - 1;
      const int nl = max(r - p.Gr - max(r - p.Gr - p.Tr, 0), 0);
      const int nr = max(min(r + p.Gr + p.Tr + 1, p.R) - (r + p.Gr + 1), 0);
      pfb_rdcfar_det rec;
      rec.map = m;
      rec.row = (uint32_t)d;
      rec.gate = (uint32_t)r;
      rec.power = p.maps[(size_t)rowi * p.pitch + r];
      rec.noise = p.noise[(size_t)rowi * p.R + r];
      rec.training_cells = (uint32_t)((nl + nr) * (2 * p.Wd + 1));
      rec.flags = nl + nr < 2 * p.Tr ? PFB_RDCFAR_DET_ONE_SIDED : 0u;
      p.det_out[pos] = rec;
    }
  }
}

unsigned grid_for(uint64_t items, unsigned per_block) {
  return (unsigned)std::min<uint64_t>(std::max<uint64_t>((items + per_block - 1) / per_block, 1), kMaxGrid);
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

}  // namespace

struct pfb_oscfar_handle {
  pfb_oscfar_config cfg{};
  Tiling tile{};
  int device = 0;
  uint32_t pitch = 0;       // resolved
  uint64_t map_cells = 0;   // ND R
  uint64_t map_words = 0;   // ND NWR
  uint64_t step_maps = 1;   // maps per step
  uint64_t no_noise = 0;    // cells of one map with nL = nR = 0
  hipStream_t stream = nullptr;
  hipEvent_t ev_switch = nullptr;
  uint64_t next_map = 0;
  DevState* d_state = nullptr;  // [0] live, [1] the copy pfb_oscfar_process restores from
  float* d_noise = nullptr;
  unsigned long long* d_words = nullptr;
  uint32_t* d_over = nullptr;
  int* d_tile = nullptr;  // tile_det, tile_over
  unsigned long long* d_tile_off = nullptr;
  size_t max_tiles = 0;
  float* d_stage = nullptr;  // host maps on their way in
  size_t stage_bytes = 0;
  pfb_rdcfar_det* d_det = nullptr;  // records on their way out to a host buffer
  size_t det_cap = 0;
  const char* last_kernel = "";
};

namespace {

void free_oscfar(pfb_oscfar_handle* h) {
  if (!h) return;
  DeviceGuard g(h->device);
  (void)hipFree(h->d_state);
  (void)hipFree(h->d_noise);
  (void)hipFree(h->d_words);
  (void)hipFree(h->d_over);
  (void)hipFree(h->d_tile);
  (void)hipFree(h->d_tile_off);
  (void)hipFree(h->d_stage);
  (void)hipFree(h->d_det);
  if (h->ev_switch) (void)hipEventDestroy(h->ev_switch);
  delete h;
}

hipError_t allocate_oscfar(pfb_oscfar_handle* h) {
  const uint64_t cells = h->step_maps * h->map_cells, words = h->step_maps * h->map_words;
  h->max_tiles = (size_t)((words + kTileWords - 1) / kTileWords);
  hipError_t e = hipSuccess;
  auto alloc = [&e](auto** p, size_t bytes) {
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(p), bytes);
  };
  alloc(&h->d_state, 2 * sizeof(DevState));
  alloc(&h->d_noise, cells * sizeof(float));
  alloc(&h->d_words, words * sizeof(unsigned long long));
  alloc(&h->d_over, words * sizeof(uint32_t));
  alloc(&h->d_tile, 2 * h->max_tiles * sizeof(int));
  alloc(&h->d_tile_off, h->max_tiles * sizeof(unsigned long long));
  if (e == hipSuccess) e = hipMemset(h->d_state, 0, 2 * sizeof(DevState));
  return e;
}

int create_oscfar(const pfb_oscfar_config* cfg, pfb_oscfar_handle** out) {
  pfb_oscfar_plan plan{};
  int rc = oscfar_check(cfg, &plan);
  if (rc != PFB_OK) return rc;
  int dev = 0;
  rc = pfb::resolve_device(cfg->device_id, &dev);
  if (rc != PFB_OK) return rc;
  pfb_oscfar_handle* h = new pfb_oscfar_handle();
  h->cfg = *cfg;
  h->tile = tiling_for(*cfg);
  h->device = dev;
  h->pitch = cfg->pitch ? cfg->pitch : cfg->gates;
  const uint64_t R = cfg->gates, Gr = cfg->guard_gates;
  h->map_cells = (uint64_t)cfg->rows * R;
  h->map_words = (uint64_t)cfg->rows * ((R + 63) / 64);
  h->step_maps = std::max<uint64_t>(1, std::min(kStepCells / h->map_cells, kStepWords / h->map_words));
  // no lead gate: r <= Gr; no lag gate: r >= R - Gr - 1
  const uint64_t lo = R > Gr + 1 ? R - Gr - 1 : 0, hi = std::min(Gr, R - 1);
  h->no_noise = hi >= lo ? (hi - lo + 1) * cfg->rows : 0;
  DeviceGuard g(dev);
  const hipError_t e = allocate_oscfar(h);
  if (e != hipSuccess) {
    rc = pfb::hip_fail(e, "pfb_oscfar_create allocation");
    free_oscfar(h);
    return rc;
  }
  *out = h;
  return PFB_OK;
}

// One step: m <= step_maps device maps, queued on the handle's stream; next_map advances
int oscfar_step(pfb_oscfar_handle* h, const float* d_maps, uint64_t m, pfb_rdcfar_det* d_det, uint64_t capacity) {
  const pfb_oscfar_config& c = h->cfg;
  OsParams p{};
  p.maps = d_maps;
  p.noise = h->d_noise;
  p.words = h->d_words;
  p.over = h->d_over;
  p.tile_det = h->d_tile;
  p.tile_over = h->d_tile + h->max_tiles;
  p.tile_off = h->d_tile_off;
  p.st = h->d_state;
  p.det_out = d_det;
  p.capacity = capacity;
  p.map0 = h->next_map;
  p.num_maps = (int)m;
  p.ND = (int)c.rows;
  p.R = (int)c.gates;
  p.pitch = (int)h->pitch;
  p.NWR = (int)((c.gates + 63) / 64);
  p.NT = (int)((c.gates + kTileGates - 1) / kTileGates);
  p.NB = (int)((c.rows + h->tile.band_rows - 1) / h->tile.band_rows);
  p.nwords = (long long)(m * h->map_words);
  p.ntiles = (int)((p.nwords + kTileWords - 1) / kTileWords);
  p.Wd = (int)c.doppler_half_width;
  p.Gr = (int)c.guard_gates;
  p.Tr = (int)c.train_gates;
  p.Pd = (int)c.peak_half_width;
  p.rank = (int)c.rank;
  p.N = (int)(2 * c.train_gates * (2 * c.doppler_half_width + 1));
  p.band_rows = h->tile.band_rows;
  p.halo_rows = h->tile.halo_rows;
  p.width = h->tile.width;
  p.alpha = c.alpha;
  p.min_power = c.min_power;
  const unsigned units = grid_for((uint64_t)m * p.NB * p.NT, 1), tiles = grid_for(p.ntiles, 1);
  if (h->tile.lds) hipLaunchKernelGGL(oscfar_cells<true>, dim3(units), dim3(kTileGates), h->tile.lds_bytes, h->stream, p);
  else hipLaunchKernelGGL(oscfar_cells<false>, dim3(units), dim3(kTileGates), 0, h->stream, p);
  hipLaunchKernelGGL(oscfar_tile_counts, dim3(tiles), dim3(256), 0, h->stream, p);
  hipLaunchKernelGGL(oscfar_scan, dim3(1), dim3(256), 0, h->stream, p);
  hipLaunchKernelGGL(oscfar_emit, dim3(tiles), dim3(256), 0, h->stream, p);
  HIP_TRY(hipGetLastError());
  h->last_kernel = kernel_name(h->tile.lds);
  h->next_map += m;
  return PFB_OK;
}

// the maps of one call in steps, device pointers, no host sync; the call's count ends in d_state->call_count
int oscfar_enqueue(pfb_oscfar_handle* h, const float* d_maps, uint64_t n, pfb_rdcfar_det* d_det, uint64_t capacity) {
  HIP_TRY(hipMemsetAsync(&h->d_state->call_count, 0, sizeof(unsigned long long), h->stream));
  const uint64_t map_floats = (uint64_t)h->cfg.rows * h->pitch;
  for (uint64_t done = 0; done < n;) {
    const uint64_t m = std::min(h->step_maps, n - done);
    const int rc = oscfar_step(h, d_maps + done * map_floats, m, d_det, capacity);
    if (rc != PFB_OK) return rc;
    done += m;
  }
  return PFB_OK;
}

int grow(void** p, size_t* have, size_t want) {
  if (want <= *have) return PFB_OK;
  (void)hipFree(*p);
  *p = nullptr;
  *have = 0;
  HIP_TRY(hipMalloc(p, want));
  *have = want;
  return PFB_OK;
}

// pfb_oscfar_process: the steps, the count, and the state back where it was when the count does not fit
int oscfar_sync_call(pfb_oscfar_handle* h, const float* maps, uint64_t n, pfb_rdcfar_det* det_out, uint64_t capacity,
                     uint64_t* count_out, uint32_t mem) {
  DeviceGuard g(h->device);
  const bool host = mem == PFB_MEM_HOST;
  const uint64_t saved_map = h->next_map;
  const uint64_t map_floats = (uint64_t)h->cfg.rows * h->pitch;
  HIP_TRY(hipMemcpyAsync(h->d_state + 1, h->d_state, sizeof(DevState), hipMemcpyDeviceToDevice, h->stream));
  pfb_rdcfar_det* d_det = det_out;
  uint64_t cap_dev = capacity;
  if (host) {  // no call reports more cells than it takes
    cap_dev = std::min<uint64_t>(capacity, n * h->map_cells);
    size_t have = h->det_cap * sizeof(pfb_rdcfar_det);
    int rc = grow(reinterpret_cast<void**>(&h->d_det), &have, (size_t)std::max<uint64_t>(cap_dev, 1) * sizeof(pfb_rdcfar_det));
    h->det_cap = have / sizeof(pfb_rdcfar_det);
    void* stage = h->d_stage;
    if (rc == PFB_OK && n > 0) rc = grow(&stage, &h->stage_bytes, (size_t)(std::min(n, h->step_maps) * map_floats * sizeof(float)));
    h->d_stage = static_cast<float*>(stage);
    if (rc != PFB_OK) return rc;
    d_det = h->d_det;
  }
  auto fail = [&](int code) {  // the state is put back before the call returns
    (void)hipStreamSynchronize(h->stream);
    h->next_map = saved_map;
    (void)hipMemcpyAsync(h->d_state, h->d_state + 1, sizeof(DevState), hipMemcpyDeviceToDevice, h->stream);
    (void)hipStreamSynchronize(h->stream);
    return code;
  };
  int rc = PFB_OK;
  if (!host) {
    rc = oscfar_enqueue(h, maps, n, d_det, cap_dev);
  } else {
    hipError_t e = hipMemsetAsync(&h->d_state->call_count, 0, sizeof(unsigned long long), h->stream);
    if (e != hipSuccess) return fail(pfb::hip_fail(e, "pfb_oscfar_process"));
    for (uint64_t done = 0; done < n && rc == PFB_OK;) {
      const uint64_t m = std::min(h->step_maps, n - done);
      e = hipMemcpyAsync(h->d_stage, maps + done * map_floats, (size_t)(m * map_floats * sizeof(float)), hipMemcpyHostToDevice, h->stream);
      if (e != hipSuccess) return fail(pfb::hip_fail(e, "pfb_oscfar_process staging"));
      rc = oscfar_step(h, h->d_stage, m, d_det, cap_dev);
      e = hipStreamSynchronize(h->stream);  // the one staging buffer is free again
      if (e != hipSuccess) return fail(pfb::hip_fail(e, "pfb_oscfar_process"));
      done += m;
    }
  }
  if (rc != PFB_OK) return fail(rc);
  unsigned long long count = 0;
  hipError_t e = hipMemcpyAsync(&count, &h->d_state->call_count, sizeof(count), hipMemcpyDeviceToHost, h->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
  if (e != hipSuccess) return fail(pfb::hip_fail(e, "pfb_oscfar_process"));
  *count_out = count;
  if (count > capacity) return fail(PFB_ERR_CAPACITY);
  if (host && count > 0) {
    e = hipMemcpy(det_out, d_det, (size_t)count * sizeof(pfb_rdcfar_det), hipMemcpyDeviceToHost);
    if (e != hipSuccess) return fail(pfb::hip_fail(e, "pfb_oscfar_process records"));  // nothing delivered: nothing taken
  }
  return PFB_OK;
}

// what every process call checks before the device is touched
int oscfar_check_call(const pfb_oscfar_handle* h, const void* maps, uint64_t n, const void* det, uint64_t capacity,
                      const void* count_out, bool device) {
  if (!h || !count_out || (n > 0 && !maps) || (capacity > 0 && !det)) return PFB_ERR_BAD_ARG;
  if (n > ((uint64_t)1 << 40) || capacity > ((uint64_t)1 << 56)) return PFB_ERR_BAD_ARG;
  if (device && ((reinterpret_cast<uintptr_t>(maps) % 4) || (reinterpret_cast<uintptr_t>(det) % 8))) return PFB_ERR_BAD_ARG;
  return PFB_OK;
}

// log of the false-alarm probability of rank k of N exponential cells at factor a: -sum log1p(a / (N - i))
double log_pfa(double a, uint64_t N, uint64_t k) {
  double s = 0.0;
  for (uint64_t i = 0; i < k; ++i) s -= std::log1p(a / (double)(N - i));
  return s;
}

}  // namespace

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
    return create_oscfar(cfg, out);
  });
}

extern "C" int pfb_oscfar_destroy(pfb_oscfar_handle* h) {
  return pfb::abi_guard([&]() -> int {
    if (!h) return PFB_ERR_BAD_ARG;
    free_oscfar(h);
    return PFB_OK;
  });
}

extern "C" int pfb_oscfar_reset(pfb_oscfar_handle* h) {
  return pfb::abi_guard([&]() -> int {
    if (!h) return PFB_ERR_BAD_ARG;
    DeviceGuard g(h->device);
    HIP_TRY(hipMemsetAsync(h->d_state, 0, sizeof(DevState), h->stream));
    h->next_map = 0;
    return PFB_OK;
  });
}

extern "C" int pfb_oscfar_set_stream(pfb_oscfar_handle* h, void* hip_stream) {
  return pfb::abi_guard([&]() -> int {
    if (!h) return PFB_ERR_BAD_ARG;
    return pfb::switch_stream(h->device, &h->stream, &h->ev_switch, static_cast<hipStream_t>(hip_stream));
  });
}

extern "C" int pfb_oscfar_sync(pfb_oscfar_handle* h) {
  return pfb::abi_guard([&]() -> int {
    if (!h) return PFB_ERR_BAD_ARG;
    DeviceGuard g(h->device);
    HIP_TRY(hipStreamSynchronize(h->stream));
    return PFB_OK;
  });
}

extern "C" int pfb_oscfar_get_device(const pfb_oscfar_handle* h, int* device_id) {
  return pfb::abi_guard([&]() -> int {
    if (!h || !device_id) return PFB_ERR_BAD_ARG;
    *device_id = h->device;
    return PFB_OK;
  });
}

extern "C" int pfb_oscfar_next_map(const pfb_oscfar_handle* h, uint64_t* map_out) {
  return pfb::abi_guard([&]() -> int {
    if (!h || !map_out) return PFB_ERR_BAD_ARG;
    *map_out = h->next_map;
    return PFB_OK;
  });
}

extern "C" int pfb_oscfar_get_stats(pfb_oscfar_handle* h, pfb_rdcfar_stats* stats_out) {
  return pfb::abi_guard([&]() -> int {
    if (!h || !stats_out) return PFB_ERR_BAD_ARG;
    DeviceGuard g(h->device);
    DevState st;
    HIP_TRY(hipMemcpyAsync(&st, h->d_state, sizeof(st), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    stats_out->maps_in = h->next_map;
    stats_out->cells_over = st.cells_over;
    stats_out->cells_without_noise = h->next_map * h->no_noise;
    stats_out->detections = st.detections;
    stats_out->dropped = st.dropped;
    return PFB_OK;
  });
}

extern "C" int pfb_oscfar_process(pfb_oscfar_handle* h, const float* maps, uint64_t num_maps, pfb_rdcfar_det* det_out,
                                  uint64_t capacity, uint64_t* count_out, uint32_t mem) {
  return pfb::abi_guard([&]() -> int {
    if (mem > PFB_MEM_DEVICE) return PFB_ERR_BAD_ARG;
    const int rc = oscfar_check_call(h, maps, num_maps, det_out, capacity, count_out, mem == PFB_MEM_DEVICE);
    if (rc != PFB_OK) return rc;
    return oscfar_sync_call(h, maps, num_maps, det_out, capacity, count_out, mem);
  });
}

extern "C" int pfb_oscfar_process_async(pfb_oscfar_handle* h, const float* d_maps, uint64_t num_maps,
                                        pfb_rdcfar_det* d_det_out, uint64_t capacity, uint64_t* d_count_out) {
  return pfb::abi_guard([&]() -> int {
    int rc = oscfar_check_call(h, d_maps, num_maps, d_det_out, capacity, d_count_out, true);
    if (rc != PFB_OK) return rc;
    if (reinterpret_cast<uintptr_t>(d_count_out) % 8) return PFB_ERR_BAD_ARG;
    DeviceGuard g(h->device);
    rc = oscfar_enqueue(h, d_maps, num_maps, d_det_out, capacity);
    if (rc != PFB_OK) return rc;
    HIP_TRY(hipMemcpyAsync(d_count_out, &h->d_state->call_count, sizeof(uint64_t), hipMemcpyDeviceToDevice, h->stream));
    return PFB_OK;
  });
}

extern "C" const char* pfb_oscfar_last_kernel(const pfb_oscfar_handle* h) { return h ? h->last_kernel : ""; }
