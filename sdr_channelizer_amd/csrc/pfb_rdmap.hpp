// pfb_rdmap.hpp -- the map detector that pfb_rdcfar.hip and pfb_oscfar.hip share, and nobody else includes: everything
// of a CFAR over range-Doppler maps but the decision of a cell.  Steps of whole maps (at most 2^24 cells and 2^18 words
// of 64 gates), the count, scan and emit passes behind a unit's cells kernel, the handle's state and the call semantics
// of pfb_rdcfar_process / _process_async (include/pfb_channelizer.h), which pfb_oscfar_* take over word for word.
//   rdmap_tile_counts  per tile of 256 words: its detections and its over cells
//   rdmap_scan         one workgroup: exclusive sum of the tile counts; the call's count and the stats
//   rdmap_emit         per tile of 256 words: a block scan places every word's records, ascending (map, row, gate)
// No atomics: every count is a scan, every record has one writer.  Grids are capped and stride.
// A unit brings its handle type H, derived from MapDetector:
//   H::Params   the kernels' parameters, derived from MapParams: the unit's own fields, then the tail named there
//   h->cfg      its config, whose fields up to peak_half_width, alpha, min_power and device_id are pfb_rdcfar_config's
//   h->cells(p, units)   completes p, launches its cells kernel on `units` workgroups and returns the kernel's name
// Everything here is internal to the including unit: the two are separate code objects with host stubs of their own.
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>

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

// What every kernel of a step reads.  A unit's Params add its own fields and then, in this order,
// `int band_rows, halo_rows, width; float alpha, min_power;` (a static_assert on sizeof pins the layout).
struct MapParams {
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
  int Wd, Gr, Tr, Pd;
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

template <class P>
__global__ void __launch_bounds__(256) rdmap_tile_counts(const P p) {
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

template <class P>
__global__ void __launch_bounds__(256) rdmap_scan(const P p) {
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

template <class P>
__global__ void __launch_bounds__(256) rdmap_emit(const P p) {
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

// ---------------------------------------------------------------------------------
// host: the state of a handle

struct MapDetector {
  Tiling tile{};
  int device = 0;
  uint32_t pitch = 0;       // resolved
  uint64_t map_cells = 0;   // ND R
  uint64_t map_words = 0;   // ND NWR
  uint64_t map_floats = 0;  // ND pitch
  uint64_t step_maps = 1;   // maps per step
  uint64_t no_noise = 0;    // cells of one map with nL = nR = 0
  hipStream_t stream = nullptr;
  hipEvent_t ev_switch = nullptr;
  uint64_t next_map = 0;
  DevState* d_state = nullptr;  // [0] live, [1] the copy sync_call restores from
  float* d_noise = nullptr;
  unsigned long long* d_words = nullptr;
  uint32_t* d_over = nullptr;
  int* d_tile = nullptr;  // tile_det, tile_over
  unsigned long long* d_tile_off = nullptr;
  size_t max_tiles = 0;
  void* d_stage = nullptr;  // host maps on their way in
  size_t stage_bytes = 0;
  void* d_det = nullptr;  // records on their way out to a host buffer
  size_t det_bytes = 0;
  const char* last_kernel = "";

  MapDetector() = default;
  MapDetector(const MapDetector&) = delete;  // owns the device memory
  MapDetector& operator=(const MapDetector&) = delete;
  ~MapDetector() {
    DeviceGuard g(device);
    (void)hipFree(d_state);
    (void)hipFree(d_noise);
    (void)hipFree(d_words);
    (void)hipFree(d_over);
    (void)hipFree(d_tile);
    (void)hipFree(d_tile_off);
    (void)hipFree(d_stage);
    (void)hipFree(d_det);
    if (ev_switch) (void)hipEventDestroy(ev_switch);
  }

  hipError_t allocate() {  // the buffers of one step, on the current device
    const uint64_t cells = step_maps * map_cells, words = step_maps * map_words;
    max_tiles = (size_t)((words + kTileWords - 1) / kTileWords);
    hipError_t e = hipSuccess;
    auto alloc = [&e](auto** p, size_t bytes) {
      if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(p), bytes);
    };
    alloc(&d_state, 2 * sizeof(DevState));
    alloc(&d_noise, cells * sizeof(float));
    alloc(&d_words, words * sizeof(unsigned long long));
    alloc(&d_over, words * sizeof(uint32_t));
    alloc(&d_tile, 2 * max_tiles * sizeof(int));
    alloc(&d_tile_off, max_tiles * sizeof(unsigned long long));
    if (e == hipSuccess) e = hipMemset(d_state, 0, 2 * sizeof(DevState));
    return e;
  }
};

// pfb_*_create once the unit has checked cfg: the device, the geometry, the buffers; `what` names the entry point
template <class H>
int create_detector(const decltype(H::cfg)& cfg, const Tiling& tile, const char* what, H** out) {
  int dev = 0;
  const int rc = resolve_device(cfg.device_id, &dev);
  if (rc != PFB_OK) return rc;
  H* h = new H();
  h->cfg = cfg;
  h->tile = tile;
  h->device = dev;
  h->pitch = cfg.pitch ? cfg.pitch : cfg.gates;
  const uint64_t R = cfg.gates, Gr = cfg.guard_gates;
  h->map_cells = (uint64_t)cfg.rows * R;
  h->map_words = (uint64_t)cfg.rows * ((R + 63) / 64);
  h->map_floats = (uint64_t)cfg.rows * h->pitch;
  h->step_maps = std::max<uint64_t>(1, std::min(kStepCells / h->map_cells, kStepWords / h->map_words));
  // no lead gate: r <= Gr; no lag gate: r >= R - Gr - 1
  const uint64_t lo = R > Gr + 1 ? R - Gr - 1 : 0, hi = std::min(Gr, R - 1);
  h->no_noise = hi >= lo ? (hi - lo + 1) * cfg.rows : 0;
  DeviceGuard g(dev);
  const hipError_t e = h->allocate();
  if (e != hipSuccess) {
    const int failed = hip_fail(e, (std::string(what) + " allocation").c_str());
    delete h;
    return failed;
  }
  *out = h;
  return PFB_OK;
}

// One step: m <= step_maps device maps, queued on the handle's stream; next_map advances
template <class H>
int step(H* h, const float* d_maps, uint64_t m, pfb_rdcfar_det* d_det, uint64_t capacity) {
  const auto& c = h->cfg;
  typename H::Params p{};
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
  p.band_rows = h->tile.band_rows;
  p.halo_rows = h->tile.halo_rows;
  p.width = h->tile.width;
  p.alpha = c.alpha;
  p.min_power = c.min_power;
  const unsigned units = grid_for((uint64_t)m * p.NB * p.NT, 1, kMaxGrid), tiles = grid_for(p.ntiles, 1, kMaxGrid);
  const char* kernel = h->cells(p, units);
  hipLaunchKernelGGL(rdmap_tile_counts<typename H::Params>, dim3(tiles), dim3(256), 0, h->stream, p);
  hipLaunchKernelGGL(rdmap_scan<typename H::Params>, dim3(1), dim3(256), 0, h->stream, p);
  hipLaunchKernelGGL(rdmap_emit<typename H::Params>, dim3(tiles), dim3(256), 0, h->stream, p);
  HIP_TRY(hipGetLastError());
  h->last_kernel = kernel;
  h->next_map += m;
  return PFB_OK;
}

// the maps of one call in steps, device pointers, no host sync; the call's count ends in d_state->call_count
template <class H>
int enqueue(H* h, const float* d_maps, uint64_t n, pfb_rdcfar_det* d_det, uint64_t capacity) {
  HIP_TRY(hipMemsetAsync(&h->d_state->call_count, 0, sizeof(unsigned long long), h->stream));
  for (uint64_t done = 0; done < n;) {
    const uint64_t m = std::min(h->step_maps, n - done);
    const int rc = step(h, d_maps + done * h->map_floats, m, d_det, capacity);
    if (rc != PFB_OK) return rc;
    done += m;
  }
  return PFB_OK;
}

// what every process call checks before the device is touched
int check_call(const MapDetector* h, const void* maps, uint64_t n, const void* det, uint64_t capacity,
                      const void* count_out, bool device) {
  if (!h || !count_out || (n > 0 && !maps) || (capacity > 0 && !det)) return PFB_ERR_BAD_ARG;
  if (n > ((uint64_t)1 << 40) || capacity > ((uint64_t)1 << 56)) return PFB_ERR_BAD_ARG;
  if (device && ((reinterpret_cast<uintptr_t>(maps) % 4) || (reinterpret_cast<uintptr_t>(det) % 8))) return PFB_ERR_BAD_ARG;
  return PFB_OK;
}

// pfb_*_process (`what` in the error details): the checks, the steps, the count, and the state back where it was when
// the count does not fit
template <class H>
int sync_call(H* h, const float* maps, uint64_t n, pfb_rdcfar_det* det_out, uint64_t capacity, uint64_t* count_out,
              uint32_t mem, const char* what) {
  if (mem > PFB_MEM_DEVICE) return PFB_ERR_BAD_ARG;
  int rc = check_call(h, maps, n, det_out, capacity, count_out, mem == PFB_MEM_DEVICE);
  if (rc != PFB_OK) return rc;
  DeviceGuard g(h->device);
  const bool host = mem == PFB_MEM_HOST;
  const uint64_t saved_map = h->next_map;
  HIP_TRY(hipMemcpyAsync(h->d_state + 1, h->d_state, sizeof(DevState), hipMemcpyDeviceToDevice, h->stream));
  pfb_rdcfar_det* d_det = det_out;
  uint64_t cap_dev = capacity;
  if (host) {  // no call reports more cells than it takes
    cap_dev = std::min<uint64_t>(capacity, n * h->map_cells);
    rc = grow(&h->d_det, &h->det_bytes, (size_t)std::max<uint64_t>(cap_dev, 1) * sizeof(pfb_rdcfar_det));
    if (rc == PFB_OK && n > 0) rc = grow(&h->d_stage, &h->stage_bytes, (size_t)(std::min(n, h->step_maps) * h->map_floats * sizeof(float)));
    if (rc != PFB_OK) return rc;
    d_det = static_cast<pfb_rdcfar_det*>(h->d_det);
  }
  auto fail = [&](int code) {  // the state is put back before the call returns
    (void)hipStreamSynchronize(h->stream);
    h->next_map = saved_map;
    (void)hipMemcpyAsync(h->d_state, h->d_state + 1, sizeof(DevState), hipMemcpyDeviceToDevice, h->stream);
    (void)hipStreamSynchronize(h->stream);
    return code;
  };
  if (!host) {
    rc = enqueue(h, maps, n, d_det, cap_dev);
  } else {
    hipError_t e = hipMemsetAsync(&h->d_state->call_count, 0, sizeof(unsigned long long), h->stream);
    if (e != hipSuccess) return fail(hip_fail(e, what));
    for (uint64_t done = 0; done < n && rc == PFB_OK;) {
      const uint64_t m = std::min(h->step_maps, n - done);
      e = hipMemcpyAsync(h->d_stage, maps + done * h->map_floats, (size_t)(m * h->map_floats * sizeof(float)), hipMemcpyHostToDevice, h->stream);
      if (e != hipSuccess) return fail(hip_fail(e, (std::string(what) + " staging").c_str()));
      rc = step(h, static_cast<const float*>(h->d_stage), m, d_det, cap_dev);
      e = hipStreamSynchronize(h->stream);  // the one staging buffer is free again
      if (e != hipSuccess) return fail(hip_fail(e, what));
      done += m;
    }
  }
  if (rc != PFB_OK) return fail(rc);
  unsigned long long count = 0;
  hipError_t e = hipMemcpyAsync(&count, &h->d_state->call_count, sizeof(count), hipMemcpyDeviceToHost, h->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
  if (e != hipSuccess) return fail(hip_fail(e, what));
  *count_out = count;
  if (count > capacity) return fail(PFB_ERR_CAPACITY);
  if (host && count > 0) {
    e = hipMemcpy(det_out, d_det, (size_t)count * sizeof(pfb_rdcfar_det), hipMemcpyDeviceToHost);
    if (e != hipSuccess) return fail(hip_fail(e, (std::string(what) + " records").c_str()));  // nothing delivered: nothing taken
  }
  return PFB_OK;
}

// pfb_*_process_async: the checks, the steps, and the call's count copied on the stream
template <class H>
int async_call(H* h, const float* d_maps, uint64_t n, pfb_rdcfar_det* d_det, uint64_t capacity, uint64_t* d_count_out) {
  int rc = check_call(h, d_maps, n, d_det, capacity, d_count_out, true);
  if (rc != PFB_OK) return rc;
  if (reinterpret_cast<uintptr_t>(d_count_out) % 8) return PFB_ERR_BAD_ARG;
  DeviceGuard g(h->device);
  rc = enqueue(h, d_maps, n, d_det, capacity);
  if (rc != PFB_OK) return rc;
  HIP_TRY(hipMemcpyAsync(d_count_out, &h->d_state->call_count, sizeof(uint64_t), hipMemcpyDeviceToDevice, h->stream));
  return PFB_OK;
}

// the bodies of pfb_*_reset, _set_stream, _sync, _get_device, _next_map and _get_stats
int reset_detector(MapDetector* h) {
  if (!h) return PFB_ERR_BAD_ARG;
  DeviceGuard g(h->device);
  HIP_TRY(hipMemsetAsync(h->d_state, 0, sizeof(DevState), h->stream));
  h->next_map = 0;
  return PFB_OK;
}

int set_detector_stream(MapDetector* h, void* hip_stream) {
  if (!h) return PFB_ERR_BAD_ARG;
  return switch_stream(h->device, &h->stream, &h->ev_switch, static_cast<hipStream_t>(hip_stream));
}

int sync_detector(MapDetector* h) {
  if (!h) return PFB_ERR_BAD_ARG;
  DeviceGuard g(h->device);
  HIP_TRY(hipStreamSynchronize(h->stream));
  return PFB_OK;
}

int detector_device(const MapDetector* h, int* device_id) {
  if (!h || !device_id) return PFB_ERR_BAD_ARG;
  *device_id = h->device;
  return PFB_OK;
}

int detector_next_map(const MapDetector* h, uint64_t* map_out) {
  if (!h || !map_out) return PFB_ERR_BAD_ARG;
  *map_out = h->next_map;
  return PFB_OK;
}

int detector_stats(MapDetector* h, pfb_rdcfar_stats* stats_out) {
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
}

}  // namespace
