// pfb_pdw_stage.hpp -- host side of the edge and pulse stages (create_pdws_channelized.m:85-135, create_pdws.m:54-105):
// the edge stage's buffers, and edges_and_pulses, which every driver of pfb_pdw.hip ends in -- tile summaries, scan,
// edge lists, one workgroup per pulse (pfb_pdw_edges.hpp, pfb_pdw_pulse.hpp), PDWs back to the host.
#pragma once

#include <algorithm>
#include <cstring>

#include "pfb_pdw_edges.hpp"
#include "pfb_pdw_pulse.hpp"
#include "pfb_pdw_scratch.hpp"

namespace {
// device buffers of the edge stage, all inside arena 0
struct EdgeStage {
  unsigned long long *f0, *f1, *off_s, *off_e, *tot, *base;
  unsigned char *fn, *state;
  ushort4* cnt;
  double *nf, *binf;  // binf == nullptr: no per-channel centre frequencies (raw stream)
};

EdgeStage take_edge_stage(Arena& ws, long long words, long long ntiles, uint32_t M, bool with_binf) {
  const size_t wm = (size_t)words * M, tm = (size_t)ntiles * M;
  EdgeStage e{};
  e.f0 = take<unsigned long long>(ws, wm);
  e.f1 = take<unsigned long long>(ws, wm);
  e.off_s = take<unsigned long long>(ws, tm);
  e.off_e = take<unsigned long long>(ws, tm);
  e.tot = take<unsigned long long>(ws, 2 * (size_t)M);
  e.base = take<unsigned long long>(ws, 2 * (size_t)M);
  e.fn = take<unsigned char>(ws, tm);
  e.state = take<unsigned char>(ws, tm);
  e.cnt = take<ushort4>(ws, tm);
  e.nf = take<double>(ws, M);
  double* binf = take<double>(ws, M);
  e.binf = with_binf ? binf : nullptr;
  return e;
}

// Called with the masks (e.f0, e.f1) and the noise floors (e.nf) on the device.
// d_check / h_check / h_nf (optional): flags of an optimistic noise-floor pass and its medians, fetched with the edge
// totals in the one sync; if the flags say the medians are not valid (bits 1 | 2) the function stops there and
// returns kRedo so that the caller can take the slow path and call again.
// Pulse: what runs per pulse.  MedianPulse is the scripts' pdw_pulse_kernel; any other tag launches its own kernel
// through Pulse::launch (pfb_dwell.hpp: the live loop's mean amplitude).  `flags` goes to that stage as it is:
// PFB_PDW_* for MedianPulse, PFB_DWELL_* for the dwell analysis.
constexpr int kRedo = 1;
struct MedianPulse {};
template <class Src, class Pulse = MedianPulse>
int edges_and_pulses(Src src, int Mi, long long ntiles, int tile_words, const EdgeStage& e, PdwCall& call, double fs, double fc, double t0,
                     unsigned flags, pfb_pdw* out, uint64_t capacity, uint64_t* count,
                     const unsigned* d_check = nullptr, unsigned* h_check = nullptr, double* h_nf = nullptr) {
  const hipStream_t st = call.st;
  const uint32_t M = (uint32_t)Mi;
  const size_t tm = (size_t)ntiles * M;
  const unsigned tblocks = (unsigned)((tm + 255) / 256);
  const bool wave_tiles = Mi == 1 && tile_words >= 64 && tile_words % 64 == 0;  // one column, long tiles: a wave per tile
  // pinned: [tot 2M u64 | base 2M u64 | nf M f64 | flags u32]
  HostPin& pin = g_pin[call.dev];
  PDW_TRY(pin_reserve(pin, (5 * (size_t)M + 1) * sizeof(unsigned long long)));
  unsigned long long* h_tot = reinterpret_cast<unsigned long long*>(pin.p);
  unsigned long long* h_base = h_tot + 2 * (size_t)M;
  double* p_nf = reinterpret_cast<double*>(h_base + 2 * (size_t)M);
  unsigned* p_check = reinterpret_cast<unsigned*>(p_nf + M);
  if (wave_tiles) {
    hipLaunchKernelGGL(pdw_tilefn_wave_kernel, dim3((unsigned)((ntiles + 3) / 4)), dim3(256), 0, st, (const unsigned long long*)e.f0,
                       (const unsigned long long*)e.f1, ntiles, tile_words, e.fn, e.cnt);
  } else {
    hipLaunchKernelGGL(pdw_tilefn_kernel, dim3(tblocks), dim3(256), 0, st, (const unsigned long long*)e.f0,
                       (const unsigned long long*)e.f1, Mi, ntiles, tile_words, e.fn, e.cnt);
  }
  if (Mi >= 32 && ntiles < 2048) {
    hipLaunchKernelGGL(pdw_tilescan_kernel<64>, dim3(Mi), dim3(64), 0, st, Mi, ntiles, (const unsigned char*)e.fn,
                       (const ushort4*)e.cnt, e.state, e.off_s, e.off_e, e.tot, e.tot + M);
  } else {  // few columns or many tiles per column: the parallelism has to come from time
    hipLaunchKernelGGL(pdw_tilescan_kernel<1024>, dim3(Mi), dim3(1024), 0, st, Mi, ntiles, (const unsigned char*)e.fn,
                       (const ushort4*)e.cnt, e.state, e.off_s, e.off_e, e.tot, e.tot + M);
  }
  PDW_TRY(hipGetLastError());
  PDW_TRY(hipMemcpyAsync(h_tot, e.tot, 2 * (size_t)M * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
  if (d_check) {
    PDW_TRY(hipMemcpyAsync(p_check, d_check, sizeof(unsigned), hipMemcpyDeviceToHost, st));
    PDW_TRY(hipMemcpyAsync(p_nf, e.nf, (size_t)M * sizeof(double), hipMemcpyDeviceToHost, st));
  }
  PDW_TRY(hipStreamSynchronize(st));
  if (d_check) {
    *h_check = *p_check;
    std::memcpy(h_nf, p_nf, (size_t)M * sizeof(double));
    if (*h_check & 3u) return kRedo;
  }
  unsigned long long total_s = 0, total_e = 0;
  for (uint32_t b = 0; b < M; ++b) {  // channels outermost, like the reference's for bin = 1:M
    h_base[b] = total_s; h_base[M + b] = total_e;
    total_s += h_tot[b]; total_e += h_tot[M + b];
  }
  *count = total_e;  // a pulse still active at the end of the data produces no PDW (the trailing test never fires)
  if (total_e > 0) {
    const unsigned long long n_out = std::min<unsigned long long>(total_e, capacity);
    long long *d_starts, *d_ends;
    pfb_pdw* d_out;
    PDW_TRY(arena_layout(call.ws2, [&](Arena& a) {
      d_starts = take<long long>(a, (size_t)total_s);
      d_ends = take<long long>(a, (size_t)total_e);
      d_out = take<pfb_pdw>(a, (size_t)n_out);
    }));
    PDW_TRY(hipMemcpyAsync(e.base, h_base, 2 * (size_t)M * sizeof(unsigned long long), hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(pdw_rebase_kernel, dim3(tblocks), dim3(256), 0, st, Mi, ntiles, e.off_s, e.off_e,
                       (const unsigned long long*)e.base, (const unsigned long long*)(e.base + M));
    if (wave_tiles) {
      hipLaunchKernelGGL(pdw_edges_wave_kernel, dim3((unsigned)((ntiles + 3) / 4)), dim3(256), 0, st, (const unsigned long long*)e.f0,
                         (const unsigned long long*)e.f1, ntiles, tile_words, (const unsigned char*)e.state,
                         (const unsigned long long*)e.off_s, (const unsigned long long*)e.off_e, d_starts, d_ends);
    } else {
      hipLaunchKernelGGL(pdw_edges_kernel, dim3(tblocks), dim3(256), 0, st, (const unsigned long long*)e.f0,
                         (const unsigned long long*)e.f1, Mi, ntiles, tile_words, (const unsigned char*)e.state,
                         (const unsigned long long*)e.off_s, (const unsigned long long*)e.off_e, d_starts, d_ends);
    }
    if (n_out > 0) {
      if constexpr (std::is_same_v<Pulse, MedianPulse>) {
        hipLaunchKernelGGL((pdw_pulse_kernel<Src, Src::kCache, Src::kThreads>), dim3((unsigned)n_out), dim3(Src::kThreads), 0, st, src, Mi, (const long long*)d_starts,
                           (const long long*)d_ends, (const unsigned long long*)e.base, (const unsigned long long*)(e.base + M),
                           (const double*)e.nf, (const double*)e.binf, fs, fc, t0, flags, d_out, n_out);
      } else {  // one column: pulse k runs from d_starts[k] to d_ends[k]
        Pulse::launch(src, (const long long*)d_starts, (const long long*)d_ends, (const double*)e.nf, fs, fc, t0, flags, d_out,
                      n_out, st);
      }
      PDW_TRY(hipGetLastError());
      PDW_TRY(hipMemcpyAsync(out, d_out, (size_t)n_out * sizeof(pfb_pdw), hipMemcpyDeviceToHost, st));
    }
    PDW_TRY(hipStreamSynchronize(st));
  }
  return PFB_OK;
}

// Tile length of the edge scan, in words.  The scan kernel walks a column's tiles with one workgroup (a strided, latency-
// bound walk), the tile kernels before and after it want >= 2^18 (tile, column) threads: at most 2^18 / M tiles per
// column, between 2048 and 16384 (measured at M = 128, 2^22 frames: scan + tile kernels 166 us at 8192 tiles per
// column, 100 us at 2048, 111 us at 1024).  The per-tile edge counts are 16-bit, which caps a tile at 2^16 samples.
int tile_words_for(long long samples, int M) {
  const long long w = (samples + 63) / 64;
  const long long max_tiles = std::min<long long>(16384, std::max<long long>(2048, (1ll << 18) / std::max(1, M)));
  int tw = kTileWords;
  while (tw < 1024 && w / tw > max_tiles) tw *= 2;
  return tw;
}
}  // namespace
