// pfb_pdw.hip -- channelized PDW extraction on the GPU (include/pfb_channelizer.h, pfb_pdw_extract).
//
// Restates the second half of the reference's matlab/create_pdws_channelized.m (lines 64-143) as
// data-parallel passes over the F x M channelizer output (frame-major complex64, fftshift-ed):
//
//   noise floor  :73    exact per-channel median of |y|.  A hashed 1-in-k row sample, read once, brackets the
//                       median (per-channel select of two sample ranks 5 sigma either side of the middle); ONE
//                       pass over the data -- every sample screened in float32, only the bracket's zone promoted
//                       to float64 -- counts what lies below the bracket and gathers what lies inside it (about
//                       2 %), and a per-channel select over those candidates picks the exact order statistics.
//                       The count proves the bracket held the median; if it did not (or the data are too tied /
//                       too short to sample) the full MSB-first radix select runs instead: 8-bit digit histograms
//                       in LDS (lane = channel, so LDS atomics never collide) until the bucket is small, then an
//                       exact finish.  The same pass leaves the comparison masks of the edge stage.
//   threshold    :74-75 NF * 10^(SNR/10)
//   edges        :85-135 the leading/trailing-edge state machine is a 2-state automaton
//                       next = active ? (mag > thr) : (mag >= thr); each tile of frames is summarised
//                       as a 2-bit transition function, the functions are scanned per channel, and the
//                       tiles are replayed with their incoming state to count and emit edge indices.
//   per pulse    :98-132 one workgroup per pulse: medians of the magnitudes and of the wrapped phase
//                       steps by rank counting or a three-scan bucket select (values cached in LDS when they fit).
//
// The raw-stream script (matlab/create_pdws.m:30-105, pfb_pdw_extract_raw) shares the edge and pulse stages; its
// one column makes the noise floor a time-parallel radix select whose leading digits are predicted from a small
// sample and proven by the first counting pass, and its masks a comparison of integer keys.  The dwell analysis of the
// event predictor (pfb_dwell_analyze, pfb_dwell.hpp) runs on the same sources, masks and edge stage.
//
// Arithmetic is float64 like the MATLAB scripts: everything that decides an outcome is computed on the exact float64
// |y|^2 (float32 only screens what cannot matter).
//
// This file is the translation unit: the stage headers in dependency order (one anonymous namespace, reopened by
// each), the channelized driver, and every extern "C" entry point of the unit.
#include "pfb_pdw_select.hpp"   // constants, keys, block_digit_pass, block_median, cached_median
#include "pfb_pdw_floor.hpp"    // noise floor: the full MSB-first radix select
#include "pfb_pdw_bracket.hpp"  // noise floor: sample gather, sample select, bracket pass
#include "pfb_pdw_finish.hpp"   // noise floor: candidate select of the bracket, patch of the provisional masks
#include "pfb_pdw_edges.hpp"    // mask, tile, scan and edge kernels
#include "pfb_pdw_pulse.hpp"    // ChanSrc, RawSrc, pdw_pulse_kernel
#include "pfb_pdw_scratch.hpp"  // error text, arenas, PdwCall, dispatch helpers
#include "pfb_pdw_stage.hpp"    // EdgeStage, edges_and_pulses, tile_words_for
#include "pfb_pdw_raw.hpp"      // raw kernels, RawStage, extract_raw
#include "pfb_dwell.hpp"        // dwell kernels, dwell_run, dwell_analyze_impl

extern "C" const char* pfb_pdw_last_error_detail(void) { return g_pdw_detail.c_str(); }
extern "C" int pfb_pdw_last_noise_floor_path(void) { return pfb::abi_guard([] { return g_pdw_path; }); }

extern "C" int pfb_pdw_release_workspace(int32_t device_id) {
  return pfb::abi_guard([&] {
  std::lock_guard<std::mutex> lock(g_ws_mutex);
  int prev = -1;
  (void)hipGetDevice(&prev);
  for (int d = 0; d < kMaxDevices; ++d) {
    if (device_id >= 0 && d != device_id) continue;
    for (Arena& a : g_ws[d]) {
      if (!a.p) continue;
      (void)hipSetDevice(d);
      (void)hipFree(a.p);
      a = Arena{};
    }
    if (g_pin[d].p) {
      (void)hipSetDevice(d);
      (void)hipHostFree(g_pin[d].p);
      g_pin[d] = HostPin{};
    }
  }
  if (prev >= 0) (void)hipSetDevice(prev);
  (void)hipGetLastError();
  return (int)PFB_OK;
  });
}

// ---- channelized (matlab/create_pdws_channelized.m:64-143) --------------------------------------------
// Nothing thrown (std::vector / std::string / std::mutex inside the drivers) crosses the C ABI: like
// pfb_pdw_release_workspace above, each entry point's body is the guard's, not indented again.
extern "C" int pfb_pdw_extract(const void* y_in, uint64_t frames, uint32_t M, uint32_t decimation, double fs_in,
                               double fc, double sample_start_time, double snr_threshold_db, uint32_t flags,
                               pfb_pdw* out, uint64_t capacity, uint64_t* count, double* noise_floor_out, uint32_t mem,
                               int32_t device_id, void* hip_stream) {
  return pfb::abi_guard([&]() -> int {
  if (!y_in || !count || M < 1 || decimation < 1 || frames < 1 || mem > PFB_MEM_DEVICE || (capacity && !out))
    return PFB_ERR_BAD_ARG;
  PdwCall call(device_id, hip_stream);
  if (call.rc != PFB_OK) return call.rc;
  const hipStream_t st = call.st;
  const long long F = (long long)frames;
  const int Mi = (int)M;
  // the transpose of MATLAB's own layout counts rows in an int; refused before anything is queued
  if ((flags & PFB_PDW_CHANNEL_MAJOR) && F >= (1ll << 31)) return PFB_ERR_UNSUPPORTED;
  const int tile_words = tile_words_for(F, Mi);
  const long long ntiles = (F + 64ll * tile_words - 1) / (64ll * tile_words);
  const long long words = ntiles * tile_words;  // whole tiles; the tail is identity-padded
  const int cgroups = (Mi + 63) / 64;
  const double fs = fs_in / (double)decimation;  // :62

  // sampled bracket: worth it once the data are several times the sample
  const bool sampled = F >= 8ll * kSampleRows;
  const long long stride = sampled ? F / kSampleRows : 1;
  const long long ns = F / stride;                                  // sampled rows
  const long long delta = (long long)std::ceil(2.5 * std::sqrt((double)ns)) + 2;  // 5 sigma of the median's sample rank
  const size_t expect = (size_t)((double)(2 * delta + 1) / (double)ns * (double)F);
  const unsigned cap = sampled ? (unsigned)std::min<size_t>((size_t)F, 2 * expect + 4096) : 0u;
  const long long key_ld = (ns + 63) / 64 * 64;  // sample keys per channel, padded to whole 256-byte lines

  const double gain = std::pow(10.0, snr_threshold_db / 10.0);  // :74-75 (dB applied to magnitude with /10)
  const int row_blocks = (int)std::min<long long>(1024, std::max<long long>(1, F / 256));
  const size_t cand_elems = std::max<size_t>((size_t)M * kCand, (size_t)M * cap);

  // Arena 0, described once (arena_layout measures with it, then places with it).  The order is part of the design:
  // d_below .. fin.ticket are consecutive because ONE memset zeroes them.
  float2 *own = nullptr, *fm = nullptr;  // the staged copy of a host matrix; the frame-major copy of a channel-major one
  unsigned *d_hist, *d_bucket, *d_cand_n, *d_flags, *d_und_n, *d_keys;
  unsigned long long *d_prefix, *d_rank, *d_below, *d_maxbelow, *d_und;
  double *d_cand, *d_thr;
  FinishShared fin{};
  EdgeStage e{};
  PDW_TRY(arena_layout(call.ws, [&](Arena& ws) {
    if (mem == PFB_MEM_HOST) own = take<float2>(ws, (size_t)F * M);
    if (flags & PFB_PDW_CHANNEL_MAJOR) fm = take<float2>(ws, (size_t)F * M);
    d_hist = take<unsigned>(ws, (size_t)M * 256);  // [channel][digit] of the full select
    d_bucket = take<unsigned>(ws, (size_t)M);
    d_prefix = take<unsigned long long>(ws, 2 * (size_t)M);  // low bracket ends, then the high ones
    d_rank = take<unsigned long long>(ws, (size_t)M);
    d_below = take<unsigned long long>(ws, (size_t)M);  // from here ...
    d_maxbelow = take<unsigned long long>(ws, (size_t)M);
    d_cand_n = take<unsigned>(ws, (size_t)M);
    d_flags = take<unsigned>(ws, 1);
    d_und_n = take<unsigned>(ws, 1);
    fin.hist = take<unsigned>(ws, (size_t)M * kFinishBins);
    fin.bucket_n = take<unsigned>(ws, (size_t)M);
    fin.lt_max = take<unsigned long long>(ws, (size_t)M);
    fin.ticket = take<unsigned>(ws, (size_t)M);  // ... to here: zeroed together
    fin.bucket = take<unsigned long long>(ws, (size_t)M * kFinishLds);
    d_und = take<unsigned long long>(ws, (size_t)kUndecided);
    d_cand = take<double>(ws, cand_elems);
    d_thr = take<double>(ws, M);
    d_keys = sampled ? take<unsigned>(ws, (size_t)M * key_ld) : nullptr;
    e = take_edge_stage(ws, words, ntiles, M, true);
  }));
  unsigned long long* const d_prefix_hi = d_prefix + M;
  const size_t zero_bytes = (size_t)(reinterpret_cast<char*>(fin.ticket + M) - reinterpret_cast<char*>(d_below));
  const float2* d_y = static_cast<const float2*>(y_in);
  if (own) {
    PDW_TRY(hipMemcpyAsync(own, y_in, (size_t)F * M * sizeof(float2), hipMemcpyHostToDevice, st));
    d_y = own;
  }
  if (fm) {
    // MATLAB's own layout (M columns of F frames): the pipeline walks rows of M channels, so the matrix is
    // transposed once into scratch (64 x 64 tiles through LDS, 512-byte reads and writes)
    PDW_TRY(pfb::launch_transpose_slab(d_y, (long long)M, (int)F, fm, (long long)M, 0, (int)sizeof(float2), st));
    d_y = fm;
  }

  std::vector<double> h_nf(M), h_binf(M);
  pfb_center_frequencies(M, fs_in, h_binf.data());  // :42, before fs is decimated
  PDW_TRY(hipMemcpyAsync(e.binf, h_binf.data(), M * sizeof(double), hipMemcpyHostToDevice, st));

  // ---- noise floor (:73), sampled bracket first.  Everything up to the edge totals is queued without a host sync:
  // the sample (gathered once, selected per channel), the bracket pass (which also leaves provisional masks), the
  // candidate select, thresholds on the device, the patch of the unclassified samples (or a full mask pass if the
  // device finds the provisional masks unusable), tile summaries and scan.  The host reads flags, medians and totals
  // in one go.
  if (sampled) {
    PDW_TRY(hipMemsetAsync(d_below, 0, zero_bytes, st));
    hipLaunchKernelGGL(pdw_sample_gather_kernel, dim3(cgroups, (unsigned)((ns + 63) / 64)), dim3(256), 0, st, d_y, ns, stride, Mi,
                       d_keys, key_ld);
    hipLaunchKernelGGL(pdw_sample_select_kernel, dim3(Mi), dim3(1024), 0, st, (const unsigned*)d_keys, ns, key_ld,
                       (unsigned long long)std::max<long long>(0, ns / 2 - delta),
                       (unsigned long long)std::min<long long>(ns - 1, ns / 2 + delta), d_prefix, d_prefix_hi);
    {
      const int row_groups = (int)((words * 64 + kBracketRows - 1) / kBracketRows);
      // many short-lived workgroups (one or two row groups each) beat a few long-lived ones here: 0.83 vs 0.92 ms
      const int gy = std::max(1, std::min(row_groups, 32 * 256 / cgroups));
      // small banks: several rows per wave-load (lanes per row = the power of two that holds M)
      auto kern = Mi > 32 ? pdw_bracket_kernel<64> : Mi > 16 ? pdw_bracket_kernel<32> : Mi > 8 ? pdw_bracket_kernel<16> : pdw_bracket_kernel<8>;
      hipLaunchKernelGGL(kern, dim3(cgroups, gy), dim3(256), 0, st, d_y, F, Mi,
                         (const unsigned long long*)d_prefix, (const unsigned long long*)d_prefix_hi, gain * gain, d_cand, cap,
                         d_cand_n, d_below, d_maxbelow, e.f0, e.f1, words, d_und, d_und_n, d_flags, row_groups);
    }
    {
      // parts per channel: enough workgroups to fill the chip, no more than a part's share is worth (>= 8192 candidates)
      const int parts = (int)std::max<long long>(1, std::min<long long>(std::min<long long>(16, 512 / Mi + 1), (long long)(expect / 8192)));
      hipLaunchKernelGGL(pdw_finish_hist_kernel, dim3(Mi, parts), dim3(1024), 0, st, F, (const double*)d_cand, cap,
                         (const unsigned*)d_cand_n, (const unsigned long long*)d_below, (const unsigned long long*)d_prefix,
                         (const unsigned long long*)d_prefix_hi, fin);
      hipLaunchKernelGGL(pdw_bracket_finish_kernel, dim3(Mi, parts), dim3(1024), 0, st, F, (const double*)d_cand, cap,
                         (const unsigned*)d_cand_n, (const unsigned long long*)d_below, (const unsigned long long*)d_maxbelow,
                         (const unsigned long long*)d_prefix, (const unsigned long long*)d_prefix_hi, gain, e.nf, d_flags, fin);
    }
    hipLaunchKernelGGL(pdw_thr_kernel, dim3((Mi + 255) / 256), dim3(256), 0, st, (const double*)e.nf, gain, d_thr, Mi);
    hipLaunchKernelGGL(pdw_patch_kernel, dim3(64), dim3(256), 0, st, d_y, Mi, (const double*)d_thr,
                       (const unsigned long long*)d_und, (const unsigned*)d_und_n, e.f0, e.f1);
    // (almost always a no-op: few workgroups, each striding over the words when it does run)
    hipLaunchKernelGGL(pdw_mask_kernel, dim3(cgroups, (unsigned)std::min<long long>((words + 3) / 4, 8192 / cgroups + 1)), dim3(256), 0, st,
                       d_y, F, Mi, (const double*)d_thr, e.f0, e.f1, words, (const unsigned*)d_flags);
    PDW_TRY(hipGetLastError());
    unsigned h_flags = 0;
    const int rc = edges_and_pulses(ChanSrc{d_y, Mi}, Mi, ntiles, tile_words, e, call, fs, fc, sample_start_time, flags, out,
                                    capacity, count, d_flags, &h_flags, h_nf.data());
    if (rc != kRedo) {
      g_pdw_path = h_flags == 0 ? 1 : 4;  // 4: flags 4 / 8 only spoiled the provisional masks, the device redid them
      if (rc == PFB_OK && noise_floor_out) std::memcpy(noise_floor_out, h_nf.data(), M * sizeof(double));
      return rc;
    }
  }
  g_pdw_path = sampled ? 3 : 2;
  {  // full radix select of rank F/2, then the exact finish
    const std::vector<unsigned long long> h_rank(M, (unsigned long long)(F / 2));
    std::vector<unsigned> h_bucket(M);
    int passes = 0;
    PDW_TRY(hipMemsetAsync(d_hist, 0, (size_t)M * 256 * sizeof(unsigned), st));
    PDW_TRY(hipMemsetAsync(d_prefix, 0, M * sizeof(unsigned long long), st));
    PDW_TRY(hipMemsetAsync(d_below, 0, M * sizeof(unsigned long long), st));
    PDW_TRY(hipMemsetAsync(d_maxbelow, 0, M * sizeof(unsigned long long), st));
    PDW_TRY(hipMemsetAsync(d_cand_n, 0, M * sizeof(unsigned), st));
    PDW_TRY(hipMemcpyAsync(d_rank, h_rank.data(), M * sizeof(unsigned long long), hipMemcpyHostToDevice, st));
    while (passes < 8) {
      hipLaunchKernelGGL(pdw_hist_kernel, dim3(cgroups, row_blocks), dim3(256), 0, st, d_y, F, 1ll, Mi, passes, d_prefix,
                         d_hist);
      hipLaunchKernelGGL(pdw_pick_kernel, dim3((Mi + 3) / 4), dim3(256), 0, st, Mi, passes, d_hist, d_prefix, d_rank,
                         d_bucket, d_below);
      ++passes;
      PDW_TRY(hipMemcpyAsync(h_bucket.data(), d_bucket, M * sizeof(unsigned), hipMemcpyDeviceToHost, st));
      PDW_TRY(hipStreamSynchronize(st));
      if (*std::max_element(h_bucket.begin(), h_bucket.end()) <= (unsigned)kCand) break;
    }
    hipLaunchKernelGGL(pdw_collect_kernel, dim3(cgroups, row_blocks), dim3(256), 0, st, d_y, F, Mi, passes, d_prefix, d_cand,
                       d_cand_n, d_maxbelow);
    hipLaunchKernelGGL(pdw_median_finish_kernel, dim3(Mi), dim3(256), 0, st, F, passes, d_cand, d_cand_n, d_prefix, d_rank,
                       d_maxbelow, e.nf);
    hipLaunchKernelGGL(pdw_thr_kernel, dim3((Mi + 255) / 256), dim3(256), 0, st, (const double*)e.nf, gain, d_thr, Mi);
    hipLaunchKernelGGL(pdw_mask_kernel, dim3(cgroups, (unsigned)std::min<long long>((words + 3) / 4, 65535)), dim3(256), 0, st, d_y, F, Mi,
                       (const double*)d_thr, e.f0, e.f1, words, (const unsigned*)nullptr);
    PDW_TRY(hipGetLastError());
    if (noise_floor_out) {
      PDW_TRY(hipMemcpyAsync(h_nf.data(), e.nf, M * sizeof(double), hipMemcpyDeviceToHost, st));
      PDW_TRY(hipStreamSynchronize(st));
      std::memcpy(noise_floor_out, h_nf.data(), M * sizeof(double));
    }
    return edges_and_pulses(ChanSrc{d_y, Mi}, Mi, ntiles, tile_words, e, call, fs, fc, sample_start_time, flags, out, capacity,
                            count);
  }
  });
}

// ---- raw stream (matlab/create_pdws.m:30-105) -------------------------------------------------------
extern "C" int pfb_pdw_extract_raw(const void* iq, uint64_t num_samples, uint32_t sample_format, uint32_t bit_width,
                                   double fs, double fc, double sample_start_time, double snr_threshold_db,
                                   double trailing_threshold_db, pfb_pdw* out, uint64_t capacity, uint64_t* count,
                                   double* noise_floor_out, uint32_t mem, int32_t device_id, void* hip_stream) {
  return pfb::abi_guard([&]() -> int {
  if (!iq || !count || num_samples < 2 || sample_format > PFB_FMT_CF32 || mem > PFB_MEM_DEVICE || (capacity && !out))
    return PFB_ERR_BAD_ARG;
  if (sample_format != PFB_FMT_CF32 && (bit_width < 1 || bit_width > 16)) return PFB_ERR_BAD_ARG;
  if (!(trailing_threshold_db <= snr_threshold_db)) return PFB_ERR_BAD_ARG;  // the masks assume lead >= trail
  PdwCall call(device_id, hip_stream);
  if (call.rc != PFB_OK) return call.rc;
  RawStage r{};
  const int rc = raw_stage(call, iq, num_samples, sample_format, bit_width, mem, r, [](Arena&) {});
  if (rc != PFB_OK) return rc;
  const RawParams p{fs, fc, sample_start_time, snr_threshold_db, trailing_threshold_db, out, capacity, count, noise_floor_out};
  return with_format(sample_format, [&](auto fmt) { return extract_raw<decltype(fmt)::value>(call, r, p); });
  });
}

// ---- dwell analysis (matlab/predict_event.m:53-121, cpp/usrp_predict_event.cpp:285-343) ----
extern "C" int pfb_dwell_analyze(const pfb_dwell_config* cfg, const void* iq, uint64_t num_samples, pfb_pdw* out,
                                 uint64_t capacity, uint64_t* count, pfb_dwell_stats* stats, void* hip_stream) {
  return pfb::abi_guard([&] { return dwell_analyze_impl(cfg, iq, num_samples, out, capacity, count, stats, hip_stream); });
}
