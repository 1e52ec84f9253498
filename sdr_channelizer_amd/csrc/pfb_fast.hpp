// pfb_fast.hpp -- the hot path: fused polyphase FIR + M-point FFT for gfx950.
//
// Replaces the arithmetic the reference delegates to dsp.Channelizer
// (/root/reference/matlab/channelizer_example.m:31,56,
//  /root/reference/matlab/create_pdws_channelized.m:33,57) together with the
// int->complex normalise (channelizer_example.m:18-21) and fftshift (:58).
//
// One workgroup = NT = D/CPT threads walks a contiguous run of frames.
//
//  FIR   Thread `tid` owns CPT adjacent columns c of the "row" view of the
//        stream (row r = the D samples whose newest member is frame r's newest
//        sample; a wave's load of one row is one contiguous, fully coalesced
//        segment).  Column c feeds branches p = (D-1-c) + D*ph, ph = 0..M/D-1,
//        whose taps h[p + M q] stay in registers, as does a sliding window of
//        the last W = M*P/D rows (already converted to float).  Every input
//        sample is loaded and converted exactly once per run.
//  FFT   A chunk of C frames of branch outputs goes through LDS as a mixed
//        radix (R0 x R1 [x R2]) Cooley-Tukey: each pass is an in-register
//        R-point DFT per thread, with one LDS exchange between passes.
//        Layout of the input of pass i inside a frame:
//            pos_i(n_i, item) = n_i*RS_i + item,  item = kk*S_i + rest
//        (S_i = prod R_{j>i}, K_i = prod R_{j<i}); RS_i / FS are padded so that
//        ds_read_b64 / ds_write_b64 are bank-conflict free (tools/fft_plan_model.py
//        checks the formulas and the padding for every instantiated plan).
//  OUT   The last pass leaves thread `kk` with channels kk + K*k: for each k the
//        threads of a frame store M/R_last contiguous complex64.
//
// No MFMA: 4P + 5 log2 M flop per sample against 12 B of HBM traffic -- the
// kernel is HBM-bound.
//
// The arithmetic above (pfb_cplx.hpp: packed complex arithmetic and DFTs; pfb_fast_cfg.hpp: plan, row loads, tables;
// pfb_fast_core.hpp: FIR, FFT passes, stores) is shared by several SCHEDULES (who computes which frames when;
// PFB_OPT_SCHEDULE, bit-identical outputs per shape).  Each has its body, its kernel, its predicates and its launcher in
// one header:
//   0 (A)  pfb_fast_sliding.hpp  one sliding run per workgroup, FIR and FFT by the same threads   (M = 256, small and mixed-radix banks)
//   2 (C)  pfb_fast_tiles.hpp    one chunk per wave, adjacent chunks per workgroup  (access-shape study; channel-major fallback)
//   3 (D)  pfb_fast_halo.hpp     short runs whose halo rows are shared through LDS
//   4 (F)  pfb_fast_halo.hpp     D with a FIR wave and an FFT wave per run          (M = 64 default)
//   6 (T)  pfb_fast_teams.hpp    a FIR team and an FFT team per workgroup           (M = 1024 / 560 default)
//   7 (H)  pfb_fast_pairs.hpp    a FIR wave and an FFT wave per long sliding run    (M = 56 default)
//   8 (C') pfb_fast_tiles.hpp    channel-major only: short sliding runs, each chunk transposed in its LDS buffer, the
//          workgroup's tile written as 256-512-byte runs per channel       (channel-major default of the single-wave plans)
//   9      channel-major only, host side (pfb_api.cpp): frame-major slabs + pfb_transpose_slab_kernel
//  11 (P)  pfb_fast_overlap.hpp  A software-pipelined inside the wave: next chunk's FIR next to this chunk's first FFT pass,
//          two LDS chunk buffers, rows two chunks ahead                    (M = 128 D = 64 default)
//  13 (W)  pfb_fast_twin.hpp     independent workgroups of a few waves, a frame per wave and chunk, all passes of a frame by
//          one wave                                                        (variant 3 of M = 1024 int16)
//  small banks (M < 64): pfb_fast_seg.hpp, SegKernel
// select_fast below resolves a call -- the KernelParams the launch policy (pfb_launch_policy.h) filled -- to the one kernel
// entry it runs: a pure function, no HIP call.  launch_blocks (pfb_fast_cfg.hpp) launches that entry, and the handle keeps
// it (pfb_last_entry), so what ran is on record next to what was asked for.
// Numbers 1, 5, 10 and 12 were studies that lost to the above (persistent strided chunks, persistent wave pairs, the team
// kernel transposing through scratch tiles, the PDW screen fused into the last pass); their measurements are in
// DESIGN.md sections 5 and 9, their code is gone.
#pragma once

#include "pfb_fast_halo.hpp"
#include "pfb_fast_overlap.hpp"
#include "pfb_fast_pairs.hpp"
#include "pfb_fast_seg.hpp"
#include "pfb_fast_sliding.hpp"
#include "pfb_fast_teams.hpp"
#include "pfb_fast_tiles.hpp"
#include "pfb_fast_twin.hpp"

namespace pfb {

// Plans with a fused channel-major instantiation.  The 16-wave plans and the three-pass plans on chunks of 4 or 2 frames
// (32- / 16-byte runs per channel) have none: a channel-major handle on them goes by frame-major slabs + the transpose
// kernel, 1.5-5x faster than their fused stores on every such plan measured (profiles/r04_channel_major_routes.txt)
template <class K>
constexpr bool kChannelMajorOk = K::NT < 1024 && !(K::NP == 3 && K::C <= 4);

// Every forced combination a plan lacks falls through to the next block, at the end to the plain sliding runs: the
// entry's schedule and tag say where it ended.
template <class K>
KernelEntry select_fast(const KernelParams& p) {
  if (p.layout == PFB_LAYOUT_CHANNEL_MAJOR) {  // schedules 8, 2 and 0; the others are frame-major tuning
    if constexpr (kChannelMajorOk<K>) {
      if constexpr (K::NT == 64) {
        if constexpr (kTileTOk<K, 4, 2>) {  // short runs transposed in LDS: schedule 8, the default where the plan allows
          if (p.schedule == 8 || p.schedule < 0) {
            // tile_waves = waves per workgroup, frames_per_block / C = chunks per wave
            const int key = p.tile_waves * 100 + (p.schedule == 8 ? p.frames_per_block / K::C : 0);
            switch (key) {
              case 401: if constexpr (kTileTOk<K, 4, 1>) return tile_t_entry<K, 4, 1>(p); break;
              case 801: if constexpr (kTileTOk<K, 8, 1>) return tile_t_entry<K, 8, 1>(p); break;
              case 202: if constexpr (kTileTOk<K, 2, 2>) return tile_t_entry<K, 2, 2>(p); break;
              case 402: if constexpr (kTileTOk<K, 4, 2>) return tile_t_entry<K, 4, 2>(p); break;
              case 104: if constexpr (kTileTOk<K, 1, 4>) return tile_t_entry<K, 1, 4>(p); break;
              case 204: if constexpr (kTileTOk<K, 2, 4>) return tile_t_entry<K, 2, 4>(p); break;
              default: break;
            }
            // measured best: 4 waves x 2 chunks on M = 56, 64, 128; 2 waves x 4 chunks on M = 32
            if constexpr (K::M <= 32 && kTileTOk<K, 2, 4>) return tile_t_entry<K, 2, 4>(p);
            return tile_t_entry<K, 4, 2>(p);
          }
        }
        // one chunk per wave, NWV adjacent chunks per workgroup: the workgroup writes NWV * C consecutive frames of
        // every channel at about the same time, which L2 merges into runs a sliding wave never produces by itself
        // (measured +17 ... +70 % over sliding runs; 16 waves win up to M = 64, 8 above)
        if (p.schedule == 2 || p.schedule < 0) {
          const int nwv = p.schedule < 0 ? (K::M <= 64 ? 16 : 8) : p.tile_waves;
          if constexpr (16 * sizeof(float2) * K::LDS_ELEMS <= 160 * 1024) {
            if (nwv == 16) return tile_entry<K, 16, true>(p);
          }
          return tile_entry<K, 8, true>(p);
        }
      }
      return sliding_entry<K, true>(p);
    } else {
      return KernelEntry{};  // no kernel: find_fast_kernel never hands this plan to a channel-major handle
    }
  }
  // (measured on cfg3, cfg5 and M=56 too: slower than their sliding runs, so only the M=64 kernels carry it)
  if constexpr (K::NT == 64 && K::NP == 2 && !K::PINGPONG) {  // wave pairs over long sliding runs
    if (p.schedule == 7) {
      // 8 pairs (16 waves, 128 registers each) where the roles fit that budget -- the shapes whose single-wave
      // kernel already runs 4 waves per SIMD -- otherwise 6 pairs (168 registers); tile_waves = 4 asks for 4
      constexpr size_t kPair = sizeof(float2) * 2 * K::BUF;
      // (workgroups of ONE or TWO pairs -- a barrier that couples 2 or 4 waves, 8 or 4 workgroups per CU -- measured: cfg2
      // 0.61-0.65 against 0.72 for its 8 halo-sharing pairs, M = 56 0.58-0.61 against 0.62, cfg5 0.44-0.49 against 0.68;
      // profiles/r03_tiny_pair_workgroups_ab.txt; four pairs at two workgroups per CU: M = 56 0.575-0.605 against 0.608)
      if (p.tile_waves == 4) return pairs_sliding_entry<K, 4, 2>(p);
      if constexpr (K::MIN_WAVES >= 4 && 8 * kPair <= 160 * 1024) {
        if (p.tile_waves >= 8) return pairs_sliding_roles_entry<K, 8, 4>(p);
      }
      return pairs_sliding_roles_entry<K, 6, 3>(p);
    }
  }
  if constexpr (kOverlapOk<K>) {  // sliding runs, FIR of the next chunk scheduled into the FFT of this one
    if (p.schedule == 11) return overlap_entry<K>(p);
  }
  if constexpr (kTwinOk<K>) {  // independent workgroups, a frame per wave and chunk
    if (p.schedule == 13) {
      if (p.layout != PFB_LAYOUT_FRAME_MAJOR) return KernelEntry{};  // no kernel
      return twin_entry<K>(p);
    }
  }
  if constexpr (kTeamsOk<K>) {  // FIR team + FFT team
    if (p.schedule == 6) return teams_entry<K>(p);
  }
  if constexpr (K::NT == 64 && K::NP == 2 && !K::PINGPONG && K::M == 64 && K::C == 8) {
    if (p.schedule == 4) {  // FIR / FFT wave pairs: tile_waves = pairs per workgroup, frames_per_block = run length
      const int key = p.tile_waves * 1000 + p.frames_per_block;
      if constexpr (K::FMT == PFB_FMT_INT16_IQ && K::M == 64 && K::P == 12) {  // tuning sweep set (cfg2 only, keeps build time sane)
        switch (key) {
          case 4064: return paired_entry<K, 4, 64, 4>(p);
          case 5064: return paired_entry<K, 5, 64, 5>(p);   // 10-wave workgroups, 5 waves per SIMD
          case 8048: return paired_entry<K, 8, 48, 4>(p);
          case 8128: return paired_entry<K, 8, 128, 4>(p);
          default: break;
        }
      }
      // the tuned shape is 8 pairs x 64 frames (16 waves, 512 frames per workgroup); instantiations whose
      // LDS image does not fit 8 pairs take 4
      constexpr size_t kPair = sizeof(float2) * 2 * K::BUF, kSlot = sizeof(typename SampleT<K::FMT>::raw_t) * (K::W - 1) * K::D;
      // (the shape a call runs by default has the output type and the store kind compiled in; the sweep set above and
      // the 4-pair option test the flags per store)
      if constexpr (8 * kPair + 9 * kSlot <= 160 * 1024) {
        if (p.tile_waves == 4) return paired_entry<K, 4, 64, 2>(p);
        return paired_roles_entry<K, 8, 64, 4>(p);
      } else {
        return paired_roles_entry<K, 4, 64, 2>(p);
      }
    }
  }
  if constexpr (K::NT == 64 && K::C == 8 && !K::PINGPONG) {
    if (p.schedule == 3) {  // shared-halo sliding windows: tile_waves runs of frames_per_block frames
      const int key = p.tile_waves * 1000 + p.frames_per_block;
      KernelEntry e;
      if (key == 8024) e = shared_entry<K, 8, 24>(p);
      else if (key == 8032) e = shared_entry<K, 8, 32>(p);
      else if (key == 8064) e = shared_entry<K, 8, 64>(p);
      else if (key == 4064) e = shared_entry<K, 4, 64>(p);
      else {
        bool done = false;
        if constexpr (K::FMT == PFB_FMT_INT16_IQ && K::M == 64 && K::P == 12) {  // tuning sweep set (cfg2 only, keeps build time sane)
          switch (key) {
            case 4032: e = shared_entry<K, 4, 32>(p); done = true; break;
            case 8048: e = shared_entry<K, 8, 48>(p); done = true; break;
            case 16024: e = shared_entry<K, 16, 24>(p); done = true; break;
            default: break;
          }
        }
        if (!done) e = shared_entry<K, 8, 24>(p);  // any other shape: the tuned default
      }
      if (e.kernel) return e;  // (no tile fits this sample format: the plain sliding runs below)
    }
  }
  if constexpr (K::NT == 64 && K::M == 64 && K::FMT == PFB_FMT_INT16_IQ && K::C == 8 && K::P == 12) {  // access-shape study schedules (cfg2 only)
    if (p.schedule == 2) {  // one chunk per wave, tile_waves adjacent chunks per workgroup
      if (p.tile_waves == 1) return tile_entry<K, 1>(p);
      return tile_entry<K, 8>(p);
    }
  }
  if constexpr (kMagStagedOk<K>) {
    if (wants_magnitude(p) && (reinterpret_cast<uintptr_t>(p.out) & 15) == 0) return sliding_entry<K, false, true>(p);
  }
  return wants_magnitude(p) ? sliding_entry<K, false, false, 1>(p) : sliding_entry<K, false, false, 0>(p);
}

}  // namespace pfb
