// pfb_fast_tiles.hpp -- schedules 2 (C) and 8 (C') of the fused kernel (pfb_fast.hpp): a chunk per wave, and the channel-major
// tile of short sliding runs transposed in LDS.
#pragma once

#include "pfb_fast_core.hpp"

namespace pfb {

template <class K, bool CM = false>
struct Tiles : FastKernel<K, CM> {
  using F = FastKernel<K, CM>;
  using typename F::raw_t; using typename F::Consts; using typename F::RowFetch;
  using F::cvt; using F::setup; using F::finish_rows; using F::tslot_frame;
  static constexpr int M = K::M, P = K::P, D = K::D, CPT = K::CPT, C = K::C, W = K::W, OS = K::OS, NT = K::NT, NW = F::NW;

  // all NW rows (halo included) of one chunk: schedule C's unit of work
  PFB_DEV void load_chunk(const KernelParams& p, long long chunk, int c0, raw_t (&raw)[NW][CPT]) {
    const long long f0 = chunk * C;
    const long long s_first = (f0 - (W - 1)) * D + p.base;
    const bool interior = p.vec_ok && s_first >= 0 && (f0 + C <= p.frames);
    const raw_t* ptr = static_cast<const raw_t*>(p.in) + s_first;  // uniform; only used when interior
    if (interior) {
#pragma unroll
      for (int i = 0; i < NW; ++i) F::template load_row<true>(p, ptr, 0, i, c0, raw[i]);
    } else {
#pragma unroll
      for (int i = 0; i < NW; ++i) F::template load_row<false>(p, ptr, f0 - (W - 1) + i, i, c0, raw[i]);
    }
  }

  // ---- schedule C: one chunk per wave, NWV adjacent chunks per (non-persistent) workgroup ---------
  // The dispatcher hands out workgroups in order, so the chip sweeps the stream as one compact,
  // monotonically advancing window (the fastest shape in tools/membench2); the W-1 halo rows a wave
  // shares with its neighbours in the workgroup are served by that CU's L1, and the ones shared with
  // the previous workgroup by the XCD's L2 (consecutive tiles are remapped onto one XCD).
  template <int NWV>
  PFB_DEV void run_tile(const KernelParams& p, float2* lds_all) {
    static_assert(NT == 64, "one wave per chunk");
    const int wave = threadIdx.x >> 6, tid = threadIdx.x & 63;
    const int c0 = tid * CPT;
    const long long nchunks = (p.frames + C - 1) / C;
    long long tile = blockIdx.x;
    tile = xcd_remap_block(tile, gridDim.x, p.xcd_remap);
    const long long chunk = tile * NWV + wave;
    if (chunk >= nchunks) return;
    float2* lds = lds_all + wave * K::LDS_ELEMS;
    Consts k;
    setup(p, tid, k);
    raw_t raw[NW][CPT];
    load_chunk(p, chunk, c0, raw);
    v2f x[NW][CPT];
#pragma unroll
    for (int i = 0; i < NW; ++i)
#pragma unroll
      for (int cc = 0; cc < CPT; ++cc) x[i][cc] = cvt(raw[i][cc]);
    F::template fir_fft_store<true>(p, k, x, lds, tid, chunk * C);
  }

  // ---- schedule C', channel-major: short sliding runs whose output is transposed in LDS ----------------------
  // Channel-major rows are out_ld elements apart, so the last pass's natural store (a few frames of 8 channels
  // per instruction) scatters 64-byte pieces over 8 DRAM pages -- tools/membench5: 4.6 TB/s write-only, 1.2 TB/s
  // when out_ld is a power of two.  Here wave w of the workgroup slides over CPW chunks, each chunk ends
  // transposed in its own LDS slot (last_pass_transposed: no extra buffer), and after one barrier the workgroup
  // writes the NWV * CPW * C frames of every column as one run: an instruction is 256-512 contiguous bytes of
  // one or two columns (5.5 TB/s in the same microbenchmark, whatever out_ld is).
  static constexpr int TSLOT = K::LDS_ELEMS + ((C + 32 - K::LDS_ELEMS % 32) % 32);  // = C (mod 32): slots on distinct banks

  template <bool INTERIOR, int CPW>
  PFB_DEV void tile_t_impl(const KernelParams& p, float2* slots, int tid, long long f_begin) {
    const int c0 = tid * CPT;
    Consts k;
    setup(p, tid, k);
    const raw_t* run_ptr = static_cast<const raw_t*>(p.in) + ((f_begin - (W - 1)) * D + p.base);
    v2f x[NW][CPT];
    raw_t raw[C][CPT];
#pragma unroll
    for (int i = 0; i < W - 1; ++i) {
      raw_t t[CPT];
      F::template load_row<INTERIOR>(p, run_ptr, f_begin - (W - 1) + i, i, c0, t);
#pragma unroll
      for (int cc = 0; cc < CPT; ++cc) x[i][cc] = cvt(t[cc]);
    }
    RowFetch rf;
    F::template begin_rows<INTERIOR>(run_ptr, rf);
    F::template load_rows<INTERIOR>(p, run_ptr, f_begin, W - 1, c0, raw, rf);
#pragma unroll
    for (int ci = 0; ci < CPW; ++ci) {
      finish_rows(c0, raw, rf);
#pragma unroll
      for (int t = 0; t < C; ++t)
#pragma unroll
        for (int cc = 0; cc < CPT; ++cc) x[W - 1 + t][cc] = cvt(raw[t][cc]);
      if (ci + 1 < CPW) F::template load_rows<INTERIOR>(p, run_ptr, f_begin + (ci + 1) * C, W - 1 + (ci + 1) * C, c0, raw, rf);
      F::template fir_fft_store<true, true>(p, k, x, slots + ci * TSLOT, tid, f_begin + ci * C);
      if (ci + 1 < CPW) {
#pragma unroll
        for (int i = 0; i < W - 1; ++i)
#pragma unroll
          for (int cc = 0; cc < CPT; ++cc) x[i][cc] = x[i + C][cc];
      }
    }
  }

  template <int NWV, int CPW>
  PFB_DEV void run_tile_t(const KernelParams& p, float2* lds_all) {
    static_assert(NT == 64 && CM, "one wave per run, channel-major output");
    constexpr int RL = NWV * CPW * C, NTH = 64 * NWV, IT = (M * RL) / NTH;
    static_assert((M * RL) % NTH == 0 && (RL & (RL - 1)) == 0 && RL % 32 == 0, "whole flush iterations over 32-frame blocks");
    const int wave = threadIdx.x >> 6, tid = threadIdx.x & 63;
    long long tile = blockIdx.x;
    tile = xcd_remap_block(tile, gridDim.x, p.xcd_remap);
    const long long tf0 = tile * RL;
    if (tf0 >= p.frames) return;  // workgroup-uniform
    const long long f_begin = tf0 + (long long)wave * (CPW * C);
    if (f_begin < p.frames) {
      float2* slots = lds_all + wave * (CPW * TSLOT);
      const bool interior = p.vec_ok && ((f_begin - (W - 1)) * D + p.base >= 0) && (f_begin + CPW * C <= p.frames);
      if (interior) tile_t_impl<true, CPW>(p, slots, tid, f_begin);
      else tile_t_impl<false, CPW>(p, slots, tid, f_begin);
    }
    team_sync<NWV == 1>();
    const bool mag = (p.flags & PFB_FLAG_MAGNITUDE) != 0;
    const v2f* t2 = reinterpret_cast<const v2f*>(lds_all);
    constexpr int HALF = IT > 8 ? 2 : 1;  // at most 8 values in flight per lane
#pragma unroll
    for (int h = 0; h < HALF; ++h) {
      v2f v[IT / HALF];
#pragma unroll
      for (int i = 0; i < IT / HALF; ++i) {
        const int e = (h * (IT / HALF) + i) * NTH + (int)threadIdx.x, col = e / RL, fr = e % RL;
        v[i] = t2[(fr / C) * TSLOT + col * C + tslot_frame(col, fr % C)];
      }
#pragma unroll
      for (int i = 0; i < IT / HALF; ++i) {
        const int e = (h * (IT / HALF) + i) * NTH + (int)threadIdx.x, col = e / RL, fr = e % RL;
        const long long f = tf0 + fr;
        if (f < p.frames) {
          const long long idx = (long long)col * p.out_ld + p.out_frame0 + f;
          if (mag) reinterpret_cast<float*>(p.out)[idx] = mag_out(v[i].x, v[i].y, p.flags);
          else store_c64(p.out + idx, v[i], p.nontemporal);
        }
      }
    }
  }
};

template <class K, int NWV, bool CM = false>
__global__ void __launch_bounds__(64 * NWV) pfb_tile_kernel(const KernelParams p) {
  carry_history(p, SampleT<K::FMT>::kBytes, 64 * NWV);
  __shared__ float2 lds[NWV * K::LDS_ELEMS];
  Tiles<K, CM>::template run_tile<NWV>(p, lds);
}

template <class K, int NWV, bool CM = false>
KernelEntry tile_entry(const KernelParams& p) {
  static constexpr KernelTag tag = kernel_tag<NWV>("tile", {CM});
  return entry_for(&pfb_tile_kernel<K, NWV, CM>, 2, tag.s, p, (long long)NWV * K::C, 64 * NWV);
}

template <class K, int NWV, int CPW>
__global__ void __launch_bounds__(64 * NWV) pfb_tile_t_kernel(const KernelParams p) {
  carry_history(p, SampleT<K::FMT>::kBytes, 64 * NWV);
  __shared__ float2 lds[NWV * CPW * Tiles<K, true>::TSLOT];
  Tiles<K, true>::template run_tile_t<NWV, CPW>(p, lds);
}

template <class K, int NWV, int CPW>
KernelEntry tile_t_entry(const KernelParams& p) {
  static constexpr KernelTag tag = kernel_tag<NWV, CPW>("tile_t");
  return entry_for(&pfb_tile_t_kernel<K, NWV, CPW>, 8, tag.s, p, (long long)NWV * CPW * K::C, 64 * NWV);
}

// the transposed tile: single-wave two-pass plans whose chunk buffer holds the transposed chunk, rows of whole
// 32-frame blocks
// (the slot swizzle of tslot_frame: power-of-two chunk and lane groups)
template <class K>
constexpr bool kTileSlotOk = 16 % K::C == 0 && ((K::M / K::R(K::NP - 1)) >= 16 || 16 % (K::M / K::R(K::NP - 1)) == 0) &&
                             K::C % ((K::M / K::R(K::NP - 1)) >= 16 ? 1 : 16 / (K::M / K::R(K::NP - 1))) == 0;

template <class K, int NWV, int CPW>
constexpr bool kTileTOk = K::NT == 64 && K::NP == 2 && !K::PINGPONG && kTileSlotOk<K> && K::M * K::C <= K::LDS_ELEMS &&
                          (NWV * CPW * K::C) % 32 == 0 && ((NWV * CPW * K::C) & (NWV * CPW * K::C - 1)) == 0 &&
                          (K::M * NWV * CPW * K::C) % (64 * NWV) == 0;

}  // namespace pfb
