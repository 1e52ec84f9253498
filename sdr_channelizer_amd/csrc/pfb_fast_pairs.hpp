// pfb_fast_pairs.hpp -- schedule 7 (H) of the fused kernel (pfb_fast.hpp): a FIR wave and an FFT wave per long sliding run.
#pragma once

#include "pfb_fast_core.hpp"

namespace pfb {

// ---- schedule H: wave pairs over long sliding runs ------------------------------------------------------
// Schedule F's split of the work (a FIR wave and an FFT wave per run, an LDS double buffer between them, one
// workgroup barrier per chunk) without its halo sharing: every pair slides over its own long run of
// frames_per_block frames like schedule A and re-reads only its own W-1 halo rows once.  For the shapes whose
// single-wave kernel needs close to 200 registers (cfg5: 24 taps and a 31-row window per lane plus a radix-16
// pass) this halves the registers per wave and doubles the waves per CU; the runs are a runtime loop, so
// they can be long.
template <class K>
struct PairSlide : FastKernel<K> {
  using F = FastKernel<K>;
  using typename F::raw_t; using typename F::Consts; using typename F::RowFetch;
  using F::cvt; using F::setup; using F::finish_rows; using F::fir_to_lds; using F::fft_from_lds;
  static constexpr int M = K::M, P = K::P, D = K::D, CPT = K::CPT, C = K::C, W = K::W, OS = K::OS, NT = K::NT, NW = F::NW;

  template <bool INTERIOR>
  PFB_DEV void pair_fir_run(const KernelParams& p, const Consts& k, float2* bufs, long long f_begin, int nch) {
    const int tid = threadIdx.x & 63;
    const int c0 = tid * CPT;
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
    for (int ci2 = 0; ci2 < nch; ci2 += 2) {
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        const int ci = ci2 + u;
        finish_rows(c0, raw, rf);
#pragma unroll
        for (int t = 0; t < C; ++t)
#pragma unroll
          for (int cc = 0; cc < CPT; ++cc) x[W - 1 + t][cc] = cvt(raw[t][cc]);
        if (ci + 1 < nch) {
          const long long rel = (long long)(ci + 1) * C + (W - 1);
          F::template load_rows<INTERIOR>(p, run_ptr, f_begin + (long long)(ci + 1) * C, rel, c0, raw, rf);
        }
        fir_to_lds(k, x, bufs + u * K::BUF, tid);
#pragma unroll
        for (int i = 0; i < W - 1; ++i)
#pragma unroll
          for (int cc = 0; cc < CPT; ++cc) x[i][cc] = x[i + C][cc];
        __syncthreads();  // chunk ci handed to the FFT wave
      }
    }
    __syncthreads();      // the FFT wave's last step
  }

  // MAGSEL / NTSEL: PFB_FLAG_MAGNITUDE and KernelParams.nontemporal as the host saw them (pass<>), -1 = tested per store
  template <int NPAIR, int MAGSEL = -1, int NTSEL = -1>
  PFB_DEV void run_pairs_sliding(const KernelParams& p, float2* lds_fft) {
    static_assert(NT == 64 && K::NP == 2 && !K::PINGPONG, "one wave per role, two in-place passes");
    const int wave = threadIdx.x >> 6, tid = threadIdx.x & 63;
    const bool fir_role = wave < NPAIR;
    const int pair = fir_role ? wave : wave - NPAIR;
    long long blk = blockIdx.x;
    blk = xcd_remap_block(blk, gridDim.x, p.xcd_remap);
    const long long f_begin = (blk * NPAIR + pair) * (long long)p.frames_per_block;
    const int nch = p.frames_per_block / C;  // even (host rounds); pairs past the end of the stream idle through the barriers
    float2* bufs = lds_fft + pair * 2 * K::BUF;
    Consts k;
    setup(p, tid, k);
    if (fir_role) {
      const bool interior = p.vec_ok && ((f_begin - (W - 1)) * D + p.base >= 0) && (f_begin + p.frames_per_block <= p.frames);
      if (f_begin >= p.frames) {
        for (int s = 0; s <= nch; ++s) __syncthreads();
      } else if (interior) {
        pair_fir_run<true>(p, k, bufs, f_begin, nch);
      } else {
        pair_fir_run<false>(p, k, bufs, f_begin, nch);
      }
    } else if (f_begin + p.frames_per_block <= p.frames) {  // every frame of the run exists: unconditional stores
#pragma unroll 1
      for (int s = 0; s <= nch; ++s) {
        if (s >= 1)
          F::template fft_from_lds<true, MAGSEL, NTSEL>(p, k, bufs + ((s - 1) & 1) * K::BUF, tid, f_begin + (long long)(s - 1) * C);
        __syncthreads();
      }
    } else {
#pragma unroll 1
      for (int s = 0; s <= nch; ++s) {
        if (s >= 1 && f_begin < p.frames)
          F::template fft_from_lds<false, MAGSEL, NTSEL>(p, k, bufs + ((s - 1) & 1) * K::BUF, tid, f_begin + (long long)(s - 1) * C);
        __syncthreads();
      }
    }
  }
};

template <class K, int NPAIR, int MINW, int MAGSEL = -1, int NTSEL = -1>
__global__ void __launch_bounds__(128 * NPAIR, MINW) pfb_pairs_sliding_kernel(const KernelParams p) {
  carry_history(p, SampleT<K::FMT>::kBytes, 128 * NPAIR);
  __shared__ float2 lds_fft[NPAIR * 2 * K::BUF];
  PairSlide<K>::template run_pairs_sliding<NPAIR, MAGSEL, NTSEL>(p, lds_fft);
}

template <class K, int NPAIR, int MINW, int MAGSEL = -1, int NTSEL = -1>
KernelEntry pairs_sliding_entry(const KernelParams& p) {
  static constexpr KernelTag tag = kernel_tag<NPAIR, MINW>("pairs_sliding", {false, false, MAGSEL, NTSEL});
  return entry_for(&pfb_pairs_sliding_kernel<K, NPAIR, MINW, MAGSEL, NTSEL>, 7, tag.s, p, (long long)NPAIR * p.frames_per_block, 128 * NPAIR);
}

// with the call's output type and store kind compiled in (with_store_roles, pfb_fast_cfg.hpp)
template <class K, int NPAIR, int MINW>
KernelEntry pairs_sliding_roles_entry(const KernelParams& p) {
  return with_store_roles(p, [&]<int MAGSEL, int NTSEL>() { return pairs_sliding_entry<K, NPAIR, MINW, MAGSEL, NTSEL>(p); });
}

}  // namespace pfb
