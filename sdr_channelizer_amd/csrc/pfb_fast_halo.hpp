// pfb_fast_halo.hpp -- schedules 3 (D) and 4 (F) of the fused kernel (pfb_fast.hpp): short runs whose halo rows are shared
// through LDS slots; F gives a run's FIR and FFT to a pair of waves.
#pragma once

#include "pfb_fast_core.hpp"

namespace pfb {

template <class K>
struct HaloShare : FastKernel<K> {
  using F = FastKernel<K>;
  using typename F::raw_t; using typename F::Consts;
  using F::cvt; using F::setup; using F::fir_to_lds; using F::fft_from_lds;
  static constexpr int M = K::M, P = K::P, D = K::D, CPT = K::CPT, C = K::C, W = K::W, OS = K::OS, NT = K::NT, NW = F::NW;

  // ---- schedule D: sliding windows with the halo shared inside the workgroup -------------------------
  // A workgroup of NWV waves covers NWV*L consecutive frames, wave w the L frames [w*L, (w+1)*L) with its
  // own register window.  Short runs keep the whole chip inside one dense, in-order sweeping window
  // (DRAM rows are finished while open: tools/membench2), but a short run's W-1 halo rows would be
  // fetched from HBM twice -- by this wave now and by its predecessor, as the tail of ITS run, a few
  // microseconds later.  So each wave PUBLISHES the raw halo rows it loads in an LDS slot, and its
  // predecessor takes the last W-1 rows of its run from that slot instead of from memory: every row
  // is fetched once, except the W-1 rows at workgroup boundaries ((W-1)/(NWV*L) extra reads).
  template <bool INTERIOR, int NWV, int L>
  PFB_DEV void shared_impl(const KernelParams& p, const Consts& k, float2* lds, raw_t* halo_mine,
                           const raw_t* halo_next, int wave, long long f_begin) {
    static_assert(L % C == 0 && L >= W - 1, "runs are whole chunks and at least one halo long");
    constexpr int TAIL0 = L - (W - 1);  // first row of the run that the successor publishes
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
      for (int cc = 0; cc < CPT; ++cc) {
        x[i][cc] = cvt(t[cc]);
        if constexpr (INTERIOR) {
          if (!(K::LANES < NT) || tid < K::LANES) halo_mine[i * D + c0 + cc] = t[cc];
        }
      }
    }
#pragma unroll
    for (int t = 0; t < C; ++t) F::template load_row<INTERIOR>(p, run_ptr, f_begin + t, W - 1 + t, c0, raw[t]);
    __syncthreads();  // every wave's halo slot is published
    const bool tail_from_lds = INTERIOR && (wave < NWV - 1);
#pragma unroll
    for (int ci = 0; ci < L / C; ++ci) {
#pragma unroll
      for (int t = 0; t < C; ++t) {
        const int r = ci * C + t;
        if (r >= TAIL0 && tail_from_lds) {
#pragma unroll
          for (int cc = 0; cc < CPT; ++cc)
            x[W - 1 + t][cc] = cvt(halo_next[(r - TAIL0) * D + ((K::LANES < NT && c0 >= D) ? 0 : c0 + cc)]);
        } else {
#pragma unroll
          for (int cc = 0; cc < CPT; ++cc) x[W - 1 + t][cc] = cvt(raw[t][cc]);
        }
      }
      if (ci + 1 < L / C) {  // prefetch the next chunk's rows (those not coming from LDS)
#pragma unroll
        for (int t = 0; t < C; ++t) {
          const int r = (ci + 1) * C + t;
          if (!(r >= TAIL0 && tail_from_lds)) F::template load_row<INTERIOR>(p, run_ptr, f_begin + r, W - 1 + r, c0, raw[t]);
        }
      }
      F::template fir_fft_store<true>(p, k, x, lds, tid, f_begin + ci * C);
#pragma unroll
      for (int i = 0; i < W - 1; ++i)
#pragma unroll
        for (int cc = 0; cc < CPT; ++cc) x[i][cc] = x[i + C][cc];
    }
  }

  template <int NWV, int L>
  PFB_DEV void run_shared(const KernelParams& p, float2* lds_fft, raw_t* lds_halo) {
    static_assert(NT == 64, "one wave per run");
    const int wave = threadIdx.x >> 6, tid = threadIdx.x & 63;
    long long blk = blockIdx.x;
    blk = xcd_remap_block(blk, gridDim.x, p.xcd_remap);
    const long long f_blk = blk * (long long)(NWV * L);
    const long long f_begin = f_blk + (long long)wave * L;
    Consts k;
    setup(p, tid, k);
    float2* lds = lds_fft + wave * K::LDS_ELEMS;
    raw_t* halo_mine = lds_halo + wave * ((W - 1) * D);
    const raw_t* halo_next = lds_halo + (wave + 1) * ((W - 1) * D);
    // workgroup-uniform: every row of every run lies inside `in`, whole runs only, aligned vectors
    const bool interior = p.vec_ok && ((f_blk - (W - 1)) * D + p.base >= 0) && (f_blk + NWV * L <= p.frames);
    if (interior) shared_impl<true, NWV, L>(p, k, lds, halo_mine, halo_next, wave, f_begin);
    else shared_impl<false, NWV, L>(p, k, lds, halo_mine, halo_next, wave, f_begin);
  }

  // ---- schedule F: schedule D with the FIR and the FFT on different waves ---------------------------
  // With one wave doing both halves the kernel needs ~114 VGPRs (4 waves per SIMD), and at 4 waves per
  // SIMD it sits on a latency floor (fusing abs() halves the written bytes and barely changes the time).
  // Here wave w < NPAIR slides the window and writes branch outputs for run w into one of two LDS
  // buffers while wave w + NPAIR transforms and stores the chunk before it: each role needs far fewer
  // registers, so more waves fit per SIMD.  One workgroup barrier per chunk hands the buffers over.
  template <bool INTERIOR, int NPAIR, int L, int DEPTH = 1>
  PFB_DEV void paired_fir_role(const KernelParams& p, float2* bufs, raw_t* halo_mine, const raw_t* halo_next,
                               int pair, long long f_begin) {
    constexpr int TAIL0 = L - (W - 1), NCH = L / C;
    static_assert(DEPTH == 1 || DEPTH == 2, "chunks of rows in flight");
    const int tid = threadIdx.x & 63;
    const int c0 = tid * CPT;
    Consts k;
    setup(p, tid, k);
    const raw_t* run_ptr = static_cast<const raw_t*>(p.in) + ((f_begin - (W - 1)) * D + p.base);
    const bool lane_on = !(K::LANES < NT) || tid < K::LANES;
    v2f x[NW][CPT];
    raw_t raw[DEPTH][C][CPT];
#pragma unroll
    for (int i = 0; i < W - 1; ++i) {
      raw_t t[CPT];
      F::template load_row<INTERIOR>(p, run_ptr, f_begin - (W - 1) + i, i, c0, t);
#pragma unroll
      for (int cc = 0; cc < CPT; ++cc) {
        x[i][cc] = cvt(t[cc]);
        if constexpr (INTERIOR) { if (lane_on) halo_mine[i * D + c0 + cc] = t[cc]; }
      }
    }
    const bool tail_from_lds = INTERIOR && (pair < NPAIR - 1);
    auto fetch = [&](int cj) {  // rows of chunk cj (those not coming from the neighbour's halo slot) into raw[cj % DEPTH]
#pragma unroll
      for (int t = 0; t < C; ++t) {
        const int r = cj * C + t;
        if (!(r >= TAIL0 && tail_from_lds)) F::template load_row<INTERIOR>(p, run_ptr, f_begin + r, W - 1 + r, c0, raw[cj % DEPTH][t]);
      }
    };
#pragma unroll
    for (int d = 0; d < DEPTH; ++d)
      if (d < NCH) fetch(d);
    __syncthreads();  // A: halo slots published
#pragma unroll
    for (int ci = 0; ci < NCH; ++ci) {
#pragma unroll
      for (int t = 0; t < C; ++t) {
        const int r = ci * C + t;
        if (r >= TAIL0 && tail_from_lds) {
#pragma unroll
          for (int cc = 0; cc < CPT; ++cc)
            x[W - 1 + t][cc] = cvt(halo_next[(r - TAIL0) * D + (lane_on ? c0 + cc : 0)]);
        } else {
#pragma unroll
          for (int cc = 0; cc < CPT; ++cc) x[W - 1 + t][cc] = cvt(raw[ci % DEPTH][t][cc]);
        }
      }
      if (ci + DEPTH < NCH) fetch(ci + DEPTH);
      fir_to_lds(k, x, bufs + (ci & 1) * K::BUF, tid);
#pragma unroll
      for (int i = 0; i < W - 1; ++i)
#pragma unroll
        for (int cc = 0; cc < CPT; ++cc) x[i][cc] = x[i + C][cc];
      __syncthreads();  // chunk ci handed to the FFT wave
    }
    __syncthreads();    // the FFT wave's last step
  }

  // MAGSEL / NTSEL: PFB_FLAG_MAGNITUDE and KernelParams.nontemporal as the host saw them (pass<>), -1 = tested per store
  template <int NPAIR, int L, int MAGSEL = -1, int NTSEL = -1>
  PFB_DEV void run_paired(const KernelParams& p, float2* lds_fft, raw_t* lds_halo) {
    static_assert(NT == 64, "one wave per run and role");
    static_assert(L % C == 0 && L >= W - 1, "runs are whole chunks and at least one halo long");
    constexpr int NCH = L / C;
    const int wave = threadIdx.x >> 6, tid = threadIdx.x & 63;
    const bool fir_role = wave < NPAIR;
    const int pair = fir_role ? wave : wave - NPAIR;
    long long blk = blockIdx.x;
    blk = xcd_remap_block(blk, gridDim.x, p.xcd_remap);
    const long long f_blk = blk * (long long)(NPAIR * L);
    const long long f_begin = f_blk + (long long)pair * L;
    float2* bufs = lds_fft + pair * 2 * K::BUF;
    const bool interior = p.vec_ok && ((f_blk - (W - 1)) * D + p.base >= 0) && (f_blk + NPAIR * L <= p.frames);
    if (fir_role) {
      raw_t* halo_mine = lds_halo + pair * ((W - 1) * D);
      const raw_t* halo_next = lds_halo + (pair + 1) * ((W - 1) * D);
      // (DEPTH = 2, rows two chunks ahead, measured on cfg2: 2.255 vs 2.243 ms -- no gain, 126 VGPRs; one chunk ahead stays)
      if (interior) paired_fir_role<true, NPAIR, L>(p, bufs, halo_mine, halo_next, pair, f_begin);
      else paired_fir_role<false, NPAIR, L>(p, bufs, halo_mine, halo_next, pair, f_begin);
    } else {
      Consts k;
      setup(p, tid, k);
      __syncthreads();  // A
      // an interior workgroup's frames all exist: its stores are unconditional (pass<>'s FULL); both loops meet the
      // same NCH + 1 barriers
      if (interior) {
#pragma unroll
        for (int s = 0; s <= NCH; ++s) {
          if (s >= 1)
            F::template fft_from_lds<true, MAGSEL, NTSEL>(p, k, bufs + ((s - 1) & 1) * K::BUF, tid, f_begin + (long long)(s - 1) * C);
          __syncthreads();
        }
      } else {
#pragma unroll
        for (int s = 0; s <= NCH; ++s) {
          if (s >= 1)
            F::template fft_from_lds<false, MAGSEL, NTSEL>(p, k, bufs + ((s - 1) & 1) * K::BUF, tid, f_begin + (long long)(s - 1) * C);
          __syncthreads();
        }
      }
    }
  }
};

template <class K, int NWV, int L>
__global__ void __launch_bounds__(64 * NWV) pfb_shared_kernel(const KernelParams p) {
  carry_history(p, SampleT<K::FMT>::kBytes, 64 * NWV);
  using raw_t = typename SampleT<K::FMT>::raw_t;
  __shared__ float2 lds_fft[NWV * K::LDS_ELEMS];
  __shared__ raw_t lds_halo[(NWV + 1) * (K::W - 1) * K::D];
  HaloShare<K>::template run_shared<NWV, L>(p, lds_fft, lds_halo);
}

template <class K, int NPAIR, int L, int MINW, int MAGSEL = -1, int NTSEL = -1>
__global__ void __launch_bounds__(128 * NPAIR, MINW) pfb_paired_kernel(const KernelParams p) {
  carry_history(p, SampleT<K::FMT>::kBytes, 128 * NPAIR);
  using raw_t = typename SampleT<K::FMT>::raw_t;
  __shared__ float2 lds_fft[NPAIR * 2 * K::BUF];
  __shared__ raw_t lds_halo[(NPAIR + 1) * (K::W - 1) * K::D];
  HaloShare<K>::template run_paired<NPAIR, L, MAGSEL, NTSEL>(p, lds_fft, lds_halo);
}

template <class K, int NPAIR, int L, int MINW, int MAGSEL = -1, int NTSEL = -1>
KernelEntry paired_entry(const KernelParams& p) {
  static constexpr KernelTag tag = kernel_tag<NPAIR, L, MINW>("paired", {false, false, MAGSEL, NTSEL});
  return entry_for(&pfb_paired_kernel<K, NPAIR, L, MINW, MAGSEL, NTSEL>, 4, tag.s, p, (long long)NPAIR * L, 128 * NPAIR);
}

// with the call's output type and store kind compiled in (with_store_roles, pfb_fast_cfg.hpp)
template <class K, int NPAIR, int L, int MINW>
KernelEntry paired_roles_entry(const KernelParams& p) {
  return with_store_roles(p, [&]<int MAGSEL, int NTSEL>() { return paired_entry<K, NPAIR, L, MINW, MAGSEL, NTSEL>(p); });
}

template <class K, int NWV>
constexpr bool kSharedFits = sizeof(float2) * NWV * K::LDS_ELEMS +
                                 sizeof(typename SampleT<K::FMT>::raw_t) * (NWV + 1) * (K::W - 1) * K::D <= 160 * 1024;

// a tile of NWV waves whose chunk buffers + shared halo do not fit one CU's LDS for this sample format (8-byte samples
// at M = 128) takes the 4-wave tile; no kernel = not even that: the caller goes on to the plain sliding runs
template <class K, int NWV, int L>
KernelEntry shared_entry(const KernelParams& p) {
  if constexpr (kSharedFits<K, NWV>) {
    static constexpr KernelTag tag = kernel_tag<NWV, L>("shared");
    // experiment bits 8.. : extra dynamic LDS in KiB (occupancy throttle for access-window studies)
    const unsigned extra_lds = (unsigned)((p.experiment >> 8) & 0xff) * 1024u;
    return entry_for(&pfb_shared_kernel<K, NWV, L>, 3, tag.s, p, (long long)NWV * L, 64 * NWV, extra_lds);
  } else if constexpr (NWV > 4 && kSharedFits<K, 4>) {
    return shared_entry<K, 4, 64>(p);
  } else {
    return KernelEntry{};
  }
}

}  // namespace pfb
