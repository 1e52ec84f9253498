// pfb_fast_sliding.hpp -- schedule 0 (A) of the fused kernel (pfb_fast.hpp): one sliding run per workgroup.
#pragma once

#include "pfb_fast_core.hpp"

namespace pfb {

// ---- schedule A: sliding window over a long contiguous run per workgroup ---------------------
// (MAGSEL / interior runs: the loop issues the same vector-memory operations on every path and is rotated -- the next
// chunk's rows, requested before this chunk's FIR, are taken at the END of the iteration -- so that the compiler's
// s_waitcnt for them counts the chunk's stores exactly instead of waiting for them too: see pass<FULL>)
template <class K, bool CM = false, bool MS = false>
struct SlidingRun : FastKernel<K, CM, MS> {
  using F = FastKernel<K, CM, MS>;
  using typename F::raw_t; using typename F::Consts; using typename F::RowFetch;
  using F::cvt; using F::setup; using F::finish_rows;
  static constexpr int M = K::M, P = K::P, D = K::D, CPT = K::CPT, C = K::C, W = K::W, OS = K::OS, NT = K::NT, NW = F::NW;

  template <bool INTERIOR, int MAGSEL = -1>
  PFB_DEV void run_impl(const KernelParams& p, const Consts& k, float2* lds, long long f_begin, long long f_end) {
    const int tid = threadIdx.x;
    const int c0 = tid * CPT;
    // uniform pointer to (row f_begin-(W-1), column 0); only dereferenced on the INTERIOR path
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
    auto take_rows = [&]() {
      finish_rows(c0, raw, rf);
#pragma unroll
      for (int t = 0; t < C; ++t)
#pragma unroll
        for (int cc = 0; cc < CPT; ++cc) x[W - 1 + t][cc] = cvt(raw[t][cc]);
    };
    take_rows();
    for (long long f0 = f_begin; f0 < f_end; f0 += C) {
      if constexpr (INTERIOR) {  // the next chunk's rows under this chunk's FFT; past the run's end: its last chunk again
        const long long nxt = f0 + C < f_end ? f0 + C : f0;
        F::template load_rows<true>(p, run_ptr, nxt, (nxt - f_begin) + (W - 1), c0, raw, rf);
      } else if (f0 + C < f_end) {
        const long long rel = (f0 - f_begin) + C + (W - 1);
        F::template load_rows<INTERIOR>(p, run_ptr, f0 + C, rel, c0, raw, rf);
      }
      F::template fir_fft_store<false, false, INTERIOR, MAGSEL>(p, k, x, lds, tid, f0);
      // slide the window by C rows
#pragma unroll
      for (int i = 0; i < W - 1; ++i)
#pragma unroll
        for (int cc = 0; cc < CPT; ++cc) x[i][cc] = x[i + C][cc];
      if (INTERIOR || f0 + C < f_end) take_rows();
    }
  }

  // (The same loop with the window as a ring -- PERIOD chunks per iteration, no slide, see run_overlap_ring -- measured on
  // cfg3: 0.676-0.686 either way at 24- and 36-frame runs; not kept here.)
  template <int MAGSEL = -1>
  PFB_DEV void run(const KernelParams& p, float2* lds) {
    // Consecutive runs go to one XCD (blocks are dealt round-robin over the 8 XCDs, so bid%8 labels
    // the XCD).  Bijective for any grid size.
    long long run = blockIdx.x;
    run = xcd_remap_block(run, gridDim.x, p.xcd_remap);
    const long long f_begin = run * p.frames_per_block;
    if (f_begin >= p.frames) return;
    const long long f_last = f_begin + p.frames_per_block;
    const long long f_end = f_last < p.frames ? f_last : p.frames;
    Consts k;
    setup(p, threadIdx.x, k);
    // every row of the run (halo included) lies inside `in`, whole chunks only, aligned vectors
    const bool interior = p.vec_ok && ((f_begin - (W - 1)) * D + p.base >= 0) && (f_last <= p.frames);
    if (interior) run_impl<true, MAGSEL>(p, k, lds, f_begin, f_end);
    else run_impl<false, MAGSEL>(p, k, lds, f_begin, f_end);
  }
};

// fused abs() has a faster schedule than complex output on the shapes whose last pass can stage its magnitudes
// in LDS (FastKernel::pass, kMagStaged): sliding runs
template <class K>
constexpr bool kMagStagedOk = K::NT == 64 && K::NP == 2 && !K::PINGPONG && K::M == 64 && K::C == 8;
// (M = 64 only: there the direct stores are 32-byte pieces.  Measured elsewhere: cfg3, whose pieces are 64 bytes,
// -3 %; M = 32 +-0; the M = 56 sliding kernel spilled with it)
template <class K>
constexpr int kMagnitudeSchedule = kMagStagedOk<K> ? (K::FMT == PFB_FMT_CF32 ? 7 : 0) : -1;  // (cf32: pairs still win)

// MAGSEL: -1 = PFB_FLAG_MAGNITUDE is tested inside (channel-major and staged-magnitude instantiations), 0 / 1 = decided
// at launch (the frame-major kernels: their store count per chunk is then path-independent, see run_impl)
template <class K, bool CM = false, bool MS = false, int MAGSEL = -1>
__global__ void __launch_bounds__(K::NT, K::MIN_WAVES) pfb_fast_kernel(const KernelParams p) {
  carry_history(p, SampleT<K::FMT>::kBytes, K::NT);
  __shared__ float2 lds[K::LDS_ELEMS];
  SlidingRun<K, CM, MS>::template run<MAGSEL>(p, lds);
}

template <class K, bool CM = false, bool MS = false, int MAGSEL = -1>
KernelEntry sliding_entry(const KernelParams& p) {
  static constexpr KernelTag tag = kernel_tag<>("sliding", {CM, MS, MAGSEL});
  return entry_for(&pfb_fast_kernel<K, CM, MS, MAGSEL>, 0, tag.s, p, p.frames_per_block, K::NT);
}

}  // namespace pfb
