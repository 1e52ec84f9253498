// pfb_fast_overlap.hpp -- schedule 11 (P) of the fused kernel (pfb_fast.hpp): sliding runs, software-pipelined inside the wave.
#pragma once

#include "pfb_fast_core.hpp"
#include <utility>

namespace pfb {

// ---- schedule P: schedule A software-pipelined inside the wave ---------------------------------------------------
// PMC of the sliding kernels (profiles/r02_rocprofv3_pmc_summary_all_shapes.txt): a wave spends 26-29 % of its cycles in
// VALU instructions and ~40 % parked on s_waitcnt -- the chunk is a dependent chain FIR -> LDS -> pass 0 -> LDS -> pass 1 ->
// stores, and at 2 waves per SIMD (the window lives in ~200 VGPRs) nothing else is there to issue meanwhile.  Here the
// FIR of chunk i + 1 (pure VALU on the register window) sits in the SAME basic block as pass 0 of chunk i (LDS reads,
// butterflies, LDS writes on the other of two chunk buffers), so the compiler's scheduler can fill the LDS round trips
// with the next chunk's FMAs; the branch outputs wait in registers and go to LDS after pass 1.  Rows are fetched two
// chunks ahead instead of one.  Same arithmetic per output as schedule A: bit-identical.
template <class K>
struct Overlap : FastKernel<K> {
  using F = FastKernel<K>;
  using typename F::raw_t; using typename F::Consts;
  using F::cvt; using F::setup;
  static constexpr int M = K::M, P = K::P, D = K::D, CPT = K::CPT, C = K::C, W = K::W, OS = K::OS, NT = K::NT, NW = F::NW;

  // the window as a RING of NWP rows (NW rounded up to whole chunks): after PERIOD chunks every row is back in its
  // register, so a chunk loop unrolled PERIOD times indexes the window with compile-time constants and never moves it
  static constexpr int NWP = (NW + C - 1) / C * C, PERIOD = NWP / C;
  static constexpr bool kRingOk = PERIOD >= 2 && PERIOD <= 4;
  static constexpr bool kBuiltinFir = OS == 2 && CPT == 1;  // cfg5's shape: no spills with the scheduler-visible FMAs (see fma_tap_lo_b)
  // (PH / NX: the window as a ring of NX rows -- logical row i is x[(i + C PH) % NX] -- for run_overlap_ring; the sliding
  // callers pass the NW logical rows themselves, PH = 0)
  template <int PH = 0, int NX = NW>
  PFB_DEV void fir_compute(const Consts& k, const v2f (&xw)[NX][CPT], v2f (&acc)[OS][CPT][C]) {
    auto x = [&](int i) -> const v2f (&)[CPT] { return xw[(i + C * PH) % NX]; };
#pragma unroll
    for (int ph = 0; ph < OS; ++ph)
#pragma unroll
      for (int cc = 0; cc < CPT; ++cc) {
        if constexpr (kBuiltinFir) {
#pragma unroll
          for (int t = 0; t < C; ++t) acc[ph][cc][t] = (v2f){0.f, 0.f};
        }
        int tok = 0;  // FMA ordering token (fma_tap_lo)
#pragma unroll
        for (int q = 0; q < P; ++q) {
          const int j = ph + OS * q;
#pragma unroll
          for (int t = 0; t < C; ++t) {
            if constexpr (kBuiltinFir) {
              if (j & 1) fma_tap_hi_b(acc[ph][cc][t], x(W - 1 + t - j)[cc], k.hp[j >> 1][cc]);
              else fma_tap_lo_b(acc[ph][cc][t], x(W - 1 + t - j)[cc], k.hp[j >> 1][cc]);
            } else {
              if (q == 0 && (j & 1)) fma_tap0_hi(acc[ph][cc][t], x(W - 1 + t - j)[cc], k.hp[j >> 1][cc]);
              else if (q == 0) fma_tap0_lo(acc[ph][cc][t], x(W - 1 + t - j)[cc], k.hp[j >> 1][cc]);
              else if (j & 1) fma_tap_hi(acc[ph][cc][t], x(W - 1 + t - j)[cc], k.hp[j >> 1][cc], tok);
              else fma_tap_lo(acc[ph][cc][t], x(W - 1 + t - j)[cc], k.hp[j >> 1][cc], tok);
            }
          }
        }
      }
  }

  PFB_DEV void fir_write(const Consts& k, const v2f (&acc)[OS][CPT][C], float2* buf, int tid) {
    if (!(K::LANES < NT) || tid < K::LANES) {
#pragma unroll
      for (int ph = 0; ph < OS; ++ph)
#pragma unroll
        for (int cc = 0; cc < CPT; ++cc)
#pragma unroll
          for (int t = 0; t < C; ++t) reinterpret_cast<v2f*>(buf)[t * K::FS + k.upos[ph][cc]] = acc[ph][cc][t] * k.conj_mul;
    }
  }

  // MAGSEL: PFB_FLAG_MAGNITUDE as a template parameter of the kernel, and (interior runs) unconditional stores: the
  // number of vector-memory operations per chunk is then the same on every path, and the compiler's s_waitcnt for the
  // rows requested two chunks ahead stops waiting for half of the previous chunk's stores as well (pass<FULL>)
  // (tried for cfg3, whose 4 columns per lane spill 16-26 registers inside this loop: pass 0's twiddles from an LDS copy
  // instead of 30 registers -- the spills stayed, the rate fell from 0.64 to 0.50; cfg3 went back to schedule 0)
  template <bool INTERIOR, int MAGSEL = -1>
  PFB_DEV void run_overlap_impl(const KernelParams& p, const Consts& k, float2* lds, long long f_begin, long long f_end) {
    static_assert(NT == 64 && K::NP == 2 && !K::PINGPONG, "single-wave two-pass plans");
    const int tid = threadIdx.x;
    const int c0 = tid * CPT;
    const raw_t* run_ptr = static_cast<const raw_t*>(p.in) + ((f_begin - (W - 1)) * D + p.base);
    const long long nchunks = (f_end - f_begin + C - 1) / C;
    v2f x[NW][CPT];
    raw_t raw[C][CPT];
    v2f acc[OS][CPT][C];
#pragma unroll
    for (int i = 0; i < W - 1; ++i) {
      raw_t t[CPT];
      F::template load_row<INTERIOR>(p, run_ptr, f_begin - (W - 1) + i, i, c0, t);
#pragma unroll
      for (int cc = 0; cc < CPT; ++cc) x[i][cc] = cvt(t[cc]);
    }
    auto load_chunk_rows = [&](long long ci) {  // chunk ci of this run (clamped: the last chunk is fetched again rather than branching)
      const long long cl = ci < nchunks ? ci : nchunks - 1;
#pragma unroll
      for (int t = 0; t < C; ++t) F::template load_row<INTERIOR>(p, run_ptr, f_begin + cl * C + t, W - 1 + cl * C + t, c0, raw[t]);
    };
    auto take_rows = [&]() {
#pragma unroll
      for (int t = 0; t < C; ++t)
#pragma unroll
        for (int cc = 0; cc < CPT; ++cc) x[W - 1 + t][cc] = cvt(raw[t][cc]);
    };
    auto slide = [&]() {
#pragma unroll
      for (int i = 0; i < W - 1; ++i)
#pragma unroll
        for (int cc = 0; cc < CPT; ++cc) x[i][cc] = x[i + C][cc];
    };
    // chunk 0 by itself
    load_chunk_rows(0);
    take_rows();
    load_chunk_rows(1);
    fir_compute(k, x, acc);
    slide();
    fir_write(k, acc, lds, tid);
    team_sync<true>();
    float2* cur = lds;
    float2* nxt = lds + K::BUF;
    // (the loop is rotated -- the rows requested at the top of an iteration are taken at its END -- so that a load and
    // its wait sit in the same iteration: across the back edge the compiler merges the loop-entry state, which has no
    // stores in flight, into its s_waitcnt count and the wait for the rows would also wait for the chunk's stores)
    take_rows();                   // rows of chunk 1
    for (long long ci = 0; ci + 1 < nchunks; ++ci) {
      load_chunk_rows(ci + 2);     // two chunks ahead
      // one basic block: the next chunk's FIR next to this chunk's first pass
      fir_compute(k, x, acc);
      F::template pass<0>(p, cur, cur, tid, f_begin + ci * C, k.tw);
      slide();
      team_sync<true>();
      F::template pass<1, INTERIOR, MAGSEL>(p, cur, nullptr, tid, f_begin + ci * C, k.tw);
      fir_write(k, acc, nxt, tid);
      team_sync<true>();
      float2* t = cur; cur = nxt; nxt = t;
      take_rows();                 // rows of chunk ci + 2 (waits for them; the chunk's stores stay in flight)
    }
    F::template pass<0>(p, cur, cur, tid, f_begin + (nchunks - 1) * C, k.tw);
    team_sync<true>();
    F::template pass<1, INTERIOR, MAGSEL>(p, cur, nullptr, tid, f_begin + (nchunks - 1) * C, k.tw);
  }

  // The same pipeline over a run of exactly PERIOD = NWP / C chunks with the window as a RING of NWP = NW rounded up to
  // whole chunks: the chunk loop is gone (PERIOD straight-line steps, every window index a compile-time constant), and so
  // are the W-1 register moves per column that slide the window after every chunk (62 of the 499 VALU instructions of
  // the cfg5 chunk loop).  Same taps, same order: bit-identical.  Interior runs only; any other run takes the loop above.
  template <int MAGSEL>
  PFB_DEV void run_overlap_ring(const KernelParams& p, const Consts& k, float2* lds, long long f_begin) {
    static_assert(NT == 64 && K::NP == 2 && !K::PINGPONG, "single-wave two-pass plans");
    const int tid = threadIdx.x;
    const int c0 = tid * CPT;
    const raw_t* run_ptr = static_cast<const raw_t*>(p.in) + ((f_begin - (W - 1)) * D + p.base);
    v2f x[NWP][CPT];
    raw_t raw[C][CPT];
    v2f acc[OS][CPT][C];
#pragma unroll
    for (int i = 0; i < W - 1; ++i) {
      raw_t t[CPT];
      F::template load_row<true>(p, run_ptr, f_begin - (W - 1) + i, i, c0, t);
#pragma unroll
      for (int cc = 0; cc < CPT; ++cc) x[i][cc] = cvt(t[cc]);
    }
    auto load_chunk_rows = [&](int ci) {
#pragma unroll
      for (int t = 0; t < C; ++t) F::template load_row<true>(p, run_ptr, f_begin + ci * C + t, W - 1 + ci * C + t, c0, raw[t]);
    };
    auto take_rows = [&]<int PH>() {  // the rows of chunk PH: logical rows W-1 ... W-2+C of phase PH
#pragma unroll
      for (int t = 0; t < C; ++t)
#pragma unroll
        for (int cc = 0; cc < CPT; ++cc) x[(W - 1 + t + C * PH) % NWP][cc] = cvt(raw[t][cc]);
    };
    load_chunk_rows(0);
    take_rows.template operator()<0>();
    load_chunk_rows(1);
    fir_compute<0, NWP>(k, x, acc);
    fir_write(k, acc, lds, tid);
    team_sync<true>();
    float2* cur = lds;
    float2* nxt = lds + K::BUF;
    take_rows.template operator()<1>();
    auto step = [&]<int CI>() {  // chunk CI's FFT next to chunk CI + 1's FIR
      if constexpr (CI + 2 < PERIOD) load_chunk_rows(CI + 2);
      fir_compute<CI + 1, NWP>(k, x, acc);
      F::template pass<0>(p, cur, cur, tid, f_begin + CI * C, k.tw);
      team_sync<true>();
      F::template pass<1, true, MAGSEL>(p, cur, nullptr, tid, f_begin + CI * C, k.tw);
      fir_write(k, acc, nxt, tid);
      team_sync<true>();
      float2* t = cur; cur = nxt; nxt = t;
      if constexpr (CI + 2 < PERIOD) take_rows.template operator()<CI + 2>();
    };
    [&]<int... CI>(std::integer_sequence<int, CI...>) { (step.template operator()<CI>(), ...); }(std::make_integer_sequence<int, PERIOD - 1>{});
    F::template pass<0>(p, cur, cur, tid, f_begin + (PERIOD - 1) * C, k.tw);
    team_sync<true>();
    F::template pass<1, true, MAGSEL>(p, cur, nullptr, tid, f_begin + (PERIOD - 1) * C, k.tw);
  }

  template <int MAGSEL = -1>
  PFB_DEV void run_overlap(const KernelParams& p, float2* lds) {
    long long run = blockIdx.x;
    run = xcd_remap_block(run, gridDim.x, p.xcd_remap);
    const long long f_begin = run * p.frames_per_block;
    if (f_begin >= p.frames) return;
    const long long f_last = f_begin + p.frames_per_block;
    const long long f_end = f_last < p.frames ? f_last : p.frames;
    Consts k;
    setup(p, threadIdx.x, k);
    const bool interior = p.vec_ok && ((f_begin - (W - 1)) * D + p.base >= 0) && (f_last <= p.frames);
    if constexpr (kRingOk) {
      if (interior && p.frames_per_block == C * PERIOD) {
        run_overlap_ring<MAGSEL>(p, k, lds, f_begin);
        return;
      }
    }
    if (interior) run_overlap_impl<true, MAGSEL>(p, k, lds, f_begin, f_end);
    else run_overlap_impl<false, MAGSEL>(p, k, lds, f_begin, f_end);
  }
};

template <class K, bool MAG>
__global__ void __launch_bounds__(K::NT, (K::MIN_WAVES > 2 ? K::MIN_WAVES - 1 : K::MIN_WAVES)) pfb_overlap_kernel(const KernelParams p) {
  carry_history(p, SampleT<K::FMT>::kBytes, K::NT);
  __shared__ float2 lds[2 * K::BUF];
  Overlap<K>::template run_overlap<MAG ? 1 : 0>(p, lds);
}

template <class K>
constexpr bool kOverlapOk = K::NT == 64 && K::NP == 2 && !K::PINGPONG;

template <class K>
KernelEntry overlap_entry(const KernelParams& p) {
  static constexpr KernelTag mag = kernel_tag<>("overlap", {.magsel = 1}), c64 = kernel_tag<>("overlap", {.magsel = 0});
  return wants_magnitude(p) ? entry_for(&pfb_overlap_kernel<K, true>, 11, mag.s, p, p.frames_per_block, K::NT)
                            : entry_for(&pfb_overlap_kernel<K, false>, 11, c64.s, p, p.frames_per_block, K::NT);
}

}  // namespace pfb
