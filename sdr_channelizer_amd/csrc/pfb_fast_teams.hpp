// pfb_fast_teams.hpp -- schedule 6 (T) of the fused kernel (pfb_fast.hpp): a FIR team and an FFT team per workgroup.
#pragma once

#include "pfb_fast_core.hpp"

namespace pfb {

// ---- schedule T: FIR team + FFT team (large M) --------------------------------------------------------
// At M = 1024 one frame needs all 1024 columns, so the FIR is a team effort (NT threads x CPT columns), and
// in the plain sliding kernel the same 16 waves then all turn to the FFT: every phase leaves either the VALU
// or the LDS idle, and the passes cost several workgroup barriers per chunk (44 % VALU-busy, waves waiting
// 63 % of their cycles: profiles/).  Here the FIR team only filters -- a sliding register window per thread,
// chunk after chunk into one of three LDS buffers -- and C more waves transform: FFT wave w takes frame w of
// the previous chunk and runs the first two passes of its M-point FFT alone (M / 64 points per lane), so
// those passes need no barrier at all, only the wave's own program order.  One workgroup barrier per chunk
// rotates the buffers.
template <class K>
struct Teams : FastKernel<K> {
  using F = FastKernel<K>;
  using typename F::raw_t; using typename F::Consts;
  using F::cvt; using F::setup; using F::fir_to_lds;
  static constexpr int M = K::M, P = K::P, D = K::D, CPT = K::CPT, C = K::C, W = K::W, OS = K::OS, NT = K::NT, NW = F::NW;

  // One non-final pass of ONE frame by one wave, in place: every read of the pass (all iterations) happens
  // before its first write, and the wave's own program order is the only synchronisation.
  template <int I>
  PFB_DEV void pass_frame(const KernelParams& p, float2* fbuf, int lane, const v2f (&tw)[2][16]) {
    constexpr int R = K::R(I), S = K::S(I), KK = K::K(I), RS = K::RS(I);
    constexpr int IPF = M / R, ITERS = (IPF + 63) / 64;
    constexpr int S1 = K::S(I + 1), RS1 = K::RS(I + 1);
    static_assert(I < K::NP - 1, "the last pass (with the stores) belongs to the FIR team");
    constexpr bool TW_REGS = (ITERS == 1) && !K::TW_TABLE;
    v2f x[ITERS][R];
#pragma unroll
    for (int it = 0; it < ITERS; ++it) {
      const int item = lane + it * 64;
      const bool active = (IPF % 64 == 0) || (item < IPF);
      const v2f* s2 = reinterpret_cast<const v2f*>(fbuf) + (active ? item : 0);
#pragma unroll
      for (int n = 0; n < R; ++n) x[it][n] = s2[n * RS];
    }
#pragma unroll
    for (int it = 0; it < ITERS; ++it) {
      const int item = lane + it * 64;
      const bool active = (IPF % 64 == 0) || (item < IPF);
      const int kk = item / S, rest = item % S;
      Dft<R>::run(x[it]);
      if constexpr (TW_REGS) {
#pragma unroll
        for (int k = 1; k < R; ++k) x[it][k] = cmul_w(x[it][k], tw[I][k]);
      } else {
        const float4* t4 = reinterpret_cast<const float4*>(p.tw_lane + K::TW_OFF(I) + (active ? rest : 0) * K::TWR(I));
#pragma unroll
        for (int k2 = 0; k2 < K::TWR(I) / 2; ++k2) {
          const float4 t = t4[k2];
          if (k2 > 0) x[it][2 * k2] = cmul_w(x[it][2 * k2], (v2f){t.x, t.y});
          if (2 * k2 + 1 < R) x[it][2 * k2 + 1] = cmul_w(x[it][2 * k2 + 1], (v2f){t.z, t.w});
        }
      }
      if (active) {
        const int n1 = rest / S1, rest2 = rest % S1;
        v2f* d2 = reinterpret_cast<v2f*>(fbuf) + n1 * RS1 + kk * S1 + rest2;
#pragma unroll
        for (int k = 0; k < R; ++k) d2[k * KK * S1] = x[it][k];
      }
    }
  }

  // FIR team: chunk ci into buffer ci % 3, then the LAST pass (and the stores) of chunk ci - 2, whose first two
  // passes the FFT team finished in the step before.  The stores are most of the FFT's memory work and the FIR
  // team has issue slots to spare, while four FFT waves doing everything were the bottleneck (2.4 of 2.9 ms).
  // (A variant of this kernel for channel-major handles -- the last pass writing frame-major scratch tiles that the FFT
  // team moved into place transposed -- measured slower than frame-major slabs plus a transpose kernel, 7.4 against 6.4 ms
  // per 2^30 samples at M = 1024, and was removed: DESIGN.md section 5.4.)
  // (The window as a ring of registers -- blocks of 10 steps at M = 1024, no slide: 50 fewer VALU instructions per two steps --
  // measured 0.611-0.612 against 0.608-0.609, nothing on M = 560 / 400 / 320: the FIR team's issue slots are not what the
  // kernel waits for; not kept.  The pipelined single-wave kernel keeps its ring, run_overlap_ring.)
  template <bool INTERIOR, int MAGSEL = -1>
  PFB_DEV void fir_team(const KernelParams& p, const Consts& k, float2* bufs, long long f_begin, int nch) {
    const int tid = threadIdx.x;
    const int c0 = tid * CPT;
    auto last_pass = [&](float2* buf, int c) {   // chunk c of this run
      // the thread index is laundered so that everything the pass derives from it (LDS and store addresses) is
      // recomputed here -- a few VALU instructions -- instead of being hoisted out of the chunk loop: hoisted, ONE of
      // them was spilled, and its reload (a vector-memory load, which returns in order) made every step wait for the
      // row prefetch issued just before it: s_waitcnt vmcnt(0) four times per iteration of the steady-state loop
      int t2 = tid;
      asm volatile("" : "+v"(t2));
      F::template pass<K::NP - 1, INTERIOR, MAGSEL>(p, buf, nullptr, t2, f_begin + (long long)c * C, k.tw);
    };
    const raw_t* run_ptr = static_cast<const raw_t*>(p.in) + ((f_begin - (W - 1)) * D + p.base);
    v2f x[NW][CPT];
    raw_t raw[2][C][CPT];  // two chunks of rows in flight: one chunk is only ~1.5 us of work, less than a loaded HBM round trip
#pragma unroll
    for (int i = 0; i < W - 1; ++i) {
      raw_t t[CPT];
      F::template load_row<INTERIOR>(p, run_ptr, f_begin - (W - 1) + i, i, c0, t);
#pragma unroll
      for (int cc = 0; cc < CPT; ++cc) x[i][cc] = cvt(t[cc]);
    }
#pragma unroll
    for (int u = 0; u < 2; ++u)
#pragma unroll
      for (int t = 0; t < C; ++t) F::template load_row<INTERIOR>(p, run_ptr, f_begin + u * C + t, W - 1 + u * C + t, c0, raw[u][t]);
    int b_fir = 0, b_last = 1;  // buffer of chunk ci, buffer of chunk ci - 2 (= (ci + 1) % 3)
    // One chunk step.  U: which of the two row sets holds chunk ci; LASTP: chunk ci - 2 exists (every step but a run's
    // first two, which are peeled off so that the steady-state loop issues the same stores on every path: see pass<FULL>).
    // (An unconditional, clamped prefetch would make the loads path-independent too, but its 64-bit row addresses cost
    // this team the registers it does not have: 8-12 spilled, reloaded inside the loop.)
    auto step = [&]<int U, bool LASTP>(int ci) {
      const long long f0 = f_begin + (long long)ci * C;
#pragma unroll
      for (int t = 0; t < C; ++t)
#pragma unroll
        for (int cc = 0; cc < CPT; ++cc) x[W - 1 + t][cc] = cvt(raw[U][t][cc]);
      if (ci + 2 < nch) {
        const long long rel = (long long)(ci + 2) * C + (W - 1);
#pragma unroll
        for (int t = 0; t < C; ++t) F::template load_row<INTERIOR>(p, run_ptr, f0 + 2 * C + t, rel + t, c0, raw[U][t]);
      }
      fir_to_lds(k, x, bufs + b_fir * K::BUF, tid);
#pragma unroll
      for (int i = 0; i < W - 1; ++i)
#pragma unroll
        for (int cc = 0; cc < CPT; ++cc) x[i][cc] = x[i + C][cc];
      if constexpr (LASTP) last_pass(bufs + b_last * K::BUF, ci - 2);
      __syncthreads();  // (barrier ci) chunk ci handed to the FFT team, buffer of chunk ci - 2 free again
      b_fir = (b_fir == 2) ? 0 : b_fir + 1;
      b_last = (b_last == 2) ? 0 : b_last + 1;
    };
    step.template operator()<0, false>(0);
    step.template operator()<1, false>(1);
    for (int ci2 = 2; ci2 < nch; ci2 += 2) {
      step.template operator()<0, true>(ci2);
      step.template operator()<1, true>(ci2 + 1);
    }
    // drain: the FFT team finishes chunk nch - 1 while chunk nch - 2 gets its last pass, then chunk nch - 1
    if (nch >= 2) last_pass(bufs + b_last * K::BUF, nch - 2);
    __syncthreads();  // (barrier nch)
    b_last = (b_last == 2) ? 0 : b_last + 1;
    last_pass(bufs + b_last * K::BUF, nch - 1);
  }

  template <int MAGSEL = -1>
  PFB_DEV void run_teams(const KernelParams& p, float2* bufs) {
    static_assert(K::NP == 3 && !K::PINGPONG && NT % 64 == 0, "three in-place passes");
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int nch = p.frames_per_block / C;  // even (host rounds); the last workgroup filters zero padding past the end
    Consts k;
    setup(p, wave < NT / 64 ? threadIdx.x : lane, k);  // FFT team: only the twiddles are used, rows `lane % S` of the passes' tables
    long long run = blockIdx.x;  // one run per workgroup, in dispatch order
    run = xcd_remap_block(run, gridDim.x, p.xcd_remap);
    const long long f_begin = run * p.frames_per_block;
    if (f_begin >= p.frames) return;
    if (wave < NT / 64) {
      const bool interior = p.vec_ok && ((f_begin - (W - 1)) * D + p.base >= 0) && (f_begin + p.frames_per_block <= p.frames);
      if (interior) fir_team<true, MAGSEL>(p, k, bufs, f_begin, nch);
      else fir_team<false, MAGSEL>(p, k, bufs, f_begin, nch);
    } else {
      // (s_setprio for either team, measured: cfg4 -3 % / 0, M=560 +1.6 % / +1 %: noise)
      const int fr = wave - NT / 64;  // my frame inside every chunk
      int b = 0;                      // buffer of chunk s - 1
#pragma unroll 1
      for (int s = 0; s <= nch; ++s) {
        if (s >= 1) {
          float2* fbuf = bufs + b * K::BUF + fr * K::FS;
          pass_frame<0>(p, fbuf, lane, k.tw);
          team_sync<true>();
          pass_frame<1>(p, fbuf, lane, k.tw);
          b = (b == 2) ? 0 : b + 1;
        }
        __syncthreads();  // (barrier s) behind it the FIR team's last pass of chunk s - 2 is done
      }
    }
  }
};

// shapes with a FIR-team / FFT-team instantiation: three in-place passes whose last pass fits the FIR team in one
// iteration per thread or more (the generic pass), a multi-wave FIR team, chunks of C frames = C FFT waves
template <class K>
constexpr bool kTeamsOk = !K::WAVE_FRAMES && K::NP == 3 && !K::PINGPONG && K::NT > 64 && (K::NT + 64 * K::C) <= 1024 &&
                          3 * sizeof(float2) * K::BUF <= 160 * 1024 && K::C % 2 == 0;

// MAG: the handle's PFB_FLAG_MAGNITUDE, decided at launch -- inside the kernel the test made the number of stores per
// step look path-dependent to the compiler, whose s_waitcnt for the row prefetch then also waited for the stores
template <class K, bool MAG>
__global__ void __launch_bounds__(K::NT + 64 * K::C, K::MIN_WAVES) pfb_teams_kernel(const KernelParams p) {
  carry_history(p, SampleT<K::FMT>::kBytes, K::NT + 64 * K::C);
  __shared__ float2 bufs[3 * K::BUF];
  Teams<K>::template run_teams<MAG ? 1 : 0>(p, bufs);
}

template <class K>
KernelEntry teams_entry(const KernelParams& p) {
  static constexpr KernelTag mag = kernel_tag<>("teams", {.magsel = 1}), c64 = kernel_tag<>("teams", {.magsel = 0});
  return wants_magnitude(p) ? entry_for(&pfb_teams_kernel<K, true>, 6, mag.s, p, p.frames_per_block, K::NT + 64 * K::C)
                            : entry_for(&pfb_teams_kernel<K, false>, 6, c64.s, p, p.frames_per_block, K::NT + 64 * K::C);
}

}  // namespace pfb
