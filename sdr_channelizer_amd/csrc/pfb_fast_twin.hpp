// pfb_fast_twin.hpp -- schedule 13 (W) of the fused kernel (pfb_fast.hpp): independent workgroups, a frame per wave and chunk.
#pragma once

#include "pfb_fast_core.hpp"

namespace pfb {

// ---- schedule W: several independent workgroups per CU (large M) --------------------------------------------
// The team kernel (schedule T) holds its sliding window as converted float pairs: 168 registers per FIR thread,
// three 34 KB chunk buffers, so ONE 12-wave workgroup per CU whose teams meet at a barrier every 4 frames; nothing
// hides a run's start-up (W-1 halo rows, two steps of fill, two of drain), so runs must be long (512 frames = 2 MB
// of input per CU), and 256 CUs each streaming their own megabytes is the access shape HBM serves worst (DESIGN.md
// section 6).  Here a workgroup is NT/64 waves, every wave does both jobs, and the state between chunks is small
// enough for TWO (M = 1024) or more workgroups per CU, which are not synchronised with each other: while one
// filters (VALU) the other transforms and stores (LDS, memory), and one's start-up is covered by the other's
// steady state, so runs can be short.
//  * the window is kept as the RAW samples (one register per int16 / int8 pair instead of two) and converted when
//    used: W-1+C conversions per column and chunk instead of C, i.e. +12 % VALU work in the FIR at M = 1024 for
//    30 instead of 60 persistent registers;
//  * a chunk is C = NT/64 frames in ONE buffer: FIR by everybody -> barrier -> wave w runs ALL passes of frame w
//    by itself (M/64 points per lane: wave-local, no barrier inside the FFT) and stores it -> barrier;
//  * a thread's two adjacent columns are two adjacent branch outputs: one ds_write_b128 (the team kernel's
//    ds_write_b64 pairs were a 2-way bank conflict, 15 % of its LDS cycles).
// Same taps, same accumulation order (taps ascending), same passes: bit-identical to the other plans of the shape.
template <class K>
struct Twin : FastKernel<K> {
  using F = FastKernel<K>;
  using typename F::raw_t; using typename F::RawVec;
  using F::cvt;
  static constexpr bool CM = false;
  static constexpr int M = K::M, P = K::P, D = K::D, CPT = K::CPT, C = K::C, W = K::W, OS = K::OS, NT = K::NT, NW = F::NW;

  template <bool MAG>
  PFB_DEV void last_pass_frame(const KernelParams& p, const float2* fbuf, int lane, long long f) {
    constexpr int I = K::NP - 1, R = K::R(I), KK = K::K(I), RS = K::RS(I);
    constexpr int IPF = M / R, ITERS = (IPF + 63) / 64;
    static_assert(K::S(I) == 1 && !CM && OS == 1, "frame-major, critically sampled");
    v2f x[ITERS][R];
#pragma unroll
    for (int it = 0; it < ITERS; ++it) {
      const int item = lane + it * 64;
      const v2f* s2 = reinterpret_cast<const v2f*>(fbuf) + ((IPF % 64 == 0) || item < IPF ? item : 0);
#pragma unroll
      for (int n = 0; n < R; ++n) x[it][n] = s2[n * RS];
    }
    const int shift = (p.flags & PFB_FLAG_FFTSHIFT) ? (M / 2) : 0;
#pragma unroll
    for (int it = 0; it < ITERS; ++it) {
      const int kk = lane + it * 64;
      Dft<R>::run(x[it]);
      if ((IPF % 64 == 0) || kk < IPF) {
        auto col_of = [&](int ch) {
          const int c2 = ch + shift;
          return c2 >= M ? c2 - M : c2;
        };
        // (a wave-uniform row pointer + an UNSIGNED 32-bit lane offset: the address form that needs no 64-bit vector
        // arithmetic and no register pair per pointer)
        auto slot = [&](auto* rowp, int k) {
          if constexpr (K::POW2) {  // fftshift swaps the row's halves: two base pointers, compile-time offsets (see pass<>)
            auto* lo = rowp + (unsigned)(kk + shift);
            auto* hi = rowp + (unsigned)(kk + (M / 2 - shift));
            return (k < R / 2) ? lo + k * KK : hi + (k - R / 2) * KK;
          } else {
            return rowp + (unsigned)col_of(kk + k * KK);
          }
        };
        if constexpr (MAG) {
          float* rowm = reinterpret_cast<float*>(p.out) + f * M;
#pragma unroll
          for (int k = 0; k < R; ++k) *slot(rowm, k) = mag_out(x[it][k].x, x[it][k].y, p.flags);
        } else {
          float2* row = p.out + f * M;
#pragma unroll
          for (int k = 0; k < R; ++k) *reinterpret_cast<v2f*>(slot(row, k)) = x[it][k];
        }
      }
    }
  }

  // taps of column pair `pr` of this thread (columns c0 + 2 pr, c0 + 2 pr + 1), two taps per register pair: the table of setup()
  PFB_DEV void load_taps_pair(const KernelParams& p, int tid, int pr, v2f (&hp)[(W + 1) / 2][2]) {
    const int c0 = tid * CPT + 2 * pr;
#pragma unroll
    for (int cc = 0; cc < 2; ++cc) {
      const int col = (K::LANES < NT && c0 >= D) ? 0 : c0 + cc;  // idle lanes read column 0's taps
      const float4* tl = reinterpret_cast<const float4*>(p.taps_lane + (size_t)col * K::WP);
#pragma unroll
      for (int q4 = 0; q4 < K::WP / 4; ++q4) {
        const float4 v = tl[q4];
        if (2 * q4 < (W + 1) / 2) hp[2 * q4][cc] = (v2f){v.x, v.y};
        if (2 * q4 + 1 < (W + 1) / 2) hp[2 * q4 + 1][cc] = (v2f){v.z, v.w};
      }
    }
  }

  // Twiddle rows of the non-final passes as this kernel keeps them in LDS: in registers they are 2 R per pass, and from
  // the global table their loads would queue behind the row prefetch (a wave's vector-memory operations return in order:
  // a pass that waits for a twiddle load waits for every HBM load issued before it).  Row stride: even (16-byte reads)
  // with an odd half, so that the sixteen lanes of a ds_read_b128 group read sixteen different bank quads.
  static constexpr int TWS(int i) { return (K::TWR(i) / 2) % 2 ? K::TWR(i) : K::TWR(i) + 2; }
  static constexpr int TWL_OFF(int i) { int o = 0; for (int j = 0; j < i; ++j) o += K::S(j) * TWS(j); return o; }
  static constexpr int TWL_ELEMS = TWL_OFF(K::NP - 1);

  PFB_DEV void fill_twiddles(const KernelParams& p, float2* twl) {
#pragma unroll
    for (int i = 0; i < K::NP - 1; ++i) {
      const int R = K::R(i), n = K::S(i) * R;
      for (int idx = threadIdx.x; idx < n; idx += NT)
        twl[TWL_OFF(i) + (idx / R) * TWS(i) + idx % R] = p.tw_lane[K::TW_OFF(i) + (idx / R) * K::TWR(i) + idx % R];
    }
  }

  // One non-final pass of one frame by one wave, in place, like pass_frame, twiddles from the LDS table.
  template <int I>
  PFB_DEV void pass_frame_lean(float2* fbuf, const float2* twl, int lane) {
    constexpr int R = K::R(I), S = K::S(I), KK = K::K(I), RS = K::RS(I);
    constexpr int IPF = M / R;
    constexpr int S1 = K::S(I + 1), RS1 = K::RS(I + 1);
    static_assert(I < K::NP - 1 && IPF <= 64 && R % 2 == 0, "one item per lane");
    const bool active = (IPF == 64) || (lane < IPF);
    const int item = active ? lane : 0;
    const int kk = item / S, rest = item % S;
    v2f x[R];
    const v2f* s2 = reinterpret_cast<const v2f*>(fbuf) + item;
#pragma unroll
    for (int n = 0; n < R; ++n) x[n] = s2[n * RS];
    const float4* t4 = reinterpret_cast<const float4*>(twl + TWL_OFF(I) + rest * TWS(I));
    const int n1 = rest / S1, rest2 = rest % S1;
    v2f* d2 = reinterpret_cast<v2f*>(fbuf) + n1 * RS1 + kk * S1 + rest2;
    Dft<R>::run(x);
#pragma unroll
    for (int k2 = 0; k2 < R / 2; ++k2) {
      const float4 t = t4[k2];
      if (k2 > 0) x[2 * k2] = cmul_w(x[2 * k2], (v2f){t.x, t.y});
      x[2 * k2 + 1] = cmul_w(x[2 * k2 + 1], (v2f){t.z, t.w});
      if (active) {
        d2[(2 * k2) * KK * S1] = x[2 * k2];
        d2[(2 * k2 + 1) * KK * S1] = x[2 * k2 + 1];
      }
    }
  }

  // CPT raw samples of row `rel` of an interior run: uniform 64-bit base in SGPRs + a 32-bit lane offset (the address
  // form that costs one register per lane; as pointer arithmetic the compiler kept a 64-bit address pair per row)
  PFB_DEV void load_row_sbase(const raw_t* run_ptr, long long rel, int c0, raw_t (&raw)[CPT]) {
    static_assert(sizeof(RawVec) % 4 == 0, "whole dwords per lane");
    typedef unsigned dwords_t __attribute__((ext_vector_type(sizeof(RawVec) / 4)));
    const int cs = (K::LANES < NT && c0 >= D) ? 0 : c0;  // lanes beyond the last column read column 0 (and never use it)
    const raw_t* rowp = run_ptr + rel * D;               // wave-uniform
    const dwords_t v = *reinterpret_cast<const dwords_t*>(rowp + (unsigned)cs);
    __builtin_memcpy(&raw[0], &v, sizeof(RawVec));
  }

  // The fast path: whole chunks of a run whose every row (halo included) lies inside `in`, aligned vectors.
  // The chunk loop is laid out so that the compiler's s_waitcnt counts are EXACT: a wave's vector-memory operations
  // return in order, the compiler counts them per path, and wherever the count differs between paths into a point it
  // assumes the fewest younger operations, i.e. waits for more than the load it needs -- typically for every store
  // issued since.  So (1) the loop is rotated: an iteration is [transform + store chunk i, its first step requesting
  // the rows of chunk i + 1] then [FIR of chunk i + 1], which keeps a load and its wait in the SAME iteration;
  // (2) nothing in the loop is conditionally issued: the prefetch past the run's end re-reads the last row, partial
  // chunks are left to the careful path, PFB_FLAG_MAGNITUDE is a template parameter of the kernel.
  static constexpr int NWV = NT / 64;        // waves per workgroup
  static constexpr int FPW = C / (NT / 64);  // frames each wave transforms per chunk
  static constexpr bool kTapsResident = K::MIN_WAVES <= 2;  // 256 registers: the taps stay; otherwise they are re-read per chunk
  static constexpr bool kLean = K::MIN_WAVES >= 4;          // 128 registers
  // r_first, G, r_hi: this workgroup's runs r_first, r_first + G, ... below r_hi (all of them whole, with their halo
  // inside `in`), chained without a bubble: the step that would request the next chunk's rows requests the next run's
  // W-1 halo rows as well (into the window registers, which are dead at that point).  G = the grid: with one workgroup
  // per run there is no second run; with a grid of resident workgroups (PFB_OPT_GRID) the taps, the twiddle table and
  // the start-up latency are paid once per workgroup, and SHORT runs become affordable -- at any moment the chip then
  // works on G consecutive short runs, a dense window sweeping through the stream (what HBM
  // delivers depends on how compact the set of concurrently touched DRAM rows is).
  template <bool MAG>
  PFB_DEV void twin_fast(const KernelParams& p, float2* lds, const float2* twl, long long r_first, long long G, long long r_hi) {
    static_assert(C % NWV == 0 && OS == 1 && K::NP == 3 && !K::PINGPONG, "whole frames per wave and chunk");
    static_assert(CPT % 2 == 0 && K::S(0) % 2 == 0 && K::RS(0) % 2 == 0 && K::FS % 2 == 0 && D % 2 == 0, "adjacent, aligned branch pairs");
    constexpr int NPR = CPT / 2;  // column pairs per thread
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);  // in an SGPR: frame indices and row pointers stay scalar
    const int c0 = (K::LANES < NT && tid >= K::LANES) ? 0 : tid * CPT;  // idle lanes (D not a multiple of 64 CPT) shadow thread 0
    const bool lane_on = !(K::LANES < NT) || tid < K::LANES;
    // Registers decide this kernel (workgroups per CU = 512 / registers / waves per workgroup).  Where they do not fit,
    // the taps (W per column) are NOT kept across the FFT: a column pair's come back from the L2-resident table every
    // chunk -- the first pair's loads are issued before the last pass, so that they land under its stores and the
    // barrier, the next pair's under the FIR of the pair before.
    constexpr int NHP = kTapsResident ? NPR : (NPR > 1 ? 2 : 1);
    v2f hp[NHP][(W + 1) / 2][2];
    const v2f conj_mul = (v2f){1.f, (p.flags & PFB_FLAG_CONJUGATE_INPUT) ? -1.f : 1.f};
    int upos[NPR];  // LDS position of the lower of a pair's two adjacent branch outputs
#pragma unroll
    for (int pr = 0; pr < NPR; ++pr) {
      const int n = D - 1 - (c0 + 2 * pr + 1);
      upos[pr] = (n / K::S(0)) * K::RS(0) + (n % K::S(0));
    }
    if constexpr (kTapsResident) {
#pragma unroll
      for (int pr = 0; pr < NPR; ++pr) load_taps_pair(p, tid, pr, hp[pr]);
    } else {
      load_taps_pair(p, tid, 0, hp[0]);
    }
    const int nch = p.frames_per_block / C;  // chunks per run
    long long r = r_first;
    const raw_t* run_ptr = static_cast<const raw_t*>(p.in) + ((r * p.frames_per_block - (W - 1)) * D + p.base);
    raw_t win[W - 1][CPT];  // rows f0-(W-1) ... f0-1, as loaded
    raw_t raw[C][CPT];      // rows f0 ... f0+C-1
#pragma unroll
    for (int i = 0; i < W - 1; ++i) load_row_sbase(run_ptr, i, c0, win[i]);
#pragma unroll
    for (int t = 0; t < C; ++t) load_row_sbase(run_ptr, W - 1 + t, c0, raw[t]);
    // FIR of a chunk's C frames for my CPT columns, a column pair at a time, then the window slides.  Row i of the NW
    // window rows feeds frame t with tap j = W-1+t-i; rows are walked newest first so that every accumulator takes its
    // taps in ascending order (the order of fir_to_lds: bit-identical sums).
    auto fir_chunk = [&]() {
#pragma unroll
      for (int pr = 0; pr < NPR; ++pr) {
        const int hb = kTapsResident ? pr : (pr & 1);
        if constexpr (!kTapsResident) { if (pr + 1 < NPR) load_taps_pair(p, tid, pr + 1, hp[(pr + 1) & 1]); }
        v2f acc[2][C];
#pragma unroll
        for (int cc = 0; cc < 2; ++cc) {
#pragma unroll
          for (int t = 0; t < C; ++t) acc[cc][t] = (v2f){0.f, 0.f};
          int tok = 0;
#pragma unroll
          for (int i = NW - 1; i >= 0; --i) {
            const v2f xi = cvt(i >= W - 1 ? raw[i - (W - 1)][2 * pr + cc] : win[i][2 * pr + cc]);
#pragma unroll
            for (int t = 0; t < C; ++t) {
              const int j = W - 1 + t - i;
              if (j >= 0 && j < W) {
                if (j & 1) fma_tap_hi(acc[cc][t], xi, hp[hb][j >> 1][cc], tok);
                else fma_tap_lo(acc[cc][t], xi, hp[hb][j >> 1][cc], tok);
              }
            }
          }
          if constexpr (kLean) {
            // (128 registers: a column's C sums leave before the next column starts -- 8-byte writes, a 2-way bank
            // conflict on C writes per column, instead of holding both columns' sums for the 16-byte write)
            if (lane_on) {
              v2f* d2 = reinterpret_cast<v2f*>(lds) + upos[pr] + (1 - cc);
#pragma unroll
              for (int t = 0; t < C; ++t) d2[t * K::FS] = acc[cc][t] * conj_mul;
            }
            asm volatile("" ::: "memory");
          }
        }
        if constexpr (!kLean) {
          if (lane_on) {
            // column c + 1 is branch n - 1 (even), column c branch n: adjacent positions, 16-byte aligned -> one ds_write_b128
            float4* d4 = reinterpret_cast<float4*>(lds + upos[pr]);
#pragma unroll
            for (int t = 0; t < C; ++t) {
              const v2f a = acc[1][t] * conj_mul, b = acc[0][t] * conj_mul;
              d4[t * (K::FS / 2)] = make_float4(a.x, a.y, b.x, b.y);
            }
          }
        }
      }
#pragma unroll
      for (int i = 0; i < W - 1; ++i)
#pragma unroll
        for (int cc = 0; cc < CPT; ++cc) win[i][cc] = (i + C >= W - 1) ? raw[i + C - (W - 1)][cc] : win[i + C][cc];
    };
    fir_chunk();
    int ci = 0;
    for (;;) {
      const long long f0 = r * p.frames_per_block + (long long)ci * C;
      bool more = true;
      __syncthreads();  // the chunk is in LDS
      // my frames of the chunk: wave + NWV fi.  What the next chunk needs is requested between the passes (no
      // vector-memory load inside them: a pass waiting for a table entry would wait for every row requested before it):
      // its rows behind the first pass 0 -- they land under the rest of the transform and its stores --, its first
      // taps behind the last pass 1
#pragma unroll
      for (int fi = 0; fi < FPW; ++fi) {
        const int fc = wave + NWV * fi;
        float2* fbuf = lds + fc * K::FS;
        pass_frame_lean<0>(fbuf, twl, lane);
        if (fi == 0) {
          asm volatile("" ::: "memory");
          if (ci + 1 < nch) {  // the run's next chunk
            ++ci;
            const long long rel = (long long)ci * C + (W - 1);
#pragma unroll
            for (int t = 0; t < C; ++t) load_row_sbase(run_ptr, rel + t, c0, raw[t]);
          } else if (r + G < r_hi) {  // my next run: its halo (the window registers are dead here) and its first chunk
            r += G;
            ci = 0;
            run_ptr = static_cast<const raw_t*>(p.in) + ((r * p.frames_per_block - (W - 1)) * D + p.base);
#pragma unroll
            for (int i = 0; i < W - 1; ++i) load_row_sbase(run_ptr, i, c0, win[i]);
#pragma unroll
            for (int t = 0; t < C; ++t) load_row_sbase(run_ptr, W - 1 + t, c0, raw[t]);
          } else {
            more = false;
          }
        }
        team_sync<true>();
        pass_frame_lean<1>(fbuf, twl, lane);
        team_sync<true>();
        if (fi == FPW - 1 && !kTapsResident) {
          asm volatile("" ::: "memory");
          load_taps_pair(p, tid, 0, hp[0]);
        }
        last_pass_frame<MAG>(p, fbuf, lane, f0 + fc);
      }
      __syncthreads();  // everybody has read the chunk out of LDS
      if (!more) break;
      fir_chunk();
    }
  }

  // The careful path, for the few runs that touch the history in front of the call's first sample, a partial last chunk
  // or a buffer the vector loads cannot take: no window kept in registers -- per chunk and column the NW rows are
  // fetched again, sample by sample with the checks of load_row<false> (all of a column's loads in flight together: a
  // run of this kind is a straggler among thousands, but a serial one would outlast the whole kernel), columns in a
  // rolled loop.  Same taps in the same order: the same bits.
  template <bool MAG>
  PFB_DEV void twin_careful(const KernelParams& p, float2* lds, const float2* twl, long long f_begin, long long f_end) {
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const raw_t* in = static_cast<const raw_t*>(p.in);
    const raw_t* hist = static_cast<const raw_t*>(p.hist);
    const v2f conj_mul = (v2f){1.f, (p.flags & PFB_FLAG_CONJUGATE_INPUT) ? -1.f : 1.f};
    for (long long f0 = f_begin; f0 < f_end; f0 += C) {
      if (!(K::LANES < NT) || tid < K::LANES) {
#pragma unroll 1
        for (int cc = 0; cc < CPT; ++cc) {
          const int c = tid * CPT + cc, n = D - 1 - c;
          const int pos = (n / K::S(0)) * K::RS(0) + (n % K::S(0));
          const float* tl = p.taps_lane + (size_t)c * K::WP;
          raw_t r[NW];
#pragma unroll
          for (int i = 0; i < NW; ++i) {
            const long long fr = f0 - (W - 1) + i;  // frame whose newest row this is
            const long long s = fr * D + p.base + c;
            r[i] = (fr >= p.frames) ? raw_t{} : ((s >= 0) ? in[s] : hist[p.hist_samples + s]);
          }
          float h[W];
#pragma unroll
          for (int j = 0; j < W; ++j) h[j] = tl[j];
          v2f acc[C];
#pragma unroll
          for (int t = 0; t < C; ++t) acc[t] = (v2f){0.f, 0.f};
#pragma unroll
          for (int i = NW - 1; i >= 0; --i) {
            const v2f xi = cvt(r[i]);
#pragma unroll
            for (int t = 0; t < C; ++t) {
              const int j = W - 1 + t - i;
              if (j >= 0 && j < W) acc[t] = fma2(xi, splat(h[j]), acc[t]);
            }
          }
#pragma unroll
          for (int t = 0; t < C; ++t) reinterpret_cast<v2f*>(lds)[t * K::FS + pos] = acc[t] * conj_mul;
        }
      }
      __syncthreads();
#pragma unroll 1
      for (int fc = wave; fc < C; fc += NWV) {
        const long long f = f0 + fc;
        float2* fbuf = lds + fc * K::FS;
        if (f < f_end) {
          pass_frame_lean<0>(fbuf, twl, lane);
          team_sync<true>();
          pass_frame_lean<1>(fbuf, twl, lane);
          team_sync<true>();
          last_pass_frame<MAG>(p, fbuf, lane, f);
        }
      }
      __syncthreads();
    }
  }

  template <bool MAG>
  PFB_DEV void run_twin(const KernelParams& p, float2* lds, float2* twl) {
    const long long G = gridDim.x, fpb = p.frames_per_block;
    long long r = blockIdx.x;
    r = xcd_remap_block(r, G, p.xcd_remap);
    const long long nruns = (p.frames + fpb - 1) / fpb;
    if (r >= nruns) return;
    // runs [r_lo, r_hi) are whole and have their halo inside `in`: the fast path; the others (the call's first run, a
    // partial last one, everything if the buffer is not aligned for the vector loads) take the careful one
    const long long need = (long long)(W - 1) * D - p.base;  // samples of halo in front of frame 0
    const long long r_lo = need > 0 ? (need + fpb * D - 1) / (fpb * D) : 0;
    const long long r_hi = p.vec_ok ? p.frames / fpb : 0;
    fill_twiddles(p, twl);  // (visible behind the chunk loops' first barrier)
    auto careful = [&](long long rr) {
      const long long fb = rr * fpb, fl = fb + fpb;
      twin_careful<MAG>(p, lds, twl, fb, fl < p.frames ? fl : p.frames);
    };
    for (; r < nruns && r < r_lo; r += G) careful(r);
    if (r < r_hi) {
      twin_fast<MAG>(p, lds, twl, r, G, r_hi);
      r += ((r_hi - 1 - r) / G + 1) * G;
    }
    for (; r < nruns; r += G) careful(r);
  }
};

// schedule 13 (W): independent workgroups of NT/64 waves, a frame per wave and chunk, two or more per CU (run_twin)
template <class K>
constexpr bool kTwinOk = K::WAVE_FRAMES && K::NP == 3 && !K::PINGPONG && K::C % (K::NT / 64) == 0 && K::D == K::M && K::CPT % 2 == 0;

template <class K, bool MAG>
__global__ void __launch_bounds__(K::NT, K::MIN_WAVES) pfb_twin_kernel(const KernelParams p) {
  carry_history(p, SampleT<K::FMT>::kBytes, K::NT);
  __shared__ float2 lds[K::BUF + Twin<K>::TWL_ELEMS];
  Twin<K>::template run_twin<MAG>(p, lds, lds + K::BUF);
}

// grid_override: resident workgroups walking runs b, b + G, ...
template <class K>
KernelEntry twin_entry(const KernelParams& p) {
  static constexpr KernelTag mag = kernel_tag<>("twin", {.magsel = 1}), c64 = kernel_tag<>("twin", {.magsel = 0});
  KernelEntry e = wants_magnitude(p) ? entry_for(&pfb_twin_kernel<K, true>, 13, mag.s, p, p.frames_per_block, K::NT)
                                     : entry_for(&pfb_twin_kernel<K, false>, 13, c64.s, p, p.frames_per_block, K::NT);
  if (p.grid_override > 0 && e.blocks > p.grid_override) e.blocks = p.grid_override;
  return e;
}

}  // namespace pfb
