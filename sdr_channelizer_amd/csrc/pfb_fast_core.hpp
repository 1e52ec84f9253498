// pfb_fast_core.hpp -- the FIR and FFT building blocks that more than one schedule of the fused kernel uses.
// Each schedule (pfb_fast_*.hpp, list in pfb_fast.hpp) is a struct of its own derived from FastKernel.
#pragma once

#include "pfb_fast_cfg.hpp"

namespace pfb {

// CM = channel-major output, out[k * out_ld + out_frame0 + m] (MATLAB's column-major F x M): its own
// instantiation, so the extra address arithmetic never costs the frame-major kernels a register.
// MS = fused abs() with the magnitudes staged in LDS (its own instantiation of the sliding-run kernel, like CM)
template <class K, bool CM = false, bool MS = false>
struct FastKernel : FastRows<K> {
  static constexpr int M = K::M, P = K::P, D = K::D, CPT = K::CPT, C = K::C, W = K::W, OS = K::OS, NT = K::NT;
  static constexpr int NW = W - 1 + C;  // window rows held in registers during a chunk

  // FULL: every frame of the chunk exists (an interior run): the stores are unconditional, so that the number of
  // vector-memory operations per step is the same on every path -- the compiler's s_waitcnt counts stay exact across
  // the chunk loop (a conditional store makes it assume the fewest, i.e. wait for MORE than the load it needs)
  // MAGSEL: -1 = PFB_FLAG_MAGNITUDE is tested here, 0 / 1 = the caller has (outside its chunk loop: same reason as FULL)
  // NTSEL: the same for KernelParams.nontemporal (the wave-pair kernels: their FFT role's unrolled chunk bodies then
  // carry neither flag test nor the store they do not use)
  template <int I, bool FULL = false, int MAGSEL = -1, int NTSEL = -1>
  PFB_DEV void pass(const KernelParams& p, float2* src, float2* dst, int tid, long long f0,
                    const v2f (&tw)[2][16]) {
    float2* const p_out = p.out;
    const long long p_frames = p.frames;
    const int nontemporal = NTSEL < 0 ? p.nontemporal : NTSEL;
    constexpr int R = K::R(I), S = K::S(I), KK = K::K(I), RS = K::RS(I);
    constexpr int IPF = M / R, ITEMS = C * IPF, ITERS = (ITEMS + NT - 1) / NT;
    constexpr bool LAST = (I == K::NP - 1);
    constexpr bool TW_REGS = (ITERS == 1) && !K::TW_TABLE;
    constexpr bool READ_BARRIER = !LAST && !K::PINGPONG && NT > 64;  // in place across several waves
    constexpr bool kMagStaged = MS && LAST;
#pragma unroll
    for (int it = 0; it < ITERS; ++it) {
      const int w = tid + it * NT;
      const bool active = (ITEMS % NT == 0) || (w < ITEMS);
      const int fc = w / IPF, item = w % IPF;
      const int kk = item / S, rest = item % S;
      v2f x[R];
      if (active) {
        const v2f* s2 = reinterpret_cast<const v2f*>(src) + fc * K::FS + item;
#pragma unroll
        for (int n = 0; n < R; ++n) x[n] = s2[n * RS];
      } else {
#pragma unroll
        for (int n = 0; n < R; ++n) x[n] = (v2f){0.f, 0.f};
      }
      if constexpr (READ_BARRIER) __syncthreads();
      Dft<R>::run(x);
      if constexpr (!LAST) {
        constexpr int S1 = K::S(I + 1), RS1 = K::RS(I + 1);
        // twiddle e^{+j 2 pi rest k / (R S)}: row `rest` of this pass's table
        if constexpr (TW_REGS) {
#pragma unroll
          for (int k = 1; k < R; ++k) x[k] = cmul_w(x[k], tw[I][k]);
        } else {
          const float4* t4 = reinterpret_cast<const float4*>(p.tw_lane + K::TW_OFF(I) + rest * K::TWR(I));
#pragma unroll
          for (int k2 = 0; k2 < K::TWR(I) / 2; ++k2) {
            const float4 t = t4[k2];
            if (k2 > 0) x[2 * k2] = cmul_w(x[2 * k2], (v2f){t.x, t.y});
            if (2 * k2 + 1 < R) x[2 * k2 + 1] = cmul_w(x[2 * k2 + 1], (v2f){t.z, t.w});
          }
        }
        const int n1 = rest / S1, rest2 = rest % S1;
        if (active) {
          v2f* d2 = reinterpret_cast<v2f*>(dst) + fc * K::FS + n1 * RS1 + kk * S1 + rest2;
#pragma unroll
          for (int k = 0; k < R; ++k) d2[k * KK * S1] = x[k];
        }
      } else {
        if constexpr (kMagStaged) {
          // fused abs() of the single-wave M = 64 kernels: a lane's 8 magnitudes are 8 channels apart, so storing them
          // directly writes 32-byte pieces.  The chunk buffer is free once the wave has read it (the LDS executes a
          // wave's accesses in order), so the magnitudes go there as rows of M floats (+8 pad: the 8 frames land on
          // distinct banks) and leave as 16 bytes per lane: 4 frames x 256 contiguous bytes per instruction.
          // (the sliding-run kernel only: there it is worth 7 %, 2.07 -> 1.93 ms per 2^30 samples, and makes sliding
          // runs the fastest way to magnitudes; on the FFT wave of the pair schedules the extra LDS trip costs 2 %.
          // select_fast picks this instantiation when the flag is set and `out` is 16-byte aligned.)
          static_assert(!CM && NT == 64 && ITERS == 1 && K::NP == 2 && !K::PINGPONG && M % 4 == 0, "single-wave two-pass plans");
          {
            constexpr int SR = M + ((8 - M % 64) + 64) % 64;  // = 8 (mod 64), a multiple of 4
            static_assert(C * SR * sizeof(float) <= K::BUF * sizeof(float2), "the staged magnitudes fit the chunk buffer");
            float* stage = reinterpret_cast<float*>(src);
            const int shift = (p.flags & PFB_FLAG_FFTSHIFT) ? (M / 2) : 0;
            team_sync<true>();
#pragma unroll
            for (int k = 0; k < R; ++k) {
              int col = kk + k * KK + shift;
              col = col >= M ? col - M : col;
              if (active) stage[fc * SR + col] = mag_out(x[k].x, x[k].y, p.flags);
            }
            team_sync<true>();
            constexpr int NV = C * M / 4;  // float4s in the chunk
#pragma unroll
            for (int j = 0; j < (NV + 63) / 64; ++j) {
              const int idx = tid + 64 * j, fr = idx / (M / 4), q = idx % (M / 4);
              if ((NV % 64 == 0 || idx < NV) && f0 + fr < p_frames) {
                const float4 v = *reinterpret_cast<const float4*>(stage + fr * SR + q * 4);
                *reinterpret_cast<float4*>(reinterpret_cast<float*>(p_out) + (f0 + fr) * M + q * 4) = v;
              }
            }
            return;
          }
        }
        const long long f = f0 + fc;
        if (active && (FULL || f < p_frames)) {
          const bool flip_odd = (OS == 2) && (p.flags & PFB_FLAG_DEROTATE) && ((p.frame0 + f) & 1);
          // derotation of the 2x oversampled bank = a sign on the odd channels of odd frames.  As ONE multiply by a
          // per-lane +-1 (exact, -0 included); `if (flip) v = -v` per store compiled to a negate, a nop and four
          // v_cndmask in front of every store, flag set or not: 14 % of the cfg5 kernel's VALU instructions
          const v2f sg0 = splat((flip_odd && (kk & 1)) ? -1.f : 1.f), sg1 = splat((flip_odd && ((kk + KK) & 1)) ? -1.f : 1.f);
          auto derot = [&](v2f v, int k) { return OS == 2 ? v * (((k * KK) & 1) ? sg1 : sg0) : v; };
          const int shift = (p.flags & PFB_FLAG_FFTSHIFT) ? (M / 2) : 0;
          // fftshift(out,2): column (k + M/2) mod M.  For a power-of-two M that swaps the two halves of
          // the row, and since KK * R == M the butterfly outputs k < R/2 land in one half and k >= R/2 in
          // the other: two base pointers plus compile-time offsets instead of one address per store.
          auto col_of = [&](int ch) {
            const int c2 = ch + shift;
            return c2 >= M ? c2 - M : c2;
          };
          auto slot = [&](auto* rowp, int k) {
            if constexpr (K::POW2) {
              auto* lo = rowp + kk + shift;
              auto* hi = rowp + kk + (M / 2 - shift);
              return (k < R / 2) ? lo + k * KK : hi + (k - R / 2) * KK;
            } else {
              return rowp + col_of(kk + k * KK);
            }
          };
          if constexpr (CM || (!K::POW2 && K::NT == 64)) {
            // Channel-major: a frame-chunk's C frames of a channel are C consecutive elements, so a store
            // instruction still fills whole 32/64-byte runs (its lanes differ in fc).  The R addresses are
            // K columns apart (wrapping at M under fftshift); they are produced one at a time -- the opaque
            // asm keeps the compiler from materialising all R 64-bit addresses ahead of the butterfly,
            // which spilled.  The single-wave frame-major kernels with a non-power-of-two M (56) take the same
            // route with column stride 1 (+5 %); the 576-thread M=560 kernel measured 7 % slower that way.
            const bool mag = MAGSEL < 0 ? (p.flags & PFB_FLAG_MAGNITUDE) != 0 : MAGSEL == 1;
            const long long esz = mag ? 4 : 8;
            const long long cs = CM ? p.out_ld : 1;  // elements between adjacent channels
            int col = col_of(kk);
            char* ptr = reinterpret_cast<char*>(p_out) + ((long long)col * cs + (CM ? p.out_frame0 + f : f * M)) * esz;
            const long long step = (long long)KK * cs * esz, wrap = (long long)M * cs * esz;
#pragma unroll
            for (int k = 0; k < R; ++k) {
              v2f v = x[k];
              if (mag) {
                *reinterpret_cast<float*>(ptr) = mag_out(v.x, v.y, p.flags);
              } else {
                v = derot(v, k);
                store_c64(reinterpret_cast<float2*>(ptr), v, nontemporal);
              }
              asm volatile("" : "+v"(ptr) : : "memory");
              col += KK;
              ptr += step;
              if (col >= M) { col -= M; ptr -= wrap; }
            }
          } else if (MAGSEL == 1 || (MAGSEL < 0 && (p.flags & PFB_FLAG_MAGNITUDE))) {  // fused abs(): 4 bytes per channel instead of 8
            float* rowm = reinterpret_cast<float*>(p_out) + f0 * M + fc * M;
#pragma unroll
            for (int k = 0; k < R; ++k) *slot(rowm, k) = mag_out(x[k].x, x[k].y, p.flags);
          } else {
            float2* row = p_out + f0 * M + fc * M;
            // (probed: R/2 16-byte stores per lane instead of R 8-byte ones -- same bytes, half the store instructions,
            // written in a wrong layout just for the timing -- gain 0.4 % cfg2, 1.5 % cfg5, 2 % cfg4, 2.7 % cfg3 BEFORE the
            // lane exchange a correct layout needs (4 DPP moves per pair): not store-issue-bound, left alone)
#pragma unroll
            for (int k = 0; k < R; ++k) {
              const v2f v = derot(x[k], k);
              store_c64(slot(row, k), v, nontemporal);
            }
          }
        }
      }
    }
  }

  // The last pass of a single-wave kernel with its outputs left in LDS instead of stored: the chunk's buffer is
  // overwritten in place by the chunk TRANSPOSED, slot[column * C + frame] (fftshift and the derotation sign
  // applied), for run_tile_t's channel-major flush.  All of the wave's reads are issued before its first write
  // (the LDS executes one wave's accesses in order), so no second buffer is needed.
  // Where frame fc of column col sits inside the column's C-frame group of a transposed slot.  The LDS serves a
  // ds_write_b64 sixteen lanes at a time over 32 banks, i.e. over float2 addresses mod 16; the sixteen lanes of a
  // last-pass store are min(16, M / R) adjacent columns x the rest in frames, and col * C + fc puts columns
  // 16 / C apart on the same banks (rocprofv3: SQ_LDS_BANK_CONFLICT 0.19 cycles per sample, a 4-way conflict on
  // every store).  XOR-ing the column's higher bits into the frame index gives the sixteen lanes sixteen different
  // addresses mod 16; the flush reads whole groups per column, so the permutation inside a group costs it nothing
  // (counter after: 0).
  PFB_DEV int tslot_frame(int col, int fc) {
    constexpr int IPF = M / K::R(K::NP - 1), NFC = IPF >= 16 ? 1 : 16 / IPF, Q = 16 / C;
    static_assert(16 % C == 0 && (IPF >= 16 || 16 % IPF == 0) && C % NFC == 0, "power-of-two chunk and lane groups");
    return fc ^ (NFC * ((col / Q) % (C / NFC)));
  }

  PFB_DEV void last_pass_transposed(const KernelParams& p, float2* slot, int tid, long long f0) {
    constexpr int I = K::NP - 1;
    constexpr int R = K::R(I), KK = K::K(I), RS = K::RS(I);
    constexpr int IPF = M / R, ITEMS = C * IPF, ITERS = (ITEMS + NT - 1) / NT;
    static_assert(NT == 64 && !K::PINGPONG && K::S(I) == 1 && M * C <= K::LDS_ELEMS, "wave-local, in place");
    v2f x[ITERS][R];
#pragma unroll
    for (int it = 0; it < ITERS; ++it) {
      const int w = tid + it * NT;
      const bool active = (ITEMS % NT == 0) || (w < ITEMS);
      const int fc = w / IPF, item = w % IPF;
      const v2f* s2 = reinterpret_cast<const v2f*>(slot) + fc * K::FS + item;
#pragma unroll
      for (int n = 0; n < R; ++n) x[it][n] = active ? s2[n * RS] : (v2f){0.f, 0.f};
    }
    team_sync<true>();
    const int shift = (p.flags & PFB_FLAG_FFTSHIFT) ? (M / 2) : 0;
    v2f* t2 = reinterpret_cast<v2f*>(slot);
#pragma unroll
    for (int it = 0; it < ITERS; ++it) {
      const int w = tid + it * NT;
      const bool active = (ITEMS % NT == 0) || (w < ITEMS);
      const int fc = w / IPF, kk = w % IPF;
      Dft<R>::run(x[it]);
      if (active) {
        const bool flip_odd = (OS == 2) && (p.flags & PFB_FLAG_DEROTATE) && ((p.frame0 + f0 + fc) & 1);
        const v2f sg0 = splat((flip_odd && (kk & 1)) ? -1.f : 1.f), sg1 = splat((flip_odd && ((kk + KK) & 1)) ? -1.f : 1.f);
        int col = kk + shift;
        if (col >= M) col -= M;
#pragma unroll
        for (int k = 0; k < R; ++k) {
          v2f v = x[it][k];
          if constexpr (OS == 2) v = v * (((k * KK) & 1) ? sg1 : sg0);  // derotation sign, one multiply (see pass<>)
          t2[col * C + tslot_frame(col, fc)] = v;
          col += KK;
          if (col >= M) col -= M;
        }
      }
    }
  }

  // ---- per-thread constants shared by both schedules -------------------------------------------
  struct Consts {
    v2f hp[(W + 1) / 2][CPT];  // taps of this thread's columns, two per register pair
    v2f tw[2][16];             // inter-pass twiddles (c, s)
    int upos[OS][CPT];         // LDS position of the FIR outputs inside a frame (pass-0 layout)
    v2f conj_mul;
  };

  PFB_DEV float tap(const Consts& k, int j, int cc) { return (j & 1) ? k.hp[j >> 1][cc].y : k.hp[j >> 1][cc].x; }

  // Per-thread constants come from two small L2-resident tables laid out for 16-byte loads (built once
  // per handle by init_tables): taps_lane[c][0..WP) = h[(D-1-c) + D*j] and, per non-final pass,
  // tw_lane[rest][k] = e^{+j 2 pi rest k / (R S)}.  A wave needs WP/4 + R/2 wide loads instead of
  // W + R-1 narrow ones, which is what makes short-lived workgroups affordable.
  PFB_DEV void setup(const KernelParams& p, int tid, Consts& k) {
    const int c0 = tid * CPT;
#pragma unroll
    for (int cc = 0; cc < CPT; ++cc) {
      const int col = (K::LANES < NT && c0 >= D) ? 0 : c0 + cc;  // idle lanes read column 0's taps
      const float4* tl = reinterpret_cast<const float4*>(p.taps_lane + (size_t)col * K::WP);
#pragma unroll
      for (int q4 = 0; q4 < K::WP / 4; ++q4) {
        const float4 v = tl[q4];
        if (2 * q4 < (W + 1) / 2) k.hp[2 * q4][cc] = (v2f){v.x, v.y};
        if (2 * q4 + 1 < (W + 1) / 2) k.hp[2 * q4 + 1][cc] = (v2f){v.z, v.w};
      }
    }
    k.conj_mul = (v2f){1.f, (p.flags & PFB_FLAG_CONJUGATE_INPUT) ? -1.f : 1.f};
#pragma unroll
    for (int i = 0; i < K::NP - 1; ++i) {
      constexpr int dummy = 0; (void)dummy;
      const int R = K::R(i), S = K::S(i), IPF = M / R;
      if (C * IPF <= NT && !K::TW_TABLE) {
        const int rest = (tid % IPF) % S;
        const float4* t4 = reinterpret_cast<const float4*>(p.tw_lane + K::TW_OFF(i) + rest * K::TWR(i));
#pragma unroll
        for (int k2 = 0; k2 < 8; ++k2) {
          if (2 * k2 < R) {
            const float4 v = t4[k2];
            k.tw[i][2 * k2] = (v2f){v.x, v.y};
            k.tw[i][2 * k2 + 1] = (v2f){v.z, v.w};  // (the pad entry of an odd row: never used)
          }
        }
      }
    }
#pragma unroll
    for (int ph = 0; ph < OS; ++ph)
#pragma unroll
      for (int cc = 0; cc < CPT; ++cc) {
        const int n = (D - 1 - (c0 + cc)) + D * ph;
        k.upos[ph][cc] = (n / K::S(0)) * K::RS(0) + (n % K::S(0));
      }
  }

  // FIR of C frames from the window x (x[i] = row f0-(W-1)+i) into LDS, then the FFT passes and the
  // stores.  u_{p_lo + D ph}[t] = sum_q h[ph + OS q] * x[row t - ph - OS q]: one v_pk_fma_f32 per tap.
  template <bool WAVE_LOCAL = false, bool TRANSPOSED = false, bool FULL = false, int MAGSEL = -1>
  PFB_DEV void fir_fft_store(const KernelParams& p, const Consts& k, const v2f (&x)[NW][CPT], float2* lds, int tid,
                             long long f0) {
    float2* buf0 = lds;
    float2* buf1 = K::PINGPONG ? lds + K::BUF : lds;
#pragma unroll
    for (int ph = 0; ph < OS; ++ph)
#pragma unroll
      for (int cc = 0; cc < CPT; ++cc) {
        v2f acc[C];  // C independent chains: tap-major order keeps dependent pk_fma's C issues apart
        int tok = 0;  // FMA ordering token (fma_tap_lo)
#pragma unroll
        for (int q = 0; q < P; ++q) {
          const int j = ph + OS * q;
#pragma unroll
          for (int t = 0; t < C; ++t) {
            if (q == 0 && (j & 1)) fma_tap0_hi(acc[t], x[W - 1 + t - j][cc], k.hp[j >> 1][cc]);
            else if (q == 0) fma_tap0_lo(acc[t], x[W - 1 + t - j][cc], k.hp[j >> 1][cc]);
            else if (j & 1) fma_tap_hi(acc[t], x[W - 1 + t - j][cc], k.hp[j >> 1][cc], tok);
            else fma_tap_lo(acc[t], x[W - 1 + t - j][cc], k.hp[j >> 1][cc], tok);
          }
        }
        if (!(K::LANES < NT) || tid < K::LANES) {
#pragma unroll
          for (int t = 0; t < C; ++t)
            reinterpret_cast<v2f*>(buf0)[t * K::FS + k.upos[ph][cc]] = acc[t] * k.conj_mul;
        }
      }
    team_sync<WAVE_LOCAL>();
    pass<0>(p, buf0, buf1, tid, f0, k.tw);
    team_sync<WAVE_LOCAL>();
    if constexpr (TRANSPOSED) {
      static_assert(K::NP == 2 && WAVE_LOCAL, "single-wave two-pass plans");
      last_pass_transposed(p, buf1, tid, f0);
      return;
    } else if constexpr (K::NP == 2) {
      pass<1, FULL, MAGSEL>(p, buf1, nullptr, tid, f0, k.tw);
    } else {
      pass<1>(p, buf1, buf0, tid, f0, k.tw);
      team_sync<WAVE_LOCAL>();
      pass<2, FULL, MAGSEL>(p, buf0, nullptr, tid, f0, k.tw);
    }
    team_sync<WAVE_LOCAL>();  // the next chunk's FIR overwrites buf0
  }

  // the two halves of fir_fft_store as separate steps (schedule F gives them to different waves)
  // A thread's two adjacent columns c0, c0 + 1 are the adjacent branch outputs n0 = D-1-c0 (odd) and n0 - 1 (even) of
  // a frame, and where pass 0's rows are unpadded (RS_0 = S_0) they are adjacent in LDS: ONE 16-byte write per frame
  // instead of two 8-byte ones whose lanes sit 16 bytes apart (a 2-way bank conflict: 15 % of the M = 1024 team kernel's
  // LDS cycles, 19 % at M = 560).
  static constexpr bool kPairWrite = CPT == 2 && K::RS(0) == K::S(0) && K::S(0) % 2 == 0 && D % 2 == 0 && K::FS % 2 == 0 &&
                                     K::BUF % 2 == 0;
  PFB_DEV void fir_to_lds(const Consts& k, const v2f (&x)[NW][CPT], float2* buf, int tid) {
    if constexpr (kPairWrite) {
#pragma unroll
      for (int ph = 0; ph < OS; ++ph) {
        v2f acc[2][C];
#pragma unroll
        for (int cc = 0; cc < 2; ++cc) {
          int tok = 0;  // FMA ordering token (fma_tap_lo)
#pragma unroll
          for (int q = 0; q < P; ++q) {
            const int j = ph + OS * q;
#pragma unroll
            for (int t = 0; t < C; ++t) {
              if (q == 0 && (j & 1)) fma_tap0_hi(acc[cc][t], x[W - 1 + t - j][cc], k.hp[j >> 1][cc]);
              else if (q == 0) fma_tap0_lo(acc[cc][t], x[W - 1 + t - j][cc], k.hp[j >> 1][cc]);
              else if (j & 1) fma_tap_hi(acc[cc][t], x[W - 1 + t - j][cc], k.hp[j >> 1][cc], tok);
              else fma_tap_lo(acc[cc][t], x[W - 1 + t - j][cc], k.hp[j >> 1][cc], tok);
            }
          }
        }
        if (!(K::LANES < NT) || tid < K::LANES) {
#pragma unroll
          for (int t = 0; t < C; ++t) {
            const v2f lo = acc[1][t] * k.conj_mul, hi = acc[0][t] * k.conj_mul;  // positions n0 - 1, n0
            *reinterpret_cast<float4*>(buf + t * K::FS + k.upos[ph][1]) = make_float4(lo.x, lo.y, hi.x, hi.y);
          }
        }
      }
      return;
    }
#pragma unroll
    for (int ph = 0; ph < OS; ++ph)
#pragma unroll
      for (int cc = 0; cc < CPT; ++cc) {
        v2f acc[C];
        int tok = 0;  // FMA ordering token (fma_tap_lo)
#pragma unroll
        for (int q = 0; q < P; ++q) {
          const int j = ph + OS * q;
#pragma unroll
          for (int t = 0; t < C; ++t) {
            if (q == 0 && (j & 1)) fma_tap0_hi(acc[t], x[W - 1 + t - j][cc], k.hp[j >> 1][cc]);
            else if (q == 0) fma_tap0_lo(acc[t], x[W - 1 + t - j][cc], k.hp[j >> 1][cc]);
            else if (j & 1) fma_tap_hi(acc[t], x[W - 1 + t - j][cc], k.hp[j >> 1][cc], tok);
            else fma_tap_lo(acc[t], x[W - 1 + t - j][cc], k.hp[j >> 1][cc], tok);
          }
        }
        if (!(K::LANES < NT) || tid < K::LANES) {
#pragma unroll
          for (int t = 0; t < C; ++t)
            reinterpret_cast<v2f*>(buf)[t * K::FS + k.upos[ph][cc]] = acc[t] * k.conj_mul;
        }
      }
  }

  template <bool FULL = false, int MAGSEL = -1, int NTSEL = -1>
  PFB_DEV void fft_from_lds(const KernelParams& p, const Consts& k, float2* buf, int tid, long long f0) {
    static_assert(K::NP == 2 && !K::PINGPONG, "two in-place passes");
    pass<0>(p, buf, buf, tid, f0, k.tw);
    team_sync<true>();
    pass<1, FULL, MAGSEL, NTSEL>(p, buf, nullptr, tid, f0, k.tw);
  }
};

}  // namespace pfb
