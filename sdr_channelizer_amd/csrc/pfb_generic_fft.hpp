// pfb_generic_fft.hpp -- the run-time-sized FFT stages shared by the generic kernels (pfb_generic_kernel in
// pfb_kernels.hip, pfb_stft_generic_kernel in pfb_stft.hip).  Both run tile_frames independent M-point transforms
// held frame after frame in LDS, kernel e^{+j 2 pi n k / M}, with the whole workgroup cooperating on every stage.
#pragma once

#include "pfb_common.h"

namespace pfb {

// Radices of the mixed-radix FFT (lengths M = 2^a 3^b 5^c 7^d): at most 12 stages (2^12 = 4096 = the largest M either
// path accepts); n = 0: M has another prime factor, plain DFT.
struct GenericPlan { int n; unsigned char r[12]; };

// 7, 5, 3 first, then 4s and a 2: every stage length divides M by construction
static inline GenericPlan make_generic_plan(int M) {
  GenericPlan plan{};
  int m = M;
  for (int r : {7, 5, 3, 4, 2})
    while (m % r == 0 && plan.n < 12) { plan.r[plan.n++] = (unsigned char)r; m /= r; }
  if (m != 1) plan.n = 0;
  return plan;
}

// Stockham autosort, radices 2 ... 7 at run time: O(M sum r) per frame instead of the plain DFT's O(M^2).  Stage with
// radix r after sub-transforms of length Ns: butterfly j takes a[j + q M/r] e^{+j 2 pi q k / (Ns r)} (k = j mod Ns), an
// r-point DFT of those (twiddles from the M-entry table tw[m] = e^{+j 2 pi m / M}: Ns r and r divide M), and leaves u_q
// at (j / Ns) Ns r + k + q Ns of the other buffer: natural order at the end.  Input in sm[0, tile_frames*M), result in
// sm[tile_frames*M, 2*tile_frames*M); ends with a workgroup barrier.
static __device__ __forceinline__ void generic_stockham(float2* sm, int tile_frames, int M, const GenericPlan& plan,
                                                        const float2* tw, int tid, int nt) {
  float2* a = sm;
  float2* b = sm + tile_frames * M;
  int Ns = 1;
  for (int st = 0; st < plan.n; ++st) {
    const int r = plan.r[st], nb = M / r, tstep = M / (Ns * r), rstep = M / r;
    for (int idx = tid; idx < tile_frames * nb; idx += nt) {
      const int t = idx / nb, j = idx - t * nb;
      const int k = j % Ns;
      float2 v[7];
      for (int q = 0; q < r; ++q) {
        const float2 x = a[t * M + j + q * nb], w = tw[(q * k * tstep) % M];
        v[q] = make_float2(x.x * w.x - x.y * w.y, x.x * w.y + x.y * w.x);
      }
      float2* dst = b + t * M + (j / Ns) * Ns * r + k;
      for (int pp = 0; pp < r; ++pp) {
        float ur = 0.f, ui = 0.f;
        for (int q = 0; q < r; ++q) {
          const float2 w = tw[((pp * q) % r) * rstep];
          ur += v[q].x * w.x - v[q].y * w.y;
          ui += v[q].x * w.y + v[q].y * w.x;
        }
        dst[pp * Ns] = make_float2(ur, ui);
      }
    }
    __syncthreads();
    float2* sw = a; a = b; b = sw;
    Ns *= r;
  }
  if (a != sm + tile_frames * M) {  // the epilogue reads the second half
    for (int idx = tid; idx < tile_frames * M; idx += nt) sm[tile_frames * M + idx] = a[idx];
    __syncthreads();
  }
}

// plain DFT of sm[0, tile_frames*M) into sm[tile_frames*M, 2*tile_frames*M); ends with a workgroup barrier
static __device__ __forceinline__ void generic_dft(float2* sm, int tile_frames, int M, const float2* tw, int tid, int nt) {
  float2* y = sm + tile_frames * M;
  for (int idx = tid; idx < tile_frames * M; idx += nt) {
    const int t = idx / M, k = idx - t * M;
    float ar = 0.f, ai = 0.f;
    int j = 0;  // (k*p) mod M, advanced incrementally
    for (int pp = 0; pp < M; ++pp) {
      const float2 u = sm[t * M + pp], w = tw[j];
      ar += u.x * w.x - u.y * w.y;
      ai += u.x * w.y + u.y * w.x;
      j += k; if (j >= M) j -= M;
    }
    y[idx] = make_float2(ar, ai);
  }
  __syncthreads();
}

}  // namespace pfb
