// pfb_ols.hpp -- the overlap-save FFT core that the matched filter (pfb_mf.hip) and its frequency-offset bank
// (pfb_mfbank.hip) share (device code only): the Stockham passes of one NFFT-point transform in LDS by a 256-thread
// workgroup and the |y|^2 row store.  A block is loaded by iq_load_span<FMT, false, NFFT> of pfb_iq_span.hpp.  The
// kernels, their parameter structs and what they do between the passes stay in the two units.
#pragma once

#include "pfb_cplx.hpp"
#include "pfb_iq_span.hpp"

namespace pfb {

constexpr int kOlsThreads = kSpanThreads;

// radices of the three passes: 16 x 8 x 8, 16 x 16 x 8, 16 x 16 x 16
template <int NFFT> struct OlsPlan;
template <> struct OlsPlan<1024> { static constexpr int R0 = 16, R1 = 8, R2 = 8; };
template <> struct OlsPlan<2048> { static constexpr int R0 = 16, R1 = 16, R2 = 8; };
template <> struct OlsPlan<4096> { static constexpr int R0 = 16, R1 = 16, R2 = 16; };

// first pass (sub-transforms of length 1, no twiddles).  MUL: the operands are src[n] * spec[n] with re and im exchanged,
// the way into the e^{-j} transform
template <int N, int R, bool MUL>
PFB_DEV void ols_first_pass(const float2* src, float2* dst, const float2* __restrict__ spec) {
  constexpr int NB = N / R;
  for (int j = threadIdx.x; j < NB; j += kOlsThreads) {
    v2f x[R];
#pragma unroll
    for (int q = 0; q < R; ++q) {
      const float2 v = src[j + q * NB];
      if constexpr (MUL) {
        const float2 h = spec[j + q * NB];
        x[q] = swp(cmul((v2f){v.x, v.y}, h.x, h.y));
      } else {
        x[q] = (v2f){v.x, v.y};
      }
    }
    Dft<R>::run(x);
    float2* d = dst + j * R;
#pragma unroll
    for (int q = 0; q < R; ++q) d[q] = make_float2(x[q].x, x[q].y);
  }
}

// Stockham pass of radix R after sub-transforms of length NS
template <int N, int R, int NS>
PFB_DEV void ols_pass(const float2* src, float2* dst, const float2* __restrict__ tw) {
  constexpr int NB = N / R, TSTEP = N / (NS * R);
  for (int j = threadIdx.x; j < NB; j += kOlsThreads) {
    const int k = j % NS;
    v2f x[R];
#pragma unroll
    for (int q = 0; q < R; ++q) {
      const float2 v = src[j + q * NB];
      x[q] = (v2f){v.x, v.y};
    }
#pragma unroll
    for (int q = 1; q < R; ++q) {
      const float2 w = tw[q * k * TSTEP];
      x[q] = cmul(x[q], w.x, w.y);
    }
    Dft<R>::run(x);
    float2* d = dst + (j / NS) * NS * R + k;
#pragma unroll
    for (int q = 0; q < R; ++q) d[q * NS] = make_float2(x[q].x, x[q].y);
  }
}

// the inverse's result holds y with re and im exchanged: the power is the same
PFB_DEV float ols_power(const float2* y, int i) {
  const float2 v = y[i];
  return v.x * v.x + v.y * v.y;
}

// o[0 .. count) = |y[0 .. count)|^2: a scalar head up to the first 16-byte boundary of o, whole 16-byte vectors, a
// scalar tail
PFB_DEV void ols_store_power(float* o, const float2* y, int count) {
  const int tid = threadIdx.x;
  const int head = min((int)(((16 - reinterpret_cast<uintptr_t>(o) % 16) % 16) / 4), count);
  const int nvec = (count - head) / 4, tail0 = head + 4 * nvec;
  if (tid < head) o[tid] = ols_power(y, tid);
  for (int v = tid; v < nvec; v += kOlsThreads) {
    const int i = head + 4 * v;
    *reinterpret_cast<float4*>(o + i) = make_float4(ols_power(y, i), ols_power(y, i + 1), ols_power(y, i + 2), ols_power(y, i + 3));
  }
  if (tid < count - tail0) o[tail0 + tid] = ols_power(y, tail0 + tid);
}

}  // namespace pfb
