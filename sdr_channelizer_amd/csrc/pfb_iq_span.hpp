// pfb_iq_span.hpp -- a span of an I/Q stream into LDS as float2: the input loader of the kernels that read "carried
// samples, then this call's" (pfb_stft.hip, pfb_mf.hip, pfb_mfbank.hip; device code only).
// The parameter struct P is the kernel's own (StftParams, MfParams, BankParams -- a template parameter, not a common
// base: a sub-struct would move kernel-argument offsets).  It has
//   const void* in;            this call's samples (device), format FMT
//   const void* carry;         carry_cap samples; the last carry_len precede in[0]
//   int carry_len, carry_cap;
// "Stream sample s" counts from the first carried sample: s < carry_len is carry[carry_cap - carry_len + s], the rest is
// in[s - carry_len].  Workgroups of kSpanThreads threads.
#pragma once

#include "pfb_cplx.hpp"

namespace pfb {

constexpr int kSpanThreads = 256;

PFB_DEV float2 swapped(float re, float im) { return make_float2(im, re); }

template <bool SWAP>
PFB_DEV float2 iq_put(float re, float im) {
  if constexpr (SWAP) return swapped(re, im);
  else return make_float2(re, im);
}

// stream sample s, components read one by one; SWAP: with re and im exchanged
template <int FMT, bool SWAP = false, class P>
PFB_DEV float2 iq_fetch(const P& p, long long s) {
  const long long g = s - p.carry_len;
  const void* b = g >= 0 ? p.in : p.carry;
  const long long i = g >= 0 ? g : p.carry_cap + g;
  if constexpr (FMT == PFB_FMT_INT16_IQ) {
    const int16_t* q = static_cast<const int16_t*>(b) + 2 * i;
    return iq_put<SWAP>((float)q[0], (float)q[1]);
  } else if constexpr (FMT == PFB_FMT_INT8_IQ) {
    const int8_t* q = static_cast<const int8_t*>(b) + 2 * i;
    return iq_put<SWAP>((float)q[0], (float)q[1]);
  } else {
    const float* q = static_cast<const float*>(b) + 2 * i;
    return iq_put<SWAP>(q[0], q[1]);
  }
}

// dst[i] = stream sample s0 + i, i < S; SWAP: with re and im exchanged.  PAD > 0: and dst[i] = 0 for S <= i < PAD, with
// S <= 0 for all zero (PAD = 0: S >= 0 and nothing past it is written).  A span that reaches into the carried samples
// is read one sample at a time; one in this call's buffer as a scalar head up to the first 16-byte boundary, whole
// 16-byte vectors, a scalar tail (int8: two samples in each 32-bit word's halves).
// The zero fill is part of this function, not of a caller's: the compiler simplifies a callee before it inlines it,
// and the int8 address arithmetic below comes out differently (same values, other instructions) without S > 0 in sight.
template <int FMT, bool SWAP, int PAD = 0, class P>
PFB_DEV void iq_load_span(const P& p, long long s0, int S, float2* dst) {
  using ST = SampleT<FMT>;
  constexpr int BPS = ST::kBytes, PER_VEC = 16 / BPS;
  const int tid = threadIdx.x;
  if constexpr (PAD > 0) {
    if (S < 0) S = 0;
    for (int i = S + tid; i < PAD; i += kSpanThreads) dst[i] = make_float2(0.f, 0.f);
    if (S == 0) return;
  }
  if (s0 < p.carry_len) {  // the span reaches into the carried samples
    for (int i = tid; i < S; i += kSpanThreads) dst[i] = iq_fetch<FMT, SWAP>(p, s0 + i);
    return;
  }
  // the process calls admit sample-aligned pointers only: every 16-byte vector holds whole samples
  const uintptr_t a0 = reinterpret_cast<uintptr_t>(p.in) + (uintptr_t)(s0 - p.carry_len) * BPS, a1 = a0 + (uintptr_t)S * BPS;
  const uintptr_t v0 = (a0 + 15) & ~(uintptr_t)15, v1 = a1 & ~(uintptr_t)15;
  int head = S, nvec = 0;  // samples before the first whole 16-byte vector, vectors
  if (v1 > v0) { head = (int)((v0 - a0) / BPS); nvec = (int)((v1 - v0) / 16); }
  const int tail0 = head + nvec * PER_VEC;
  for (int i = tid; i < head; i += kSpanThreads) dst[i] = iq_fetch<FMT, SWAP>(p, s0 + i);
  for (int i = tail0 + tid; i < S; i += kSpanThreads) dst[i] = iq_fetch<FMT, SWAP>(p, s0 + i);
  const uint4* src = reinterpret_cast<const uint4*>(v0);
  for (int i = tid; i < nvec; i += kSpanThreads) {
    const uint4 w = src[i];
    float2* d = dst + head + i * PER_VEC;
    float re, im;
    if constexpr (FMT == PFB_FMT_INT16_IQ) {
      const unsigned u[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
      for (int e = 0; e < 4; ++e) { ST::cvt(u[e], re, im); d[e] = iq_put<SWAP>(re, im); }
    } else if constexpr (FMT == PFB_FMT_INT8_IQ) {
      const unsigned u[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        ST::cvt((uint16_t)(u[e] & 0xffffu), re, im); d[2 * e] = iq_put<SWAP>(re, im);
        ST::cvt((uint16_t)(u[e] >> 16), re, im); d[2 * e + 1] = iq_put<SWAP>(re, im);
      }
    } else {
      d[0] = iq_put<SWAP>(__uint_as_float(w.x), __uint_as_float(w.y));
      d[1] = iq_put<SWAP>(__uint_as_float(w.z), __uint_as_float(w.w));
    }
  }
}

}  // namespace pfb
