// pfb_cplx.hpp -- packed-fp32 complex arithmetic and the in-register DFTs that the fused channelizer kernels
// (pfb_fast.hpp) and the STFT kernels (pfb_stft.hip) share.
#pragma once

#include "pfb_common.h"

namespace pfb {

// ---------------------------------------------------------------------------------
// Packed-fp32 complex arithmetic.  A complex value is one v2f (re, im) in an aligned VGPR
// pair, so every add / fma below is ONE v_pk_*_f32 issue (gfx950 issues a wave64 VALU op in
// 4 cycles whether it is scalar-fp32 or packed: packing halves the issue count, and the
// kernel is issue-bound long before it is flop-bound).

#define PFB_DEV static __device__ __forceinline__

typedef float v2f __attribute__((ext_vector_type(2)));

constexpr float kSqrtHalf = 0.70710678118654752f;
constexpr float kCosPi8 = 0.92387953251128674f;
constexpr float kSinPi8 = 0.38268343236508977f;

PFB_DEV v2f swp(v2f a) { return __builtin_shufflevector(a, a, 1, 0); }
PFB_DEV v2f splat(float s) { return (v2f){s, s}; }
PFB_DEV v2f fma2(v2f a, v2f b, v2f c) { return __builtin_elementwise_fma(a, b, c); }
// a * (c + j s): pk_mul + pk_fma (the swap and the broadcast ride on op_sel)
PFB_DEV v2f cmul(v2f a, float c, float s) { return fma2(swp(a), (v2f){-s, s}, a * splat(c)); }
// same with the twiddle held as ONE register pair w = (c, s): two instructions, no extra
// register for -s (neg_lo negates s for the real part only)
PFB_DEV v2f cmul_w(v2f a, v2f w) {
  v2f t, r;
  asm("v_pk_mul_f32 %0, %1, %2 op_sel_hi:[1,0]" : "=v"(t) : "v"(a), "v"(w));
  asm("v_pk_fma_f32 %0, %1, %2, %3 op_sel:[1,1,0] op_sel_hi:[0,1,1] neg_lo:[0,1,0]"
      : "=v"(r) : "v"(a), "v"(w), "v"(t));
  return r;
}
// acc += x * h.lo / h.hi (tap broadcast to both halves by op_sel): two taps share one register pair,
// which the compiler will not do by itself (it materialises a splat pair per tap)
PFB_DEV void fma_tap_lo(v2f& acc, v2f x, v2f h, int& tok) {
  (void)tok;
  asm("v_pk_fma_f32 %0, %1, %2, %0 op_sel_hi:[1,0,1]" : "+v"(acc) : "v"(x), "v"(h));
}
PFB_DEV void fma_tap_hi(v2f& acc, v2f x, v2f h, int& tok) {
  (void)tok;
  asm("v_pk_fma_f32 %0, %1, %2, %0 op_sel:[0,1,0] op_sel_hi:[1,1,1]" : "+v"(acc) : "v"(x), "v"(h));
}
// the first tap of a chain: acc = x * h + 0 with the zero as the instruction's inline constant -- the same operation on
// the same values as an FMA into a zeroed register pair, without the v_mov_b64 that zeroed it (C per column and chunk)
PFB_DEV void fma_tap0_lo(v2f& acc, v2f x, v2f h) {
  asm("v_pk_fma_f32 %0, %1, %2, 0 op_sel_hi:[1,0,0]" : "=v"(acc) : "v"(x), "v"(h));
}
PFB_DEV void fma_tap0_hi(v2f& acc, v2f x, v2f h) {
  asm("v_pk_fma_f32 %0, %1, %2, 0 op_sel:[0,1,0] op_sel_hi:[1,1,0]" : "=v"(acc) : "v"(x), "v"(h));
}
// The same FMAs as builtins: the broadcast is a shufflevector of the tap PAIR, which the backend folds into op_sel /
// op_sel_hi (checked in the ISA: no v_mov, one v_pk_fma_f32 per tap).  Inline asm hides the instruction from the
// scheduler: it clusters the FMAs of one accumulator, and on gfx950 the result of a packed-fp32 instruction cannot be read
// by the very next VALU instruction, so the hazard recognizer pads every such pair with an s_nop (118 per 250 FMAs in the
// cfg5 loop, 4 issue cycles each; 75 with the builtins, the rest sit in the FFT's cmul_w).  As builtins the scheduler
// interleaves the C accumulators itself -- at the price of longer live ranges: every other kernel spills with them
// (cfg2's pair kernel 6 registers, cfg3 36, the cfg4 teams 74), so only the software-pipelined cfg5 kernel takes them.
PFB_DEV void fma_tap_lo_b(v2f& acc, v2f x, v2f h) { acc = __builtin_elementwise_fma(x, __builtin_shufflevector(h, h, 0, 0), acc); }
PFB_DEV void fma_tap_hi_b(v2f& acc, v2f x, v2f h) { acc = __builtin_elementwise_fma(x, __builtin_shufflevector(h, h, 1, 1), acc); }
PFB_DEV v2f add_j(v2f a, v2f b) { return fma2(swp(b), (v2f){-1.f, 1.f}, a); }  // a + j b
PFB_DEV v2f sub_j(v2f a, v2f b) { return fma2(swp(b), (v2f){1.f, -1.f}, a); }  // a - j b

// Sync between the phases of one team.  A team that is the whole workgroup uses the workgroup
// barrier (a single-wave workgroup's barrier is free); single-wave teams inside a bigger workgroup
// only need program order within the wave: the LDS executes one wave's accesses in order, so the
// fences just stop the compiler from moving LDS accesses across the phase boundary.
template <bool WAVE_LOCAL>
PFB_DEV void team_sync() {
  if constexpr (WAVE_LOCAL) {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  } else {
    __syncthreads();
  }
}

// one complex64 output element; nontemporal = streaming store (output is write-once)
PFB_DEV void store_c64(float2* dst, v2f v, int nontemporal) {
  if (nontemporal) __builtin_nontemporal_store(v, reinterpret_cast<v2f*>(dst));
  else *reinterpret_cast<v2f*>(dst) = v;
}

// ---------------------------------------------------------------------------------
// In-register N-point DFT, kernel e^{+j 2 pi n k / N}, natural order in and out.

// X[K] = E + W^K O,  X[K+N/2] = E - W^K O,   W = e^{+j 2 pi / N}, N <= 16
template <int N, int K>
PFB_DEV void butterfly(v2f& lo, v2f& hi, v2f e, v2f o) {
  static_assert(16 % N == 0, "small DFT sizes only");
  constexpr int q = K * (16 / N);  // sixteenths of a turn, 0..7
  static_assert(q >= 0 && q < 8, "only the upper half plane is needed");
  if constexpr (q == 0) {
    lo = e + o; hi = e - o;
  } else if constexpr (q == 4) {  // W = +j
    lo = add_j(e, o); hi = sub_j(e, o);
  } else {
    constexpr float c = (q == 1) ? kCosPi8 : (q == 2) ? kSqrtHalf : (q == 3) ? kSinPi8
                        : (q == 5) ? -kSinPi8 : (q == 6) ? -kSqrtHalf : -kCosPi8;
    constexpr float s = (q == 1) ? kSinPi8 : (q == 2) ? kSqrtHalf : (q == 3) ? kCosPi8
                        : (q == 5) ? kCosPi8 : (q == 6) ? kSqrtHalf : kSinPi8;
    const v2f t = cmul(o, c, s);
    lo = e + t; hi = e - t;
  }
}

template <int N> struct Dft;

template <> struct Dft<2> {
  PFB_DEV void run(v2f (&x)[2]) {
    const v2f a = x[0];
    x[0] = a + x[1]; x[1] = a - x[1];
  }
};

template <> struct Dft<4> {
  PFB_DEV void run(v2f (&x)[4]) {
    const v2f t0 = x[0] + x[2], t1 = x[0] - x[2], t2 = x[1] + x[3], t3 = x[1] - x[3];
    x[0] = t0 + t2; x[2] = t0 - t2;
    x[1] = add_j(t1, t3); x[3] = sub_j(t1, t3);
  }
};

// 7-point DFT (the reference's own band count is fs*1e-6 = 56 = 8 x 7, channelizer_example.m:29):
// pair n with 7-n, X[k] = A_k + j B_k, X[7-k] = A_k - j B_k with
// A_k = x0 + sum_n (x_n + x_{7-n}) cos(2 pi k n / 7),  B_k = sum_n (x_n - x_{7-n}) sin(2 pi k n / 7)
template <> struct Dft<7> {
  PFB_DEV void run(v2f (&x)[7]) {
    constexpr float c1 = 0.62348980185873353f, c2 = -0.22252093395631440f, c3 = -0.90096886790241913f;
    constexpr float s1 = 0.78183148246802981f, s2 = 0.97492791218182361f, s3 = 0.43388373911755812f;
    const v2f p1 = x[1] + x[6], p2 = x[2] + x[5], p3 = x[3] + x[4];
    const v2f d1 = x[1] - x[6], d2 = x[2] - x[5], d3 = x[3] - x[4];
    const v2f x0 = x[0];
    const v2f a1 = fma2(p3, splat(c3), fma2(p2, splat(c2), fma2(p1, splat(c1), x0)));
    const v2f a2 = fma2(p3, splat(c1), fma2(p2, splat(c3), fma2(p1, splat(c2), x0)));
    const v2f a3 = fma2(p3, splat(c2), fma2(p2, splat(c1), fma2(p1, splat(c3), x0)));
    const v2f b1 = fma2(d3, splat(s3), fma2(d2, splat(s2), d1 * splat(s1)));
    const v2f b2 = fma2(d3, splat(-s1), fma2(d2, splat(-s3), d1 * splat(s2)));
    const v2f b3 = fma2(d3, splat(s2), fma2(d2, splat(-s1), d1 * splat(s3)));
    x[0] = x0 + p1 + p2 + p3;
    x[1] = add_j(a1, b1); x[6] = sub_j(a1, b1);
    x[2] = add_j(a2, b2); x[5] = sub_j(a2, b2);
    x[3] = add_j(a3, b3); x[4] = sub_j(a3, b3);
  }
};

// 5- and 10-point DFTs: the reference's other band count is round(fs / 0.1e6) = 560 = 10 x 8 x 7
// (generate_channelized_training_iq.m:95-96).  Same pairing as the 7-point one.
template <> struct Dft<5> {
  PFB_DEV void run(v2f (&x)[5]) {
    constexpr float c1 = 0.30901699437494742f, c2 = -0.80901699437494742f;
    constexpr float s1 = 0.95105651629515357f, s2 = 0.58778525229247313f;
    const v2f p1 = x[1] + x[4], p2 = x[2] + x[3];
    const v2f d1 = x[1] - x[4], d2 = x[2] - x[3];
    const v2f x0 = x[0];
    const v2f a1 = fma2(p2, splat(c2), fma2(p1, splat(c1), x0));
    const v2f a2 = fma2(p2, splat(c1), fma2(p1, splat(c2), x0));
    const v2f b1 = fma2(d2, splat(s2), d1 * splat(s1));
    const v2f b2 = fma2(d2, splat(-s1), d1 * splat(s2));
    x[0] = x0 + p1 + p2;
    x[1] = add_j(a1, b1); x[4] = sub_j(a1, b1);
    x[2] = add_j(a2, b2); x[3] = sub_j(a2, b2);
  }
};

template <> struct Dft<10> {
  PFB_DEV void run(v2f (&x)[10]) {
    // W_10^k = e^{+j 2 pi k / 10}
    constexpr float c1 = 0.80901699437494742f, s1 = 0.58778525229247313f;
    constexpr float c2 = 0.30901699437494742f, s2 = 0.95105651629515357f;
    v2f e[5], o[5];
#pragma unroll
    for (int k = 0; k < 5; ++k) { e[k] = x[2 * k]; o[k] = x[2 * k + 1]; }
    Dft<5>::run(e);
    Dft<5>::run(o);
    const v2f t1 = cmul(o[1], c1, s1), t2 = cmul(o[2], c2, s2), t3 = cmul(o[3], -c2, s2), t4 = cmul(o[4], -c1, s1);
    x[0] = e[0] + o[0]; x[5] = e[0] - o[0];
    x[1] = e[1] + t1;   x[6] = e[1] - t1;
    x[2] = e[2] + t2;   x[7] = e[2] - t2;
    x[3] = e[3] + t3;   x[8] = e[3] - t3;
    x[4] = e[4] + t4;   x[9] = e[4] - t4;
  }
};

// 3-, 6- and 12-point DFTs: band counts with a factor 3 (numBands = fs * 1e-6 at 12, 24, 30, 48, 96, 120 Msps,
// channelizer_example.m:29).  W_3 = e^{+j 2 pi / 3} = -1/2 + j sqrt(3)/2.
template <> struct Dft<3> {
  PFB_DEV void run(v2f (&x)[3]) {
    constexpr float s = 0.86602540378443865f;
    const v2f p = x[1] + x[2], d = x[1] - x[2];
    const v2f a = fma2(p, splat(-0.5f), x[0]), b = d * splat(s);
    x[0] = x[0] + p;
    x[1] = add_j(a, b);
    x[2] = sub_j(a, b);
  }
};

template <> struct Dft<6> {
  PFB_DEV void run(v2f (&x)[6]) {
    constexpr float s = 0.86602540378443865f;
    v2f e[3] = {x[0], x[2], x[4]}, o[3] = {x[1], x[3], x[5]};
    Dft<3>::run(e);
    Dft<3>::run(o);
    const v2f t1 = cmul(o[1], 0.5f, s), t2 = cmul(o[2], -0.5f, s);  // W_6^1, W_6^2
    x[0] = e[0] + o[0]; x[3] = e[0] - o[0];
    x[1] = e[1] + t1;   x[4] = e[1] - t1;
    x[2] = e[2] + t2;   x[5] = e[2] - t2;
  }
};

template <> struct Dft<12> {
  PFB_DEV void run(v2f (&x)[12]) {
    constexpr float s = 0.86602540378443865f;
    v2f e[6], o[6];
#pragma unroll
    for (int k = 0; k < 6; ++k) { e[k] = x[2 * k]; o[k] = x[2 * k + 1]; }
    Dft<6>::run(e);
    Dft<6>::run(o);
    // W_12^k = e^{+j 2 pi k / 12}: (s, 1/2), (1/2, s), j, (-1/2, s), (-s, 1/2)
    const v2f t1 = cmul(o[1], s, 0.5f), t2 = cmul(o[2], 0.5f, s), t4 = cmul(o[4], -0.5f, s), t5 = cmul(o[5], -s, 0.5f);
    x[0] = e[0] + o[0];       x[6] = e[0] - o[0];
    x[1] = e[1] + t1;         x[7] = e[1] - t1;
    x[2] = e[2] + t2;         x[8] = e[2] - t2;
    x[3] = add_j(e[3], o[3]); x[9] = sub_j(e[3], o[3]);
    x[4] = e[4] + t4;         x[10] = e[4] - t4;
    x[5] = e[5] + t5;         x[11] = e[5] - t5;
  }
};

// 14 = 2 x 7 (560 = 14 x 10 x 4 keeps every non-final pass of the team kernel at one item per lane)
template <> struct Dft<14> {
  PFB_DEV void run(v2f (&x)[14]) {
    // W_14^k = e^{+j 2 pi k / 14}, k = 1..6
    constexpr float c1 = 0.90096886790241915f, s1 = 0.43388373911755812f;
    constexpr float c2 = 0.62348980185873359f, s2 = 0.78183148246802980f;
    constexpr float c3 = 0.22252093395631445f, s3 = 0.97492791218182362f;
    v2f e[7], o[7];
#pragma unroll
    for (int k = 0; k < 7; ++k) { e[k] = x[2 * k]; o[k] = x[2 * k + 1]; }
    Dft<7>::run(e);
    Dft<7>::run(o);
    const v2f t1 = cmul(o[1], c1, s1), t2 = cmul(o[2], c2, s2), t3 = cmul(o[3], c3, s3);
    const v2f t4 = cmul(o[4], -c3, s3), t5 = cmul(o[5], -c2, s2), t6 = cmul(o[6], -c1, s1);
    x[0] = e[0] + o[0]; x[7] = e[0] - o[0];
    x[1] = e[1] + t1;   x[8] = e[1] - t1;
    x[2] = e[2] + t2;   x[9] = e[2] - t2;
    x[3] = e[3] + t3;   x[10] = e[3] - t3;
    x[4] = e[4] + t4;   x[11] = e[4] - t4;
    x[5] = e[5] + t5;   x[12] = e[5] - t5;
    x[6] = e[6] + t6;   x[13] = e[6] - t6;
  }
};

template <int N, int K>
struct DftCombine {
  PFB_DEV void run(v2f (&x)[N], const v2f (&e)[N / 2], const v2f (&o)[N / 2]) {
    butterfly<N, K>(x[K], x[K + N / 2], e[K], o[K]);
    if constexpr (K + 1 < N / 2) DftCombine<N, K + 1>::run(x, e, o);
  }
};

template <int N> struct Dft {
  PFB_DEV void run(v2f (&x)[N]) {
    v2f e[N / 2], o[N / 2];
#pragma unroll
    for (int k = 0; k < N / 2; ++k) { e[k] = x[2 * k]; o[k] = x[2 * k + 1]; }
    Dft<N / 2>::run(e);
    Dft<N / 2>::run(o);
    DftCombine<N, 0>::run(x, e, o);
  }
};

}  // namespace pfb
