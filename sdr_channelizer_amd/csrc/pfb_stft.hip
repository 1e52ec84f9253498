// pfb_stft.hip -- gfx950 kernels of the short-time Fourier transform (pfb_stft_* in include/pfb_channelizer.h).
//
//   pfb_stft_fused<NFFT, FMT>   nfft in {256, 512, 768, 1024, 2048} x {int8, int16, cf32}, any L <= nfft, any
//                               1 <= H <= L, every output kind and row order
//   pfb_stft_generic_kernel     any nfft <= 4096: 2^a 3^b 5^c 7^d by the mixed-radix Stockham stages the channelizer's
//                               generic kernel uses (pfb_generic_fft.hpp), a plain DFT otherwise
//
// Fused kernel: short-lived 256-thread workgroups in dispatch order, workgroup b covering frames [b T, b T + T).
//   LOAD   the tile's input span, (T-1) H + L samples, once (pfb_iq_span.hpp): 16 bytes per lane where the span lies in
//          this call's buffer, converted to float and kept in LDS -- overlapping frames read their shared samples from LDS, not
//          from HBM.
//   FFT    Stockham passes of compile-time radix (R0 x R1 [x R2]), each butterfly an in-register Dft<R> of
//          pfb_cplx.hpp with one LDS exchange between passes.  The first pass reads the span, multiplies by the window
//          table (window x 2^-(bw-1), one float per point) and supplies the zero padding n >= L.  Dft<R> is the
//          e^{+j} kernel: the span is stored with re and im swapped and every result is read back swapped,
//          DFT-(x) = swap(DFT+(swap(x))), so the e^{-j} transform costs nothing.
//   STORE  the row rotation ('centered' or FFT order) is applied while reading the last pass's buffer, so every frame
//          leaves as consecutive 16-byte-per-lane stores (the tile's T * nfft outputs are one contiguous run).
// LDS: two T x nfft complex buffers (the span, at most T L <= T nfft samples, lives in the first), 32-36 KiB.
#include "pfb_cplx.hpp"
#include "pfb_generic_fft.hpp"
#include "pfb_iq_span.hpp"

namespace pfb {

namespace {

// FFT plan of a fused length: radices of the passes (R2 = 1: two passes) and frames per workgroup (T nfft ~ 2048:
// 32-36 KiB of LDS, four or five workgroups per CU; DESIGN.md section 11 has the measurements)
template <int NFFT> struct StftCfg;
template <> struct StftCfg<256> { static constexpr int R0 = 16, R1 = 16, R2 = 1, T = 8; };
template <> struct StftCfg<512> { static constexpr int R0 = 8, R1 = 8, R2 = 8, T = 4; };
template <> struct StftCfg<768> { static constexpr int R0 = 12, R1 = 8, R2 = 8, T = 3; };
template <> struct StftCfg<1024> { static constexpr int R0 = 16, R1 = 8, R2 = 8, T = 2; };
template <> struct StftCfg<2048> { static constexpr int R0 = 16, R1 = 16, R2 = 8, T = 1; };

constexpr int kStftThreads = kSpanThreads;

// first pass (sub-transforms of length 1, no twiddles): windowed, zero-padded frame t read from the span
template <int N, int R>
PFB_DEV void stft_first_pass(const float2* span, float2* dst, int frames, int L, int H, const float* __restrict__ win) {
  constexpr int NB = N / R;
  for (int b = threadIdx.x; b < frames * NB; b += kStftThreads) {
    const int t = b / NB, j = b - t * NB;
    v2f x[R];
#pragma unroll
    for (int q = 0; q < R; ++q) {
      const int n = j + q * NB;
      if (n < L) {
        const float2 v = span[t * H + n];
        x[q] = (v2f){v.x, v.y} * splat(win[n]);
      } else {
        x[q] = (v2f){0.f, 0.f};  // zero padding: never a product with a (possibly non-finite) sample
      }
    }
    Dft<R>::run(x);
    float2* d = dst + t * N + j * R;
#pragma unroll
    for (int q = 0; q < R; ++q) d[q] = make_float2(x[q].x, x[q].y);
  }
}

// Stockham pass of radix R after sub-transforms of length NS (pfb_generic_fft.hpp, radix and lengths at compile time)
template <int N, int R, int NS>
PFB_DEV void stft_pass(const float2* src, float2* dst, int frames, const float2* __restrict__ tw) {
  constexpr int NB = N / R, TSTEP = N / (NS * R);
  for (int b = threadIdx.x; b < frames * NB; b += kStftThreads) {
    const int t = b / NB, j = b - t * NB, k = j % NS;
    v2f x[R];
#pragma unroll
    for (int q = 0; q < R; ++q) {
      const float2 v = src[t * N + j + q * NB];
      x[q] = (v2f){v.x, v.y};
    }
#pragma unroll
    for (int q = 1; q < R; ++q) {
      const float2 w = tw[q * k * TSTEP];
      x[q] = cmul(x[q], w.x, w.y);
    }
    Dft<R>::run(x);
    float2* d = dst + t * N + (j / NS) * NS * R + k;
#pragma unroll
    for (int q = 0; q < R; ++q) d[q * NS] = make_float2(x[q].x, x[q].y);
  }
}

PFB_DEV float stft_real_out(float2 v, int output, float scale, float db_floor) {
  const float m2 = (v.x * v.x + v.y * v.y) * scale;
  return output == PFB_STFT_DB ? 10.f * log10f(m2 + db_floor) : m2;
}

// the epilogue shared by both kernels: output element idx of the tile (frame idx / N, row idx % N) from the last
// pass's buffer y (frames of N bins in FFT order, values swapped)
PFB_DEV float2 stft_row(const float2* y, int idx, int N, int shift) {
  const int t = idx / N, r = idx - t * N;
  int bin = r + shift;
  if (bin >= N) bin -= N;
  const float2 v = y[t * N + bin];
  return make_float2(v.y, v.x);
}

// 'centered': row r holds bin k_r = r - nfft/2 + 1 (even) / r - (nfft-1)/2 (odd), i.e. FFT bin (r + shift) mod nfft
inline __host__ __device__ int stft_shift(int N, int order) {
  return order == PFB_STFT_TWOSIDED ? 0 : (N % 2 == 0 ? N / 2 + 1 : (N + 1) / 2);
}

// NC: the FFT length at compile time (fused kernels), 0 = p.nfft (generic)
template <int NC>
PFB_DEV void stft_store(const StftParams& p, const float2* y, long long f0, int frames) {
  const int N = NC ? NC : p.nfft, tid = threadIdx.x, E = frames * N, shift = stft_shift(N, p.order);
  if (p.output == PFB_STFT_COMPLEX) {
    float2* o = static_cast<float2*>(p.out) + f0 * N;
    if (reinterpret_cast<uintptr_t>(o) % 16 == 0 && E % 2 == 0) {
      for (int v = tid; v < E / 2; v += kStftThreads) {
        const float2 a = stft_row(y, 2 * v, N, shift), b = stft_row(y, 2 * v + 1, N, shift);
        reinterpret_cast<float4*>(o)[v] = make_float4(a.x, a.y, b.x, b.y);
      }
    } else {
      for (int i = tid; i < E; i += kStftThreads) o[i] = stft_row(y, i, N, shift);
    }
  } else {
    float* o = static_cast<float*>(p.out) + f0 * N;
    if (reinterpret_cast<uintptr_t>(o) % 16 == 0 && E % 4 == 0) {
      for (int v = tid; v < E / 4; v += kStftThreads) {
        float r[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) r[e] = stft_real_out(stft_row(y, 4 * v + e, N, shift), p.output, p.scale, p.db_floor);
        reinterpret_cast<float4*>(o)[v] = make_float4(r[0], r[1], r[2], r[3]);
      }
    } else {
      for (int i = tid; i < E; i += kStftThreads) o[i] = stft_real_out(stft_row(y, i, N, shift), p.output, p.scale, p.db_floor);
    }
  }
}

// LOADSTORE: the timing study of pfb_stft_set_experiment (pfb_channelizer_dev.h) -- the same span loads and output
// stores with the window and the FFT passes left out (the stores read the span buffer): where the kernel's time goes
template <int NFFT, int FMT, bool LOADSTORE>
__global__ void __launch_bounds__(kStftThreads) pfb_stft_fused(const StftParams p) {
  using Cfg = StftCfg<NFFT>;
  constexpr int T = Cfg::T;
  __shared__ float2 buf_a[T * NFFT];
  __shared__ float2 buf_b[T * NFFT];
  const long long f0 = (long long)blockIdx.x * T;
  const int frames = (int)min((long long)T, p.frames - f0);
  iq_load_span<FMT, true>(p, f0 * p.H, (frames - 1) * p.H + p.L, buf_a);  // re and im exchanged
  __syncthreads();
  if constexpr (LOADSTORE) {
    stft_store<NFFT>(p, buf_a, f0, frames);
    return;
  }
  stft_first_pass<NFFT, Cfg::R0>(buf_a, buf_b, frames, p.L, p.H, p.win);
  __syncthreads();
  stft_pass<NFFT, Cfg::R1, Cfg::R0>(buf_b, buf_a, frames, p.tw);
  __syncthreads();
  if constexpr (Cfg::R2 > 1) {
    stft_pass<NFFT, Cfg::R2, Cfg::R0 * Cfg::R1>(buf_a, buf_b, frames, p.tw);
    __syncthreads();
    stft_store<NFFT>(p, buf_b, f0, frames);
  } else {
    stft_store<NFFT>(p, buf_a, f0, frames);
  }
}

template <int NFFT, int FMT, bool LOADSTORE>
hipError_t launch_stft_fused(const StftParams& p, hipStream_t s) {
  static_assert(StftCfg<NFFT>::R0 * StftCfg<NFFT>::R1 * StftCfg<NFFT>::R2 == NFFT, "plan must cover the length");
  if (p.frames <= 0) return hipSuccess;
  const long long blocks = (p.frames + StftCfg<NFFT>::T - 1) / StftCfg<NFFT>::T;
  hipLaunchKernelGGL((pfb_stft_fused<NFFT, FMT, LOADSTORE>), dim3((unsigned)blocks), dim3(kStftThreads), 0, s, p);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------------
// generic kernel: tile frames per workgroup, sm holds 2 x tile x nfft complex

PFB_DEV float2 stft_fetch_rt(const StftParams& p, long long s) {
  if (p.fmt == PFB_FMT_INT16_IQ) return iq_fetch<PFB_FMT_INT16_IQ>(p, s);
  if (p.fmt == PFB_FMT_INT8_IQ) return iq_fetch<PFB_FMT_INT8_IQ>(p, s);
  return iq_fetch<PFB_FMT_CF32>(p, s);
}

__global__ void __launch_bounds__(256) pfb_stft_generic_kernel(const StftParams p, int tile, GenericPlan plan) {
  extern __shared__ float2 sm[];
  const int N = p.nfft, tid = threadIdx.x, nt = blockDim.x;
  const long long f0 = (long long)blockIdx.x * tile;
  const int frames = (int)min((long long)tile, p.frames - f0);
  for (int idx = tid; idx < tile * N; idx += nt) {
    const int t = idx / N, n = idx - t * N;
    float2 v = make_float2(0.f, 0.f);
    if (t < frames && n < p.L) {
      const float2 x = stft_fetch_rt(p, (f0 + t) * p.H + n);
      v = swapped(x.x * p.win[n], x.y * p.win[n]);
    }
    sm[idx] = v;
  }
  __syncthreads();
  if (plan.n > 0) generic_stockham(sm, tile, N, plan, p.tw, tid, nt);
  else generic_dft(sm, tile, N, p.tw, tid, nt);
  const float2* y = sm + tile * N;
  const int shift = stft_shift(N, p.order);
  for (int i = tid; i < frames * N; i += nt) {
    const float2 v = stft_row(y, i, N, shift);
    const long long o = f0 * N + i;
    if (p.output == PFB_STFT_COMPLEX) static_cast<float2*>(p.out)[o] = v;
    else static_cast<float*>(p.out)[o] = stft_real_out(v, p.output, p.scale, p.db_floor);
  }
}

hipError_t launch_stft_generic(const StftParams& p, hipStream_t s) {
  if (p.frames <= 0) return hipSuccess;
  int tile = 4096 / p.nfft;
  if (tile < 1) tile = 1;
  if (tile > 16) tile = 16;
  const size_t shmem = (size_t)tile * p.nfft * sizeof(float2) * 2;
  if (shmem > 64 * 1024) return hipErrorInvalidValue;
  const GenericPlan plan = make_generic_plan(p.nfft);
  const long long blocks = (p.frames + tile - 1) / tile;
  hipLaunchKernelGGL(pfb_stft_generic_kernel, dim3((unsigned)blocks), dim3(256), shmem, s, p, tile, plan);
  return hipGetLastError();
}

struct StftEntry {
  int nfft, fmt;
  StftKernelInfo info;
};

#define PFB_STFT_ROW(N, FMT, TAG)                                                                   \
  {N, FMT, {launch_stft_fused<N, FMT, false>, "pfb_stft_fused<N" #N "," TAG ">", launch_stft_fused<N, FMT, true>, \
            "pfb_stft_loadstore<N" #N "," TAG ">"}}
#define PFB_STFT_ROWS(N) PFB_STFT_ROW(N, PFB_FMT_INT8_IQ, "int8"), PFB_STFT_ROW(N, PFB_FMT_INT16_IQ, "int16"), \
                         PFB_STFT_ROW(N, PFB_FMT_CF32, "cf32")
const StftEntry kStftFused[] = {PFB_STFT_ROWS(256), PFB_STFT_ROWS(512), PFB_STFT_ROWS(768), PFB_STFT_ROWS(1024),
                                PFB_STFT_ROWS(2048)};
#undef PFB_STFT_ROWS
#undef PFB_STFT_ROW

const StftKernelInfo kStftGeneric = {launch_stft_generic, "pfb_stft_generic", nullptr, nullptr};

}  // namespace

const StftKernelInfo* find_stft_fused(int nfft, int fmt) {
  for (const StftEntry& e : kStftFused)
    if (e.nfft == nfft && e.fmt == fmt) return &e.info;
  return nullptr;
}

const StftKernelInfo* stft_generic_kernel() { return &kStftGeneric; }

}  // namespace pfb
