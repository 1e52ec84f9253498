// pfb_mf.hip -- matched filter (pulse compression) of an I/Q stream against a coded-pulse replica (pfb_mf_* in
// include/pfb_channelizer.h), kernels and host side.  The pulses it looks for are the reference's own:
//   matlab/generate_pulsed_iq.m:17-19,43-59              LFM sweeps and Barker-13 chips
//   tx_rx_pulses_usrp.cpp:24,141-142,212-242,284-291     a 13-chip burst sent and the dwell received, two .iq records
//   matlab/generate_training_iq.m:16-22                  pulse widths up to 1000 us (56 000 samples at 56 MS/s)
// Arithmetic:
//   x[n] = (I[n] + jQ[n]) / 2^(bit_width-1)            (cf32: as given)
//   y[m] = g * sum_{n=0}^{K-1} conj(r[n]) * x[m+n]        m = 0, 1, ...  (stream-absolute), complete windows only
// by overlap-save fast convolution in fp32: a block of NFFT samples is transformed, multiplied by the replica's
// spectrum and transformed back; the outputs whose window does not wrap are kept.  The spectra are made on the host in
// float64 with g, 2^-(bit_width-1) and the 1/NFFT of the inverse folded in, rounded once to float32.
//
//   pfb_mf_fused<NFFT, FMT>     NFFT in {1024, 2048, 4096} x {int8, int16, cf32}, K <= NFFT/2.  One short-lived
//                               256-thread workgroup per block of V = NFFT - K + 1 outputs, in dispatch order:
//     LOAD     the block's NFFT samples once (iq_load_span, pfb_iq_span.hpp), 16 bytes per lane where the span lies in
//              this call's buffer, the carried samples from the carry buffer; samples past the call's end are zero
//     FORWARD  three Stockham passes of compile-time radix (16 x 8 x 8, 16 x 16 x 8, 16 x 16 x 16), each butterfly an
//              in-register Dft<R> of pfb_cplx.hpp with one LDS exchange between passes (pfb_ols.hpp, shared with
//              pfb_mfbank.hip)
//     MULTIPLY by the spectrum (L2-resident) while the inverse's first pass reads its operands
//     INVERSE  the same three passes: Dft<R> is the e^{+j} kernel, which is the FORWARD direction here (the spectrum is
//              made for it); the e^{-j} transform back is DFT-(x) = swap(DFT+(swap(x))), re and im exchanged when the
//              products are formed and again when the outputs are read (pfb_stft.hip uses the same identity)
//     STORE    the block's complete outputs, complex or |y|^2, as 16-byte-per-lane runs between a scalar head and tail
//   LDS: two NFFT-point complex buffers, 16 / 32 / 64 KiB.
//
//   partitioned route           any K <= 65536: B = NFFT/2, the replica zero-padded to P = ceil(K/B) partitions of B
//                               samples with spectra H_p
//     pfb_mf_spectra<NFFT, FMT>   the fused kernel's front half: X_j = FFT(x[jB .. jB + NFFT)) to the workspace
//     pfb_mf_combine<NFFT>        Y_i = sum_p X_{i+p} H_p from 16-byte coalesced reads (p ascending: a fixed order),
//                                 the inverse passes in LDS, outputs [iB, iB + B) stored
//   The handle owns the workspace (grow-only, at most 64 MiB): a long call is walked in chunks of output blocks, each
//   chunk recomputing the P - 1 spectra it shares with the next.
//
// Blocks start where a call starts, so two cuttings of one stream round differently (they agree to the tolerance the
// header states); the same sequence of calls gives the same bits.  No atomics anywhere.
// Host side: the replica checks, the spectra and the stream state (carry, position, staging) are pfb_ols_host.h's,
// shared with pfb_mfbank.hip; the route, the NFFT rule, mf_check's order, the workspace and the entry points are here.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <new>
#include <vector>

#include "pfb_iq_span.hpp"
#include "pfb_ols.hpp"
#include "pfb_ols_host.h"

namespace {

using namespace pfb;

constexpr int kThreads = kOlsThreads;
constexpr uint64_t kWorkspaceCap = (uint64_t)64 << 20;  // partitioned route: bytes of spectra held at once
constexpr uint64_t kStageBytes = (uint64_t)64 << 20;    // per side of the host staging

// Kernel-side view of one call.  "Stream sample s" counts from the first carried sample: s < carry_len is
// carry[carry_cap - carry_len + s], the rest is in[s - carry_len] (iq_load_span reads in, carry, carry_len and
// carry_cap); local output m covers stream samples [m, m + K).
struct MfParams {
  const void* in;       // this call's samples (device)
  const void* carry;    // carry_cap samples; the last carry_len precede in[0]
  void* out;            // `outputs` complex64 or float32
  const float2* spec;   // partitions x NFFT: the spectra, scale folded in
  const float2* tw;     // tw[m] = exp(+j 2 pi m / NFFT)
  float2* work;         // partitioned: the spectra X of the chunk, slot s = block block0 + s
  long long total;      // carry_len + samples of the call
  long long outputs;    // local outputs of the call
  long long block0;     // partitioned: first block of the chunk
  int carry_len, carry_cap;
  int K, partitions, output;
};

// DFT+ of a (natural order) into b; a is overwritten.  Ends behind a barrier.
template <int NFFT>
PFB_DEV void mf_forward(float2* a, float2* b, const float2* tw) {
  using Cfg = OlsPlan<NFFT>;
  ols_first_pass<NFFT, Cfg::R0, false>(a, b, nullptr);
  __syncthreads();
  ols_pass<NFFT, Cfg::R1, Cfg::R0>(b, a, tw);
  __syncthreads();
  ols_pass<NFFT, Cfg::R2, Cfg::R0 * Cfg::R1>(a, b, tw);
  __syncthreads();
}

// DFT+ of (MUL: b * spec exchanged, else b as it is) into a; b is overwritten.  Ends behind a barrier.
template <int NFFT, bool MUL>
PFB_DEV void mf_inverse(float2* b, float2* a, const float2* spec, const float2* tw) {
  using Cfg = OlsPlan<NFFT>;
  ols_first_pass<NFFT, Cfg::R0, MUL>(b, a, spec);
  __syncthreads();
  ols_pass<NFFT, Cfg::R1, Cfg::R0>(a, b, tw);
  __syncthreads();
  ols_pass<NFFT, Cfg::R2, Cfg::R0 * Cfg::R1>(b, a, tw);
  __syncthreads();
}

// y holds the inverse's result with re and im exchanged
PFB_DEV float2 mf_value(const float2* y, int i) {
  const float2 v = y[i];
  return make_float2(v.y, v.x);
}

// local outputs [m0, m0 + count) from y[0 .. count): a scalar head up to the first 16-byte boundary of the output, whole
// 16-byte vectors, a scalar tail
PFB_DEV void mf_store(const MfParams& p, const float2* y, long long m0, int count) {
  const int tid = threadIdx.x;
  if (count <= 0) return;
  if (p.output == PFB_MF_COMPLEX) {
    float2* o = static_cast<float2*>(p.out) + m0;
    const int head = min((int)((reinterpret_cast<uintptr_t>(o) % 16) / 8), count);
    const int nvec = (count - head) / 2, tail0 = head + 2 * nvec;
    if (tid < head) o[tid] = mf_value(y, tid);
    for (int v = tid; v < nvec; v += kThreads) {
      const float2 c0 = mf_value(y, head + 2 * v), c1 = mf_value(y, head + 2 * v + 1);
      *reinterpret_cast<float4*>(o + head + 2 * v) = make_float4(c0.x, c0.y, c1.x, c1.y);
    }
    if (tid < count - tail0) o[tail0 + tid] = mf_value(y, tail0 + tid);
  } else {
    ols_store_power(static_cast<float*>(p.out) + m0, y, count);
  }
}

template <int NFFT, int FMT>
__global__ void __launch_bounds__(kThreads) pfb_mf_fused(const MfParams p) {
  __shared__ float2 buf_a[NFFT];
  __shared__ float2 buf_b[NFFT];
  const int V = NFFT - p.K + 1;
  const long long m0 = (long long)blockIdx.x * V;
  iq_load_span<FMT, false, NFFT>(p, m0, (int)min((long long)NFFT, p.total - m0), buf_a);
  __syncthreads();
  mf_forward<NFFT>(buf_a, buf_b, p.tw);
  mf_inverse<NFFT, true>(buf_b, buf_a, p.spec, p.tw);
  mf_store(p, buf_a, m0, (int)min((long long)V, p.outputs - m0));
}

// partitioned route, front half: slot blockIdx.x of the workspace = DFT+ of stream samples [j B, j B + NFFT),
// j = block0 + blockIdx.x
template <int NFFT, int FMT>
__global__ void __launch_bounds__(kThreads) pfb_mf_spectra(const MfParams p) {
  __shared__ float2 buf_a[NFFT];
  __shared__ float2 buf_b[NFFT];
  const long long s0 = (p.block0 + blockIdx.x) * (NFFT / 2);
  iq_load_span<FMT, false, NFFT>(p, s0, (int)max(0ll, min((long long)NFFT, p.total - s0)), buf_a);
  __syncthreads();
  mf_forward<NFFT>(buf_a, buf_b, p.tw);
  float4* dst = reinterpret_cast<float4*>(p.work + (size_t)blockIdx.x * NFFT);
  for (int v = threadIdx.x; v < NFFT / 2; v += kThreads) {
    const float2 c0 = buf_b[2 * v], c1 = buf_b[2 * v + 1];
    dst[v] = make_float4(c0.x, c0.y, c1.x, c1.y);
  }
}

// acc += x * h
PFB_DEV v2f cfma(v2f acc, v2f x, v2f h) {
  return fma2(swp(x), (v2f){-h.y, h.y}, fma2(x, splat(h.x), acc));
}

// partitioned route, back half: output block i = block0 + blockIdx.x from slots blockIdx.x + p, p = 0 .. P-1
template <int NFFT>
__global__ void __launch_bounds__(kThreads) pfb_mf_combine(const MfParams p) {
  __shared__ float2 buf_a[NFFT];
  __shared__ float2 buf_b[NFFT];
  constexpr int E = NFFT / (2 * kThreads);  // 16-byte vectors (two bins) per lane
  v2f acc[E][2];
#pragma unroll
  for (int e = 0; e < E; ++e) acc[e][0] = acc[e][1] = (v2f){0.f, 0.f};
  for (int q = 0; q < p.partitions; ++q) {
    const float4* X = reinterpret_cast<const float4*>(p.work + ((size_t)blockIdx.x + q) * NFFT);
    const float4* H = reinterpret_cast<const float4*>(p.spec + (size_t)q * NFFT);
#pragma unroll
    for (int e = 0; e < E; ++e) {
      const float4 x = X[threadIdx.x + e * kThreads], h = H[threadIdx.x + e * kThreads];
      acc[e][0] = cfma(acc[e][0], (v2f){x.x, x.y}, (v2f){h.x, h.y});
      acc[e][1] = cfma(acc[e][1], (v2f){x.z, x.w}, (v2f){h.z, h.w});
    }
  }
#pragma unroll
  for (int e = 0; e < E; ++e) {  // re and im exchanged: the way into the e^{-j} transform
    const int k = 2 * (threadIdx.x + e * kThreads);
    buf_b[k] = make_float2(acc[e][0].y, acc[e][0].x);
    buf_b[k + 1] = make_float2(acc[e][1].y, acc[e][1].x);
  }
  __syncthreads();
  mf_inverse<NFFT, false>(buf_b, buf_a, nullptr, p.tw);
  const long long m0 = (p.block0 + blockIdx.x) * (NFFT / 2);
  mf_store(p, buf_a, m0, (int)min((long long)(NFFT / 2), p.outputs - m0));
}

using MfLaunchFn = void (*)(const MfParams&, unsigned, hipStream_t);
template <int NFFT, int FMT>
void launch_fused(const MfParams& p, unsigned grid, hipStream_t s) {
  hipLaunchKernelGGL((pfb_mf_fused<NFFT, FMT>), dim3(grid), dim3(kThreads), 0, s, p);
}
template <int NFFT, int FMT>
void launch_spectra(const MfParams& p, unsigned grid, hipStream_t s) {
  hipLaunchKernelGGL((pfb_mf_spectra<NFFT, FMT>), dim3(grid), dim3(kThreads), 0, s, p);
}
template <int NFFT>
void launch_combine(const MfParams& p, unsigned grid, hipStream_t s) {
  hipLaunchKernelGGL((pfb_mf_combine<NFFT>), dim3(grid), dim3(kThreads), 0, s, p);
}

struct MfEntry {
  int nfft, fmt;
  MfLaunchFn fused, spectra, combine;
  const char* fused_name;
  const char* partitioned_name;
};
#define PFB_MF_ROW(N, FMT, TAG)                                                                         \
  {N, FMT, launch_fused<N, FMT>, launch_spectra<N, FMT>, launch_combine<N>, "pfb_mf_fused<N" #N "," TAG ">", \
   "pfb_mf_partitioned<N" #N "," TAG ">"}
#define PFB_MF_ROWS(N) PFB_MF_ROW(N, PFB_FMT_INT8_IQ, "int8"), PFB_MF_ROW(N, PFB_FMT_INT16_IQ, "int16"), PFB_MF_ROW(N, PFB_FMT_CF32, "cf32")
const MfEntry kMfKernels[] = {PFB_MF_ROWS(1024), PFB_MF_ROWS(2048), PFB_MF_ROWS(4096)};
#undef PFB_MF_ROWS
#undef PFB_MF_ROW

const MfEntry* find_mf(int nfft, int fmt) {
  for (const MfEntry& e : kMfKernels)
    if (e.nfft == nfft && e.fmt == fmt) return &e;
  return nullptr;
}

// ---------------------------------------------------------------------------------
// host: checks, plan, spectra

// Everything pfb_mf_describe and pfb_mf_create check before the device, in the order the header states; fills *plan,
// and *spec (when asked for) with the float32 spectra
int mf_check(const pfb_mf_config* cfg, pfb_mf_plan* plan, std::vector<float2>* spec) {
  if (!cfg || !plan || cfg->struct_size != sizeof(pfb_mf_config) || !cfg->replica) return PFB_ERR_BAD_ARG;
  const uint32_t K = cfg->replica_length, nf = cfg->fft_length;
  if (K == 0 || cfg->output > PFB_MF_POWER || (cfg->flags & ~(uint32_t)PFB_MF_NORMALIZE) ||
      cfg->route > PFB_MF_ROUTE_PARTITIONED || !(nf == 0 || nf == 1024 || nf == 2048 || nf == 4096))
    return PFB_ERR_BAD_ARG;
  double gain = 1.0;
  int rc = replica_gain(cfg->replica, K, (cfg->flags & PFB_MF_NORMALIZE) != 0, &gain);
  if (rc != PFB_OK) return rc;
  uint32_t bw = 0;
  rc = replica_format(cfg->sample_format, cfg->bit_width, &bw);
  if (rc != PFB_OK) return rc;
  if (K > kOlsMaxReplica) return PFB_ERR_UNSUPPORTED;
  const uint32_t fused_max = nf ? nf / 2 : 2048;  // the longest replica a fused kernel of the asked length takes
  if (cfg->route == PFB_MF_ROUTE_FUSED && K > fused_max) return PFB_ERR_UNSUPPORTED;
  const bool fused = cfg->route == PFB_MF_ROUTE_FUSED || (cfg->route == PFB_MF_ROUTE_AUTO && K <= fused_max);
  // fft_length = 0: the faster length per K range as measured.  Fused, a block costs 6.6 / 13.8 /
  // 35 ns at 1024 / 2048 / 4096 points and yields NFFT - K + 1 outputs: 1024 wins up to K ~ 90 (measured: at 13, not at
  // 104), 2048 from there to its limit of 1024 (measured at 104, 512 and 1024).  Partitioned: 2048 at one partition,
  // 4096 from K = 5600 on (a tie there, 1.7 times faster at 56 000).
  uint32_t N = nf;
  if (N == 0) N = fused ? (K <= 64 ? 1024u : K <= 1024 ? 2048u : 4096u) : (K <= 1024 ? 2048u : 4096u);
  const uint32_t B = N / 2, P = fused ? 1 : (K + B - 1) / B;
  plan->fft_length = N;
  plan->route = fused ? PFB_MF_ROUTE_FUSED : PFB_MF_ROUTE_PARTITIONED;
  plan->partitions = P;
  plan->block_outputs = fused ? N - K + 1 : B;
  plan->workspace_bytes = fused ? 0 : (kWorkspaceCap / ((uint64_t)N * sizeof(float2))) * (uint64_t)N * sizeof(float2);
  if (!spec) return PFB_OK;
  // H_p: partition p of B replica samples; fused: the one partition holds all K <= B samples
  return replica_spectra(cfg->replica, K, N, B, P, gain, bw, spec);
}

}  // namespace

struct pfb_mf_handle {
  pfb::OlsStream st;  // out_elem: complex64, or float32 for power
  int partitions = 1, block_outputs = 0;
  bool fused = true;
  int output = 0;
  int device = 0;
  float2* d_work = nullptr;  // partitioned: spectra of the chunk in flight (grow-only)
  uint64_t work_slots = 0;
  const MfEntry* kern = nullptr;
  const char* last_kernel = "";
};

namespace {

void free_mf(pfb_mf_handle* h) {
  if (!h) return;
  DeviceGuard g(h->device);
  h->st.release();
  (void)hipFree(h->d_work);
  delete h;
}

int create_mf(const pfb_mf_config* cfg, pfb_mf_handle** out) {
  pfb_mf_plan plan{};
  std::vector<float2> spec;
  int rc = mf_check(cfg, &plan, &spec);
  if (rc != PFB_OK) return rc;
  int dev = 0;
  rc = pfb::resolve_device(cfg->device_id, &dev);
  if (rc != PFB_OK) return rc;
  pfb_mf_handle* h = new pfb_mf_handle();
  h->partitions = (int)plan.partitions;
  h->block_outputs = (int)plan.block_outputs;
  h->fused = plan.route == PFB_MF_ROUTE_FUSED;
  h->output = (int)cfg->output;
  h->device = dev;
  h->st.out_elem = h->output == PFB_MF_COMPLEX ? 8 : 4;
  h->kern = find_mf((int)plan.fft_length, (int)cfg->sample_format);
  DeviceGuard g(dev);
  const hipError_t e = h->st.allocate(cfg->replica_length, plan.fft_length, cfg->sample_format, cfg->bit_width, spec);
  if (e != hipSuccess) {
    rc = pfb::hip_fail(e, "pfb_mf_create allocation");
    free_mf(h);
    return rc;
  }
  *out = h;
  return PFB_OK;
}

// the kernels of one call and the carry update for device-resident buffers; no host sync (a partitioned call that grows
// the workspace waits for the device)
int mf_enqueue(pfb_mf_handle* h, const void* d_iq, uint64_t n, void* d_out, uint64_t outputs) {
  pfb::OlsStream& st = h->st;
  if (outputs > 0) {
    MfParams p{};
    p.in = d_iq;
    p.carry = st.d_carry[st.cur];
    p.out = d_out;
    p.spec = st.d_spec;
    p.tw = st.d_tw;
    p.carry_len = (int)st.carried();
    p.carry_cap = st.K - 1;
    p.total = (long long)(st.carried() + n);
    p.outputs = (long long)outputs;
    p.K = st.K;
    p.partitions = h->partitions;
    p.output = h->output;
    const uint64_t blocks = (outputs + (uint64_t)h->block_outputs - 1) / (uint64_t)h->block_outputs;
    if (blocks > 0x7fffffffull) return PFB_ERR_UNSUPPORTED;
    if (h->fused) {
      h->kern->fused(p, (unsigned)blocks, st.stream);
      HIP_TRY(hipGetLastError());
      h->last_kernel = h->kern->fused_name;
    } else {
      const uint64_t extra = (uint64_t)h->partitions - 1;
      const uint64_t max_slots = kWorkspaceCap / ((uint64_t)st.nfft * sizeof(float2));  // 2048 .. 8192, > extra
      const uint64_t per_chunk = max_slots - extra, need = std::min(blocks, per_chunk) + extra;
      if (need > h->work_slots) {  // frees only after the device has drained: earlier calls are done with the old one
        (void)hipFree(h->d_work);
        h->d_work = nullptr;
        h->work_slots = 0;
        HIP_TRY(hipMalloc((void**)&h->d_work, need * (uint64_t)st.nfft * sizeof(float2)));
        h->work_slots = need;
      }
      p.work = h->d_work;
      for (uint64_t i0 = 0; i0 < blocks; i0 += per_chunk) {  // stream order keeps one chunk's spectra from the next
        const uint64_t nb = std::min(per_chunk, blocks - i0);
        p.block0 = (long long)i0;
        h->kern->spectra(p, (unsigned)(nb + extra), st.stream);
        HIP_TRY(hipGetLastError());
        h->kern->combine(p, (unsigned)nb, st.stream);
        HIP_TRY(hipGetLastError());
      }
      h->last_kernel = h->kern->partitioned_name;
    }
  }
  return st.advance(d_iq, n);
}

// Host buffers (pageable or page-locked) through the staged pipeline: an output sample is a "frame", a step at most
// 64 MiB on either side.  Blocks start where a step starts: another step size rounds differently.
int mf_host(pfb_mf_handle* h, const void* iq, uint64_t n, void* out, uint64_t limit = UINT64_MAX) {
  const uint64_t chunk = std::min<uint64_t>(limit, kStageBytes / 8);  // a step completes at most `chunk` outputs
  const pfb::StageSteps steps{
      chunk, chunk, (size_t)h->st.bps, (size_t)h->st.out_elem,
      [h](uint64_t m) { return h->st.outputs_for(m); },
      [h](const void* d_in, uint64_t m, void* d_out, uint64_t f, int64_t, int64_t) {
        return mf_enqueue(h, d_in, m, d_out, f);
      }};
  return pfb::stage_host(h->st.stage, h->st.stream, steps, iq, n, pfb::StageOut{out});
}

}  // namespace

extern "C" int pfb_mf_describe(const pfb_mf_config* cfg, pfb_mf_plan* plan_out) {
  return pfb::abi_guard([&]() -> int {
    pfb_mf_plan plan{};
    std::vector<float2> spec;
    const int rc = mf_check(cfg, plan_out ? &plan : nullptr, &spec);
    if (rc == PFB_OK) *plan_out = plan;
    return rc;
  });
}

extern "C" int pfb_mf_create(const pfb_mf_config* cfg, pfb_mf_handle** out) {
  return pfb::abi_guard([&]() -> int {
    if (!out) return PFB_ERR_BAD_ARG;
    *out = nullptr;
    return create_mf(cfg, out);
  });
}

extern "C" int pfb_mf_destroy(pfb_mf_handle* h) {
  return pfb::abi_guard([&]() -> int {
    if (!h) return PFB_ERR_BAD_ARG;
    free_mf(h);
    return PFB_OK;
  });
}

extern "C" int pfb_mf_reset(pfb_mf_handle* h) {
  return pfb::abi_guard([&]() -> int {
    if (!h) return PFB_ERR_BAD_ARG;
    h->st.pos = 0;  // nothing carried: the carry buffer is never read before it is written again
    return PFB_OK;
  });
}

extern "C" int pfb_mf_set_stream(pfb_mf_handle* h, void* hip_stream) {
  return pfb::abi_guard([&]() -> int {
    if (!h) return PFB_ERR_BAD_ARG;
    return pfb::switch_stream(h->device, &h->st.stream, &h->st.ev_switch, static_cast<hipStream_t>(hip_stream));
  });
}

extern "C" int pfb_mf_sync(pfb_mf_handle* h) {
  return pfb::abi_guard([&]() -> int {
    if (!h) return PFB_ERR_BAD_ARG;
    DeviceGuard g(h->device);
    HIP_TRY(hipStreamSynchronize(h->st.stream));
    return PFB_OK;
  });
}

extern "C" int pfb_mf_get_device(const pfb_mf_handle* h, int* device_id) {
  return pfb::abi_guard([&]() -> int {
    if (!h || !device_id) return PFB_ERR_BAD_ARG;
    *device_id = h->device;
    return PFB_OK;
  });
}

extern "C" int pfb_mf_outputs_for(const pfb_mf_handle* h, uint64_t num_samples, uint64_t* outputs_out) {
  return pfb::abi_guard([&]() -> int {
    if (!h || !outputs_out || num_samples > ((uint64_t)1 << 62)) return PFB_ERR_BAD_ARG;
    *outputs_out = h->st.outputs_for(num_samples);
    return PFB_OK;
  });
}

extern "C" int pfb_mf_next_index(const pfb_mf_handle* h, uint64_t* index_out) {
  return pfb::abi_guard([&]() -> int {
    if (!h || !index_out) return PFB_ERR_BAD_ARG;
    *index_out = h->st.pos - h->st.carried();  // = max(0, pos - K + 1): the outputs so far
    return PFB_OK;
  });
}

extern "C" int pfb_mf_process_async(pfb_mf_handle* h, const void* d_iq, uint64_t num_samples, void* d_out,
                                    uint64_t capacity_outputs, uint64_t* outputs_out) {
  return pfb::abi_guard([&]() -> int {
    if (!h) return PFB_ERR_BAD_ARG;
    uint64_t f = 0;
    const int rc = h->st.check_call(d_iq, num_samples, d_out, capacity_outputs, outputs_out, true, &f);
    if (rc != PFB_OK) return rc;
    DeviceGuard g(h->device);
    return mf_enqueue(h, d_iq, num_samples, d_out, f);
  });
}

extern "C" int pfb_mf_process(pfb_mf_handle* h, const void* iq, uint64_t num_samples, void* out, uint64_t capacity_outputs,
                              uint64_t* outputs_out, uint32_t mem) {
  return pfb::abi_guard([&]() -> int {
    if (mem > PFB_MEM_DEVICE || !h) return PFB_ERR_BAD_ARG;
    uint64_t f = 0;
    int rc = h->st.check_call(iq, num_samples, out, capacity_outputs, outputs_out, mem == PFB_MEM_DEVICE, &f);
    if (rc != PFB_OK) return rc;
    DeviceGuard g(h->device);
    if (mem == PFB_MEM_HOST) return mf_host(h, iq, num_samples, out);
    rc = mf_enqueue(h, iq, num_samples, out, f);
    if (rc != PFB_OK) return rc;
    HIP_TRY(hipStreamSynchronize(h->st.stream));
    return PFB_OK;
  });
}

extern "C" int pfb_mf_process_iq_file(pfb_mf_handle* h, const char* path, void* out, uint64_t capacity_outputs,
                                      uint64_t* outputs_out, pfb_iq_info* info_out) {
  return pfb::abi_guard([&]() -> int {
    if (!h || !path) return PFB_ERR_BAD_ARG;
    pfb::Record rec;
    const int rc = rec.open(path, h->st.fmt, h->st.bit_width);
    if (info_out) *info_out = rec.info;
    if (rc != PFB_OK) return rc;
    const uint64_t need = h->st.outputs_for(rec.info.packet.numSamples);
    if (outputs_out) *outputs_out = need;
    if (need > capacity_outputs) return PFB_ERR_CAPACITY;
    if (need > 0 && !out) return PFB_ERR_BAD_ARG;
    // the payload in record chunks of 2^24 samples, each staged in steps of at most 2^22 (pfb_stft_process_iq_file)
    uint64_t done = 0;
    const int rc2 = rec.read((uint64_t)1 << 24, [&](const char* buf, uint64_t, uint64_t m) {
      const uint64_t f = h->st.outputs_for(m);
      DeviceGuard g(h->device);
      const int r = mf_host(h, buf, m, static_cast<char*>(out) + done * (uint64_t)h->st.out_elem, (uint64_t)1 << 22);
      done += f;
      return r;
    });
    if (outputs_out) *outputs_out = done;
    return rc2;
  });
}

extern "C" const char* pfb_mf_last_kernel(const pfb_mf_handle* h) { return h ? h->last_kernel : ""; }
