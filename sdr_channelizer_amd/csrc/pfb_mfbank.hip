// pfb_mfbank.hip -- a bank of frequency-offset hypotheses on the matched filter (pfb_mfbank_* in
// include/pfb_channelizer.h): delay and carrier of a coded pulse in one pass, kernels and host side.
// The matched filter (pfb_mf.hip) finds a pulse only at the carrier its replica was made for, and the reference's own
// signals do not give one: generate_pulsed_iq.m:13 and generate_training_iq.m:13 draw the carrier at random in +-fs/2,
// the TX / RX pair of tx_rx_pulses_usrp.cpp comes from two oscillators, and a Barker-13 pulse of 13 x 39 samples loses
// 59 % of its peak power to an offset of fs/1024 and all of it (0.0066, at a wrong sample) to 37 such bins.
// Arithmetic, with x, r, K and g as pfb_mf.hip has them:
//   q_h    = (first_bin + h) * bin_step                    h = 0 .. H-1
//   y_h[m] = g * sum_{n=0}^{K-1} conj(r[n]) * e^{-j 2 pi q_h n / NFFT} * x[m+n]        p_h[m] = |y_h[m]|^2
// Why whole bins are enough and cost no table: a replica modulated by e^{+j 2 pi q n / NFFT}, q an integer, has the
// spectrum of the plain replica rotated by q bins.  With the e^{+j} forward transform used here the spectrum table of
// pfb_mf.hip, R[c] = scale * sum_n conj(r[n]) e^{-j 2 pi n c / NFFT}, becomes R_q[c] = R[(c + q) mod NFFT] (7e-14 in
// float64).  Between two hypotheses one bin apart a pulse of K <= NFFT/2 samples is off by at most half a bin from the
// nearer one, where the correlation keeps sinc(K / (2 NFFT)) of its amplitude: at K = NFFT/2 that is sinc(1/4) = 0.900,
// -0.91 dB, and less loss for every shorter replica.
//
//   pfb_mfbank_fused<NFFT, FMT, OUT>   NFFT in {1024, 2048, 4096} x {int8, int16, cf32} x {best, surface}, K <= NFFT/2.
//                                      One 256-thread workgroup per block of V = NFFT - K + 1 outputs:
//     LOAD, FORWARD   as pfb_mf_fused, by the same functions (pfb_iq_span.hpp, pfb_ols.hpp): the block's NFFT samples
//                     once, three Stockham passes
//     KEEP      the block's spectrum X goes to registers in the operand layout of the inverse's first pass, 16 values per
//               lane of the NFFT/16 lanes that run it: the LDS stays at two NFFT-point buffers (16 / 32 / 64 KiB), two
//               workgroups of the 4096-point kernel share a CU where a third buffer (96 KiB) would leave one.  The
//               third buffer is kept as a per-length compile-time choice (kKeepInLdsLengths, none by default): it was
//               built and measured against the registers, DESIGN.md section 18 has the figures
//     per h     the inverse's first pass from X * R[(n + q_h) mod NFFT] (the table is L2-resident) with re and im
//               exchanged, the two remaining passes, then
//       BEST      each lane compares the powers of the cells it will store with its running (power, h) pairs: h = 0
//                 starts them, a strictly greater power replaces, so ties keep the lowest h and a NaN displaces nothing
//       SURFACE   row h of the block stored as pfb_mf.hip stores power (ols_store_power)
//               The result alternates between the two buffers, so a hypothesis costs three barriers.
//     STORE     BEST: the cells once, {float power; int32 h}, 16-byte vectors between a scalar head and tail
// Blocks start where a call starts (the same sequence of calls gives the same bits); no atomics anywhere.
// Host side: the replica checks, the spectrum and the stream state (carry, position, staging) are pfb_ols_host.h's,
// shared with pfb_mf.hip; the hypothesis grid, bank_check's order and the entry points are here.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <new>
#include <vector>

#include "pfb_iq_span.hpp"
#include "pfb_ols.hpp"
#include "pfb_ols_host.h"

namespace {

using namespace pfb;

constexpr int kThreads = kOlsThreads;
constexpr uint64_t kStageBytes = (uint64_t)64 << 20;    // per side of the host staging

// KEEP: where a block's spectrum waits between two hypotheses, registers or a third LDS buffer (header comment).  The
// macro is for A/B builds: -DPFB_MFBANK_KEEP_IN_LDS=7168 keeps it in LDS at every length.
#ifndef PFB_MFBANK_KEEP_IN_LDS
#define PFB_MFBANK_KEEP_IN_LDS 0
#endif
constexpr int kKeepInLdsLengths = PFB_MFBANK_KEEP_IN_LDS;  // the FFT lengths (powers of two) or-ed together
template <int NFFT> constexpr bool kKeepInLds = (kKeepInLdsLengths & NFFT) != 0;

// Kernel-side view of one call; stream samples and local outputs are counted as in pfb_mf.hip's MfParams, and
// iq_load_span reads in, carry, carry_len and carry_cap
struct BankParams {
  const void* in;        // this call's samples (device)
  const void* carry;     // carry_cap samples; the last carry_len precede in[0]
  void* out;             // BEST: `outputs` cells; SURFACE: H rows of row_pitch floats
  const float2* spec;    // NFFT: the plain replica's spectrum, scale folded in
  const float2* tw;      // tw[m] = exp(+j 2 pi m / NFFT)
  long long total;       // carry_len + samples of the call
  long long outputs;     // local outputs of the call
  long long row_pitch;   // SURFACE: elements between two rows
  int carry_len, carry_cap;
  int K, H;
  int q0, qstep;         // q_h mod NFFT = (q0 + h * qstep) mod NFFT, both in [0, NFFT)
};

// BEST: the running (power, h) of one cell
PFB_DEV void bank_pick(float& best, int& arg, float pw, int h) {
  if (h == 0 || pw > best) { best = pw; arg = h; }
}

template <int NFFT, int FMT, int OUT>
__global__ void __launch_bounds__(kThreads) pfb_mfbank_fused(const BankParams p) {
  using Cfg = OlsPlan<NFFT>;
  constexpr int kR0 = Cfg::R0;              // radix of the first pass: 16 at every length
  constexpr int NB = NFFT / kR0;            // lanes of the inverse's first pass: 64 / 128 / 256
  constexpr int E = NFFT / (2 * kThreads);  // BEST: 16-byte vectors (two cells) per lane, at most
  __shared__ float2 buf_a[NFFT];
  __shared__ float2 buf_b[NFFT];
  __shared__ float2 buf_x[kKeepInLds<NFFT> ? NFFT : 1];
  const int tid = threadIdx.x;
  const int V = NFFT - p.K + 1;
  const long long m0 = (long long)blockIdx.x * V;
  const int count = (int)min((long long)V, p.outputs - m0);  // >= 1: the grid is ceil(outputs / V)
  iq_load_span<FMT, false, NFFT>(p, m0, (int)min((long long)NFFT, p.total - m0), buf_a);
  __syncthreads();
  ols_first_pass<NFFT, kR0, false>(buf_a, buf_b, nullptr);
  __syncthreads();
  ols_pass<NFFT, Cfg::R1, kR0>(buf_b, buf_a, p.tw);
  __syncthreads();
  float2* const spectrum = kKeepInLds<NFFT> ? buf_x : buf_b;
  ols_pass<NFFT, Cfg::R2, kR0 * Cfg::R1>(buf_a, spectrum, p.tw);
  __syncthreads();
  // KEEP in registers: X[tid + q NB].  No barrier before buf_a is written again: its last readers passed the one above;
  // buf_b is next written behind the first barrier of the loop
  v2f X[kR0];
  if constexpr (!kKeepInLds<NFFT>) {
    if (tid < NB) {
#pragma unroll
      for (int q = 0; q < kR0; ++q) {
        const float2 v = buf_b[tid + q * NB];
        X[q] = (v2f){v.x, v.y};
      }
    }
  }
  // BEST: the cells this lane stores, as in the store below
  const int head = OUT == PFB_MFBANK_BEST ? min((int)((reinterpret_cast<uintptr_t>(static_cast<float2*>(p.out) + m0) % 16) / 8), count) : 0;
  const int nvec = (count - head) / 2, tail0 = head + 2 * nvec;
  float best[2 * E + 2];
  int arg[2 * E + 2];
#pragma unroll
  for (int e = 0; e < 2 * E + 2; ++e) { best[e] = 0.f; arg[e] = 0; }

  float2* ya = buf_a;  // where the inverse of this hypothesis ends
  float2* yb = buf_b;
  int q = p.q0;
  for (int h = 0; h < p.H; ++h) {
    if (tid < NB) {  // first pass: X[n] * R[(n + q_h) mod NFFT], re and im exchanged on the way into the e^{-j} transform
      v2f x[kR0];
#pragma unroll
      for (int k = 0; k < kR0; ++k) {
        const float2 r = p.spec[(tid + k * NB + q) & (NFFT - 1)];
        if constexpr (kKeepInLds<NFFT>) {
          const float2 v = buf_x[tid + k * NB];
          X[k] = (v2f){v.x, v.y};
        }
        x[k] = swp(cmul(X[k], r.x, r.y));
      }
      Dft<kR0>::run(x);
      float2* d = ya + tid * kR0;
#pragma unroll
      for (int k = 0; k < kR0; ++k) d[k] = make_float2(x[k].x, x[k].y);
    }
    __syncthreads();
    ols_pass<NFFT, Cfg::R1, kR0>(ya, yb, p.tw);
    __syncthreads();
    ols_pass<NFFT, Cfg::R2, kR0 * Cfg::R1>(yb, ya, p.tw);
    __syncthreads();
    if constexpr (OUT == PFB_MFBANK_BEST) {
      if (tid < head) bank_pick(best[2 * E], arg[2 * E], ols_power(ya, tid), h);
#pragma unroll
      for (int e = 0; e < E; ++e) {
        const int v = tid + e * kThreads;
        if (v < nvec) {
          bank_pick(best[2 * e], arg[2 * e], ols_power(ya, head + 2 * v), h);
          bank_pick(best[2 * e + 1], arg[2 * e + 1], ols_power(ya, head + 2 * v + 1), h);
        }
      }
      if (tid < count - tail0) bank_pick(best[2 * E + 1], arg[2 * E + 1], ols_power(ya, tail0 + tid), h);
    } else {
      ols_store_power(static_cast<float*>(p.out) + (long long)h * p.row_pitch + m0, ya, count);
    }
    // the next hypothesis ends in the other buffer: what is read above is written again only behind its first barrier
    float2* t = ya; ya = yb; yb = t;
    q = (q + p.qstep) & (NFFT - 1);
  }
  if constexpr (OUT == PFB_MFBANK_BEST) {
    float2* o = static_cast<float2*>(p.out) + m0;  // a cell: {float power; int32 hypothesis}
    if (tid < head) o[tid] = make_float2(best[2 * E], __int_as_float(arg[2 * E]));
#pragma unroll
    for (int e = 0; e < E; ++e) {
      const int v = tid + e * kThreads;
      if (v < nvec)
        *reinterpret_cast<float4*>(o + head + 2 * v) =
            make_float4(best[2 * e], __int_as_float(arg[2 * e]), best[2 * e + 1], __int_as_float(arg[2 * e + 1]));
    }
    if (tid < count - tail0) o[tail0 + tid] = make_float2(best[2 * E + 1], __int_as_float(arg[2 * E + 1]));
  }
}

using BankLaunchFn = void (*)(const BankParams&, unsigned, hipStream_t);
template <int NFFT, int FMT, int OUT>
void launch_bank(const BankParams& p, unsigned grid, hipStream_t s) {
  hipLaunchKernelGGL((pfb_mfbank_fused<NFFT, FMT, OUT>), dim3(grid), dim3(kThreads), 0, s, p);
}

struct BankEntry {
  int nfft, fmt, output;
  BankLaunchFn launch;
  const char* name;
};
#define PFB_BANK_ROW(N, FMT, TAG)                                                                               \
  {N, FMT, PFB_MFBANK_BEST, launch_bank<N, FMT, PFB_MFBANK_BEST>, "pfb_mfbank_fused<N" #N "," TAG ",best>"},     \
  {N, FMT, PFB_MFBANK_SURFACE, launch_bank<N, FMT, PFB_MFBANK_SURFACE>, "pfb_mfbank_fused<N" #N "," TAG ",surface>"}
#define PFB_BANK_ROWS(N) PFB_BANK_ROW(N, PFB_FMT_INT8_IQ, "int8"), PFB_BANK_ROW(N, PFB_FMT_INT16_IQ, "int16"), PFB_BANK_ROW(N, PFB_FMT_CF32, "cf32")
const BankEntry kBankKernels[] = {PFB_BANK_ROWS(1024), PFB_BANK_ROWS(2048), PFB_BANK_ROWS(4096)};
#undef PFB_BANK_ROWS
#undef PFB_BANK_ROW

const BankEntry* find_bank(int nfft, int fmt, int output) {
  for (const BankEntry& e : kBankKernels)
    if (e.nfft == nfft && e.fmt == fmt && e.output == output) return &e;
  return nullptr;
}

// ---------------------------------------------------------------------------------
// host: checks, plan, spectrum

// the hypothesis grid alone: what pfb_mfbank_frequencies needs of a config; *nfft_out = the FFT length it counts bins of
bool bank_grid_ok(const pfb_mfbank_config* cfg, uint32_t* nfft_out) {
  const uint32_t nf = cfg->fft_length;
  if (!(nf == 0 || nf == 1024 || nf == 2048 || nf == 4096)) return false;
  const uint32_t N = nf ? nf : 4096;
  if (cfg->bin_step == 0 || cfg->num_hypotheses == 0 || (uint64_t)cfg->num_hypotheses * cfg->bin_step > N) return false;
  *nfft_out = N;
  return true;
}

// Everything pfb_mfbank_describe and pfb_mfbank_create check before the device, in the order the header states (that
// of pfb_mf_create); fills *plan, and *spec (when asked for) with the float32 spectrum
int bank_check(const pfb_mfbank_config* cfg, pfb_mfbank_plan* plan, std::vector<float2>* spec) {
  if (!cfg || !plan || cfg->struct_size != sizeof(pfb_mfbank_config) || !cfg->replica) return PFB_ERR_BAD_ARG;
  const uint32_t K = cfg->replica_length;
  uint32_t N = 0;
  if (K == 0 || cfg->output > PFB_MFBANK_SURFACE || (cfg->flags & ~(uint32_t)PFB_MF_NORMALIZE) || !bank_grid_ok(cfg, &N))
    return PFB_ERR_BAD_ARG;
  double gain = 1.0;
  int rc = replica_gain(cfg->replica, K, (cfg->flags & PFB_MF_NORMALIZE) != 0, &gain);
  if (rc != PFB_OK) return rc;
  uint32_t bw = 0;
  rc = replica_format(cfg->sample_format, cfg->bit_width, &bw);
  if (rc != PFB_OK) return rc;
  if (K > kOlsMaxReplica || K > N / 2) return PFB_ERR_UNSUPPORTED;  // the fused route only
  plan->fft_length = N;
  plan->block_outputs = N - K + 1;
  plan->num_hypotheses = cfg->num_hypotheses;
  const bool keep_lds = N == 1024 ? kKeepInLds<1024> : N == 2048 ? kKeepInLds<2048> : kKeepInLds<4096>;
  plan->lds_bytes = (keep_lds ? 3 : 2) * N * (uint32_t)sizeof(float2);
  if (!spec) return PFB_OK;
  // R[k] = scale * sum_{n < K} conj(r[n]) e^{-j 2 pi n k / N}: one partition of K samples
  return replica_spectra(cfg->replica, K, N, K, 1, gain, bw, spec);
}

}  // namespace

struct pfb_mfbank_handle {
  pfb::OlsStream st;  // out_elem: a cell, or float32 for the surface
  int block_outputs = 0, H = 0;
  int q0 = 0, qstep = 0;  // mod nfft
  int output = 0;
  int device = 0;
  const BankEntry* kern = nullptr;
  const char* last_kernel = "";
};

namespace {

void free_bank(pfb_mfbank_handle* h) {
  if (!h) return;
  DeviceGuard g(h->device);
  h->st.release();
  delete h;
}

int create_bank(const pfb_mfbank_config* cfg, pfb_mfbank_handle** out) {
  pfb_mfbank_plan plan{};
  std::vector<float2> spec;
  int rc = bank_check(cfg, &plan, &spec);
  if (rc != PFB_OK) return rc;
  int dev = 0;
  rc = pfb::resolve_device(cfg->device_id, &dev);
  if (rc != PFB_OK) return rc;
  pfb_mfbank_handle* h = new pfb_mfbank_handle();
  const long long N = (long long)plan.fft_length;
  h->block_outputs = (int)plan.block_outputs;
  h->H = (int)cfg->num_hypotheses;
  h->q0 = (int)((((long long)cfg->first_bin * (long long)cfg->bin_step) % N + N) % N);
  h->qstep = (int)((long long)cfg->bin_step % N);
  h->output = (int)cfg->output;
  h->device = dev;
  h->st.out_elem = h->output == PFB_MFBANK_BEST ? 8 : 4;
  h->kern = find_bank((int)N, (int)cfg->sample_format, h->output);
  DeviceGuard g(dev);
  const hipError_t e = h->st.allocate(cfg->replica_length, plan.fft_length, cfg->sample_format, cfg->bit_width, spec);
  if (e != hipSuccess) {
    rc = pfb::hip_fail(e, "pfb_mfbank_create allocation");
    free_bank(h);
    return rc;
  }
  *out = h;
  return PFB_OK;
}

// the kernel of one call and the carry update for device-resident buffers; no host sync
int bank_enqueue(pfb_mfbank_handle* h, const void* d_iq, uint64_t n, void* d_out, uint64_t outputs, uint64_t row_pitch) {
  pfb::OlsStream& st = h->st;
  if (outputs > 0) {
    BankParams p{};
    p.in = d_iq;
    p.carry = st.d_carry[st.cur];
    p.out = d_out;
    p.spec = st.d_spec;
    p.tw = st.d_tw;
    p.total = (long long)(st.carried() + n);
    p.outputs = (long long)outputs;
    p.row_pitch = (long long)row_pitch;
    p.carry_len = (int)st.carried();
    p.carry_cap = st.K - 1;
    p.K = st.K;
    p.H = h->H;
    p.q0 = h->q0;
    p.qstep = h->qstep;
    const uint64_t blocks = (outputs + (uint64_t)h->block_outputs - 1) / (uint64_t)h->block_outputs;
    if (blocks > 0x7fffffffull) return PFB_ERR_UNSUPPORTED;
    h->kern->launch(p, (unsigned)blocks, st.stream);
    HIP_TRY(hipGetLastError());
    h->last_kernel = h->kern->name;
  }
  return st.advance(d_iq, n);
}

// what every process call checks before the device is touched; *f = the outputs it completes
int bank_check_call(const pfb_mfbank_handle* h, const void* iq, uint64_t n, const void* out, uint64_t cap, uint64_t row_pitch,
                    uint64_t* outputs_out, bool device, uint64_t* f) {
  if (!h) return PFB_ERR_BAD_ARG;
  const int rc = h->st.check_call(iq, n, out, cap, outputs_out, device, f);
  if (rc != PFB_OK) return rc;
  if (h->output == PFB_MFBANK_SURFACE && (row_pitch < *f || row_pitch > ((uint64_t)1 << 40))) return PFB_ERR_BAD_ARG;
  return PFB_OK;
}

// Host buffers through the staged pipeline, as pfb_mf.hip's: an output is a "frame" of one cell (BEST) or of a column
// of H floats (SURFACE, the staged step a H x f matrix that lands in columns [row0, row0 + f) of the caller's rows), a
// step at most 64 MiB on either side.  Blocks start where a step starts.
int bank_host(pfb_mfbank_handle* h, const void* iq, uint64_t n, void* out, uint64_t row_pitch, uint64_t row0,
              uint64_t limit = UINT64_MAX) {
  const bool surface = h->output == PFB_MFBANK_SURFACE;
  const size_t frame = surface ? (size_t)h->H * 4 : 8;
  const uint64_t chunk = std::min<uint64_t>(limit, kStageBytes / frame);  // a step completes at most `chunk` outputs
  const pfb::StageSteps steps{
      chunk, chunk, (size_t)h->st.bps, frame,
      [h](uint64_t m) { return h->st.outputs_for(m); },
      [h](const void* d_in, uint64_t m, void* d_out, uint64_t f, int64_t ld, int64_t) {
        return bank_enqueue(h, d_in, m, d_out, f, (uint64_t)ld);
      }};
  pfb::StageOut dst{out};
  if (surface) {
    dst.ld = row_pitch;
    dst.row0 = row0;
    dst.cols = h->H;
  } else {
    dst.row0 = row0;
  }
  return pfb::stage_host(h->st.stage, h->st.stream, steps, iq, n, dst);
}

}  // namespace

extern "C" int pfb_mfbank_describe(const pfb_mfbank_config* cfg, pfb_mfbank_plan* plan_out) {
  return pfb::abi_guard([&]() -> int {
    pfb_mfbank_plan plan{};
    std::vector<float2> spec;
    const int rc = bank_check(cfg, plan_out ? &plan : nullptr, &spec);
    if (rc == PFB_OK) *plan_out = plan;
    return rc;
  });
}

extern "C" int pfb_mfbank_frequencies(const pfb_mfbank_config* cfg, double fs, double* out) {
  return pfb::abi_guard([&]() -> int {
    uint32_t N = 0;
    if (!cfg || !out || cfg->struct_size != sizeof(pfb_mfbank_config) || !std::isfinite(fs) || !bank_grid_ok(cfg, &N))
      return PFB_ERR_BAD_ARG;
    for (uint32_t h = 0; h < cfg->num_hypotheses; ++h)
      out[h] = (double)(((long long)cfg->first_bin + (long long)h) * (long long)cfg->bin_step) * fs / (double)N;
    return PFB_OK;
  });
}

extern "C" int pfb_mfbank_create(const pfb_mfbank_config* cfg, pfb_mfbank_handle** out) {
  return pfb::abi_guard([&]() -> int {
    if (!out) return PFB_ERR_BAD_ARG;
    *out = nullptr;
    return create_bank(cfg, out);
  });
}

extern "C" int pfb_mfbank_destroy(pfb_mfbank_handle* h) {
  return pfb::abi_guard([&]() -> int {
    if (!h) return PFB_ERR_BAD_ARG;
    free_bank(h);
    return PFB_OK;
  });
}

extern "C" int pfb_mfbank_reset(pfb_mfbank_handle* h) {
  return pfb::abi_guard([&]() -> int {
    if (!h) return PFB_ERR_BAD_ARG;
    h->st.pos = 0;  // nothing carried: the carry buffer is never read before it is written again
    return PFB_OK;
  });
}

extern "C" int pfb_mfbank_set_stream(pfb_mfbank_handle* h, void* hip_stream) {
  return pfb::abi_guard([&]() -> int {
    if (!h) return PFB_ERR_BAD_ARG;
    return pfb::switch_stream(h->device, &h->st.stream, &h->st.ev_switch, static_cast<hipStream_t>(hip_stream));
  });
}

extern "C" int pfb_mfbank_sync(pfb_mfbank_handle* h) {
  return pfb::abi_guard([&]() -> int {
    if (!h) return PFB_ERR_BAD_ARG;
    DeviceGuard g(h->device);
    HIP_TRY(hipStreamSynchronize(h->st.stream));
    return PFB_OK;
  });
}

extern "C" int pfb_mfbank_get_device(const pfb_mfbank_handle* h, int* device_id) {
  return pfb::abi_guard([&]() -> int {
    if (!h || !device_id) return PFB_ERR_BAD_ARG;
    *device_id = h->device;
    return PFB_OK;
  });
}

extern "C" int pfb_mfbank_outputs_for(const pfb_mfbank_handle* h, uint64_t num_samples, uint64_t* outputs_out) {
  return pfb::abi_guard([&]() -> int {
    if (!h || !outputs_out || num_samples > ((uint64_t)1 << 62)) return PFB_ERR_BAD_ARG;
    *outputs_out = h->st.outputs_for(num_samples);
    return PFB_OK;
  });
}

extern "C" int pfb_mfbank_next_index(const pfb_mfbank_handle* h, uint64_t* index_out) {
  return pfb::abi_guard([&]() -> int {
    if (!h || !index_out) return PFB_ERR_BAD_ARG;
    *index_out = h->st.pos - h->st.carried();  // = max(0, pos - K + 1): the outputs so far
    return PFB_OK;
  });
}

extern "C" int pfb_mfbank_process_async(pfb_mfbank_handle* h, const void* d_iq, uint64_t num_samples, void* d_out,
                                        uint64_t capacity_outputs, uint64_t row_pitch, uint64_t* outputs_out) {
  return pfb::abi_guard([&]() -> int {
    uint64_t f = 0;
    const int rc = bank_check_call(h, d_iq, num_samples, d_out, capacity_outputs, row_pitch, outputs_out, true, &f);
    if (rc != PFB_OK) return rc;
    DeviceGuard g(h->device);
    return bank_enqueue(h, d_iq, num_samples, d_out, f, row_pitch);
  });
}

extern "C" int pfb_mfbank_process(pfb_mfbank_handle* h, const void* iq, uint64_t num_samples, void* out,
                                  uint64_t capacity_outputs, uint64_t row_pitch, uint64_t* outputs_out, uint32_t mem) {
  return pfb::abi_guard([&]() -> int {
    if (mem > PFB_MEM_DEVICE) return PFB_ERR_BAD_ARG;
    uint64_t f = 0;
    int rc = bank_check_call(h, iq, num_samples, out, capacity_outputs, row_pitch, outputs_out, mem == PFB_MEM_DEVICE, &f);
    if (rc != PFB_OK) return rc;
    DeviceGuard g(h->device);
    if (mem == PFB_MEM_HOST) return bank_host(h, iq, num_samples, out, row_pitch, 0);
    rc = bank_enqueue(h, iq, num_samples, out, f, row_pitch);
    if (rc != PFB_OK) return rc;
    HIP_TRY(hipStreamSynchronize(h->st.stream));
    return PFB_OK;
  });
}

extern "C" int pfb_mfbank_process_iq_file(pfb_mfbank_handle* h, const char* path, void* out, uint64_t capacity_outputs,
                                          uint64_t row_pitch, uint64_t* outputs_out, pfb_iq_info* info_out) {
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
    if (h->output == PFB_MFBANK_SURFACE && (row_pitch < need || row_pitch > ((uint64_t)1 << 40))) return PFB_ERR_BAD_ARG;
    // the payload in record chunks of 2^24 samples, each staged in steps of at most 2^22 (pfb_mf_process_iq_file)
    uint64_t done = 0;
    const int rc2 = rec.read((uint64_t)1 << 24, [&](const char* buf, uint64_t, uint64_t m) {
      const uint64_t f = h->st.outputs_for(m);
      DeviceGuard g(h->device);
      const int r = bank_host(h, buf, m, out, row_pitch, done, (uint64_t)1 << 22);
      done += f;
      return r;
    });
    if (outputs_out) *outputs_out = done;
    return rc2;
  });
}

extern "C" const char* pfb_mfbank_last_kernel(const pfb_mfbank_handle* h) { return h ? h->last_kernel : ""; }
