// pfb_pd.hip -- pulse-Doppler integration of a compressed stream (pfb_pd_* in include/pfb_channelizer.h, where the
// arithmetic is defined): many short transforms DOWN THE COLUMNS of a K x R matrix whose rows lie L samples apart.
//   pd_dft<R1,R2,R3>   one workgroup per (CPI, tile of TG adjacent gates); ND = R1 R2 R3.  Consecutive lanes hold
//                      consecutive gates, so every global access is a run of gates of one row and every LDS access a
//                      run of one row of the ND x TG tile (8-byte elements, unit stride: conflict-free).  Decimation in
//                      frequency, in place: pass s takes the R_s rows j + q m of a block of R_s m rows, runs Dft<R_s> of
//                      pfb_cplx.hpp in registers, multiplies by W^(j p) and puts them back.  The first pass reads global
//                      memory (window applied, rows >= K and gates >= R as zeros) and the last one writes it, so the tile
//                      crosses LDS once per inner pass boundary.  The digit reversal and the sign (Dft<> runs e^{+j}:
//                      Z[d] = X+[-d mod ND]) are folded into the row the last pass stores to: row d leaves as one run
//                      of gates.  PFB_PD_BEST keeps the last pass's powers, lays them out by written row in the LDS
//                      the tile has left, and reduces over the rows in ascending order.
//   pd_noncoherent     the same loads, one lane per gate, the K squared magnitudes added in order
//   pd_gather          the gate samples of the part of a call that belongs to the open CPI, into the K x R carry
//   pd_count           the async call's count, host-known, written in stream order
// The host keeps all the state there is (stream index, CPI counter, whether a CPI is open): how many CPIs a call closes
// depends on lengths alone.  No atomics, no inline assembly of its own, no MFMA.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <new>
#include <string>
#include <type_traits>
#include <vector>

#include "pfb_common.h"
#include "pfb_cplx.hpp"
#include "pfb_host.h"

namespace {

using namespace pfb;

constexpr uint64_t kStepSamples = (uint64_t)1 << 22;   // per staging step of a host buffer
constexpr uint64_t kMaxCarryBytes = (uint64_t)64 << 20;
constexpr uint64_t kMaxIndex = (uint64_t)1 << 62;
constexpr int kThreads = 256;
// The ND x TG tile of complex64: 32 KiB up to ND = 512, so that five workgroups share a CU's 160 KiB and one's loads run
// under another's passes (measured on 2^27 samples, complex out: 0.49 to 0.56 ms against 0.78 with 64 KiB tiles up to
// ND = 256, 0.75 against 0.81 at ND = 512); 64 KiB at ND = 1024, where half the tile would leave row pieces of 32 bytes
// (1.12 ms against 0.93) and twice the tile, 16 gates in 128 KiB, leaves a CU one workgroup (1.30 against 0.90).
// ND = 8 and 16 have no tile.
constexpr int tile_elems_of(int nd) { return nd <= 512 ? 4096 : 8192; }
constexpr int tile_gates_of(int nd) { return nd <= 16 ? kThreads : tile_elems_of(nd) / nd; }

struct PdParams {
  const float2* src;     // gate 0 of pulse 0 of the launch's first CPI
  long long row_stride;  // L in the stream, R in the carry
  long long cpi_stride;  // K L
  const float* win;
  const float2* tw;      // e^{+j 2 pi m / ND}
  void* out;             // the launch's first CPI
  int R, K, tiles;
  int kind;
  int half;              // ND/2 with PFB_PD_CENTERED, else 0
};

__device__ __forceinline__ float power_of(v2f z) { return __fmaf_rn(z.x, z.x, z.y * z.y); }

// the windowed sample of pulse k at absolute gate g; a zero outside the matrix
__device__ __forceinline__ v2f load_gate(const PdParams& p, const float2* cpi, int k, int g) {
  if (k >= p.K || g >= p.R) return (v2f){0.f, 0.f};
  const float2 z = cpi[(long long)k * p.row_stride + g];
  const float w = p.win[k];
  return (v2f){w * z.x, w * z.y};
}

// the row transform index k is written to: d = -k mod ND, shifted by half a turn when centered
template <int ND>
__device__ __forceinline__ int row_of(int k, int half) { return (((ND - k) & (ND - 1)) + half) & (ND - 1); }

template <int ND>
__device__ __forceinline__ void store_row(const PdParams& p, long long cpi, int rho, int g, v2f z) {
  const long long at = (cpi * ND + rho) * (long long)p.R + g;
  if (p.kind == PFB_PD_COMPLEX) static_cast<float2*>(p.out)[at] = make_float2(z.x, z.y);
  else static_cast<float*>(p.out)[at] = power_of(z);
}

__device__ __forceinline__ void store_cell(const PdParams& p, long long cpi, int g, float power, int rho) {
  pfb_mfbank_cell c;
  c.power = power;
  c.hypothesis = p.half ? rho - p.half : rho;
  static_cast<pfb_mfbank_cell*>(p.out)[cpi * (long long)p.R + g] = c;
}

// one decimation-in-frequency pass of radix R over the ND x TG tile; DONE = the product of the radices before it.
// The first pass issues all of a thread's loads (16 or 32) before it transforms any of them.
template <int ND, int TG, int R, int DONE, bool FIRST>
__device__ __forceinline__ void inner_pass(v2f* lds, const PdParams& p, const float2* cpi, int g0) {
  constexpr int Ls = ND / DONE, m = Ls / R, items = (ND / R) * TG, iters = items / kThreads;
  static_assert(m > 1, "the last pass stores to global memory");
  static_assert(items % kThreads == 0, "whole iterations");
  v2f x[iters][R];
  if constexpr (FIRST) {
#pragma unroll
    for (int i = 0; i < iters; ++i) {
      const int it = (int)threadIdx.x + i * kThreads;
#pragma unroll
      for (int q = 0; q < R; ++q) x[i][q] = load_gate(p, cpi, (it / TG) % m + q * m, g0 + it % TG);
    }
  }
#pragma unroll
  for (int i = 0; i < iters; ++i) {
    const int it = (int)threadIdx.x + i * kThreads;
    const int gate = it % TG, bf = it / TG;
    const int blk = bf / m, j = bf % m, base = blk * Ls + j;
    if constexpr (!FIRST) {
#pragma unroll
      for (int q = 0; q < R; ++q) x[i][q] = lds[(base + q * m) * TG + gate];
    }
    Dft<R>::run(x[i]);
    // a wave's 64 lanes are gates of one row when TG >= 64: its twiddles come by scalar loads
    const int ju = TG >= 64 ? __builtin_amdgcn_readfirstlane(j) : j;
    lds[base * TG + gate] = x[i][0];
#pragma unroll
    for (int q = 1; q < R; ++q) {
      const float2 w = p.tw[ju * q * DONE];  // W_Ls^(j q)
      lds[(base + q * m) * TG + gate] = cmul(x[i][q], w.x, w.y);
    }
  }
}

template <int R1, int R2, int R3>
__global__ void __launch_bounds__(kThreads) pd_dft(const PdParams p) {
  constexpr int ND = R1 * R2 * R3, TG = tile_gates_of(ND);
  constexpr int RL = R3 > 1 ? R3 : R2 > 1 ? R2 : R1;  // the last pass's radix
  constexpr int items = (ND / RL) * TG, iters = items / kThreads;
  static_assert(items % kThreads == 0 && TG <= kThreads && kThreads % TG == 0, "whole iterations");
  const int tile = (int)(blockIdx.x % (unsigned)p.tiles);
  const long long cpi = (long long)(blockIdx.x / (unsigned)p.tiles);
  const int g0 = tile * TG;
  const float2* src = p.src + cpi * p.cpi_stride;

  if constexpr (R2 == 1) {  // one pass: global memory, registers, global memory
    const int g = g0 + (int)threadIdx.x;
    v2f x[ND];
#pragma unroll
    for (int q = 0; q < ND; ++q) x[q] = load_gate(p, src, q, g);
    Dft<ND>::run(x);
    if (g >= p.R) return;
    if (p.kind != PFB_PD_BEST) {
#pragma unroll
      for (int q = 0; q < ND; ++q) store_row<ND>(p, cpi, row_of<ND>(q, p.half), g, x[q]);
      return;
    }
    // written row rho holds d = (rho - half) mod ND = X+[(half - rho) mod ND]: walked with constant indices
    float bp = 0.f;
    int bi = 0;
    auto walk = [&](auto centered) {
      constexpr int H = decltype(centered)::value ? ND / 2 : 0;
      bp = power_of(x[H]);  // rho = 0
#pragma unroll
      for (int rho = 1; rho < ND; ++rho) {
        const float v = power_of(x[(H - rho + ND) & (ND - 1)]);
        if (v > bp) { bp = v; bi = rho; }
      }
    };
    if (p.half) walk(std::true_type());
    else walk(std::false_type());
    store_cell(p, cpi, g, bp, bi);
  } else {
    __shared__ v2f lds[ND * TG];
    inner_pass<ND, TG, R1, 1, true>(lds, p, src, g0);
    __syncthreads();
    if constexpr (R3 > 1) {
      inner_pass<ND, TG, R2, R1, false>(lds, p, src, g0);
      __syncthreads();
    }
    // last pass: block b holds rows b RL .. b RL + RL-1; its output q is transform index kbase(b) + q ND/RL
    auto kbase = [](int blk) { return R3 > 1 ? blk / R2 + R1 * (blk % R2) : blk; };
    if (p.kind != PFB_PD_BEST) {
      for (int it = threadIdx.x; it < items; it += kThreads) {
        const int gate = it % TG, blk = it / TG;
        v2f x[RL];
#pragma unroll
        for (int q = 0; q < RL; ++q) x[q] = lds[(blk * RL + q) * TG + gate];
        Dft<RL>::run(x);
        if (g0 + gate < p.R) {
          const int k0 = kbase(blk);
#pragma unroll
          for (int q = 0; q < RL; ++q) store_row<ND>(p, cpi, row_of<ND>(k0 + q * (ND / RL), p.half), g0 + gate, x[q]);
        }
      }
      return;
    }
    float pw[iters][RL];
#pragma unroll
    for (int i = 0; i < iters; ++i) {
      const int it = (int)threadIdx.x + i * kThreads;
      const int gate = it % TG, blk = it / TG;
      v2f x[RL];
#pragma unroll
      for (int q = 0; q < RL; ++q) x[q] = lds[(blk * RL + q) * TG + gate];
      Dft<RL>::run(x);
#pragma unroll
      for (int q = 0; q < RL; ++q) pw[i][q] = power_of(x[q]);
    }
    __syncthreads();  // every read of the tile is done: its first half now holds the powers, by written row
    float* rows = reinterpret_cast<float*>(lds);
#pragma unroll
    for (int i = 0; i < iters; ++i) {
      const int it = (int)threadIdx.x + i * kThreads;
      const int gate = it % TG, k0 = kbase(it / TG);
#pragma unroll
      for (int q = 0; q < RL; ++q) rows[row_of<ND>(k0 + q * (ND / RL), p.half) * TG + gate] = pw[i][q];
    }
    __syncthreads();
    // 256 / TG threads per gate, each walks ND TG / 256 rows in ascending order; -1 stands for "nothing yet": a power
    // is >= 0 or NaN, so the first number displaces it and a NaN does not.  Only row 0 starts the walk as it is.
    constexpr int parts = kThreads / TG, per = ND / parts;
    const int gate = (int)threadIdx.x % TG, part = (int)threadIdx.x / TG;
    float bp = part == 0 ? rows[gate] : -1.f;
    int bi = part * per;
    for (int i = part == 0 ? 1 : 0; i < per; ++i) {
      const int rho = part * per + i;
      const float v = rows[rho * TG + gate];
      if (v > bp) { bp = v; bi = rho; }
    }
    float* part_p = rows + ND * TG;  // the tile's second half is free: the powers fill the first
    int* part_i = reinterpret_cast<int*>(part_p + kThreads);
    part_p[threadIdx.x] = bp;
    part_i[threadIdx.x] = bi;
    __syncthreads();
    if (part == 0 && g0 + gate < p.R) {
      for (int q = 1; q < parts; ++q) {
        const float v = part_p[q * TG + gate];
        if (v > bp) { bp = v; bi = part_i[q * TG + gate]; }
      }
      store_cell(p, cpi, g0 + gate, bp, bi);
    }
  }
}

__global__ void __launch_bounds__(kThreads) pd_noncoherent(const PdParams p) {
  const int tile = (int)(blockIdx.x % (unsigned)p.tiles);
  const long long cpi = (long long)(blockIdx.x / (unsigned)p.tiles);
  const int g = tile * kThreads + (int)threadIdx.x;
  if (g >= p.R) return;
  const float2* src = p.src + cpi * p.cpi_stride;
  float acc = 0.f;
  for (int k0 = 0; k0 < p.K; k0 += 8) {  // eight loads in flight; the sum stays in pulse order (a pulse >= K adds 0)
    v2f z[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) z[i] = load_gate(p, src, k0 + i, g);
#pragma unroll
    for (int i = 0; i < 8; ++i) acc = __fadd_rn(acc, power_of(z[i]));
  }
  static_cast<float*>(p.out)[cpi * (long long)p.R + g] = acc;
}

// offsets [from, to) of the open CPI (0 = its first sample) lie at y[delta + offset]: their gate samples into the carry
__global__ void __launch_bounds__(kThreads) pd_gather(const float2* y, long long delta, long long from, long long to,
                                                      int k0, int L, int R, float2* carry) {
  const int k = k0 + (int)blockIdx.y;
  const int r = (int)(blockIdx.x * kThreads + threadIdx.x);
  if (r >= R) return;
  const long long off = (long long)k * L + r;
  if (off >= from && off < to) carry[(long long)k * R + r] = y[delta + off];
}

__global__ void pd_count(unsigned long long* dst, unsigned long long value) { *dst = value; }

// ---------------------------------------------------------------------------------
// host: checks and plan

uint32_t resolve_length(uint32_t K, uint32_t nd) {  // 0: not in the set, or K does not fit
  if (nd == 0)
    for (nd = 8; nd < K && nd < 2048; nd <<= 1) {}
  if (nd < 8 || nd > 1024 || (nd & (nd - 1)) || K > nd) return 0;
  return nd;
}

const char* kernel_name(uint32_t nd, uint32_t output) {
  if (output == PFB_PD_NONCOHERENT) return "pfb_pd_noncoherent";
  switch (nd) {
    case 8: return "pfb_pd_dft<8>";
    case 16: return "pfb_pd_dft<16>";
    case 32: return "pfb_pd_dft<8,4>";
    case 64: return "pfb_pd_dft<8,8>";
    case 128: return "pfb_pd_dft<16,8>";
    case 256: return "pfb_pd_dft<16,16>";
    case 512: return "pfb_pd_dft<8,8,8>";
    default: return "pfb_pd_dft<16,8,8>";
  }
}

size_t out_elem_bytes(uint32_t output) { return output == PFB_PD_COMPLEX || output == PFB_PD_BEST ? 8 : 4; }

// Everything pfb_pd_describe and pfb_pd_create check before the device, in the order the header states
int pd_check(const pfb_pd_config* cfg, pfb_pd_plan* plan) {
  if (!cfg || !plan || cfg->struct_size != sizeof(pfb_pd_config)) return PFB_ERR_BAD_ARG;
  const uint64_t L = cfg->pri, R = cfg->num_gates, K = cfg->num_pulses;
  if (L == 0 || R == 0 || K == 0 || R > L) return PFB_ERR_BAD_ARG;
  const uint32_t nd = resolve_length(cfg->num_pulses, cfg->doppler_length);
  if (nd == 0) return PFB_ERR_BAD_ARG;
  if (L > ((uint64_t)1 << 24) || cfg->origin > kMaxIndex) return PFB_ERR_BAD_ARG;
  if (cfg->output > PFB_PD_NONCOHERENT || (cfg->flags & ~(uint32_t)PFB_PD_CENTERED)) return PFB_ERR_BAD_ARG;
  if (cfg->window)
    for (uint64_t k = 0; k < K; ++k)
      if (!std::isfinite(cfg->window[k])) return PFB_ERR_BAD_ARG;
  if (K * R * sizeof(float2) > kMaxCarryBytes) return PFB_ERR_UNSUPPORTED;
  const bool rows = cfg->output == PFB_PD_COMPLEX || cfg->output == PFB_PD_POWER;
  plan->doppler_length = nd;
  plan->tile_gates = cfg->output == PFB_PD_NONCOHERENT ? (uint32_t)kThreads : (uint32_t)tile_gates_of((int)nd);
  plan->carry_bytes = K * R * sizeof(float2);
  plan->cpi_samples = (K - 1) * L + R;
  plan->cpi_outputs = rows ? (uint64_t)nd * R : R;
  std::memset(plan->kernel, 0, sizeof(plan->kernel));
  std::snprintf(plan->kernel, sizeof(plan->kernel), "%s", kernel_name(nd, cfg->output));
  return PFB_OK;
}

struct HostState {     // all there is: what a call closes depends on lengths alone
  uint64_t index = 0;  // stream index of the next sample
  uint64_t cpi = 0;    // the open CPI, or the next one to open: its first sample is not before `index` unless open
  bool open = false;
};

// What a failed call leaves behind: the state as before it.  The carry then still holds the open CPI's earlier samples
// -- a repeat of the call gathers the rest into the same places -- unless the call had closed that CPI and begun the
// next one in the carry (`reused`): its samples are gone, so it is dropped, as pfb_pd_set_index(index) would drop it.
void put_back(HostState* hs, const HostState& saved, bool reused, uint64_t origin, uint64_t KL) {
  *hs = saved;
  if (!saved.open || !reused) return;
  hs->open = false;
  hs->cpi = saved.index > origin ? (saved.index - origin + KL - 1) / KL : 0;
}

}  // namespace

struct pfb_pd_handle {
  pfb_pd_config cfg{};
  pfb_pd_plan plan{};
  int device = 0;
  hipStream_t stream = nullptr;
  hipEvent_t ev_switch = nullptr;
  HostState hs;
  float* d_win = nullptr;
  float2* d_tw = nullptr;
  float2* d_carry = nullptr;
  void* d_stage = nullptr;  // host samples on their way in
  size_t stage_bytes = 0;
  void* d_out = nullptr;    // a step's CPIs on their way out to a host buffer
  size_t out_bytes = 0;
  std::string name_stream, name_carry;
  const char* last_kernel = "";
  bool carry_reused = false;  // since the call began: the carry was zeroed for another CPI
};

namespace {

void free_pd(pfb_pd_handle* h) {
  if (!h) return;
  DeviceGuard g(h->device);
  (void)hipFree(h->d_win);
  (void)hipFree(h->d_tw);
  (void)hipFree(h->d_carry);
  (void)hipFree(h->d_stage);
  (void)hipFree(h->d_out);
  if (h->ev_switch) (void)hipEventDestroy(h->ev_switch);
  delete h;
}

hipError_t allocate_pd(pfb_pd_handle* h) {
  const uint32_t K = h->cfg.num_pulses;
  std::vector<float> w(K, 1.f);
  if (h->cfg.window) std::copy(h->cfg.window, h->cfg.window + K, w.begin());
  h->cfg.window = nullptr;  // the caller's array is not read again
  hipError_t e = hipMalloc(reinterpret_cast<void**>(&h->d_win), K * sizeof(float));
  if (e == hipSuccess) e = hipMemcpy(h->d_win, w.data(), K * sizeof(float), hipMemcpyHostToDevice);
  if (e == hipSuccess) e = pfb::upload_twiddles(h->plan.doppler_length, &h->d_tw);
  if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&h->d_carry), (size_t)h->plan.carry_bytes);
  return e;
}

int create_pd(const pfb_pd_config* cfg, pfb_pd_handle** out) {
  pfb_pd_plan plan{};
  int rc = pd_check(cfg, &plan);
  if (rc != PFB_OK) return rc;
  int dev = 0;
  rc = pfb::resolve_device(cfg->device_id, &dev);
  if (rc != PFB_OK) return rc;
  pfb_pd_handle* h = new pfb_pd_handle();
  h->cfg = *cfg;
  h->plan = plan;
  h->device = dev;
  h->name_stream = std::string(plan.kernel) + "[stream]";
  h->name_carry = std::string(plan.kernel) + "[carry]";
  DeviceGuard g(dev);
  const hipError_t e = allocate_pd(h);
  if (e != hipSuccess) {
    rc = pfb::hip_fail(e, "pfb_pd_create allocation");
    free_pd(h);
    return rc;
  }
  *out = h;
  return PFB_OK;
}

uint64_t cpi_bytes(const pfb_pd_handle* h) { return h->plan.cpi_outputs * out_elem_bytes(h->cfg.output); }

// the CPIs that n more samples complete
uint64_t cpis_for(const pfb_pd_handle* h, uint64_t n) {
  const uint64_t KL = (uint64_t)h->cfg.num_pulses * h->cfg.pri;
  const uint64_t end = h->cfg.origin + h->hs.cpi * KL + h->plan.cpi_samples;  // one past the sample that completes it
  const uint64_t n1 = h->hs.index + n;
  return end > n1 ? 0 : (n1 - end) / KL + 1;
}

// transform `count` CPIs that lie cpi_stride apart from `src`, rows row_stride apart, into `out`
int launch_cpis(pfb_pd_handle* h, const float2* src, uint64_t row_stride, uint64_t count, void* out, bool from_carry) {
  const pfb_pd_config& c = h->cfg;
  const uint32_t TG = h->plan.tile_gates;
  PdParams p{};
  p.row_stride = (long long)row_stride;
  p.cpi_stride = (long long)((uint64_t)c.num_pulses * c.pri);
  p.win = h->d_win;
  p.tw = h->d_tw;
  p.R = (int)c.num_gates;
  p.K = (int)c.num_pulses;
  p.tiles = (int)((c.num_gates + TG - 1) / TG);
  p.kind = (int)c.output;
  p.half = (c.flags & PFB_PD_CENTERED) ? (int)h->plan.doppler_length / 2 : 0;
  const uint64_t per_launch = std::max<uint64_t>(1, ((uint64_t)1 << 30) / (uint64_t)p.tiles);
  for (uint64_t done = 0; done < count;) {
    const uint64_t m = std::min(per_launch, count - done);
    p.src = src + done * (uint64_t)p.cpi_stride;
    p.out = static_cast<char*>(out) + done * cpi_bytes(h);
    const dim3 grid((unsigned)(m * (uint64_t)p.tiles)), block(kThreads);
    if (c.output == PFB_PD_NONCOHERENT) {
      hipLaunchKernelGGL(pd_noncoherent, grid, block, 0, h->stream, p);
    } else {
      switch (h->plan.doppler_length) {
        case 8: hipLaunchKernelGGL((pd_dft<8, 1, 1>), grid, block, 0, h->stream, p); break;
        case 16: hipLaunchKernelGGL((pd_dft<16, 1, 1>), grid, block, 0, h->stream, p); break;
        case 32: hipLaunchKernelGGL((pd_dft<8, 4, 1>), grid, block, 0, h->stream, p); break;
        case 64: hipLaunchKernelGGL((pd_dft<8, 8, 1>), grid, block, 0, h->stream, p); break;
        case 128: hipLaunchKernelGGL((pd_dft<16, 8, 1>), grid, block, 0, h->stream, p); break;
        case 256: hipLaunchKernelGGL((pd_dft<16, 16, 1>), grid, block, 0, h->stream, p); break;
        case 512: hipLaunchKernelGGL((pd_dft<8, 8, 8>), grid, block, 0, h->stream, p); break;
        default: hipLaunchKernelGGL((pd_dft<16, 8, 8>), grid, block, 0, h->stream, p); break;
      }
    }
    done += m;
  }
  HIP_TRY(hipGetLastError());
  h->last_kernel = from_carry ? h->name_carry.c_str() : h->name_stream.c_str();
  return PFB_OK;
}

// samples [a, b) of the stream, a call that starts at stream index n0 in y, into the open CPI's carry
int gather(pfb_pd_handle* h, const float2* y, uint64_t n0, uint64_t a, uint64_t b) {
  if (b <= a) return PFB_OK;
  const pfb_pd_config& c = h->cfg;
  const uint64_t L = c.pri, R = c.num_gates;
  const uint64_t first = c.origin + h->hs.cpi * (uint64_t)c.num_pulses * L;  // a >= first
  const uint64_t from = a - first, to = b - first;
  const uint64_t k0 = from / L, k1 = std::min<uint64_t>((to - 1) / L, c.num_pulses - 1);
  if (k1 < k0) return PFB_OK;
  const long long delta = first >= n0 ? (long long)(first - n0) : -(long long)(n0 - first);
  const dim3 grid((unsigned)((R + kThreads - 1) / kThreads), (unsigned)(k1 - k0 + 1));
  hipLaunchKernelGGL(pd_gather, grid, dim3(kThreads), 0, h->stream, y, delta, (long long)from, (long long)to, (int)k0, (int)L,
                     (int)R, h->d_carry);
  HIP_TRY(hipGetLastError());
  return PFB_OK;
}

// n device samples at y, queued on the handle's stream; the CPIs they complete go to `out` from its start, their number
// to *closed, and the host state advances
int pd_enqueue(pfb_pd_handle* h, const float2* y, uint64_t n, void* out, uint64_t* closed) {
  const pfb_pd_config& c = h->cfg;
  HostState& hs = h->hs;
  const uint64_t L = c.pri, R = c.num_gates, KL = (uint64_t)c.num_pulses * L, span = h->plan.cpi_samples;
  const uint64_t n0 = hs.index, n1 = n0 + n;
  uint64_t cnt = 0;
  if (n > 0 && hs.open) {
    const uint64_t end = c.origin + hs.cpi * KL + span;
    int rc = gather(h, y, n0, n0, std::min(n1, end));
    if (rc != PFB_OK) return rc;
    if (end <= n1) {
      rc = launch_cpis(h, h->d_carry, R, 1, out, true);
      if (rc != PFB_OK) return rc;
      cnt = 1;
      hs.open = false;
      ++hs.cpi;
    }
  }
  if (n > 0 && !hs.open) {
    uint64_t first = c.origin + hs.cpi * KL;  // >= n0
    if (first + span <= n1) {
      const uint64_t m = (n1 - first - span) / KL + 1;
      const int rc = launch_cpis(h, y + (first - n0), L, m, static_cast<char*>(out) + cnt * cpi_bytes(h), false);
      if (rc != PFB_OK) return rc;
      cnt += m;
      hs.cpi += m;
      first += m * KL;
    }
    if (first < n1) {  // this CPI opens here and ends in a later call
      h->carry_reused = true;
      HIP_TRY(hipMemsetAsync(h->d_carry, 0, (size_t)h->plan.carry_bytes, h->stream));
      hs.open = true;
      const int rc = gather(h, y, n0, first, n1);
      if (rc != PFB_OK) return rc;
    }
  }
  hs.index = n1;
  *closed = cnt;
  return PFB_OK;
}

int pd_flush_open(pfb_pd_handle* h, void* out) {  // the open CPI, from the carry as it stands
  const int rc = launch_cpis(h, h->d_carry, h->cfg.num_gates, 1, out, true);
  if (rc != PFB_OK) return rc;
  h->hs.open = false;
  ++h->hs.cpi;
  return PFB_OK;
}

void undo(pfb_pd_handle* h, const HostState& saved) {
  put_back(&h->hs, saved, h->carry_reused, h->cfg.origin, (uint64_t)h->cfg.num_pulses * h->cfg.pri);
}

// A host-pointer call: steps of kStepSamples through one staging buffer, each step's CPIs back before the next.  A step
// that fails ends the call with the state put_back leaves.
int pd_host_call(pfb_pd_handle* h, const float2* y, uint64_t n, bool flush, char* out) {
  const HostState saved = h->hs;
  h->carry_reused = false;
  auto fail = [&](int code) {
    (void)hipStreamSynchronize(h->stream);
    undo(h, saved);
    return code;
  };
  uint64_t total = 0;
  for (uint64_t done = 0; flush ? done == 0 : done < n;) {
    const uint64_t m = flush ? 0 : std::min(kStepSamples, n - done);
    const uint64_t expect = flush ? 1 : cpis_for(h, m);
    int rc = grow(&h->d_out, &h->out_bytes, (size_t)(expect * cpi_bytes(h)));
    if (rc == PFB_OK && m > 0) rc = grow(&h->d_stage, &h->stage_bytes, (size_t)(std::min(n, kStepSamples) * sizeof(float2)));
    if (rc != PFB_OK) return fail(rc);
    uint64_t cnt = 0;
    if (flush) {
      rc = pd_flush_open(h, h->d_out);
      cnt = 1;
    } else {
      const hipError_t e = hipMemcpyAsync(h->d_stage, y + done, (size_t)(m * sizeof(float2)), hipMemcpyHostToDevice, h->stream);
      if (e != hipSuccess) return fail(pfb::hip_fail(e, "pfb_pd_process staging"));
      rc = pd_enqueue(h, static_cast<const float2*>(h->d_stage), m, h->d_out, &cnt);
    }
    if (rc != PFB_OK) return fail(rc);
    hipError_t e = hipSuccess;
    if (cnt > 0) e = hipMemcpyAsync(out + total * cpi_bytes(h), h->d_out, (size_t)(cnt * cpi_bytes(h)), hipMemcpyDeviceToHost, h->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);  // the one staging buffer is free again
    if (e != hipSuccess) return fail(pfb::hip_fail(e, "pfb_pd_process"));
    total += cnt;
    done += m + (flush ? 1 : 0);
  }
  return PFB_OK;
}

// what every process call checks before the device is touched
int pd_check_call(const pfb_pd_handle* h, const void* y, uint64_t n, const void* out, uint64_t capacity, const void* count_out,
                  bool device) {
  if (!h || !count_out || (n > 0 && !y) || (capacity > 0 && !out)) return PFB_ERR_BAD_ARG;
  if (n > kMaxIndex || h->hs.index + n > kMaxIndex) return PFB_ERR_BAD_ARG;
  if (device && ((reinterpret_cast<uintptr_t>(y) % sizeof(float2)) || (reinterpret_cast<uintptr_t>(out) % out_elem_bytes(h->cfg.output))))
    return PFB_ERR_BAD_ARG;
  return PFB_OK;
}

}  // namespace

extern "C" int pfb_pd_describe(const pfb_pd_config* cfg, pfb_pd_plan* plan_out) {
  return pfb::abi_guard([&]() -> int {
    pfb_pd_plan plan{};
    const int rc = pd_check(cfg, plan_out ? &plan : nullptr);
    if (rc == PFB_OK) *plan_out = plan;
    return rc;
  });
}

extern "C" int pfb_pd_doppler_frequencies(const pfb_pd_config* cfg, double fs, double* out) {
  return pfb::abi_guard([&]() -> int {
    if (!cfg || !out || cfg->struct_size != sizeof(pfb_pd_config) || !std::isfinite(fs)) return PFB_ERR_BAD_ARG;
    const uint32_t nd = cfg->num_pulses ? resolve_length(cfg->num_pulses, cfg->doppler_length) : 0;
    if (nd == 0 || cfg->pri == 0 || cfg->pri > (1u << 24) || (cfg->flags & ~(uint32_t)PFB_PD_CENTERED)) return PFB_ERR_BAD_ARG;
    const int first = (cfg->flags & PFB_PD_CENTERED) ? -(int)(nd / 2) : 0;
    for (uint32_t i = 0; i < nd; ++i) out[i] = (double)(first + (int)i) * fs / ((double)nd * (double)cfg->pri);
    return PFB_OK;
  });
}

extern "C" int pfb_pd_create(const pfb_pd_config* cfg, pfb_pd_handle** out) {
  return pfb::abi_guard([&]() -> int {
    if (!out) return PFB_ERR_BAD_ARG;
    *out = nullptr;
    return create_pd(cfg, out);
  });
}

extern "C" int pfb_pd_destroy(pfb_pd_handle* h) {
  return pfb::abi_guard([&]() -> int {
    if (!h) return PFB_ERR_BAD_ARG;
    free_pd(h);
    return PFB_OK;
  });
}

extern "C" int pfb_pd_reset(pfb_pd_handle* h) {
  return pfb::abi_guard([&]() -> int {
    if (!h) return PFB_ERR_BAD_ARG;
    h->hs = HostState();
    return PFB_OK;
  });
}

extern "C" int pfb_pd_set_stream(pfb_pd_handle* h, void* hip_stream) {
  return pfb::abi_guard([&]() -> int {
    if (!h) return PFB_ERR_BAD_ARG;
    return pfb::switch_stream(h->device, &h->stream, &h->ev_switch, static_cast<hipStream_t>(hip_stream));
  });
}

extern "C" int pfb_pd_sync(pfb_pd_handle* h) {
  return pfb::abi_guard([&]() -> int {
    if (!h) return PFB_ERR_BAD_ARG;
    DeviceGuard g(h->device);
    HIP_TRY(hipStreamSynchronize(h->stream));
    return PFB_OK;
  });
}

extern "C" int pfb_pd_get_device(const pfb_pd_handle* h, int* device_id) {
  return pfb::abi_guard([&]() -> int {
    if (!h || !device_id) return PFB_ERR_BAD_ARG;
    *device_id = h->device;
    return PFB_OK;
  });
}

extern "C" int pfb_pd_cpis_for(const pfb_pd_handle* h, uint64_t num_samples, uint64_t* cpis_out) {
  return pfb::abi_guard([&]() -> int {
    if (!h || !cpis_out || num_samples > kMaxIndex || h->hs.index + num_samples > kMaxIndex) return PFB_ERR_BAD_ARG;
    *cpis_out = cpis_for(h, num_samples);
    return PFB_OK;
  });
}

extern "C" int pfb_pd_next_index(const pfb_pd_handle* h, uint64_t* index_out) {
  return pfb::abi_guard([&]() -> int {
    if (!h || !index_out) return PFB_ERR_BAD_ARG;
    *index_out = h->hs.index;
    return PFB_OK;
  });
}

extern "C" int pfb_pd_set_index(pfb_pd_handle* h, uint64_t next_sample) {
  return pfb::abi_guard([&]() -> int {
    if (!h || next_sample > kMaxIndex) return PFB_ERR_BAD_ARG;
    const uint64_t KL = (uint64_t)h->cfg.num_pulses * h->cfg.pri, o = h->cfg.origin;
    h->hs.open = false;
    h->hs.index = next_sample;
    h->hs.cpi = next_sample > o ? (next_sample - o + KL - 1) / KL : 0;  // the first CPI that starts at or after it
    return PFB_OK;
  });
}

extern "C" int pfb_pd_process(pfb_pd_handle* h, const void* y, uint64_t num_samples, void* out, uint64_t capacity_cpis,
                              uint64_t* cpis_out, uint32_t mem) {
  return pfb::abi_guard([&]() -> int {
    if (mem > PFB_MEM_DEVICE) return PFB_ERR_BAD_ARG;
    int rc = pd_check_call(h, y, num_samples, out, capacity_cpis, cpis_out, mem == PFB_MEM_DEVICE);
    if (rc != PFB_OK) return rc;
    const uint64_t need = cpis_for(h, num_samples);
    *cpis_out = need;
    if (need > capacity_cpis) return PFB_ERR_CAPACITY;
    DeviceGuard g(h->device);
    if (mem == PFB_MEM_HOST) return pd_host_call(h, static_cast<const float2*>(y), num_samples, false, static_cast<char*>(out));
    const HostState saved = h->hs;
    h->carry_reused = false;
    uint64_t cnt = 0;
    rc = pd_enqueue(h, static_cast<const float2*>(y), num_samples, out, &cnt);
    if (rc == PFB_OK) {
      const hipError_t e = hipStreamSynchronize(h->stream);
      if (e != hipSuccess) rc = pfb::hip_fail(e, "pfb_pd_process");
    }
    if (rc != PFB_OK) undo(h, saved);
    return rc;
  });
}

extern "C" int pfb_pd_process_async(pfb_pd_handle* h, const void* d_y, uint64_t num_samples, void* d_out,
                                    uint64_t capacity_cpis, uint64_t* d_cpis_out) {
  return pfb::abi_guard([&]() -> int {
    int rc = pd_check_call(h, d_y, num_samples, d_out, capacity_cpis, d_cpis_out, true);
    if (rc != PFB_OK) return rc;
    if (reinterpret_cast<uintptr_t>(d_cpis_out) % 8) return PFB_ERR_BAD_ARG;
    if (cpis_for(h, num_samples) > capacity_cpis) return PFB_ERR_CAPACITY;
    DeviceGuard g(h->device);
    const HostState saved = h->hs;
    h->carry_reused = false;
    uint64_t cnt = 0;
    rc = pd_enqueue(h, static_cast<const float2*>(d_y), num_samples, d_out, &cnt);
    if (rc == PFB_OK) {
      hipLaunchKernelGGL(pd_count, dim3(1), dim3(1), 0, h->stream, reinterpret_cast<unsigned long long*>(d_cpis_out),
                         (unsigned long long)cnt);
      const hipError_t e = hipGetLastError();
      if (e != hipSuccess) rc = pfb::hip_fail(e, "pfb_pd_process_async");
    }
    if (rc != PFB_OK) undo(h, saved);
    return rc;
  });
}

extern "C" int pfb_pd_flush(pfb_pd_handle* h, void* out, uint64_t capacity_cpis, uint64_t* cpis_out, uint32_t mem) {
  return pfb::abi_guard([&]() -> int {
    if (mem > PFB_MEM_DEVICE || !h || !cpis_out || (capacity_cpis > 0 && !out)) return PFB_ERR_BAD_ARG;
    if (mem == PFB_MEM_DEVICE && reinterpret_cast<uintptr_t>(out) % out_elem_bytes(h->cfg.output)) return PFB_ERR_BAD_ARG;
    *cpis_out = h->hs.open ? 1 : 0;
    if (!h->hs.open) return PFB_OK;
    if (capacity_cpis < 1) return PFB_ERR_CAPACITY;
    DeviceGuard g(h->device);
    if (mem == PFB_MEM_HOST) return pd_host_call(h, nullptr, 0, true, static_cast<char*>(out));
    const HostState saved = h->hs;
    h->carry_reused = false;
    int rc = pd_flush_open(h, out);
    if (rc == PFB_OK) {
      const hipError_t e = hipStreamSynchronize(h->stream);
      if (e != hipSuccess) rc = pfb::hip_fail(e, "pfb_pd_flush");
    }
    if (rc != PFB_OK) undo(h, saved);
    return rc;
  });
}

extern "C" const char* pfb_pd_last_kernel(const pfb_pd_handle* h) { return h ? h->last_kernel : ""; }
