// pfb_chsyn.hip -- the channel synthesizer (pfb_chsyn_* in include/pfb_channelizer.h, where the arithmetic is defined):
// the twin of the channelizer, F frames of M channel values in, F*D samples of the full-rate stream out.
//   v_m[p] = sum_k w[c(k)] y[m, c(k)] e^{+j 2 pi k p / M}
//   x[bD + d] = scale * sum_{q < Q} g[d + qD] v_{b-q}[(d + qD) mod M]         (q ascending, one FMA per term)
// Both routes make a frame's row v_m the same way wherever the frame sits (tile, call, chunk, staging step) and carry
// the last Q-1 ROWS (not input frames: the weights of a frame are the ones in force when it was taken) in one of two
// device buffers, read from one and written to the other by the same launch.  With the fixed q order that makes the
// output the same bits under any cutting of the stream, within one route.
//
//   generic route, any M      pfb_chsyn_rows: tile_frames frames per workgroup through generic_stockham / generic_dft of
//                             pfb_generic_fft.hpp (weights and column order applied at the load) into the workspace,
//                             slot f = frame f of the chunk; the workgroups also write the next carried rows.
//                             pfb_chsyn_fir<FMT>: one output sample per lane out of the workspace and the carried rows.
//                             The workspace is grow-only, at most 64 MiB; a longer call is walked in chunks.
//   fused route               pfb_chsyn_fused<M, R0, R1, FMT>, M = R0 R1 in {56, 64, 128, 256}: a 256-thread workgroup
//                             owns T consecutive output blocks b0 .. b0+T-1 and holds rows b0-Q+1 .. b0+T-1 in LDS.
//     LOAD   frames with 16-byte lane loads where the pointer and ld allow (8-byte otherwise), times the weights,
//            stored transposed: u[R1 a + b] at slot (b, a) of the row; rows before the call from the carry buffer
//     PASS 1 item (row, b): Dft<R0> over a in registers, times W_M^{b c}, back in place
//     PASS 2 item (row, c): Dft<R1> over b in registers, back in place: v[c + R0 d] sits at slot (d, c), natural order
//     FIR    a lane makes 2 (cf32) or 4 (int16) consecutive samples: per q one 16-byte read of g (lanes of a wave read
//            consecutive d) and one or two 16-byte LDS reads, one 16-byte store at the end (4 / 8-byte stores when
//            `out` is not 16-byte aligned)
//     CARRY  the last workgroup writes rows F-Q+1 .. F-1 to the other carry buffer
//   A row is R1 groups of R0 values, each group followed by 2 values of padding: groups start on 16 bytes, and the
//   R0-value runs pass 1 reads from consecutive lanes do not fall on one bank.  LDS = (T + Q - 1) rows <= 64 KiB.
// No atomics; every store is a vector store from plain C++.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <new>
#include <vector>

#include "pfb_cplx.hpp"
#include "pfb_generic_fft.hpp"
#include "pfb_host.h"

namespace {

using namespace pfb;

constexpr int kThreads = 256;
constexpr uint32_t kMaxM = 4096, kMaxP = 24;
constexpr uint64_t kWorkspaceCap = (uint64_t)64 << 20;  // generic route: bytes of rows held at once
constexpr uint64_t kStageBytes = (uint64_t)64 << 20;    // per side of the host staging
constexpr int kLdsComplex = 8192;                       // 64 KiB of float2
constexpr int kPad = 2;                                 // padding values behind every R0 group of a fused row

// Kernel-side view of one launch.  Local frame f >= 0 is y[f * ld ..]; local frame f < 0 is row f + Q - 1 of carry_in.
struct ChsynParams {
  const float2* y;
  const float* w;          // M weights by column
  const float* g;          // M * P_g taps
  const float2* tw;        // tw[m] = exp(+j 2 pi m / M)
  const float2* carry_in;  // Q - 1 rows of M
  float2* carry_out;       // the rows the next launch starts from
  float2* work;            // generic: slot f = v of local frame f
  void* out;               // frames * D samples
  long long ld, frames;
  long long frame0;        // absolute index of local frame 0 (PFB_CHSYN_DEROTATE)
  float scale, full;       // full = 2^(bit_width-1) of the int16 output
  int M, D, Q, T;
  int tile_frames;         // generic: frames per workgroup of pfb_chsyn_rows
  unsigned flags;
  int vec_in, vec_out;     // fused: 16-byte loads / stores are aligned
  GenericPlan plan;
};

PFB_DEV int chsyn_quant(float x, float full) {
  const float t = fminf(fmaxf(roundf(x * full), -full), full - 1.f);
  return x == x ? (int)t : 0;
}
PFB_DEV uint32_t chsyn_pack(v2f x, float full) {
  return ((uint32_t)chsyn_quant(x.x, full) & 0xffffu) | ((uint32_t)chsyn_quant(x.y, full) << 16);
}

// the row index the FIR reads for tap block q of output offset d: (d + qD) mod M, moved by (m D) mod M under DEROTATE
// (m = the absolute index of the row's frame).  D is M or M/2.
PFB_DEV int chsyn_row_index(const ChsynParams& p, int d, int q, long long m) {
  if (p.D == p.M) return d;
  const long long par = (long long)q + ((p.flags & PFB_CHSYN_DEROTATE) ? m : 0);
  return d + ((par & 1) ? p.D : 0);
}

// ---------------------------------------------------------------------------------
// generic route

__global__ void __launch_bounds__(kThreads) pfb_chsyn_rows(const ChsynParams p) {
  extern __shared__ __align__(16) float2 sm[];
  const int M = p.M, TF = p.tile_frames, tid = threadIdx.x;
  const long long f0 = (long long)blockIdx.x * TF;
  const int shift = (p.flags & PFB_CHSYN_FFTSHIFT) ? (M + 1) / 2 : 0;
  for (int idx = tid; idx < TF * M; idx += kThreads) {
    const int t = idx / M, c = idx - t * M;
    const long long f = f0 + t;
    float2 u = make_float2(0.f, 0.f);
    if (f < p.frames) {
      const float2 v = p.y[f * p.ld + c];
      const float w = p.w[c];
      u = make_float2(v.x * w, v.y * w);
    }
    int k = c + shift;
    if (k >= M) k -= M;
    sm[t * M + k] = u;
  }
  __syncthreads();
  if (p.plan.n > 0) generic_stockham(sm, TF, M, p.plan, p.tw, tid, kThreads);
  else generic_dft(sm, TF, M, p.tw, tid, kThreads);
  const long long keep0 = p.frames - (p.Q - 1);  // local frames >= keep0 are carried on
  for (int idx = tid; idx < TF * M; idx += kThreads) {
    const int t = idx / M, pp = idx - t * M;
    const long long f = f0 + t;
    if (f >= p.frames) break;
    const float2 v = sm[TF * M + idx];
    p.work[f * M + pp] = v;
    if (f >= keep0) p.carry_out[(f - keep0) * M + pp] = v;
  }
  // carried rows that stay carried (a launch of fewer than Q - 1 frames): new row r is local frame keep0 + r < 0
  if (keep0 < 0) {
    const long long stay = min(-keep0, (long long)(p.Q - 1)) * M;
    for (long long i = (long long)blockIdx.x * kThreads + tid; i < stay; i += (long long)gridDim.x * kThreads)
      p.carry_out[i] = p.carry_in[p.frames * M + i];
  }
}

template <int FMT>
__global__ void __launch_bounds__(kThreads) pfb_chsyn_fir(const ChsynParams p) {
  const long long s = (long long)blockIdx.x * kThreads + threadIdx.x;
  if (s >= p.frames * p.D) return;
  const long long b = s / p.D;
  const int d = (int)(s - b * p.D);
  v2f acc = (v2f){0.f, 0.f};
  for (int q = 0; q < p.Q; ++q) {
    const long long f = b - q;
    const float2* row = f >= 0 ? p.work + f * p.M : p.carry_in + (f + p.Q - 1) * p.M;
    const float2 v = row[chsyn_row_index(p, d, q, p.frame0 + f)];
    acc = fma2((v2f){v.x, v.y}, splat(p.g[d + q * p.D]), acc);
  }
  acc = acc * splat(p.scale);
  if constexpr (FMT == PFB_FMT_CF32) static_cast<float2*>(p.out)[s] = make_float2(acc.x, acc.y);
  else static_cast<uint32_t*>(p.out)[s] = chsyn_pack(acc, p.full);
}

// ---------------------------------------------------------------------------------
// fused route

template <int M, int R0, int R1, int FMT>
__global__ void __launch_bounds__(kThreads) pfb_chsyn_fused(const ChsynParams p) {
  static_assert(R0 * R1 == M && R0 % 4 == 0, "a row is R1 groups of R0 values");
  constexpr int GS = R0 + kPad;      // group stride
  constexpr int RS = R1 * GS;        // row stride
  constexpr int V = FMT == PFB_FMT_CF32 ? 2 : 4;  // samples per lane: 16 bytes of output
  extern __shared__ __align__(16) float2 sm[];
  const int tid = threadIdx.x, D = p.D, Q = p.Q;
  const long long b0 = (long long)blockIdx.x * p.T;
  const int nb = (int)min((long long)p.T, p.frames - b0);  // output blocks of this workgroup
  const int rows = nb + Q - 1;                             // row r = local frame b0 - (Q - 1) + r
  const int nc = (int)max(0ll, min((long long)(Q - 1) - b0, (long long)rows));  // rows that come from the carry buffer

  // LOAD
  for (int i = tid; i < nc * (M / 2); i += kThreads) {  // carried rows: already transformed, natural order
    const int r = i / (M / 2), pp = 2 * (i - r * (M / 2));
    const float2* src = p.carry_in + (b0 + r) * M + pp;  // local frame b0 - (Q-1) + r is carried row b0 + r
    const float4 v = *reinterpret_cast<const float4*>(src);
    *reinterpret_cast<float4*>(&sm[r * RS + (pp / R0) * GS + pp % R0]) = v;
  }
  const int shift = (p.flags & PFB_CHSYN_FFTSHIFT) ? M / 2 : 0;  // M is even
  for (int i = tid; i < (rows - nc) * (M / 2); i += kThreads) {
    const int rr = i / (M / 2), c = 2 * (i - rr * (M / 2)), r = nc + rr;
    const float2* src = p.y + (b0 - (Q - 1) + r) * p.ld + c;
    float2 u0, u1;
    if (p.vec_in) {
      const float4 v = *reinterpret_cast<const float4*>(src);
      u0 = make_float2(v.x, v.y); u1 = make_float2(v.z, v.w);
    } else {
      u0 = src[0]; u1 = src[1];
    }
    const float2 w = *reinterpret_cast<const float2*>(p.w + c);
    u0.x *= w.x; u0.y *= w.x; u1.x *= w.y; u1.y *= w.y;
    int k = c + shift;
    if (k >= M) k -= M;  // k even: k + 1 < M
    float2* row = sm + r * RS;
    row[(k % R1) * GS + k / R1] = u0;
    row[((k + 1) % R1) * GS + (k + 1) / R1] = u1;
  }
  __syncthreads();

  // PASS 1
  for (int it = tid; it < (rows - nc) * R1; it += kThreads) {
    const int rr = it / R1, b = it - rr * R1;
    float2* grp = sm + (nc + rr) * RS + b * GS;
    v2f x[R0];
#pragma unroll
    for (int a = 0; a < R0; ++a) x[a] = (v2f){grp[a].x, grp[a].y};
    Dft<R0>::run(x);
#pragma unroll
    for (int c = 1; c < R0; ++c) {
      const float2 w = p.tw[b * c];
      x[c] = cmul(x[c], w.x, w.y);
    }
#pragma unroll
    for (int c = 0; c < R0; ++c) grp[c] = make_float2(x[c].x, x[c].y);
  }
  __syncthreads();

  // PASS 2
  for (int it = tid; it < (rows - nc) * R0; it += kThreads) {
    const int rr = it / R0, c = it - rr * R0;
    float2* col = sm + (nc + rr) * RS + c;
    v2f x[R1];
#pragma unroll
    for (int b = 0; b < R1; ++b) x[b] = (v2f){col[b * GS].x, col[b * GS].y};
    Dft<R1>::run(x);
#pragma unroll
    for (int d = 0; d < R1; ++d) col[d * GS] = make_float2(x[d].x, x[d].y);
  }
  __syncthreads();

  // FIR
  const int groups = nb * (D / V);
  for (int gi = tid; gi < groups; gi += kThreads) {
    const int bl = gi / (D / V), d0 = (gi - bl * (D / V)) * V;
    v2f acc[V];
#pragma unroll
    for (int e = 0; e < V; ++e) acc[e] = (v2f){0.f, 0.f};
    for (int q = 0; q < Q; ++q) {
      const int pp = chsyn_row_index(p, d0, q, p.frame0 + b0 + bl - q);
      const float2* src = sm + (bl + Q - 1 - q) * RS + (pp / R0) * GS + pp % R0;
      const float* gq = p.g + d0 + q * D;
      float gv[V];
      if constexpr (V == 2) {
        const float2 t = *reinterpret_cast<const float2*>(gq);
        gv[0] = t.x; gv[1] = t.y;
      } else {
        const float4 t = *reinterpret_cast<const float4*>(gq);
        gv[0] = t.x; gv[1] = t.y; gv[2] = t.z; gv[3] = t.w;
      }
#pragma unroll
      for (int e = 0; e < V; e += 2) {
        const float4 v = *reinterpret_cast<const float4*>(src + e);
        acc[e] = fma2((v2f){v.x, v.y}, splat(gv[e]), acc[e]);
        acc[e + 1] = fma2((v2f){v.z, v.w}, splat(gv[e + 1]), acc[e + 1]);
      }
    }
#pragma unroll
    for (int e = 0; e < V; ++e) acc[e] = acc[e] * splat(p.scale);
    const long long s = (b0 + bl) * D + d0;
    if constexpr (FMT == PFB_FMT_CF32) {
      float2* o = static_cast<float2*>(p.out) + s;
      if (p.vec_out) {
        *reinterpret_cast<float4*>(o) = make_float4(acc[0].x, acc[0].y, acc[1].x, acc[1].y);
      } else {
        o[0] = make_float2(acc[0].x, acc[0].y);
        o[1] = make_float2(acc[1].x, acc[1].y);
      }
    } else {
      uint32_t* o = static_cast<uint32_t*>(p.out) + s;
      const uint4 v = make_uint4(chsyn_pack(acc[0], p.full), chsyn_pack(acc[1], p.full), chsyn_pack(acc[2], p.full),
                                 chsyn_pack(acc[3], p.full));
      if (p.vec_out) {
        *reinterpret_cast<uint4*>(o) = v;
      } else {
        o[0] = v.x; o[1] = v.y; o[2] = v.z; o[3] = v.w;
      }
    }
  }

  // CARRY: the workgroup that holds the call's last frame has every row the next call starts from
  if (b0 + nb == p.frames && Q > 1) {
    const int r0 = nb;  // row of local frame frames - (Q - 1)
    for (int i = tid; i < (Q - 1) * (M / 2); i += kThreads) {
      const int j = i / (M / 2), pp = 2 * (i - j * (M / 2));
      const float4 v = *reinterpret_cast<const float4*>(&sm[(r0 + j) * RS + (pp / R0) * GS + pp % R0]);
      *reinterpret_cast<float4*>(p.carry_out + (long long)j * M + pp) = v;
    }
  }
}

using ChsynLaunchFn = void (*)(const ChsynParams&, unsigned, size_t, hipStream_t);
template <int M, int R0, int R1, int FMT>
void launch_fused(const ChsynParams& p, unsigned grid, size_t lds, hipStream_t s) {
  hipLaunchKernelGGL((pfb_chsyn_fused<M, R0, R1, FMT>), dim3(grid), dim3(kThreads), lds, s, p);
}

struct ChsynEntry {
  int M, fmt, row_stride;
  ChsynLaunchFn launch;
  const char* name;
};
#define PFB_CHSYN_ROWS(M, R0, R1)                                                                                  \
  {M, PFB_FMT_CF32, R1 * (R0 + kPad), launch_fused<M, R0, R1, PFB_FMT_CF32>, "pfb_chsyn_fused<M" #M ",cf32>"},   \
  {M, PFB_FMT_INT16_IQ, R1 * (R0 + kPad), launch_fused<M, R0, R1, PFB_FMT_INT16_IQ>, "pfb_chsyn_fused<M" #M ",int16>"}
const ChsynEntry kChsynKernels[] = {PFB_CHSYN_ROWS(56, 8, 7), PFB_CHSYN_ROWS(64, 8, 8), PFB_CHSYN_ROWS(128, 16, 8),
                                    PFB_CHSYN_ROWS(256, 16, 16)};
#undef PFB_CHSYN_ROWS

const ChsynEntry* find_chsyn(int M, int fmt) {
  for (const ChsynEntry& e : kChsynKernels)
    if (e.M == M && e.fmt == fmt) return &e;
  return nullptr;
}

// ---------------------------------------------------------------------------------
// host: checks and plan

// frames per workgroup of pfb_chsyn_rows: two tiles of tile*M values in at most 32 KiB of LDS (64 KiB at M = 4096)
int generic_tile(int M) { return std::max(1, std::min(16, 2048 / M)); }

// Everything pfb_chsyn_describe and pfb_chsyn_create check before the device, in the order the header states
int chsyn_check(const pfb_chsyn_config* cfg, pfb_chsyn_plan* plan) {
  if (!cfg || !plan || cfg->struct_size != sizeof(pfb_chsyn_config) || !cfg->taps) return PFB_ERR_BAD_ARG;
  const uint32_t M = cfg->num_channels, P = cfg->taps_per_channel;
  if (M < 2 || P == 0) return PFB_ERR_BAD_ARG;
  uint32_t D = cfg->decimation ? cfg->decimation : M;
  if (!(D == M || (M % 2 == 0 && D == M / 2))) return PFB_ERR_BAD_ARG;
  if (!std::isfinite(cfg->scale) || !std::isfinite((float)cfg->scale)) return PFB_ERR_BAD_ARG;
  if ((cfg->flags & ~(uint32_t)(PFB_CHSYN_FFTSHIFT | PFB_CHSYN_DEROTATE)) || cfg->route > PFB_CHSYN_ROUTE_GENERIC ||
      cfg->layout > PFB_LAYOUT_CHANNEL_MAJOR)
    return PFB_ERR_BAD_ARG;
  const bool in_domain = M <= kMaxM && P <= kMaxP;  // the taps of a shape outside it are not looked at
  if (in_domain)
    for (uint32_t i = 0; i < M * P; ++i)
      if (!std::isfinite(cfg->taps[i])) return PFB_ERR_BAD_ARG;
  if (cfg->output_format != PFB_FMT_CF32 && cfg->output_format != PFB_FMT_INT16_IQ) return PFB_ERR_BAD_FORMAT;
  if (cfg->output_format == PFB_FMT_INT16_IQ && (cfg->bit_width < 2 || cfg->bit_width > 16)) return PFB_ERR_BAD_FORMAT;
  if (!in_domain || cfg->layout == PFB_LAYOUT_CHANNEL_MAJOR) return PFB_ERR_UNSUPPORTED;
  const uint32_t Q = M * P / D;
  // fused: T = 4 (Q - 1) output blocks per workgroup re-read a quarter of what they load; at least 16, and no more
  // than the 64 KiB of LDS hold beside the Q - 1 rows in front of them
  const ChsynEntry* e = find_chsyn((int)M, (int)cfg->output_format);
  uint32_t T = 0;
  if (e) {
    const uint32_t cap = (uint32_t)(kLdsComplex / e->row_stride);
    if (cap >= Q) T = std::min(cap - (Q - 1), std::max(4 * (Q - 1), 16u));
  }
  if (cfg->route == PFB_CHSYN_ROUTE_FUSED && T == 0) return PFB_ERR_UNSUPPORTED;
  const bool fused = cfg->route != PFB_CHSYN_ROUTE_GENERIC && T > 0;
  plan->route = fused ? PFB_CHSYN_ROUTE_FUSED : PFB_CHSYN_ROUTE_GENERIC;
  plan->decimation = D;
  plan->q = Q;
  plan->tile_frames = fused ? T : (uint32_t)generic_tile((int)M);
  plan->carried_bytes = (uint64_t)(Q - 1) * M * sizeof(float2);
  plan->workspace_bytes = fused ? 0 : (kWorkspaceCap / ((uint64_t)M * sizeof(float2))) * (uint64_t)M * sizeof(float2);
  return PFB_OK;
}

}  // namespace

struct pfb_chsyn_handle {
  int M = 0, D = 0, Q = 0, T = 0;
  bool fused = false;
  int fmt = 0, bit_width = 0;
  unsigned flags = 0;
  float scale = 1.f;
  int device = 0;
  int out_elem = 8;     // bytes per output sample
  uint64_t frame = 0;   // absolute index of the next frame
  float* d_g = nullptr;
  float* d_w = nullptr;
  float2* d_tw = nullptr;
  float2* d_carry[2] = {nullptr, nullptr};  // Q - 1 rows each; d_carry[cur] precedes the next frame
  int cur = 0;
  float2* d_work = nullptr;  // generic: rows of the chunk in flight (grow-only)
  uint64_t work_frames = 0;
  pfb::GenericPlan gplan{};
  hipStream_t stream = nullptr;
  hipEvent_t ev_switch = nullptr;
  const ChsynEntry* kern = nullptr;
  const char* last_kernel = "";
  pfb::HostStage stage;
};

namespace {

void free_chsyn(pfb_chsyn_handle* h) {
  if (!h) return;
  DeviceGuard g(h->device);
  (void)hipFree(h->d_g);
  (void)hipFree(h->d_w);
  (void)hipFree(h->d_tw);
  (void)hipFree(h->d_carry[0]);
  (void)hipFree(h->d_carry[1]);
  (void)hipFree(h->d_work);
  h->stage.release();
  if (h->ev_switch) (void)hipEventDestroy(h->ev_switch);
  delete h;
}

size_t carry_bytes(const pfb_chsyn_handle* h) { return (size_t)std::max(h->Q - 1, 1) * h->M * sizeof(float2); }

int create_chsyn(const pfb_chsyn_config* cfg, pfb_chsyn_handle** out) {
  pfb_chsyn_plan plan{};
  int rc = chsyn_check(cfg, &plan);
  if (rc != PFB_OK) return rc;
  int dev = 0;
  rc = pfb::resolve_device(cfg->device_id, &dev);
  if (rc != PFB_OK) return rc;
  pfb_chsyn_handle* h = new pfb_chsyn_handle();
  h->M = (int)cfg->num_channels;
  h->D = (int)plan.decimation;
  h->Q = (int)plan.q;
  h->fused = plan.route == PFB_CHSYN_ROUTE_FUSED;
  h->T = (int)plan.tile_frames;
  h->fmt = (int)cfg->output_format;
  h->bit_width = h->fmt == PFB_FMT_CF32 ? 1 : (int)cfg->bit_width;
  h->flags = cfg->flags;
  h->scale = (float)(cfg->scale != 0.0 ? cfg->scale : (double)h->D);
  h->device = dev;
  h->out_elem = h->fmt == PFB_FMT_CF32 ? 8 : 4;
  h->kern = h->fused ? find_chsyn(h->M, h->fmt) : nullptr;
  h->gplan = pfb::make_generic_plan(h->M);
  DeviceGuard g(dev);
  const size_t g_bytes = (size_t)h->M * cfg->taps_per_channel * sizeof(float), w_bytes = (size_t)h->M * sizeof(float);
  const std::vector<float> ones((size_t)h->M, 1.f);
  hipError_t e = hipMalloc((void**)&h->d_g, g_bytes);
  if (e == hipSuccess) e = hipMalloc((void**)&h->d_w, w_bytes);
  if (e == hipSuccess) e = pfb::upload_twiddles((uint32_t)h->M, &h->d_tw);
  if (e == hipSuccess) e = hipMalloc((void**)&h->d_carry[0], carry_bytes(h));
  if (e == hipSuccess) e = hipMalloc((void**)&h->d_carry[1], carry_bytes(h));
  if (e == hipSuccess) e = hipMemcpy(h->d_g, cfg->taps, g_bytes, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(h->d_w, ones.data(), w_bytes, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemset(h->d_carry[0], 0, carry_bytes(h));
  if (e == hipSuccess) e = hipMemset(h->d_carry[1], 0, carry_bytes(h));
  if (e != hipSuccess) {
    rc = pfb::hip_fail(e, "pfb_chsyn_create allocation");
    free_chsyn(h);
    return rc;
  }
  *out = h;
  return PFB_OK;
}

// the kernels of one call for device-resident buffers; no host sync (a generic call that grows the workspace waits
// for the device)
int chsyn_enqueue(pfb_chsyn_handle* h, const void* d_y, uint64_t n, uint64_t ld, void* d_out) {
  if (n == 0) return PFB_OK;
  ChsynParams p{};
  p.w = h->d_w;
  p.g = h->d_g;
  p.tw = h->d_tw;
  p.ld = (long long)ld;
  p.scale = h->scale;
  p.full = (float)(1 << (h->bit_width - 1));
  p.M = h->M;
  p.D = h->D;
  p.Q = h->Q;
  p.T = h->T;
  p.flags = h->flags;
  p.plan = h->gplan;
  p.tile_frames = generic_tile(h->M);
  if (h->fused) {
    const uint64_t grid = (n + (uint64_t)h->T - 1) / (uint64_t)h->T;
    if (grid > 0x7fffffffull) return PFB_ERR_UNSUPPORTED;
    p.y = static_cast<const float2*>(d_y);
    p.out = d_out;
    p.frames = (long long)n;
    p.frame0 = (long long)h->frame;
    p.carry_in = h->d_carry[h->cur];
    p.carry_out = h->d_carry[h->cur ^ 1];
    p.vec_in = reinterpret_cast<uintptr_t>(d_y) % 16 == 0 && ld % 2 == 0;
    p.vec_out = reinterpret_cast<uintptr_t>(d_out) % 16 == 0;
    h->kern->launch(p, (unsigned)grid, (size_t)(h->T + h->Q - 1) * h->kern->row_stride * sizeof(float2), h->stream);
    HIP_TRY(hipGetLastError());
    h->cur ^= 1;
    h->frame += n;
    h->last_kernel = h->kern->name;
    return PFB_OK;
  }
  const uint64_t per_chunk = std::max<uint64_t>(1, kWorkspaceCap / ((uint64_t)h->M * sizeof(float2)));
  const uint64_t need = std::min(n, per_chunk);
  if (need > h->work_frames) {  // frees only after the device has drained: earlier calls are done with the old one
    (void)hipFree(h->d_work);
    h->d_work = nullptr;
    h->work_frames = 0;
    HIP_TRY(hipMalloc((void**)&h->d_work, need * (uint64_t)h->M * sizeof(float2)));
    h->work_frames = need;
  }
  p.work = h->d_work;
  const size_t lds = (size_t)2 * p.tile_frames * h->M * sizeof(float2);
  for (uint64_t i0 = 0; i0 < n; i0 += per_chunk) {  // stream order keeps one chunk's rows from the next
    const uint64_t nf = std::min(per_chunk, n - i0);
    p.y = static_cast<const float2*>(d_y) + i0 * ld;
    p.out = static_cast<char*>(d_out) + i0 * (uint64_t)h->D * (uint64_t)h->out_elem;
    p.frames = (long long)nf;
    p.frame0 = (long long)h->frame;
    p.carry_in = h->d_carry[h->cur];
    p.carry_out = h->d_carry[h->cur ^ 1];
    const uint64_t tiles = (nf + (uint64_t)p.tile_frames - 1) / (uint64_t)p.tile_frames;
    const uint64_t blocks = (nf * (uint64_t)h->D + kThreads - 1) / kThreads;
    if (blocks > 0x7fffffffull) return PFB_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(pfb_chsyn_rows, dim3((unsigned)tiles), dim3(kThreads), lds, h->stream, p);
    HIP_TRY(hipGetLastError());
    if (h->fmt == PFB_FMT_CF32)
      hipLaunchKernelGGL(pfb_chsyn_fir<PFB_FMT_CF32>, dim3((unsigned)blocks), dim3(kThreads), 0, h->stream, p);
    else
      hipLaunchKernelGGL(pfb_chsyn_fir<PFB_FMT_INT16_IQ>, dim3((unsigned)blocks), dim3(kThreads), 0, h->stream, p);
    HIP_TRY(hipGetLastError());
    h->cur ^= 1;
    h->frame += nf;
  }
  h->last_kernel = h->fmt == PFB_FMT_CF32 ? "pfb_chsyn_generic<cf32>" : "pfb_chsyn_generic<int16>";
  return PFB_OK;
}

// what every process call checks before the device is touched; *s = the samples it writes
int chsyn_check_call(const pfb_chsyn_handle* h, const void* y, uint64_t n, uint64_t* ld, const void* out, uint64_t cap,
                     uint64_t* samples_out, bool device, uint64_t* s) {
  if (!h || !ld || (n > 0 && !y) || n > ((uint64_t)1 << 40) || h->frame + n < h->frame) return PFB_ERR_BAD_ARG;
  if (*ld == 0) *ld = (uint64_t)h->M;
  if (*ld < (uint64_t)h->M || *ld > ((uint64_t)1 << 31)) return PFB_ERR_BAD_ARG;
  *s = n * (uint64_t)h->D;
  if (samples_out) *samples_out = *s;
  if (*s > cap) return PFB_ERR_CAPACITY;
  if (*s > 0 && !out) return PFB_ERR_BAD_ARG;
  if (device && (reinterpret_cast<uintptr_t>(y) % 8 || reinterpret_cast<uintptr_t>(out) % (uintptr_t)h->out_elem))
    return PFB_ERR_BAD_ARG;
  return PFB_OK;
}

// Host buffers through the staged pipeline: a frame of ld values is a "sample", the D samples it completes a "frame"
int stage_frames(pfb_chsyn_handle* h, const void* y, uint64_t n, uint64_t ld, void* out) {
  const uint64_t chunk = std::max<uint64_t>(1, kStageBytes / (ld * sizeof(float2)));
  const pfb::StageSteps steps{
      chunk, chunk, (size_t)ld * sizeof(float2), (size_t)h->D * (size_t)h->out_elem,
      [](uint64_t m) { return m; },
      [h, ld](const void* d_in, uint64_t m, void* d_out, uint64_t, int64_t, int64_t) {
        return chsyn_enqueue(h, d_in, m, ld, d_out);
      }};
  return pfb::stage_host(h->stage, h->stream, steps, y, n, pfb::StageOut{out});
}

// Host frames.  With ld > M the last frame ends M values in: it is staged on its own, so that nothing behind the
// caller's last value is read (the cut changes no bit).
int chsyn_host(pfb_chsyn_handle* h, const void* y, uint64_t n, uint64_t ld, void* out) {
  if (n == 0) return PFB_OK;
  if (ld == (uint64_t)h->M) return stage_frames(h, y, n, ld, out);
  const int rc = stage_frames(h, y, n - 1, ld, out);
  if (rc != PFB_OK) return rc;
  const char* last = static_cast<const char*>(y) + (n - 1) * ld * sizeof(float2);
  return stage_frames(h, last, 1, (uint64_t)h->M, static_cast<char*>(out) + (n - 1) * (uint64_t)h->D * (uint64_t)h->out_elem);
}

}  // namespace

extern "C" int pfb_chsyn_describe(const pfb_chsyn_config* cfg, pfb_chsyn_plan* plan_out) {
  return pfb::abi_guard([&]() -> int {
    pfb_chsyn_plan plan{};
    const int rc = chsyn_check(cfg, plan_out ? &plan : nullptr);
    if (rc == PFB_OK) *plan_out = plan;
    return rc;
  });
}

extern "C" int pfb_chsyn_create(const pfb_chsyn_config* cfg, pfb_chsyn_handle** out) {
  return pfb::abi_guard([&]() -> int {
    if (!out) return PFB_ERR_BAD_ARG;
    *out = nullptr;
    return create_chsyn(cfg, out);
  });
}

extern "C" int pfb_chsyn_destroy(pfb_chsyn_handle* h) {
  return pfb::abi_guard([&]() -> int {
    if (!h) return PFB_ERR_BAD_ARG;
    free_chsyn(h);
    return PFB_OK;
  });
}

extern "C" int pfb_chsyn_reset(pfb_chsyn_handle* h) {
  return pfb::abi_guard([&]() -> int {
    if (!h) return PFB_ERR_BAD_ARG;
    DeviceGuard g(h->device);
    HIP_TRY(hipMemsetAsync(h->d_carry[h->cur], 0, carry_bytes(h), h->stream));  // frames before frame 0 are zero
    h->frame = 0;
    return PFB_OK;
  });
}

extern "C" int pfb_chsyn_set_stream(pfb_chsyn_handle* h, void* hip_stream) {
  return pfb::abi_guard([&]() -> int {
    if (!h) return PFB_ERR_BAD_ARG;
    return pfb::switch_stream(h->device, &h->stream, &h->ev_switch, static_cast<hipStream_t>(hip_stream));
  });
}

extern "C" int pfb_chsyn_sync(pfb_chsyn_handle* h) {
  return pfb::abi_guard([&]() -> int {
    if (!h) return PFB_ERR_BAD_ARG;
    DeviceGuard g(h->device);
    HIP_TRY(hipStreamSynchronize(h->stream));
    return PFB_OK;
  });
}

extern "C" int pfb_chsyn_get_device(const pfb_chsyn_handle* h, int* device_id) {
  return pfb::abi_guard([&]() -> int {
    if (!h || !device_id) return PFB_ERR_BAD_ARG;
    *device_id = h->device;
    return PFB_OK;
  });
}

extern "C" int pfb_chsyn_set_frame_index(pfb_chsyn_handle* h, uint64_t next_frame) {
  return pfb::abi_guard([&]() -> int {
    if (!h || next_frame > ((uint64_t)1 << 62)) return PFB_ERR_BAD_ARG;
    h->frame = next_frame;
    return PFB_OK;
  });
}

extern "C" int pfb_chsyn_get_frame_index(const pfb_chsyn_handle* h, uint64_t* next_frame) {
  return pfb::abi_guard([&]() -> int {
    if (!h || !next_frame) return PFB_ERR_BAD_ARG;
    *next_frame = h->frame;
    return PFB_OK;
  });
}

extern "C" int pfb_chsyn_samples_for(const pfb_chsyn_handle* h, uint64_t num_frames, uint64_t* samples_out) {
  return pfb::abi_guard([&]() -> int {
    if (!h || !samples_out || num_frames > ((uint64_t)1 << 40)) return PFB_ERR_BAD_ARG;
    *samples_out = num_frames * (uint64_t)h->D;
    return PFB_OK;
  });
}

extern "C" int pfb_chsyn_set_weights(pfb_chsyn_handle* h, const float* weights) {
  return pfb::abi_guard([&]() -> int {
    if (!h) return PFB_ERR_BAD_ARG;
    std::vector<float> w((size_t)h->M, 1.f);
    if (weights) {
      for (int c = 0; c < h->M; ++c)
        if (!std::isfinite(weights[c])) return PFB_ERR_BAD_ARG;
      w.assign(weights, weights + h->M);
    }
    DeviceGuard g(h->device);
    HIP_TRY(hipStreamSynchronize(h->stream));  // the frames already queued keep the weights they were queued with
    HIP_TRY(hipMemcpy(h->d_w, w.data(), w.size() * sizeof(float), hipMemcpyHostToDevice));
    return PFB_OK;
  });
}

extern "C" int pfb_chsyn_process_async(pfb_chsyn_handle* h, const void* d_y, uint64_t num_frames, uint64_t ld,
                                       void* d_out, uint64_t capacity_samples, uint64_t* samples_out) {
  return pfb::abi_guard([&]() -> int {
    uint64_t s = 0;
    const int rc = chsyn_check_call(h, d_y, num_frames, &ld, d_out, capacity_samples, samples_out, true, &s);
    if (rc != PFB_OK) return rc;
    DeviceGuard g(h->device);
    return chsyn_enqueue(h, d_y, num_frames, ld, d_out);
  });
}

extern "C" int pfb_chsyn_process(pfb_chsyn_handle* h, const void* y, uint64_t num_frames, uint64_t ld, void* out,
                                 uint64_t capacity_samples, uint64_t* samples_out, uint32_t mem) {
  return pfb::abi_guard([&]() -> int {
    if (mem > PFB_MEM_DEVICE) return PFB_ERR_BAD_ARG;
    uint64_t s = 0;
    int rc = chsyn_check_call(h, y, num_frames, &ld, out, capacity_samples, samples_out, mem == PFB_MEM_DEVICE, &s);
    if (rc != PFB_OK) return rc;
    DeviceGuard g(h->device);
    if (mem == PFB_MEM_HOST) return chsyn_host(h, y, num_frames, ld, out);
    rc = chsyn_enqueue(h, y, num_frames, ld, out);
    if (rc != PFB_OK) return rc;
    HIP_TRY(hipStreamSynchronize(h->stream));
    return PFB_OK;
  });
}

extern "C" const char* pfb_chsyn_last_kernel(const pfb_chsyn_handle* h) { return h ? h->last_kernel : ""; }
