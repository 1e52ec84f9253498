// pfb_fast_cfg.hpp -- what every fused kernel is configured and launched with: the plan (FastCfg), the workgroup
// remap over the XCDs, the row loads, the per-handle tables, the kernel tags and the one host-side launch.  See pfb_fast.hpp.
#pragma once

#include "pfb_cplx.hpp"

namespace pfb {

// ---------------------------------------------------------------------------------
// Kernel configuration

template <int M_, int P_, int D_, int CPT_, int FMT_, int C_, int NP_, int R0_, int R1_, int R2_, int RS0_,
          int RS1_, int RS2_, int FS_, bool PINGPONG_, int MIN_WAVES_, bool TW_TABLE_ = false, bool WAVE_FRAMES_ = false>
struct FastCfg {
  static constexpr bool WAVE_FRAMES = WAVE_FRAMES_;  // schedule W only: every wave transforms whole frames by itself
  static constexpr int M = M_, P = P_, D = D_, CPT = CPT_, FMT = FMT_, C = C_, NP = NP_;
  static constexpr int LANES = D / CPT;                  // threads that own columns
  static constexpr int NT = (LANES + 63) / 64 * 64;      // threads per workgroup (whole waves)
  static constexpr bool POW2 = (M & (M - 1)) == 0;
  static constexpr int W = M * P / D;  // window rows = taps per column
  static constexpr int OS = M / D;     // branches per column (1, or 2 when oversampled)
  static constexpr int FS = FS_;       // frame stride in LDS (complex elements)
  static constexpr bool PINGPONG = PINGPONG_;
  static constexpr bool TW_TABLE = TW_TABLE_;  // inter-pass twiddles re-read from the L1-resident table
                                               // every chunk instead of living in registers
  static constexpr int MIN_WAVES = MIN_WAVES_;
  static constexpr int R(int i) { return i == 0 ? R0_ : i == 1 ? R1_ : R2_; }
  static constexpr int RS(int i) { return i == 0 ? RS0_ : i == 1 ? RS1_ : RS2_; }
  static constexpr int S(int i) { int s = 1; for (int j = i + 1; j < NP; ++j) s *= R(j); return s; }
  static constexpr int K(int i) { int k = 1; for (int j = 0; j < i; ++j) k *= R(j); return k; }
  static constexpr int WP = (W + 3) / 4 * 4;  // taps per column padded to whole float4s
  static constexpr int TAPS_LANE_FLOATS = D * WP;  // per-column tap table built by init_tables
  // inter-pass twiddle table: per non-final pass S rows of R entries, rows padded to an even length so that every row
  // starts on a 16-byte boundary (odd radices -- 5, 7, 3 -- in front of the last pass)
  static constexpr int TWR(int i) { return R(i) + (R(i) & 1); }
  static constexpr int TW_OFF(int i) { int o = 0; for (int j = 0; j < i; ++j) o += S(j) * TWR(j); return o; }
  static constexpr int TW_LANE_ELEMS = TW_OFF(NP - 1) > 0 ? TW_OFF(NP - 1) : 1;  // inter-pass twiddle rows
  static constexpr int BUF = C * FS;   // one chunk buffer (complex elements)
  static constexpr int LDS_ELEMS = BUF * (PINGPONG ? 2 : 1);
  static_assert(D % CPT == 0, "columns split evenly over threads");
  static_assert(M % D == 0 && (M * P) % D == 0, "D divides M");
  static_assert(NP >= 2 && NP <= 3, "2 or 3 passes");
  static_assert(R0_ * R1_ * (NP_ == 3 ? R2_ : 1) == M_, "radices multiply to M");
  static_assert(R(0) * RS(0) <= FS && R(1) * RS(1) <= FS && (NP < 3 || R(2) * RS(2) <= FS), "frame fits");
  // in-place non-final passes need every read of the pass to precede every write: one iteration per
  // thread, and (multi-wave teams) a barrier between the reads and the writes
  static_assert(PINGPONG || WAVE_FRAMES || (C * (M / R(0)) <= NT && (NP < 3 || C * (M / R(1)) <= NT)),
                "multi-iteration non-final passes need ping-pong buffers");
};

// ---------------------------------------------------------------------------------

// Workgroups are dealt round-robin over the 8 XCDs (blockIdx % 8 labels the XCD), each with its own L2.  mode 1:
// consecutive runs go to ONE XCD (XCD x walks the x-th eighth of the stream): a run's halo rows are its predecessor's
// last rows, read from that L2 -- eight sweeps through the stream.  mode G > 1: each XCD takes G consecutive runs at a
// time, the eight XCDs 8 G consecutive runs: one window sweeping the stream, G - 1 of G halos still inside an XCD (the
// blocks past the last whole group of 8 G stay where they are).  Bijective for any grid size.
PFB_DEV long long xcd_remap_block(long long blk, long long nb, int mode) {
  if (mode == 1) {
    const long long q = nb >> 3, r = nb & 7, xc = blk & 7;
    return (xc < r ? xc * (q + 1) : r * (q + 1) + (xc - r) * q) + (blk >> 3);
  }
  if (mode > 1) {
    const long long G = mode, span = 8 * G, base = (blk / span) * span;
    if (base + span <= nb) {
      const long long in = blk - base;
      return base + (in & 7) * G + (in >> 3);
    }
  }
  return blk;
}

// History carried by the channelizer launch itself: called at the top of every channelizer kernel.  When the host asks
// for it (hist_out), the first workgroup in launch order copies the last hist_samples raw samples of `in` there, which
// is what pfb_update_history_kernel computes for a call at least one history long -- one launch per call instead of two
// dependent ones.  hist_out is the handle's OTHER history buffer, which no workgroup of this launch reads.  Every other
// workgroup pays one scalar compare; there is no barrier in here.  16-byte moves where source and destination allow,
// samples otherwise, four loads in flight per thread (bps = bytes per sample: 2, 4 or 8; nt = threads of the workgroup).
template <class T>
PFB_DEV void carry_copy(T* dst, const T* src, int count, int tid, int nt) {
  int i = tid;
  for (; i + 3 * nt < count; i += 4 * nt) {
    const T a = src[i], b = src[i + nt], c = src[i + 2 * nt], d = src[i + 3 * nt];
    dst[i] = a;
    dst[i + nt] = b;
    dst[i + 2 * nt] = c;
    dst[i + 3 * nt] = d;
  }
  for (; i < count; i += nt) dst[i] = src[i];
}

PFB_DEV void carry_history(const KernelParams& p, int bps, int nt) {
  if (p.hist_out == nullptr || blockIdx.x != 0) return;
  const char* src = static_cast<const char*>(p.in) + (p.n_in - p.hist_samples) * (long long)bps;
  char* dst = static_cast<char*>(p.hist_out);
  const int bytes = p.hist_samples * bps;
  const int tid = threadIdx.x;
  int done = 0;
  if (((reinterpret_cast<uintptr_t>(src) | reinterpret_cast<uintptr_t>(dst)) & 15) == 0) {
    carry_copy(reinterpret_cast<uint4*>(dst), reinterpret_cast<const uint4*>(src), bytes / 16, tid, nt);
    done = bytes / 16 * 16;
  }
  const int rest = (bytes - done) / bps;  // samples: all of them, or the few behind the last whole 16 bytes
  if (bps == 2) carry_copy(reinterpret_cast<uint16_t*>(dst + done), reinterpret_cast<const uint16_t*>(src + done), rest, tid, nt);
  else if (bps == 4) carry_copy(reinterpret_cast<uint32_t*>(dst + done), reinterpret_cast<const uint32_t*>(src + done), rest, tid, nt);
  else carry_copy(reinterpret_cast<uint2*>(dst + done), reinterpret_cast<const uint2*>(src + done), rest, tid, nt);
}

// Sample conversion and the row loads of every schedule (FastKernel's base: the schedules reach both through one alias).
template <class K>
struct FastRows {
  using ST = SampleT<K::FMT>;
  using raw_t = typename ST::raw_t;
  static constexpr int D = K::D, CPT = K::CPT, C = K::C, NT = K::NT;

  struct alignas(sizeof(raw_t) * CPT) RawVec { raw_t v[CPT]; };

  PFB_DEV v2f cvt(raw_t r) {
    float re, im;
    ST::cvt(r, re, im);
    return (v2f){re, im};
  }

  // Row r of the stream -> CPT raw samples for this thread.  r is uniform across the workgroup.
  // INTERIOR runs (every row inside `in`, aligned) take the unchecked vector load; runs that touch
  // the history, the end of the stream or a misaligned buffer take the checked per-sample path.
  template <bool INTERIOR>
  PFB_DEV void load_row(const KernelParams& p, const raw_t* run_ptr, long long r, long long r_rel, int c0,
                        raw_t (&raw)[CPT]) {
    if (K::LANES < NT && c0 >= D) {  // lanes beyond the last column (D not a multiple of 64)
#pragma unroll
      for (int cc = 0; cc < CPT; ++cc) raw[cc] = raw_t{};
      return;
    }
    if constexpr (INTERIOR) {
      const RawVec* vp = reinterpret_cast<const RawVec*>(run_ptr + r_rel * D + c0);
      RawVec v;
      if constexpr (sizeof(RawVec) == 4) {
        if (p.experiment & 1) {  // streaming (nontemporal) row loads
          const uint32_t u = __builtin_nontemporal_load(reinterpret_cast<const uint32_t*>(vp));
          __builtin_memcpy(&v, &u, 4);
        } else {
          v = *vp;
        }
      } else {
        v = *vp;
      }
#pragma unroll
      for (int cc = 0; cc < CPT; ++cc) raw[cc] = v.v[cc];
    } else {
      if (r >= p.frames) {  // padding frames of a partial last chunk
#pragma unroll
        for (int cc = 0; cc < CPT; ++cc) raw[cc] = raw_t{};
        return;
      }
      const long long s0 = r * D + p.base;
      const raw_t* in = static_cast<const raw_t*>(p.in);
      const raw_t* hist = static_cast<const raw_t*>(p.hist);
#pragma unroll
      for (int cc = 0; cc < CPT; ++cc) {
        const long long s = s0 + c0 + cc;
        raw[cc] = (s >= 0) ? in[s] : hist[p.hist_samples + s];
      }
    }
  }

  // The C rows of a chunk.  2-byte samples, one column per lane, rows that are not whole cache lines (M = 56 int8:
  // 112-byte rows, 21 % of roofline with one 2-byte load per row): pairs of rows are fetched as ONE dword load --
  // lanes [0, D/2) take row r (two columns each), lanes [D/2, D) row r + 1 -- and, when the chunk is consumed, two
  // ds_bpermutes hand every lane its own column of both rows.  load_rows only issues the loads (they stay in flight
  // under the previous chunk's arithmetic like the ordinary row loads); finish_rows does the exchange.  (With
  // 128-byte rows, M = 64 int8, pairing measured +2 % complex, -10 % with fused abs(): off.)  Needs the run's rows on a 4-byte boundary.
  static constexpr bool kPairedRows = sizeof(raw_t) == 2 && CPT == 1 && C % 2 == 0 && D % 2 == 0 && D < 64 && NT == 64;
  struct RowFetch {
    uint32_t pw[C / 2 > 0 ? C / 2 : 1];
    bool paired;
  };

  template <bool INTERIOR>
  PFB_DEV void begin_rows(const raw_t* run_ptr, RowFetch& rf) {
    rf.paired = kPairedRows && INTERIOR && (reinterpret_cast<uintptr_t>(run_ptr) & 3) == 0;
  }

  template <bool INTERIOR>
  PFB_DEV void load_rows(const KernelParams& p, const raw_t* run_ptr, long long f_first, long long rel_first, int c0,
                         raw_t (&raw)[C][CPT], RowFetch& rf) {
    if constexpr (kPairedRows && INTERIOR) {
      if (rf.paired) {
        const int lane = threadIdx.x & 63;
#pragma unroll
        for (int t = 0; t < C; t += 2) {
          const uint32_t* rp = reinterpret_cast<const uint32_t*>(run_ptr + (rel_first + t) * D);
          rf.pw[t / 2] = lane < D ? rp[lane] : 0u;
        }
        return;
      }
    }
#pragma unroll
    for (int t = 0; t < C; ++t) load_row<INTERIOR>(p, run_ptr, f_first + t, rel_first + t, c0, raw[t]);
  }

  PFB_DEV void finish_rows(int c0, raw_t (&raw)[C][CPT], const RowFetch& rf) {
    if constexpr (kPairedRows) {
      if (rf.paired) {
        const int src = (c0 < D ? c0 : 0) >> 1, sh = (c0 & 1) * 16;
#pragma unroll
        for (int t = 0; t < C; t += 2) {
          const uint32_t a = (uint32_t)__builtin_amdgcn_ds_bpermute(src * 4, (int)rf.pw[t / 2]);
          const uint32_t b = (uint32_t)__builtin_amdgcn_ds_bpermute((D / 2 + src) * 4, (int)rf.pw[t / 2]);
          raw[t][0] = c0 < D ? (raw_t)((a >> sh) & 0xffffu) : raw_t{};
          raw[t + 1][0] = c0 < D ? (raw_t)((b >> sh) & 0xffffu) : raw_t{};
        }
      }
    }
  }
};

// Builds the per-column tap table and the inter-pass twiddle rows (once per handle).
template <class K>
__global__ void __launch_bounds__(256) pfb_init_tables_kernel(const float* taps, const float2* tw, float* taps_lane,
                                                             float2* tw_lane) {
  for (int idx = threadIdx.x; idx < K::TAPS_LANE_FLOATS; idx += 256) {
    const int c = idx / K::WP, j = idx % K::WP;
    taps_lane[idx] = (j < K::W) ? taps[(K::D - 1 - c) + K::D * j] : 0.f;
  }
#pragma unroll
  for (int i = 0; i < K::NP - 1; ++i) {
    const int R = K::R(i), S = K::S(i), KK = K::K(i);
    const int RP = K::TWR(i);
    for (int idx = threadIdx.x; idx < S * RP; idx += 256) {
      const int rest = idx / RP, kk = idx % RP;
      tw_lane[K::TW_OFF(i) + idx] = kk < R ? tw[rest * kk * KK] : make_float2(0.f, 0.f);
    }
  }
}

template <class K>
hipError_t init_tables(const float* taps, const float2* tw, float* taps_lane, float2* tw_lane, hipStream_t s) {
  hipLaunchKernelGGL(pfb_init_tables_kernel<K>, dim3(1), dim3(256), 0, s, taps, tw, taps_lane, tw_lane);
  return hipGetLastError();
}

// Host side of every launch of the family, and the only one: the entry a plan's select resolved the call to.
inline hipError_t launch_blocks(const KernelEntry& e, const KernelParams& p, hipStream_t s) {
  if (p.frames <= 0) return hipSuccess;
  if (e.kernel == nullptr) return hipErrorInvalidValue;  // the plan has no kernel for this call
  hipLaunchKernelGGL(e.kernel, dim3((unsigned)e.blocks), dim3((unsigned)e.threads), e.dyn_lds, s, p);
  return hipGetLastError();
}

inline bool wants_magnitude(const KernelParams& p) { return (p.flags & PFB_FLAG_MAGNITUDE) != 0; }

// A kernel's tag (grammar: pfb_channelizer_dev.h): its family, its integer template arguments as the source writes them
// and its compile-time roles.  Every schedule header builds the tag in the function that takes the kernel's address, from
// that function's own template arguments, so that one kernel has one tag.
struct KernelTag {
  char s[40] = {};
  int n = 0;
  constexpr void put(const char* t) { while (*t) s[n++] = *t++; }
  constexpr void num(int v) { if (v >= 10) num(v / 10); s[n++] = (char)('0' + v % 10); }
};
struct TagRoles { bool cm = false, ms = false; int magsel = -1, ntsel = -1; };

template <int... ARGS>
constexpr KernelTag kernel_tag(const char* family, TagRoles r = {}) {
  KernelTag t;
  t.put(family);
  if constexpr (sizeof...(ARGS) > 0) {
    bool first = true;
    ((t.put(first ? "<" : ","), t.num(ARGS), first = false), ...);
    t.put(">");
  }
  if (r.cm) t.put("+cm");
  if (r.ms) t.put("+ms");
  if (r.magsel >= 0) t.put(r.magsel ? "+mag" : "+c64");
  if (r.ntsel > 0) t.put("+nt");
  return t;
}

// the entry of `kernel` (schedule number `schedule`) for this call: workgroups of `threads` threads, `per` frames each
inline KernelEntry entry_for(KernelFn kernel, int schedule, const char* tag, const KernelParams& p, long long per,
                             int threads, unsigned dyn_lds = 0) {
  return KernelEntry{kernel, (p.frames + per - 1) / per, threads, dyn_lds, schedule, tag};
}

// The call's output type and store kind as compile-time roles <MAGSEL, NTSEL> of a kernel: complex temporal, complex
// nontemporal, or magnitudes (whose stores are always temporal).
template <class F>
KernelEntry with_store_roles(const KernelParams& p, F&& entry) {
  if (wants_magnitude(p)) return entry.template operator()<1, 0>();
  return p.nontemporal ? entry.template operator()<0, 1>() : entry.template operator()<0, 0>();
}

}  // namespace pfb
