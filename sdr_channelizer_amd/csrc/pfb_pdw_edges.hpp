// pfb_pdw_edges.hpp -- the edge stage's kernels: comparison masks, tile summaries, scan, edge lists.
//
// The leading/trailing-edge state machine (create_pdws_channelized.m:85-135, create_pdws.m:54-105) is a
// 2-state automaton driven by two comparisons per sample: inactive -> active on mag >= lead (:87 / :57),
// active stays active while mag > trail (:94 / :63; the channelized script has lead == trail).  One pass
// over the data records the two comparison bits per sample (64 samples per word); everything after that
// -- tile summaries, the scan, the edge lists -- works on the bit masks, 1/64 of the data.
#pragma once

#include "pfb_pdw_select.hpp"

namespace {
constexpr int kTileWords = kTile / 64;  // smallest tile, in 64-sample words

// Per-sample transition functions of one word: sample i maps state s to (s ? f1 : f0) bit i.  Returns the
// prefix compositions: bit i of p0 / p1 = state after sample i when the word is entered inactive / active
// (Kogge-Stone over function composition; bit 0 is the earliest sample).
__device__ __forceinline__ void word_scan(unsigned long long f0, unsigned long long f1, unsigned long long& p0,
                                          unsigned long long& p1) {
  p0 = f0;
  p1 = f1;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const unsigned long long e0 = p0 << d, e1 = (p1 << d) | ((1ull << d) - 1ull);  // earlier span; identity shifted in
    const unsigned long long n0 = (e0 & p1) | (~e0 & p0), n1 = (e1 & p1) | (~e1 & p0);
    p0 = n0;
    p1 = n1;
  }
}

// comparison masks of the F x M matrix, laid out [word][channel].  grid = (column groups, word groups of
// 4): one word (64 frames) per wave, lane = channel.  Frames past F are the identity (f0 = 0, f1 = 1).
// only_if != nullptr: run only when *only_if has bit 4 or 8 set (the bracket pass's provisional masks are unusable)
__global__ void __launch_bounds__(256) pdw_mask_kernel(const float2* y, long long F, int M, const double* thr,
                                                       unsigned long long* f0, unsigned long long* f1, long long words,
                                                       const unsigned* only_if) {
  if (only_if && (*only_if & 12u) == 0u) return;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int col = blockIdx.x * 64 + lane;
  if (col >= M) return;
  const double t = thr[col];
  for (long long w = (long long)blockIdx.y * 4 + wave; w < words; w += 4ll * gridDim.y) {  // grid-stride over the words
    const long long r0 = w * 64;
    unsigned long long a = 0ull, b = 0ull;
    if (r0 + 64 <= F) {
#pragma unroll 8
      for (int i = 0; i < 64; ++i) {
        const double m = mag_of(y[(r0 + i) * M + col]);
        a |= (unsigned long long)(m >= t) << i;
        b |= (unsigned long long)(m > t) << i;
      }
    } else {
      for (int i = 0; i < 64; ++i) {
        if (r0 + i < F) {
          const double m = mag_of(y[(r0 + i) * M + col]);
          a |= (unsigned long long)(m >= t) << i;
          b |= (unsigned long long)(m > t) << i;
        } else {
          b |= 1ull << i;
        }
      }
    }
    f0[w * M + col] = a;
    f1[w * M + col] = b;
  }
}

// tile summaries for BOTH incoming states: fn[tile][col] = f(0) | f(1) << 1 and the edge counts of either
// trajectory, cnt[tile][col] = (starts from 0, ends from 0, starts from 1, ends from 1): with both in
// hand nothing has to be recounted once the scan has told which state each tile really starts in.
// One thread per (tile, channel), channel fastest.
__global__ void __launch_bounds__(256) pdw_tilefn_kernel(const unsigned long long* f0, const unsigned long long* f1, int M,
                                                         long long ntiles, int tile_words, unsigned char* fn, ushort4* cnt) {
  const long long g = (long long)blockIdx.x * 256 + threadIdx.x;
  if (g >= ntiles * M) return;
  const int col = (int)(g % M);
  const long long tile = g / M;
  int s0 = 0, s1 = 1;
  unsigned a0 = 0, e0 = 0, a1 = 0, e1 = 0;
  for (int j = 0; j < tile_words; ++j) {
    const long long w = tile * tile_words + j;
    unsigned long long p0, p1;
    word_scan(f0[w * M + col], f1[w * M + col], p0, p1);
    const unsigned long long S0 = s0 ? p1 : p0, S1 = s1 ? p1 : p0;
    const unsigned long long P0 = (S0 << 1) | (unsigned long long)s0, P1 = (S1 << 1) | (unsigned long long)s1;
    a0 += (unsigned)__popcll(S0 & ~P0); e0 += (unsigned)__popcll(~S0 & P0);
    a1 += (unsigned)__popcll(S1 & ~P1); e1 += (unsigned)__popcll(~S1 & P1);
    s0 = (int)(S0 >> 63); s1 = (int)(S1 >> 63);
  }
  fn[g] = (unsigned char)(s0 | (s1 << 1));
  cnt[g] = make_ushort4((unsigned short)a0, (unsigned short)e0, (unsigned short)a1, (unsigned short)e1);
}

// per column: incoming state of every tile, then the exclusive prefix of the edge counts of the
// trajectory each tile really follows, and the column totals.  One workgroup of BT threads per column
// (one wave when there are many columns, 16 waves for the one-column raw stream): each thread owns a
// contiguous segment of tiles; transition functions, then counts, are scanned across the workgroup
// (thread order = time order: shuffles inside a wave, wave totals through LDS) and each thread replays
// its segment.
__device__ __forceinline__ int compose_fn(int first, int then) {  // h(s) = then(first(s)), 2-bit encodings
  return ((then >> (first & 1)) & 1) | (((then >> ((first >> 1) & 1)) & 1) << 1);
}

template <int BT>
__global__ void __launch_bounds__(BT) pdw_tilescan_kernel(int M, long long ntiles, const unsigned char* fn,
                                                          const ushort4* cnt, unsigned char* state_in,
                                                          unsigned long long* off_s, unsigned long long* off_e,
                                                          unsigned long long* tot_s, unsigned long long* tot_e) {
  constexpr int NW = BT / 64;
  __shared__ int wave_fn[NW];
  __shared__ unsigned long long wave_a[NW], wave_b[NW];
  const int col = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long long per = (ntiles + BT - 1) / BT;
  const long long t0 = (long long)tid * per < ntiles ? (long long)tid * per : ntiles;
  const long long t1 = (t0 + per < ntiles) ? t0 + per : ntiles;
  int f = 0x2;  // identity: f(0)=0, f(1)=1  -> bits (f0 | f1<<1) = 0b10
  {
    long long t = t0;
    for (; t + 8 <= t1; t += 8) {  // eight loads in flight: the chain through f is cheap, the strided bytes are not
      int g[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) g[u] = fn[(t + u) * M + col];
#pragma unroll
      for (int u = 0; u < 8; ++u) f = compose_fn(f, g[u]);
    }
    for (; t < t1; ++t) f = compose_fn(f, fn[t * M + col]);
  }
  // inclusive scan of function composition across the wave, then across waves
  int inc = f;
  for (int d = 1; d < 64; d <<= 1) {
    const int prev = __shfl_up(inc, d);
    if (lane >= d) inc = compose_fn(prev, inc);
  }
  int exc = __shfl_up(inc, 1);
  if (lane == 0) exc = 0x2;
  if (NW > 1) {
    if (lane == 63) wave_fn[wave] = inc;
    __syncthreads();
    int before = 0x2;
    for (int w = 0; w < wave; ++w) before = compose_fn(before, wave_fn[w]);
    exc = compose_fn(before, exc);
  }
  const int s_in = exc & 1;  // state entering my segment when the stream starts inactive: exc(0)
  int s = s_in;
  unsigned long long a = 0, b = 0;
  {
    auto step = [&](long long t, ushort4 c, int g) {
      state_in[t * M + col] = (unsigned char)s;
      a += s ? c.z : c.x;
      b += s ? c.w : c.y;
      s = (g >> s) & 1;
    };
    long long t = t0;
    for (; t + 8 <= t1; t += 8) {
      ushort4 c[8];
      int g[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) { c[u] = cnt[(t + u) * M + col]; g[u] = fn[(t + u) * M + col]; }
#pragma unroll
      for (int u = 0; u < 8; ++u) step(t + u, c[u], g[u]);
    }
    for (; t < t1; ++t) step(t, cnt[t * M + col], fn[t * M + col]);
  }
  unsigned long long ia = a, ib = b;
  for (int d = 1; d < 64; d <<= 1) {
    const unsigned long long pa = __shfl_up(ia, d), pb = __shfl_up(ib, d);
    if (lane >= d) { ia += pa; ib += pb; }
  }
  if (NW > 1) {
    if (lane == 63) { wave_a[wave] = ia; wave_b[wave] = ib; }
    __syncthreads();
    unsigned long long ba = 0, bb = 0;
    for (int w = 0; w < wave; ++w) { ba += wave_a[w]; bb += wave_b[w]; }
    ia += ba; ib += bb;
  }
  unsigned long long ea = ia - a, eb = ib - b;  // exclusive
  s = s_in;
  {
    auto step = [&](long long t, ushort4 c, int g) {
      off_s[t * M + col] = ea; off_e[t * M + col] = eb;
      ea += s ? c.z : c.x;
      eb += s ? c.w : c.y;
      s = (g >> s) & 1;
    };
    long long t = t0;
    for (; t + 8 <= t1; t += 8) {
      ushort4 c[8];
      int g[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) { c[u] = cnt[(t + u) * M + col]; g[u] = fn[(t + u) * M + col]; }
#pragma unroll
      for (int u = 0; u < 8; ++u) step(t + u, c[u], g[u]);
    }
    for (; t < t1; ++t) step(t, cnt[t * M + col], fn[t * M + col]);
  }
  if (tid == BT - 1) { tot_s[col] = ia; tot_e[col] = ib; }
}

// replay a tile from its incoming state and write the leading / trailing edge sample indices
__global__ void __launch_bounds__(256) pdw_edges_kernel(const unsigned long long* f0, const unsigned long long* f1, int M,
                                                        long long ntiles, int tile_words, const unsigned char* state_in,
                                                        const unsigned long long* off_s, const unsigned long long* off_e,
                                                        long long* starts, long long* ends) {
  const long long g = (long long)blockIdx.x * 256 + threadIdx.x;
  if (g >= ntiles * M) return;
  const int col = (int)(g % M);
  const long long tile = g / M;
  int s = state_in[g];
  unsigned long long os = off_s[g], oe = off_e[g];
  for (int j = 0; j < tile_words; ++j) {
    const long long w = tile * tile_words + j;
    unsigned long long p0, p1;
    word_scan(f0[w * M + col], f1[w * M + col], p0, p1);
    const unsigned long long S = s ? p1 : p0, P = (S << 1) | (unsigned long long)s;
    unsigned long long up = S & ~P, down = ~S & P;
    while (up) { starts[os++] = w * 64 + (__ffsll((long long)up) - 1); up &= up - 1; }
    while (down) { ends[oe++] = w * 64 + (__ffsll((long long)down) - 1); down &= down - 1; }
    s = (int)(S >> 63);
  }
}

// One-column streams (the raw recorder stream) with long tiles: a thread per tile would be 16 384 threads walking 256
// words each.  A WAVE per tile instead: lane l summarises words [l wpl, (l + 1) wpl) exactly as pdw_tilefn_kernel
// summarises a tile (function + edge counts for both incoming states), the lanes' functions are scanned by composition
// (shuffles), which gives every lane the state it is entered in on either trajectory, and the counts add up.
__device__ __forceinline__ void lane_summary(const unsigned long long* f0, const unsigned long long* f1, long long w0, int wpl,
                                             int& fn, unsigned (&c)[4]) {
  int s0 = 0, s1 = 1;
  c[0] = c[1] = c[2] = c[3] = 0u;
  for (int j = 0; j < wpl; ++j) {
    unsigned long long p0, p1;
    word_scan(f0[w0 + j], f1[w0 + j], p0, p1);
    const unsigned long long S0 = s0 ? p1 : p0, S1 = s1 ? p1 : p0;
    const unsigned long long P0 = (S0 << 1) | (unsigned long long)s0, P1 = (S1 << 1) | (unsigned long long)s1;
    c[0] += (unsigned)__popcll(S0 & ~P0); c[1] += (unsigned)__popcll(~S0 & P0);
    c[2] += (unsigned)__popcll(S1 & ~P1); c[3] += (unsigned)__popcll(~S1 & P1);
    s0 = (int)(S0 >> 63); s1 = (int)(S1 >> 63);
  }
  fn = s0 | (s1 << 1);
}

// exclusive scan of the lanes' functions by composition: the function that maps the tile's incoming state to the state
// this lane is entered in; `total` = all 64 lanes composed
__device__ __forceinline__ int lane_prefix_fn(int fn, int lane, int& total) {
  int inc = fn;
  for (int d = 1; d < 64; d <<= 1) {
    const int prev = __shfl_up(inc, d);
    if (lane >= d) inc = compose_fn(prev, inc);
  }
  total = __shfl(inc, 63);
  const int exc = __shfl_up(inc, 1);
  return lane == 0 ? 0x2 : exc;  // identity for the first lane
}

__global__ void __launch_bounds__(256) pdw_tilefn_wave_kernel(const unsigned long long* f0, const unsigned long long* f1,
                                                              long long ntiles, int tile_words, unsigned char* fn,
                                                              ushort4* cnt) {
  const int lane = threadIdx.x & 63;
  const long long tile = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (tile >= ntiles) return;
  const int wpl = tile_words / 64;
  int g;
  unsigned c[4];
  lane_summary(f0, f1, tile * tile_words + (long long)lane * wpl, wpl, g, c);
  int total;
  const int pre = lane_prefix_fn(g, lane, total);
  const int in0 = pre & 1, in1 = (pre >> 1) & 1;  // the state this lane is entered in when the tile is entered in 0 / 1
  unsigned a0 = in0 ? c[2] : c[0], e0 = in0 ? c[3] : c[1], a1 = in1 ? c[2] : c[0], e1 = in1 ? c[3] : c[1];
  for (int d = 32; d > 0; d >>= 1) {
    a0 += __shfl_xor(a0, d); e0 += __shfl_xor(e0, d);
    a1 += __shfl_xor(a1, d); e1 += __shfl_xor(e1, d);
  }
  if (lane == 0) {
    fn[tile] = (unsigned char)total;
    cnt[tile] = make_ushort4((unsigned short)a0, (unsigned short)e0, (unsigned short)a1, (unsigned short)e1);
  }
}

__global__ void __launch_bounds__(256) pdw_edges_wave_kernel(const unsigned long long* f0, const unsigned long long* f1,
                                                             long long ntiles, int tile_words, const unsigned char* state_in,
                                                             const unsigned long long* off_s, const unsigned long long* off_e,
                                                             long long* starts, long long* ends) {
  const int lane = threadIdx.x & 63;
  const long long tile = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (tile >= ntiles) return;
  const int wpl = tile_words / 64;
  const long long w0 = tile * tile_words + (long long)lane * wpl;
  int g;
  unsigned c[4];
  lane_summary(f0, f1, w0, wpl, g, c);
  int total;
  const int pre = lane_prefix_fn(g, lane, total);
  int s = (pre >> (int)state_in[tile]) & 1;  // the state this lane is really entered in
  const unsigned ns = s ? c[2] : c[0], ne = s ? c[3] : c[1];
  unsigned is = ns, ie = ne;  // inclusive prefix sums over the lanes
  for (int d = 1; d < 64; d <<= 1) {
    const unsigned ps = __shfl_up(is, d), pe = __shfl_up(ie, d);
    if (lane >= d) { is += ps; ie += pe; }
  }
  unsigned long long os = off_s[tile] + (is - ns), oe = off_e[tile] + (ie - ne);
  for (int j = 0; j < wpl; ++j) {
    const long long w = w0 + j;
    unsigned long long p0, p1;
    word_scan(f0[w], f1[w], p0, p1);
    const unsigned long long S = s ? p1 : p0, P = (S << 1) | (unsigned long long)s;
    unsigned long long up = S & ~P, down = ~S & P;
    while (up) { starts[os++] = w * 64 + (__ffsll((long long)up) - 1); up &= up - 1; }
    while (down) { ends[oe++] = w * 64 + (__ffsll((long long)down) - 1); down &= down - 1; }
    s = (int)(S >> 63);
  }
}

// make the per-tile offsets absolute: add the column bases (columns outermost = the reference's order)
__global__ void pdw_rebase_kernel(int M, long long ntiles, unsigned long long* off_s, unsigned long long* off_e,
                                  const unsigned long long* base_s, const unsigned long long* base_e) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= ntiles * M) return;
  const int col = (int)(i % M);
  off_s[i] += base_s[col];
  off_e[i] += base_e[col];
}
}  // namespace
