// pfb_host.cpp -- the host plumbing declared in pfb_host.h.
#include "pfb_host.h"

#include <fcntl.h>
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <thread>
#include <vector>

namespace pfb {

thread_local std::string g_detail;

int hip_fail(hipError_t e, const char* what) {
  char buf[256];
  std::snprintf(buf, sizeof(buf), "%s: %s (%d)", what, hipGetErrorString(e), (int)e);
  g_detail = buf;
  (void)hipGetLastError();  // clear the sticky error
  return (e == hipErrorNoDevice || e == hipErrorInvalidDevice || e == hipErrorInsufficientDriver)
             ? PFB_ERR_NO_DEVICE
             : (e == hipErrorOutOfMemory ? PFB_ERR_NO_MEMORY : PFB_ERR_HIP);
}

int resolve_device(int requested, int* dev) {
  int ndev = 0;
  const hipError_t ce = hipGetDeviceCount(&ndev);
  if (ce != hipSuccess || ndev <= 0) {
    g_detail = std::string("hipGetDeviceCount: ") + (ce == hipSuccess ? "0 devices" : hipGetErrorString(ce));
    (void)hipGetLastError();
    return PFB_ERR_NO_DEVICE;
  }
  *dev = requested;
  if (*dev < 0) HIP_TRY(hipGetDevice(dev));
  if (*dev >= ndev) return PFB_ERR_BAD_ARG;
  return PFB_OK;
}

int switch_stream(int device, hipStream_t* stream, hipEvent_t* ev_switch, hipStream_t next) {
  if (next == *stream) return PFB_OK;
  DeviceGuard g(device);
  if (!*ev_switch) HIP_TRY(hipEventCreateWithFlags(ev_switch, hipEventDisableTiming));
  HIP_TRY(hipEventRecord(*ev_switch, *stream));
  HIP_TRY(hipStreamWaitEvent(next, *ev_switch, 0));
  *stream = next;
  return PFB_OK;
}

int grow(void** p, size_t* have, size_t want) {
  if (want <= *have) return PFB_OK;
  (void)hipFree(*p);
  *p = nullptr;
  *have = 0;
  HIP_TRY(hipMalloc(p, want));
  *have = want;
  return PFB_OK;
}

unsigned grid_for(uint64_t items, unsigned per_block, unsigned cap) {
  return (unsigned)std::min<uint64_t>(std::max<uint64_t>((items + per_block - 1) / per_block, 1), cap);
}

hipError_t upload_twiddles(uint32_t n, float2** d_tw) {
  std::vector<float2> tw(n);
  const double two_pi = 6.283185307179586476925286766559;
  for (uint32_t m = 0; m < n; ++m) {
    tw[m].x = (float)std::cos(two_pi * (double)m / (double)n);
    tw[m].y = (float)std::sin(two_pi * (double)m / (double)n);
  }
  const hipError_t e = hipMalloc((void**)d_tw, n * sizeof(float2));
  return e == hipSuccess ? hipMemcpy(*d_tw, tw.data(), n * sizeof(float2), hipMemcpyHostToDevice) : e;
}

// -- staged host pipeline ----------------------------------------------------------

int HostStage::ensure(size_t in, size_t out) {
  if (in > in_bytes || (in > 0 && !d_in[1])) {
    const size_t nb = std::max(in, in_bytes);
    for (void*& p : d_in) { (void)hipFree(p); p = nullptr; }
    in_bytes = 0;
    HIP_TRY(hipMalloc(&d_in[0], nb));
    HIP_TRY(hipMalloc(&d_in[1], nb));
    in_bytes = nb;
  }
  if (out > out_bytes || (out > 0 && !d_out[1])) {
    const size_t nb = std::max(out, out_bytes);
    for (void*& p : d_out) { (void)hipFree(p); p = nullptr; }
    out_bytes = 0;
    HIP_TRY(hipMalloc(&d_out[0], nb));
    HIP_TRY(hipMalloc(&d_out[1], nb));
    out_bytes = nb;
  }
  return PFB_OK;
}

void HostStage::release() {
  for (int i = 0; i < 2; ++i) {
    (void)hipFree(d_in[i]);
    (void)hipFree(d_out[i]);
    if (ev_in[i]) (void)hipEventDestroy(ev_in[i]);
    if (ev_k[i]) (void)hipEventDestroy(ev_k[i]);
    if (ev_out[i]) (void)hipEventDestroy(ev_out[i]);
  }
  if (s_in) (void)hipStreamDestroy(s_in);
  if (s_out) (void)hipStreamDestroy(s_out);
  *this = HostStage{};
}

namespace {

int stage_host_steps(HostStage& st, hipStream_t stream, const StageSteps& steps, const void* in, uint64_t n,
                     const StageOut& out) {
  const uint64_t frames_total = steps.frames_for(n);
  const int rc = st.ensure((size_t)std::min<uint64_t>(steps.chunk, n ? n : 1) * steps.in_bps,
                           out.device ? 0
                                      : (size_t)std::min<uint64_t>(steps.max_frames, frames_total ? frames_total : 1) *
                                            steps.frame_bytes);
  if (rc != PFB_OK) return rc;
  if (!st.s_in) {
    HIP_TRY(hipStreamCreateWithFlags(&st.s_in, hipStreamNonBlocking));
    HIP_TRY(hipStreamCreateWithFlags(&st.s_out, hipStreamNonBlocking));
    for (int i = 0; i < 2; ++i) {
      HIP_TRY(hipEventCreateWithFlags(&st.ev_in[i], hipEventDisableTiming));
      HIP_TRY(hipEventCreateWithFlags(&st.ev_k[i], hipEventDisableTiming));
      HIP_TRY(hipEventCreateWithFlags(&st.ev_out[i], hipEventDisableTiming));
    }
  }
  const size_t elem = out.ld ? steps.frame_bytes / (size_t)out.cols : 0;  // channel-major: bytes per value
  const char* src = static_cast<const char*>(in);
  char* dst = static_cast<char*>(out.ptr);
  uint64_t done = 0, frames_done = 0;
  // whatever the caller queued on the handle's stream comes first
  HIP_TRY(hipEventRecord(st.ev_k[1], stream));
  HIP_TRY(hipStreamWaitEvent(st.s_in, st.ev_k[1], 0));
  int rc2 = PFB_OK;
  for (uint64_t i = 0; done < n; ++i) {
    const int b = (int)(i & 1);
    const uint64_t m = std::min<uint64_t>(steps.chunk, n - done);
    const uint64_t f = steps.frames_for(m);
    const uint64_t row = out.row0 + frames_done;
    if (i >= 2) HIP_TRY(hipStreamWaitEvent(st.s_in, st.ev_k[b], 0));  // the kernel of chunk i-2 has read this input buffer
    HIP_TRY(hipMemcpyAsync(st.d_in[b], src + done * steps.in_bps, (size_t)m * steps.in_bps, hipMemcpyHostToDevice,
                           st.s_in));
    HIP_TRY(hipEventRecord(st.ev_in[b], st.s_in));
    HIP_TRY(hipStreamWaitEvent(stream, st.ev_in[b], 0));
    if (out.device) {
      if (!out.ld)
        rc2 = steps.enqueue(st.d_in[b], m, dst + row * steps.frame_bytes, f, (int64_t)f, 0);
      else
        rc2 = steps.enqueue(st.d_in[b], m, dst, f, (int64_t)out.ld, (int64_t)row);
      if (rc2 != PFB_OK) break;
      HIP_TRY(hipEventRecord(st.ev_k[b], stream));
      done += m;
      frames_done += f;
      continue;
    }
    if (i >= 2) HIP_TRY(hipStreamWaitEvent(stream, st.ev_out[b], 0));  // chunk i-2 has left this output buffer
    rc2 = steps.enqueue(st.d_in[b], m, st.d_out[b], f, (int64_t)f, 0);
    if (rc2 != PFB_OK) break;
    HIP_TRY(hipEventRecord(st.ev_k[b], stream));
    HIP_TRY(hipStreamWaitEvent(st.s_out, st.ev_k[b], 0));
    if (f > 0) {
      if (!out.ld) {
        HIP_TRY(hipMemcpyAsync(dst + row * steps.frame_bytes, st.d_out[b], (size_t)f * steps.frame_bytes,
                               hipMemcpyDeviceToHost, st.s_out));
      } else {  // column k of this chunk -> rows [row, row + f) of column k of the matrix
        HIP_TRY(hipMemcpy2DAsync(dst + row * elem, (size_t)out.ld * elem, st.d_out[b], (size_t)f * elem,
                                 (size_t)f * elem, (size_t)out.cols, hipMemcpyDeviceToHost, st.s_out));
      }
    }
    HIP_TRY(hipEventRecord(st.ev_out[b], st.s_out));
    done += m;
    frames_done += f;
  }
  HIP_TRY(hipStreamSynchronize(st.s_in));
  if (out.device) return rc2;
  HIP_TRY(hipStreamSynchronize(stream));
  HIP_TRY(hipStreamSynchronize(st.s_out));
  return rc2;
}

}  // namespace

int stage_host(HostStage& st, hipStream_t stream, const StageSteps& steps, const void* in, uint64_t n,
               const StageOut& out) {
  const int rc = stage_host_steps(st, stream, steps, in, n, out);
  if (rc != PFB_OK) {
    // a failed step returned from the middle of the pipeline: copies to and from the CALLER's buffers may still be
    // in flight on the three streams -- drain them before the caller is told it may free or reuse those buffers
    if (st.s_in) (void)hipStreamSynchronize(st.s_in);
    (void)hipStreamSynchronize(stream);
    if (st.s_out) (void)hipStreamSynchronize(st.s_out);
    (void)hipGetLastError();
  }
  return rc;
}

// -- .iq records ---------------------------------------------------------------------

namespace {

// read exactly `bytes` at `offset` of fd into dst with `nthreads` concurrent pread streams (one thread copies out
// of the page cache at ~7 GB/s, less than PCIe takes; four keep the link busy)
bool pread_parallel(int fd, char* dst, size_t bytes, off_t offset, int nthreads) {
  auto read_range = [fd](char* d, size_t len, off_t off) {
    while (len > 0) {
      const ssize_t r = ::pread(fd, d, len, off);
      if (r <= 0) return false;
      d += r; len -= (size_t)r; off += r;
    }
    return true;
  };
  if (nthreads <= 1 || bytes < ((size_t)4 << 20)) return read_range(dst, bytes, offset);
  const size_t part = ((bytes / (size_t)nthreads) + 4095) & ~(size_t)4095;
  std::vector<std::thread> th;
  std::vector<char> ok((size_t)nthreads, 1);
  for (int t = 0; t < nthreads; ++t) {
    const size_t lo = std::min(bytes, part * (size_t)t), hi = std::min(bytes, part * (size_t)(t + 1));
    if (hi > lo) th.emplace_back([&, t, lo, hi] { ok[(size_t)t] = read_range(dst + lo, hi - lo, offset + (off_t)lo); });
  }
  for (auto& x : th) x.join();
  for (char c : ok) if (!c) return false;
  return true;
}

}  // namespace

Record::~Record() {
  if (fd >= 0) ::close(fd);
}

int Record::open(const char* path, int fmt, int bit_width) {
  const int f = ::open(path, O_RDONLY);
  if (f < 0) { g_detail = std::string("cannot open ") + path; return PFB_ERR_BAD_ARG; }
  unsigned char head[PFB_IQ_HEADER_BYTES];
  const ssize_t got = ::pread(f, head, sizeof(head), 0);
  int rc = pfb_iq_parse_header(head, got > 0 ? (size_t)got : 0, &info);
  if (rc == PFB_OK && fmt >= 0 && ((int)info.sample_format != fmt || (int)info.packet.bitWidth != bit_width))
    rc = PFB_ERR_BAD_FORMAT;  // the handle's scale / unpack would not match this record
  if (rc == PFB_OK) {
    struct stat st;
    const long long size = ::fstat(f, &st) == 0 ? (long long)st.st_size : -1;
    if (size - (long long)info.header_bytes != (long long)info.packet.numSamples * (long long)info.bytes_per_sample)
      rc = PFB_ERR_BAD_FORMAT;
  }
  if (rc != PFB_OK) { ::close(f); return rc; }
  fd = f;
  return PFB_OK;
}

int Record::read(uint64_t chunk, const std::function<int(const char*, uint64_t, uint64_t)>& consume) {
  const uint64_t n = info.packet.numSamples;
  const size_t bps = info.bytes_per_sample;
  if (n == 0) return PFB_OK;
  const size_t chunk_bytes = (size_t)std::min<uint64_t>(chunk, n) * bps;
  char* bufs[2] = {static_cast<char*>(pfb_host_alloc(chunk_bytes)), static_cast<char*>(pfb_host_alloc(chunk_bytes))};
  if (!bufs[0] || !bufs[1]) {
    pfb_host_free(bufs[0]);
    pfb_host_free(bufs[1]);
    return PFB_ERR_NO_MEMORY;
  }
  const unsigned hw = std::thread::hardware_concurrency();
  const int readers = (int)std::max(1u, std::min(4u, hw ? hw / 2 : 1u));
  auto read_chunk = [&](char* dst, uint64_t first, uint64_t m) {
    return pread_parallel(fd, dst, (size_t)m * bps, (off_t)info.header_bytes + (off_t)(first * bps), readers);
  };
  int rc = read_chunk(bufs[0], 0, std::min<uint64_t>(chunk, n)) ? PFB_OK : PFB_ERR_BAD_FORMAT;
  uint64_t done = 0;
  for (uint64_t i = 0; done < n && rc == PFB_OK; ++i) {
    const uint64_t m = std::min<uint64_t>(chunk, n - done);
    const uint64_t m_next = std::min<uint64_t>(chunk, n - done - m);
    bool next_ok = true;
    std::thread reader;
    if (m_next > 0) reader = std::thread([&, i, m_next] { next_ok = read_chunk(bufs[(i + 1) & 1], done + m, m_next); });
    rc = consume(bufs[i & 1], done, m);
    if (reader.joinable()) reader.join();
    if (rc == PFB_OK && !next_ok) rc = PFB_ERR_BAD_FORMAT;
    done += m;
  }
  pfb_host_free(bufs[0]);
  pfb_host_free(bufs[1]);
  return rc;
}

}  // namespace pfb
