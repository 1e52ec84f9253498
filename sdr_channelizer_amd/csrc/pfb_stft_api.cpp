// pfb_stft_api.cpp -- host side of the short-time Fourier transform (pfb_stft_* in include/pfb_channelizer.h): the
// handle (window, twiddles, carried samples), kernel choice, host and .iq paths over pfb_host.h; kernels in pfb_stft.hip.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <new>
#include <vector>

#include "pfb_common.h"
#include "pfb_channelizer_dev.h"
#include "pfb_host.h"

using pfb::DeviceGuard;

struct pfb_stft_handle {
  int L = 0, H = 0, nfft = 0;
  int fmt = 0, bit_width = 0, output = 0, order = 0, kernel_opt = 0;
  float scale = 1.f, db_floor = 0.f;
  int device = 0;
  int bps = 0;               // bytes per input sample
  int out_elem = 8;          // complex64, or float32 for power / dB
  float* d_win = nullptr;    // L: window x 2^-(bit_width-1)
  float2* d_tw = nullptr;    // nfft: e^{+j 2 pi m / nfft}
  void* d_carry[2] = {nullptr, nullptr};  // L raw samples each; the last carry_len are the start of the next frame
  int cur = 0;
  uint64_t carry_len = 0;    // < L
  hipStream_t stream = nullptr;
  const pfb::StftKernelInfo* kern = nullptr;
  const char* last_kernel = "";
  int experiment = 0;          // pfb_stft_set_experiment (pfb_channelizer_dev.h): 1 = loads and stores only
  pfb::HostStage stage;        // host path
  hipEvent_t ev_switch = nullptr;
};

pfb::OutputDesc pfb::describe_output(const pfb_stft_handle* h) {
  pfb::OutputDesc d;
  d.device = h->device;
  d.stream = h->stream;
  d.fmt = h->fmt;
  d.bit_width = h->bit_width;
  d.bps = h->bps;
  d.width = (uint32_t)h->nfft;
  d.element = h->output == PFB_STFT_COMPLEX ? PFB_WF_COMPLEX : PFB_WF_POWER;
  d.layout = PFB_WF_ROWS;
  d.reducible = h->output != PFB_STFT_DB;
  d.carry_max = (uint64_t)h->L - 1;
  return d;
}

namespace {

void free_stft(pfb_stft_handle* h) {
  if (!h) return;
  DeviceGuard g(h->device);
  (void)hipFree(h->d_win);
  (void)hipFree(h->d_tw);
  (void)hipFree(h->d_carry[0]);
  (void)hipFree(h->d_carry[1]);
  h->stage.release();
  if (h->ev_switch) (void)hipEventDestroy(h->ev_switch);
  delete h;
}

uint64_t stft_frames_for(const pfb_stft_handle* h, uint64_t n) {
  const uint64_t total = h->carry_len + n;
  return total >= (uint64_t)h->L ? (total - (uint64_t)h->L) / (uint64_t)h->H + 1 : 0;
}

// kernel + carry update for device-resident buffers; no host sync
int stft_enqueue(pfb_stft_handle* h, const void* d_iq, uint64_t n, void* d_out, uint64_t frames) {
  if (frames > 0) {
    pfb::StftParams p{};
    p.in = d_iq;
    p.carry = h->d_carry[h->cur];
    p.out = d_out;
    p.win = h->d_win;
    p.tw = h->d_tw;
    p.n_in = (long long)n;
    p.frames = (long long)frames;
    p.carry_len = (int)h->carry_len;
    p.carry_cap = h->L;
    p.L = h->L; p.H = h->H; p.nfft = h->nfft;
    p.fmt = h->fmt; p.output = h->output; p.order = h->order;
    p.scale = h->scale; p.db_floor = h->db_floor;
    const bool study = h->experiment == 1;
    HIP_TRY((study ? h->kern->launch_loadstore : h->kern->launch)(p, h->stream));
    h->last_kernel = study ? h->kern->name_loadstore : h->kern->name;
  }
  if (n > 0) {  // the last L samples of [carry | in]: the next frame starts in them
    HIP_TRY(pfb::launch_update_history(h->d_carry[h->cur], d_iq, (long long)n, h->d_carry[h->cur ^ 1], h->L, h->bps,
                                       h->stream));
    h->cur ^= 1;
  }
  h->carry_len = h->carry_len + n - frames * (uint64_t)h->H;
  return PFB_OK;
}

// Host buffers (pageable or page-locked) go through the staged pipeline in chunks of at most `chunk` samples, so sized
// that neither side of the staging exceeds 64 MiB (a hop of 1 makes nfft outputs per input sample).  Any cut of the
// stream gives the same bits, so the chunk size never shows in the output.
int process_host(pfb_stft_handle* h, const void* iq, uint64_t n, void* out, uint64_t chunk = UINT64_MAX) {
  const uint64_t frame_bytes = (uint64_t)h->nfft * h->out_elem, budget = (uint64_t)64 << 20;
  chunk = std::min<uint64_t>(chunk, std::min<uint64_t>((uint64_t)1 << 24, budget / h->bps));
  chunk = std::min<uint64_t>(chunk, std::max<uint64_t>(1, budget / frame_bytes) * (uint64_t)h->H);
  const pfb::StageSteps steps{
      chunk, (h->L - 1 + chunk) / (uint64_t)h->H + 1, (size_t)h->bps, (size_t)frame_bytes,
      [h](uint64_t m) { return stft_frames_for(h, m); },
      [h](const void* d_in, uint64_t m, void* d_out, uint64_t f, int64_t, int64_t) {
        return stft_enqueue(h, d_in, m, d_out, f);
      }};
  return pfb::stage_host(h->stage, h->stream, steps, iq, n, pfb::StageOut{out});
}

}  // namespace

extern "C" {

int pfb_stft_create(const pfb_stft_config* cfg, pfb_stft_handle** out) {
  return pfb::abi_guard([&]() -> int {
  if (!cfg || !out) return PFB_ERR_BAD_ARG;
  *out = nullptr;
  if (cfg->struct_size != sizeof(pfb_stft_config) || !cfg->window) return PFB_ERR_BAD_ARG;
  const uint32_t L = cfg->window_length;
  const uint32_t H = cfg->hop ? cfg->hop : L;
  const uint32_t nfft = cfg->fft_length ? cfg->fft_length : L;
  if (L < 1 || H > L || nfft < L) return PFB_ERR_BAD_ARG;
  if (cfg->output > PFB_STFT_DB || cfg->freq_order > PFB_STFT_TWOSIDED || cfg->kernel > PFB_STFT_KERNEL_FUSED)
    return PFB_ERR_BAD_ARG;
  // both are applied in float32: they must survive the conversion (no overflow to inf, no underflow to 0)
  const auto in_float = [](double v) { return v == 0 || (v >= (double)FLT_MIN && v <= (double)FLT_MAX); };
  if (!std::isfinite(cfg->scale) || cfg->scale < 0 || !std::isfinite(cfg->db_floor) || cfg->db_floor < 0 ||
      !in_float(cfg->scale) || !in_float(cfg->db_floor))
    return PFB_ERR_BAD_ARG;
  if (nfft > 4096) return PFB_ERR_UNSUPPORTED;  // as pfb_create for M > 4096
  if (cfg->sample_format > PFB_FMT_CF32) return PFB_ERR_BAD_FORMAT;
  int bw = (int)cfg->bit_width;
  if (cfg->sample_format == PFB_FMT_INT8_IQ && (bw < 1 || bw > 8)) return PFB_ERR_BAD_FORMAT;
  if (cfg->sample_format == PFB_FMT_INT16_IQ && (bw < 1 || bw > 16)) return PFB_ERR_BAD_FORMAT;
  if (cfg->sample_format == PFB_FMT_CF32) bw = 1;  // scale 1
  const pfb::StftKernelInfo* fused = pfb::find_stft_fused((int)nfft, (int)cfg->sample_format);
  if (cfg->kernel == PFB_STFT_KERNEL_FUSED && !fused) return PFB_ERR_UNSUPPORTED;

  int dev = 0;
  const int drc = pfb::resolve_device(cfg->device_id, &dev);
  if (drc != PFB_OK) return drc;

  pfb_stft_handle* h = new (std::nothrow) pfb_stft_handle();
  if (!h) return PFB_ERR_NO_MEMORY;
  h->L = (int)L; h->H = (int)H; h->nfft = (int)nfft;
  h->fmt = (int)cfg->sample_format; h->bit_width = bw;
  h->output = (int)cfg->output; h->order = (int)cfg->freq_order; h->kernel_opt = (int)cfg->kernel;
  h->scale = cfg->scale == 0 ? 1.f : (float)cfg->scale;
  h->db_floor = (float)cfg->db_floor;
  h->device = dev;
  h->bps = pfb::bytes_per_sample(h->fmt);
  h->out_elem = cfg->output == PFB_STFT_COMPLEX ? 8 : 4;
  h->kern = (cfg->kernel != PFB_STFT_KERNEL_GENERIC && fused) ? fused : pfb::stft_generic_kernel();

  DeviceGuard g(dev);
  std::vector<float> win(L);
  const float scale = std::ldexp(1.0f, -(bw - 1));  // power of two: w*scale is exact
  for (uint32_t i = 0; i < L; ++i) win[i] = cfg->window[i] * scale;
  const size_t carry_bytes = (size_t)L * h->bps;
  hipError_t e = hipMalloc((void**)&h->d_win, L * sizeof(float));
  if (e == hipSuccess) e = pfb::upload_twiddles(nfft, &h->d_tw);
  if (e == hipSuccess) e = hipMalloc(&h->d_carry[0], carry_bytes);
  if (e == hipSuccess) e = hipMalloc(&h->d_carry[1], carry_bytes);
  if (e == hipSuccess) e = hipMemcpy(h->d_win, win.data(), L * sizeof(float), hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemset(h->d_carry[0], 0, carry_bytes);
  if (e == hipSuccess) e = hipMemset(h->d_carry[1], 0, carry_bytes);
  if (e != hipSuccess) {
    const int rc = pfb::hip_fail(e, "pfb_stft_create allocation");
    free_stft(h);
    return rc;
  }
  *out = h;
  return PFB_OK;
  });
}

int pfb_stft_destroy(pfb_stft_handle* h) {
  return pfb::abi_guard([&]() -> int {
  if (!h) return PFB_ERR_BAD_ARG;
  free_stft(h);
  return PFB_OK;
  });
}

int pfb_stft_reset(pfb_stft_handle* h) {
  return pfb::abi_guard([&]() -> int {
  if (!h) return PFB_ERR_BAD_ARG;
  h->carry_len = 0;  // the carried samples are never read again; nothing on the device to clear
  return PFB_OK;
  });
}

int pfb_stft_set_stream(pfb_stft_handle* h, void* hip_stream) {
  return pfb::abi_guard([&]() -> int {
  if (!h) return PFB_ERR_BAD_ARG;
  return pfb::switch_stream(h->device, &h->stream, &h->ev_switch, static_cast<hipStream_t>(hip_stream));
  });
}

int pfb_stft_frames_for(const pfb_stft_handle* h, uint64_t n, uint64_t* frames_out) {
  if (!h || !frames_out) return PFB_ERR_BAD_ARG;
  *frames_out = stft_frames_for(h, n);
  return PFB_OK;
}

int pfb_stft_process_async(pfb_stft_handle* h, const void* d_iq, uint64_t n, void* d_out, uint64_t cap,
                           uint64_t* frames_out) {
  return pfb::abi_guard([&]() -> int {
  if (!h || (n > 0 && !d_iq)) return PFB_ERR_BAD_ARG;
  const uint64_t f = stft_frames_for(h, n);
  if (frames_out) *frames_out = f;
  if (f > cap) return PFB_ERR_CAPACITY;
  if (f > 0 && !d_out) return PFB_ERR_BAD_ARG;
  if (reinterpret_cast<uintptr_t>(d_iq) % h->bps || reinterpret_cast<uintptr_t>(d_out) % h->out_elem) return PFB_ERR_BAD_ARG;
  DeviceGuard g(h->device);
  return stft_enqueue(h, d_iq, n, d_out, f);
  });
}

int pfb_stft_sync(pfb_stft_handle* h) {
  return pfb::abi_guard([&]() -> int {
  if (!h) return PFB_ERR_BAD_ARG;
  DeviceGuard g(h->device);
  HIP_TRY(hipStreamSynchronize(h->stream));
  return PFB_OK;
  });
}

int pfb_stft_process(pfb_stft_handle* h, const void* iq, uint64_t n, void* out, uint64_t cap, uint64_t* frames_out,
                     uint32_t mem) {
  return pfb::abi_guard([&]() -> int {
  if (!h || (n > 0 && !iq) || mem > PFB_MEM_DEVICE) return PFB_ERR_BAD_ARG;
  const uint64_t f = stft_frames_for(h, n);
  if (frames_out) *frames_out = f;
  if (f > cap) return PFB_ERR_CAPACITY;
  if (f > 0 && !out) return PFB_ERR_BAD_ARG;
  DeviceGuard g(h->device);
  if (mem == PFB_MEM_DEVICE) {
    if (reinterpret_cast<uintptr_t>(iq) % h->bps || reinterpret_cast<uintptr_t>(out) % h->out_elem) return PFB_ERR_BAD_ARG;
    const int rc = stft_enqueue(h, iq, n, out, f);
    if (rc != PFB_OK) return rc;
    HIP_TRY(hipStreamSynchronize(h->stream));
    return PFB_OK;
  }
  return process_host(h, iq, n, out);
  });
}

int pfb_stft_process_iq_file(pfb_stft_handle* h, const char* path, void* out, uint64_t cap, uint64_t* frames_out,
                             pfb_iq_info* info_out) {
  return pfb::abi_guard([&]() -> int {
  if (!h || !path) return PFB_ERR_BAD_ARG;
  pfb::Record rec;
  const int rc = rec.open(path, h->fmt, h->bit_width);
  if (info_out) *info_out = rec.info;
  if (rc != PFB_OK) return rc;
  const uint64_t need = stft_frames_for(h, rec.info.packet.numSamples);
  if (frames_out) *frames_out = need;
  if (need > cap) return PFB_ERR_CAPACITY;
  if (need > 0 && !out) return PFB_ERR_BAD_ARG;
  // the payload in record chunks of 2^24 samples, each staged in steps of at most 2^22 so that the pipeline has
  // copies to overlap inside every chunk (the channelizer's .iq front end does the same); the record is never held
  // in memory
  const uint64_t frame_bytes = (uint64_t)h->nfft * h->out_elem;
  uint64_t frames_done = 0;
  const int rc2 = rec.read((uint64_t)1 << 24, [&](const char* buf, uint64_t, uint64_t m) {
    const uint64_t f = stft_frames_for(h, m);
    DeviceGuard g(h->device);
    const int r = process_host(h, buf, m, static_cast<char*>(out) + frames_done * frame_bytes, (uint64_t)1 << 22);
    frames_done += f;
    return r;
  });
  if (frames_out) *frames_out = frames_done;
  return rc2;
  });
}

int pfb_stft_axes(uint32_t nfft, uint32_t L, uint32_t H, double fs, uint32_t order, uint64_t first_frame,
                  uint64_t frames, double* f_out, double* t_out) {
  if (nfft < 1 || L < 1 || H < 1 || H > L || L > nfft || order > PFB_STFT_TWOSIDED || !std::isfinite(fs) || fs <= 0)
    return PFB_ERR_BAD_ARG;
  if (f_out) {
    // k_r = r - shift' with shift' = nfft/2 - 1 (even, stft 'centered'), (nfft-1)/2 (odd), 0 (twosided)
    const long long lo = order == PFB_STFT_TWOSIDED ? 0 : (nfft % 2 == 0 ? (long long)nfft / 2 - 1 : ((long long)nfft - 1) / 2);
    for (uint32_t r = 0; r < nfft; ++r) f_out[r] = (double)((long long)r - lo) * fs / (double)nfft;
  }
  if (t_out)
    for (uint64_t m = 0; m < frames; ++m) t_out[m] = ((double)(first_frame + m) * (double)H + (double)L / 2.0) / fs;
  return PFB_OK;
}

const char* pfb_stft_last_kernel(const pfb_stft_handle* h) { return h ? h->last_kernel : ""; }

int pfb_stft_get_device(const pfb_stft_handle* h, int* device_id) {
  if (!h || !device_id) return PFB_ERR_BAD_ARG;
  *device_id = h->device;
  return PFB_OK;
}

int pfb_stft_set_experiment(pfb_stft_handle* h, int experiment) {
  if (!h || experiment < 0 || experiment > 1) return PFB_ERR_BAD_ARG;
  if (experiment == 1 && !h->kern->launch_loadstore) return PFB_ERR_UNSUPPORTED;
  h->experiment = experiment;
  return PFB_OK;
}

}  // extern "C"
