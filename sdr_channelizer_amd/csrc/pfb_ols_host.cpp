// pfb_ols_host.cpp -- the replica checks, the spectrum builder and the stream state declared in pfb_ols_host.h.
#include "pfb_ols_host.h"

#include <algorithm>
#include <cmath>
#include <utility>

#include "pfb_common.h"

namespace pfb {

void dft_minus(std::vector<std::complex<double>>& a) {
  const size_t n = a.size();
  for (size_t i = 1, j = 0; i < n; ++i) {
    size_t bit = n >> 1;
    for (; j & bit; bit >>= 1) j ^= bit;
    j ^= bit;
    if (i < j) std::swap(a[i], a[j]);
  }
  std::vector<std::complex<double>> w(n / 2);
  for (size_t k = 0; k < n / 2; ++k) {
    const double ang = -2.0 * M_PI * (double)k / (double)n;
    w[k] = {std::cos(ang), std::sin(ang)};
  }
  for (size_t len = 2; len <= n; len <<= 1)
    for (size_t i = 0; i < n; i += len)
      for (size_t k = 0; k < len / 2; ++k) {
        const std::complex<double> u = a[i + k], v = a[i + k + len / 2] * w[k * (n / len)];
        a[i + k] = u + v;
        a[i + k + len / 2] = u - v;
      }
}

int replica_gain(const float* replica, uint32_t K, bool normalize, double* gain) {
  double energy = 0.0;
  for (uint64_t i = 0; i < 2 * (uint64_t)K; ++i) {
    if (!std::isfinite(replica[i])) return PFB_ERR_BAD_ARG;
    energy += (double)replica[i] * (double)replica[i];
  }
  if (normalize && energy == 0.0) return PFB_ERR_BAD_ARG;
  *gain = normalize ? 1.0 / energy : 1.0;
  return PFB_OK;
}

int replica_format(uint32_t sample_format, uint32_t bit_width, uint32_t* bw) {
  if (sample_format > PFB_FMT_CF32) return PFB_ERR_BAD_FORMAT;
  if (sample_format == PFB_FMT_INT8_IQ && (bit_width < 1 || bit_width > 8)) return PFB_ERR_BAD_FORMAT;
  if (sample_format == PFB_FMT_INT16_IQ && (bit_width < 1 || bit_width > 16)) return PFB_ERR_BAD_FORMAT;
  *bw = sample_format == PFB_FMT_CF32 ? 1 : bit_width;  // cf32: scale 1
  return PFB_OK;
}

int replica_spectra(const float* replica, uint32_t K, uint32_t N, uint32_t B, uint32_t P, double gain, uint32_t bw,
                    std::vector<float2>* spec) {
  const double scale = gain * std::ldexp(1.0, -((int)bw - 1)) / (double)N;
  spec->assign((size_t)P * N, make_float2(0.f, 0.f));
  std::vector<std::complex<double>> a(N);
  for (uint32_t q = 0; q < P; ++q) {
    std::fill(a.begin(), a.end(), std::complex<double>(0.0, 0.0));
    for (uint32_t n = 0; n < B && (uint64_t)q * B + n < K; ++n) {
      const float* r = replica + 2 * ((size_t)q * B + n);
      a[n] = {(double)r[0], -(double)r[1]};
    }
    dft_minus(a);
    for (uint32_t k = 0; k < N; ++k) {
      const float re = (float)(a[k].real() * scale), im = (float)(a[k].imag() * scale);
      if (!std::isfinite(re) || !std::isfinite(im)) return PFB_ERR_BAD_ARG;  // the spectrum must fit float32
      (*spec)[(size_t)q * N + k] = make_float2(re, im);
    }
  }
  return PFB_OK;
}

hipError_t OlsStream::allocate(uint32_t replica_length, uint32_t fft_length, uint32_t sample_format, uint32_t bit_width_cfg,
                               const std::vector<float2>& spec) {
  K = (int)replica_length;
  nfft = (int)fft_length;
  fmt = (int)sample_format;
  bit_width = fmt == PFB_FMT_CF32 ? 1 : (int)bit_width_cfg;
  bps = bytes_per_sample(fmt);
  const size_t carry_bytes = (size_t)std::max(K - 1, 1) * bps, spec_bytes = spec.size() * sizeof(float2);
  hipError_t e = hipMalloc((void**)&d_spec, spec_bytes);
  if (e == hipSuccess) e = upload_twiddles((uint32_t)nfft, &d_tw);
  if (e == hipSuccess) e = hipMalloc(&d_carry[0], carry_bytes);
  if (e == hipSuccess) e = hipMalloc(&d_carry[1], carry_bytes);
  if (e == hipSuccess) e = hipMemcpy(d_spec, spec.data(), spec_bytes, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemset(d_carry[0], 0, carry_bytes);
  if (e == hipSuccess) e = hipMemset(d_carry[1], 0, carry_bytes);
  return e;
}

void OlsStream::release() {
  (void)hipFree(d_spec);
  (void)hipFree(d_tw);
  (void)hipFree(d_carry[0]);
  (void)hipFree(d_carry[1]);
  stage.release();
  if (ev_switch) (void)hipEventDestroy(ev_switch);
}

int OlsStream::check_call(const void* iq, uint64_t n, const void* out, uint64_t cap, uint64_t* outputs_out, bool device,
                          uint64_t* f) const {
  if ((n > 0 && !iq) || n > ((uint64_t)1 << 62) || pos + n < pos) return PFB_ERR_BAD_ARG;
  *f = outputs_for(n);
  if (outputs_out) *outputs_out = *f;
  if (*f > cap) return PFB_ERR_CAPACITY;
  if (*f > 0 && !out) return PFB_ERR_BAD_ARG;
  if (device && (reinterpret_cast<uintptr_t>(iq) % (uintptr_t)bps || reinterpret_cast<uintptr_t>(out) % (uintptr_t)out_elem))
    return PFB_ERR_BAD_ARG;
  return PFB_OK;
}

int OlsStream::advance(const void* d_iq, uint64_t n) {
  if (n > 0 && K > 1) {
    HIP_TRY(launch_update_history(d_carry[cur], d_iq, (long long)n, d_carry[cur ^ 1], K - 1, bps, stream));
    cur ^= 1;
  }
  pos += n;
  return PFB_OK;
}

}  // namespace pfb
