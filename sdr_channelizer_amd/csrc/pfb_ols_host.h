// pfb_ols_host.h -- host side of "a stream filtered against a replica by overlap-save" that pfb_mf.hip and
// pfb_mfbank.hip share (defined in pfb_ols_host.cpp): the replica checks, the spectrum builder and the stream state of a
// handle.  mf_check and bank_check call the checks in the order the public header states; what is theirs alone (route,
// NFFT rule, hypothesis grid) stays with them.
#pragma once

#include <complex>
#include <vector>

#include "pfb_host.h"

namespace pfb {

constexpr uint32_t kOlsMaxReplica = 65536;  // the longest replica of pfb_mf_create and pfb_mfbank_create

// in-place radix-2 DFT, kernel e^{-j 2 pi n k / n}, n a power of two; twiddles straight from cos / sin of the index
void dft_minus(std::vector<std::complex<double>>& a);

// Finite values and the energy of K complex replica samples: PFB_ERR_BAD_ARG for a non-finite value, and for zero
// energy with normalize.  *gain = 1 / energy (normalize) or 1.
int replica_gain(const float* replica, uint32_t K, bool normalize, double* gain);

// Sample format and its bit width: PFB_ERR_BAD_FORMAT.  *bw = the bit width that scales the samples (cf32: 1)
int replica_format(uint32_t sample_format, uint32_t bit_width, uint32_t* bw);

// spec[p N + k] = scale * sum_{n < B} conj(r[p B + n]) e^{-j 2 pi n k / N}, p < P, r zero from K on, in float64 and
// rounded once; scale = gain * 2^-(bw-1) / N.  PFB_ERR_BAD_ARG where a value does not fit float32.
int replica_spectra(const float* replica, uint32_t K, uint32_t N, uint32_t B, uint32_t P, double gain, uint32_t bw,
                    std::vector<float2>* spec);

// The stream state of a handle: what K, the input format and the samples so far decide, and the device arrays every
// kernel of the stream reads.  Calls are made on the handle's device.
struct OlsStream {
  int K = 0, nfft = 0;
  int fmt = 0, bit_width = 0;
  int bps = 0;        // bytes per input sample
  int out_elem = 8;   // bytes per output element: the owner sets it
  uint64_t pos = 0;   // samples since create / reset
  float2* d_spec = nullptr;
  float2* d_tw = nullptr;
  void* d_carry[2] = {nullptr, nullptr};  // K - 1 raw samples each; the last min(pos, K - 1) precede the next call
  int cur = 0;
  hipStream_t stream = nullptr;
  hipEvent_t ev_switch = nullptr;
  HostStage stage;

  uint64_t carried() const { return pos < (uint64_t)K - 1 ? pos : (uint64_t)K - 1; }
  uint64_t outputs_for(uint64_t n) const {
    const uint64_t total = carried() + n;
    return total >= (uint64_t)K ? total - (uint64_t)K + 1 : 0;
  }
  // the fields above from a checked config; the spectra, the twiddles of nfft and two zeroed carry buffers on the device
  hipError_t allocate(uint32_t replica_length, uint32_t fft_length, uint32_t sample_format, uint32_t bit_width_cfg,
                      const std::vector<float2>& spec);
  void release();
  // what every process call checks before the device is touched; *f = the outputs it completes
  int check_call(const void* iq, uint64_t n, const void* out, uint64_t cap, uint64_t* outputs_out, bool device,
                 uint64_t* f) const;
  // after the kernels of a call of n samples at d_iq: the last K - 1 samples of [carry | in] become the carry
  int advance(const void* d_iq, uint64_t n);
};

}  // namespace pfb
