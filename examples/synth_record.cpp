// synth_record.cpp -- a C++ host, no Python, that makes the reference's two test signals as .iq records over the C ABI
// (pfb_synth_* in pfb_channelizer.h) and reads them back:
//   <dir>/training.iq  /root/reference/matlab/generate_training_iq.m: carrier, PW, PRI and start index drawn as
//                      :13-26 draws them, phase from zero (:44-48), int16(x*2^15) (:95-98), the format-1 record (:107-127)
//   <dir>/pulsed.iq    /root/reference/matlab/generate_pulsed_iq.m:12-77 with LFM_EXTENT = 5 MHz and BARKER_13 = true,
//                      as a format-3 record (the script itself only plots)
// One line per record on stdout holds everything needed to make the same samples again.
//
//   g++ -O2 -Iinclude examples/synth_record.cpp -Lsdr_channelizer_amd -lpfb_channelizer \
//       -Wl,-rpath,$PWD/sdr_channelizer_amd -o examples/synth_record
//   ./examples/synth_record 12345 /tmp [T_seconds = 0.1]
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <random>
#include <string>
#include <vector>

#include "pfb_channelizer.h"

static int fail(const char* what, int status) {
  std::fprintf(stderr, "%s: %s [%s]\n", what, pfb_strerror(status), pfb_last_error_detail());
  return 1;
}

// write cfg's first record_samples samples to `path`, read the header back, print the line
static int make_record(const char* kind, const std::string& path, int file_format, pfb_synth_config cfg) {
  pfb_synth_params q;
  int status = pfb_synth_describe(&cfg, &q, nullptr);  // host only: what pulse width the Barker chips leave
  if (status != PFB_OK) return fail("pfb_synth_describe", status);
  pfb_synth_handle* src = nullptr;
  if ((status = pfb_synth_create(&cfg, &src)) != PFB_OK) return fail("pfb_synth_create", status);
  status = pfb_synth_write_iq_file(src, path.c_str(), file_format, 0, (uint32_t)cfg.record_samples, nullptr);
  pfb_synth_destroy(src);
  if (status != PFB_OK) return fail("pfb_synth_write_iq_file", status);

  std::ifstream fin(path, std::ifstream::binary);
  std::vector<char> head(PFB_IQ_HEADER_BYTES);
  fin.read(head.data(), (std::streamsize)head.size());
  pfb_iq_info info;
  if ((status = pfb_iq_parse_header(head.data(), (size_t)fin.gcount(), &info)) != PFB_OK) return fail(path.c_str(), status);
  uint64_t pulses = 0;  // the ones that fit: (idx + numSamplesForPw) < length(mag), idx 1-based
  for (uint64_t s = cfg.first_pulse; s + 1 + q.pulse_samples < cfg.record_samples; s += cfg.period_samples) ++pulses;
  std::printf("%s %s f0=%.17g pw=%u pri=%u first=%llu n=%llu lfm=%.17g barker=%d pulses=%llu read_back=%u format=%d board=%s\n",
              kind, path.c_str(), cfg.f0, cfg.pulse_samples, cfg.period_samples, (unsigned long long)cfg.first_pulse,
              (unsigned long long)cfg.record_samples, cfg.lfm_extent_hz, (cfg.flags & PFB_SYNTH_BARKER13) ? 1 : 0,
              (unsigned long long)pulses, info.packet.numSamples, info.file_format, info.packet.boardName);
  return 0;
}

int main(int argc, char** argv) {
  if (argc < 3) {
    std::fprintf(stderr, "usage: %s <seed> <output directory> [T_seconds]\n", argv[0]);
    return 1;
  }
  std::mt19937_64 gen(std::strtoull(argv[1], nullptr, 10));
  const auto rnd = [&gen]() { return (double)(gen() >> 11) * 0x1p-53; };  // MATLAB's rand: uniform in [0, 1)
  const std::string dir = argv[2];
  const double fs = 56e6, T = argc > 3 ? std::atof(argv[3]) : 100e-3;

  pfb_synth_config cfg{};
  cfg.struct_size = sizeof(cfg);
  cfg.sample_format = PFB_FMT_INT16_IQ;
  cfg.bit_width = 16;                 // maxVal = 2^(16-1), generate_training_iq.m:95
  cfg.device_id = -1;
  cfg.fs = fs;
  cfg.amplitude = 1.0;                // mag = 1: +1.0 saturates at 32767 as int16() does
  cfg.noise_sigma = 0.0;              // the scripts add none

  // generate_training_iq.m:13-26
  cfg.f0 = -(fs / 2) + fs * rnd();
  const double PW = 10e-6 + (1000e-6 - 10e-6) * rnd();
  const double min_pri = std::max(10e-6, PW);
  const double PRI = min_pri + (10000e-6 - min_pri) * rnd();
  const double pri_samples = std::round(PRI * fs);
  const double start_idx = std::round((1.0 + std::floor(rnd() * pri_samples)) / fs * fs);  // randi, then t0 and back
  cfg.pulse_samples = (uint32_t)std::round(fs * PW);
  cfg.period_samples = (uint32_t)pri_samples;
  cfg.first_pulse = (uint64_t)start_idx - 1;  // the script's idx is 1-based
  cfg.record_samples = (uint64_t)std::llround(fs * T);
  cfg.flags = PFB_SYNTH_PHASE_FROM_ZERO | PFB_SYNTH_ROUND_MATLAB;
  if (make_record("training", dir + "/training.iq", 1, cfg)) return 1;

  // generate_pulsed_iq.m:12-19 with both switches on
  cfg.f0 = -(fs / 2) + fs * rnd();
  cfg.pulse_samples = (uint32_t)std::llround(fs * 100e-6);
  cfg.period_samples = (uint32_t)std::llround(fs * 1000e-6);
  cfg.first_pulse = 0;                // idx = 1
  cfg.record_samples = (uint64_t)std::llround(fs * 10e-3);
  cfg.lfm_extent_hz = 5e6;
  cfg.flags = PFB_SYNTH_BARKER13 | PFB_SYNTH_ROUND_MATLAB;
  return make_record("pulsed", dir + "/pulsed.iq", 3, cfg);
}
