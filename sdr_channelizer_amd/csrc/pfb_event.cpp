// pfb_event.cpp -- the host-only half of the event predictor (include/pfb_channelizer.h, "dwell analysis and event
// prediction"): the argument check pfb_dwell_analyze and pfb_dwell_from_iq_file share, the SNR-vs-TOA parabola
// (matlab/predict_event.m:125-130, cpp/usrp_predict_event.cpp:28-52) and the next-event rule (m:134-138, cpp:354-372).
// Nothing here touches the device.
#include <algorithm>
#include <cmath>
#include <vector>

#include "pfb_common.h"  // abi_guard
#include "pfb_host.h"

namespace pfb {

int dwell_check_config(const pfb_dwell_config* cfg, bool from_file) {
  if (!cfg || cfg->struct_size != sizeof(pfb_dwell_config)) return PFB_ERR_BAD_ARG;
  if (cfg->statistic > PFB_DWELL_STAT_MEDIAN || (cfg->flags & ~(uint32_t)PFB_DWELL_SKIP_FREQ)) return PFB_ERR_BAD_ARG;
  if (!(cfg->sat_fraction >= 0.0 && cfg->sat_fraction <= 1.0)) return PFB_ERR_BAD_ARG;
  if (!std::isfinite(cfg->snr_threshold_db) || !std::isfinite(std::pow(10.0, cfg->snr_threshold_db / 10.0)))
    return PFB_ERR_BAD_ARG;
  if (from_file) return PFB_OK;  // format, bit width and fs are the record's
  if (cfg->sample_format > PFB_FMT_CF32 || cfg->mem > PFB_MEM_DEVICE || !std::isfinite(cfg->fs)) return PFB_ERR_BAD_ARG;
  if (cfg->sample_format != PFB_FMT_CF32 && (cfg->bit_width < 1 || cfg->bit_width > 16)) return PFB_ERR_BAD_ARG;
  return PFB_OK;
}

}  // namespace pfb

extern "C" int pfb_event_fit(const pfb_pdw* pdws, uint64_t n, double* t_peak, double* snr_peak, double coef[3]) {
  return pfb::abi_guard([&]() -> int {
    if (!pdws || !t_peak || !snr_peak || !coef || n < 3) return PFB_ERR_BAD_ARG;
    // A = [1 tau tau^2] (n x 3), b = snr: Householder reflections column by column (what Eigen's householderQr and
    // polyfit's backslash do), applied to b on the way; R p = Q^T b by back substitution
    std::vector<double> a(3 * (size_t)n), b((size_t)n);
    const double t0 = pdws[0].toa;
    for (uint64_t i = 0; i < n; ++i) {
      const double tau = pdws[i].toa - t0;
      a[i] = 1.0; a[n + i] = tau; a[2 * n + i] = tau * tau;
      b[i] = pdws[i].snr;
    }
    double r[3][3] = {};
    for (int k = 0; k < 3; ++k) {
      double* col = &a[(size_t)k * n];
      double norm = 0.0;
      for (uint64_t i = (uint64_t)k; i < n; ++i) norm = std::hypot(norm, col[i]);
      const double alpha = col[k] > 0.0 ? -norm : norm;
      r[k][k] = alpha;
      if (norm == 0.0) continue;  // rank-deficient: the zero pivot makes the solution non-finite below
      col[k] -= alpha;            // v = x - alpha e_k, kept in place
      double vv = 0.0;
      for (uint64_t i = (uint64_t)k; i < n; ++i) vv += col[i] * col[i];
      if (vv == 0.0) continue;
      auto reflect = [&](double* y) {
        double dot = 0.0;
        for (uint64_t i = (uint64_t)k; i < n; ++i) dot += col[i] * y[i];
        const double f = 2.0 * dot / vv;
        for (uint64_t i = (uint64_t)k; i < n; ++i) y[i] -= f * col[i];
      };
      for (int c = k + 1; c < 3; ++c) {
        reflect(&a[(size_t)c * n]);
        r[k][c] = a[(size_t)c * n + k];
      }
      reflect(b.data());
    }
    double p[3];
    for (int k = 2; k >= 0; --k) {
      double s = b[k];
      for (int c = k + 1; c < 3; ++c) s -= r[k][c] * p[c];
      p[k] = s / r[k][k];
    }
    coef[0] = p[0]; coef[1] = p[1]; coef[2] = p[2];
    const double tau_peak = -p[1] / (2.0 * p[2]);  // m:129, cpp:51
    *t_peak = t0 + tau_peak;
    *snr_peak = p[0] + tau_peak * (p[1] + tau_peak * p[2]);  // m:130
    const bool finite = std::isfinite(p[0]) && std::isfinite(p[1]) && std::isfinite(p[2]) && std::isfinite(tau_peak);
    return (finite && p[2] < 0.0) ? PFB_OK : PFB_ERR_UNSUPPORTED;
  });
}

extern "C" int pfb_event_next(const double* event_times, uint64_t n, uint32_t convention, double* next,
                              int32_t* have_next) {
  return pfb::abi_guard([&]() -> int {
    if (!next || !have_next || convention > 1 || (n > 0 && !event_times)) return PFB_ERR_BAD_ARG;
    *have_next = 0;
    if (convention == 0 ? n < 2 : n <= 5) return PFB_OK;  // m:134 length(event) > 1; cpp:354 size() > 5
    std::vector<double> d((size_t)n - 1);
    for (uint64_t k = 1; k < n; ++k) d[k - 1] = event_times[k] - event_times[k - 1];  // m:135 diff, cpp:359-362
    std::sort(d.begin(), d.end());
    const size_t m = d.size();
    const double med = (convention == 1 || (m & 1)) ? d[m / 2] : 0.5 * (d[m / 2 - 1] + d[m / 2]);  // cpp:367 / MATLAB median
    *next = event_times[n - 1] + med;  // m:135, cpp:371
    *have_next = 1;
    return PFB_OK;
  });
}
