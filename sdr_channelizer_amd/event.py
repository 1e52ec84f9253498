"""Dwell analysis and event prediction over the C ABI: the last layer of the reference (matlab/predict_event.m:53-138,
cpp/usrp_predict_event.cpp:285-375).  analyze_dwell finds a dwell's pulses (pfb_dwell_analyze: the MATLAB script's
median statistics or the live C++ loop's mean ones) and reports the gain finders' saturation figures; fit_event fits the
SNR-vs-TOA parabola; next_event schedules the next capture; EventPredictor strings them together as the two sources do."""
from __future__ import annotations

import ctypes as C
import math
from dataclasses import dataclass

import numpy as np

from . import _lib as L
from .pdw import PDW_DTYPE, _out_buffer, _take

STATISTICS = {"mean": L.PFB_DWELL_STAT_MEAN, "median": L.PFB_DWELL_STAT_MEDIAN}
CONVENTIONS = {"matlab": 0, "cpp": 1}


@dataclass
class DwellStats:
    """pfb_dwell_stats: one pass over the dwell.  mean_mag / peak_mag of |x|, x = (I + jQ)/2^(bit_width-1);
    peak_component = max |I|, |Q| on the same scale; saturated_components: the gain finders' count; noise_floor and
    threshold: the ones the edges used; any_pulse_saturated: over the PDWs returned."""
    num_samples: int
    saturated_components: int
    pulses: int
    mean_mag: float
    peak_mag: float
    peak_component: float
    noise_floor: float
    threshold: float
    any_pulse_saturated: bool

    @classmethod
    def _from_c(cls, s: L.PfbDwellStats) -> "DwellStats":
        return cls(int(s.num_samples), int(s.saturated_components), int(s.pulses), float(s.mean_mag), float(s.peak_mag),
                   float(s.peak_component), float(s.noise_floor), float(s.threshold), bool(s.any_pulse_saturated))


def _config(statistic, snr_threshold_db, skip_freq, sat_fraction, device, fmt=0, bit_width=12, mem=0, fs=0.0, fc=0.0,
            t0=0.0) -> L.PfbDwellConfig:
    if statistic not in STATISTICS:
        raise ValueError(f"statistic must be one of {sorted(STATISTICS)}")
    return L.PfbDwellConfig(C.sizeof(L.PfbDwellConfig), fmt, int(bit_width), STATISTICS[statistic],
                            L.PFB_DWELL_SKIP_FREQ if skip_freq else 0, mem, int(device), float(fs), float(fc), float(t0),
                            float(snr_threshold_db), float(sat_fraction))


def _finish(rc, where, out, count, capacity, stats):
    if rc != L.PFB_OK:
        detail = L.load().pfb_pdw_last_error_detail().decode()
        raise L.PfbError(rc, where + (f" [{detail}]" if detail else ""))
    k = int(count.value)
    return _take(out, min(k, capacity)), DwellStats._from_c(stats)


def analyze_dwell(iq, fs: float, fc: float, t0: float, *, statistic: str = "mean", bit_width: int = 12,
                  snr_threshold_db: float = 20.0, skip_freq: bool = False, sat_fraction: float = 0.98,
                  capacity: int = 1 << 20, device: int = -1):
    """One dwell -> (pdws, stats).  iq as extract_pdws_raw takes it: (n, 2) int8 / int16 (bit_width as in the record
    header) or (n,) complex64, a numpy array or a torch CUDA tensor (used in place, on the current stream).

    statistic="mean" is usrp_predict_event.cpp:287-343 (noise floor and pulse amplitude are means, toa is 0-based),
    "median" predict_event.m:64-121 (medians, toa 1-based: extract_pdws_raw with equal thresholds).  skip_freq (mean
    only): freq comes back NaN and no phase work is done -- the live loop reads toa and snr only.  More pulses than
    ``capacity`` is not an error here: stats.pulses counts them all, the first ``capacity`` are returned."""
    lib = L.load()
    is_torch = type(iq).__module__.startswith("torch")
    if is_torch and iq.is_cuda:
        import torch
        if not iq.is_contiguous():
            raise ValueError("need a contiguous tensor")
        fmt = {torch.int8: L.PFB_FMT_INT8_IQ, torch.int16: L.PFB_FMT_INT16_IQ, torch.complex64: L.PFB_FMT_CF32}[iq.dtype]
        n = int(iq.shape[0])
        ptr, mem, keep = C.c_void_p(iq.data_ptr()), L.PFB_MEM_DEVICE, iq
        stream = C.c_void_p(torch.cuda.current_stream(iq.device).cuda_stream)
        device = iq.device.index
    else:
        a = np.ascontiguousarray(np.asarray(iq))
        if a.dtype == np.complex64:
            fmt = L.PFB_FMT_CF32
        elif a.dtype in (np.int8, np.int16) and a.ndim == 2 and a.shape[1] == 2:
            fmt = L.PFB_FMT_INT8_IQ if a.dtype == np.int8 else L.PFB_FMT_INT16_IQ
        else:
            raise ValueError("iq must be (n, 2) int8/int16 or (n,) complex64")
        n = int(a.shape[0])
        ptr, mem, keep, stream = C.c_void_p(a.ctypes.data), L.PFB_MEM_HOST, a, C.c_void_p(0)
    cfg = _config(statistic, snr_threshold_db, skip_freq, sat_fraction, device, fmt, bit_width, mem, fs, fc, t0)
    out = _out_buffer(capacity)
    count, stats = C.c_uint64(0), L.PfbDwellStats()
    rc = lib.pfb_dwell_analyze(C.byref(cfg), ptr, n, out.ctypes.data_as(C.POINTER(L.PfbPdw)), capacity, C.byref(count),
                               C.byref(stats), stream)
    del keep
    return _finish(rc, "pfb_dwell_analyze", out, count, capacity, stats)


def dwell_from_iq_file(path: str, *, statistic: str = "mean", snr_threshold_db: float = 20.0, skip_freq: bool = False,
                       sat_fraction: float = 0.98, capacity: int = 1 << 20, device: int = -1):
    """One record from disk (pfb_dwell_from_iq_file): format, bit width, fs, fc and start time are the header's.
    Returns (pdws, stats, info)."""
    cfg = _config(statistic, snr_threshold_db, skip_freq, sat_fraction, device)
    out = _out_buffer(capacity)
    count, stats, info = C.c_uint64(0), L.PfbDwellStats(), L.PfbIqInfo()
    rc = L.load().pfb_dwell_from_iq_file(path.encode(), C.byref(cfg), out.ctypes.data_as(C.POINTER(L.PfbPdw)), capacity,
                                         C.byref(count), C.byref(stats), C.byref(info))
    return _finish(rc, "pfb_dwell_from_iq_file", out, count, capacity, stats) + (info,)


def fit_event(pdws):
    """The parabola of snr against toa (pfb_event_fit; predict_event.m:125-130, usrp_predict_event.cpp:28-52), fitted on
    toa - toa[0].  Returns (t_peak, snr_peak, coef) with coef = [p0, p1, p2] of p0 + p1*tau + p2*tau^2, or None when the
    fit has no maximum (not concave, degenerate).  Fewer than three PDWs raise."""
    a = np.ascontiguousarray(pdws, dtype=PDW_DTYPE)
    t_peak, snr_peak, coef = C.c_double(), C.c_double(), (C.c_double * 3)()
    rc = L.load().pfb_event_fit(a.ctypes.data_as(C.POINTER(L.PfbPdw)), len(a), C.byref(t_peak), C.byref(snr_peak), coef)
    if rc == L.PFB_ERR_UNSUPPORTED:
        return None
    L.check(rc, "pfb_event_fit")
    return t_peak.value, snr_peak.value, np.array(coef[:])


def next_event(event_times, convention: str = "matlab"):
    """last + median(diff(event_times)) (pfb_event_next), or None while the convention has too few events:
    "matlab" (predict_event.m:134-138) needs two and takes MATLAB's median, "cpp" (usrp_predict_event.cpp:354-372) needs
    six and takes sorted[size/2]."""
    t = np.ascontiguousarray(event_times, dtype=np.float64)
    nxt, have = C.c_double(), C.c_int32()
    L.check(L.load().pfb_event_next(t.ctypes.data_as(C.POINTER(C.c_double)), len(t), CONVENTIONS[convention],
                                    C.byref(nxt), C.byref(have)), "pfb_event_next")
    return nxt.value if have.value else None


class EventPredictor:
    """The loop both sources run around a dwell: analyse it, and if it holds an event, fit the peak, remember it and
    predict the next one.

    convention="matlab" is predict_event.m: median statistics, a dwell counts when max |x| > 0.9 (:53), the next event
    needs two events.  convention="cpp" is usrp_predict_event.cpp: mean statistics without frequencies, a dwell counts
    when it has more than ten pulses (:348), the next event needs six.  ``events`` is the list of peak times so far."""

    def __init__(self, convention: str = "cpp", *, snr_threshold_db: float = 20.0, bit_width: int = 12,
                 capacity: int = 1 << 20):
        if convention not in CONVENTIONS:
            raise ValueError(f"convention must be one of {sorted(CONVENTIONS)}")
        self.convention = convention
        self.snr_threshold_db = snr_threshold_db
        self.bit_width = bit_width
        self.capacity = capacity
        self.events: list[float] = []
        self.next_event_time: float | None = None
        self.saturated = False

    def update(self, iq, fs: float, fc: float, t0: float):
        """One dwell.  Returns (t_peak, snr_peak) of the event found in it, or None (gated out, or no maximum);
        next_event_time is then None too, as the C++ loop clears it (:234).  pdws and stats of the dwell stay in
        last_pdws / last_stats."""
        cpp = self.convention == "cpp"
        pdws, stats = analyze_dwell(iq, fs, fc, t0, statistic="mean" if cpp else "median", bit_width=self.bit_width,
                                    snr_threshold_db=self.snr_threshold_db, skip_freq=cpp, capacity=self.capacity)
        self.last_pdws, self.last_stats = pdws, stats
        self.saturated = stats.any_pulse_saturated   # cpp:339
        self.next_event_time = None
        gate = len(pdws) > 10 if cpp else stats.peak_mag > 0.9
        fit = fit_event(pdws) if gate and len(pdws) >= 3 else None
        if fit is None:
            return None
        t_peak, snr_peak, _ = fit
        self.events.append(t_peak)
        self.next_event_time = next_event(self.events, self.convention)
        return t_peak, snr_peak

    def gain_step_db(self) -> float:
        """The C++ loop's gain control (:211-214): drop the receive gain by 1 dB after a dwell with a saturated pulse."""
        return -1.0 if self.saturated else 0.0

    def capture_start(self, dwell_duration: float):
        """When to start the next dwell so that the predicted event sits in its middle (:233), None = now (:239)."""
        return None if self.next_event_time is None or not math.isfinite(self.next_event_time) \
            else self.next_event_time - dwell_duration / 2
