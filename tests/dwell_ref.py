"""Float64 numpy restatement of the two dwell loops pfb_dwell_analyze replaces (plain numpy, no GPU):

  MEAN    cpp/usrp_predict_event.cpp:287-343 -- the live loop; arithmetic in float64 (the source's float32
          cwiseAbs()/mean() is not reproduced, as include/pfb_channelizer.h says), the means by math.fsum
  MEDIAN  matlab/predict_event.m:64-121

and of the figures of pfb_dwell_stats.  |x| is sqrt(I^2 + Q^2) * 2^-(bit_width-1) with I^2 + Q^2 exact (an integer, or
one rounding of an exact float64 sum for complex64 data), so max |x| and every comparison with the threshold are exact
statements about the data.  `analyze` walks the edge automaton in closed form where no |x| equals the threshold and
sample by sample (edges_loop, the literal loop of both sources) where one does."""
from __future__ import annotations

import math

import numpy as np

SAMP_MAX = 0.9999   # predict_event.m:118, usrp_predict_event.cpp:336


def components(iq, bit_width: int):
    """(re, im) of x = (I + jQ) / 2^(bit_width-1) as float64 (predict_event.m:48-51); complex64 data as is"""
    a = np.asarray(iq)
    if a.dtype == np.complex64:
        return a.real.astype(np.float64), a.imag.astype(np.float64)
    full = float(2 ** (bit_width - 1))
    return a[:, 0].astype(np.float64) / full, a[:, 1].astype(np.float64) / full


def magnitudes(iq, bit_width: int) -> np.ndarray:
    a = np.asarray(iq)
    if a.dtype == np.complex64:
        re, im = components(a, bit_width)
        return np.sqrt(re * re + im * im)
    i, q = a[:, 0].astype(np.int64), a[:, 1].astype(np.int64)
    return np.sqrt((i * i + q * q).astype(np.float64)) / float(2 ** (bit_width - 1))


def edges_loop(mag: np.ndarray, thr: float):
    """the loop of both sources (m:73-83, cpp:301-318): 0-based (leading, trailing) sample of every finished pulse"""
    pulses, active, toa = [], False, 0
    for jj in range(len(mag)):
        if not active:
            if mag[jj] >= thr:
                active, toa = True, jj
        elif mag[jj] <= thr:
            active = False
            pulses.append((toa, jj))
    return pulses


def edges(mag: np.ndarray, thr: float):
    if (mag == thr).any() or not np.isfinite(thr):
        return edges_loop(mag, thr)
    s = np.concatenate([[False], mag > thr, ])       # state after every sample, inactive in front of the first
    lead = np.flatnonzero(s[1:] & ~s[:-1])
    trail = np.flatnonzero(~s[1:] & s[:-1])
    return list(zip(lead[:len(trail)].tolist(), trail.tolist()))   # a pulse still active at the end gives none


def clearance(mag: np.ndarray, thr: float) -> float:
    """the smallest relative distance of any |x| from the threshold: the designs of tests/test_gpu_dwell.py keep it
    above 1e-9, so that no rounding of the noise floor can move an edge"""
    return float(np.min(np.abs(mag - thr)) / thr) if thr > 0 else 0.0


def phase_step_median(re: np.ndarray, im: np.ndarray) -> float:
    """m:102-105: median of the phase steps (degrees) wrapped into [-180, 180]"""
    d = np.diff(np.arctan2(im, re) * (180.0 / np.pi))
    d[d < -180.0] += 360.0
    d[d > 180.0] -= 360.0
    return float(np.median(d))


def stats(iq, bit_width: int, sat_fraction: float = 0.98) -> dict:
    """pfb_dwell_stats' data figures.  saturated_components: the gain finders' test on the raw integers, in double
    (usrp_find_max_unsaturated_gain.cpp:146, blade_find_max_unsaturated_gain.cpp:268); +-sat_fraction for complex64"""
    a = np.asarray(iq)
    re, im = components(a, bit_width)
    mag = magnitudes(a, bit_width)
    if a.dtype == np.complex64:
        c = np.concatenate([re, im])
        lo, hi = -sat_fraction, sat_fraction
    else:
        full = float(2 ** (bit_width - 1))
        c = a.astype(np.float64).ravel()
        lo, hi = sat_fraction * -full, sat_fraction * (full - 1.0)
    return dict(num_samples=len(mag), saturated_components=int(np.count_nonzero((c <= lo) | (c >= hi))),
                mean_mag=math.fsum(mag) / len(mag), peak_mag=float(mag.max()),
                peak_component=float(max(np.abs(re).max(), np.abs(im).max())))


def analyze(iq, fs: float, fc: float, t0: float, *, statistic: str = "mean", bit_width: int = 12,
            snr_threshold_db: float = 20.0, skip_freq: bool = False) -> dict:
    """noise floor, threshold and the PDW fields as arrays (i0, j: the 0-based leading and trailing sample)"""
    re, im = components(iq, bit_width)
    mag = magnitudes(iq, bit_width)
    n = len(mag)
    nf = math.fsum(mag) / n if statistic == "mean" else float(np.median(mag))   # cpp:288-289 / m:64
    thr = nf * 10.0 ** (snr_threshold_db / 10.0)                                # cpp:291 / m:66
    out = {k: [] for k in ("i0", "j", "toa", "pw", "snr", "mag", "sat", "freq")}
    for i0, j in edges(mag, thr):
        if statistic == "mean":
            amp = math.fsum(mag[i0:j]) / (j - i0)      # cpp:311 amp = mag(toa), :334 += mag(jj), :325 /= (jj - toa)
            toa = i0 / fs + t0                         # cpp:321 (0-based)
        else:
            amp = float(np.median(mag[i0:j + 1]))      # m:89
            toa = (i0 + 1) / fs + t0                   # m:86 (1-based)
        inside = slice(i0 + 1, j)                      # m:117-120, cpp:332-340: neither edge sample
        sat = bool(((np.abs(re[inside]) >= SAMP_MAX) | (np.abs(im[inside]) >= SAMP_MAX)).any())
        if statistic == "mean" and skip_freq:
            freq = math.nan
        else:
            med = phase_step_median(re[i0:j + 1], im[i0:j + 1])   # m:102-105
            with np.errstate(divide="ignore"):
                freq = float(fc + fs / (np.float64(360.0) / med))  # m:110
        with np.errstate(divide="ignore", invalid="ignore"):
            snr = float(10.0 * np.log10(np.float64(amp) / nf))     # m:93, cpp:329
        for k, v in zip(out, (i0, j, toa, (j - i0) / fs, snr, amp, int(sat), freq)):
            out[k].append(v)
    res = {k: np.array(v, dtype=np.int64 if k in ("i0", "j", "sat") else np.float64) for k, v in out.items()}
    res.update(noise_floor=nf, threshold=thr, clearance=clearance(mag, thr), n=n)
    return res
