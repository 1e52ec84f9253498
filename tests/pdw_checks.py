"""The checks the PDW and dwell tests share: PDWs against the oracle's (compare; check_case for a design of
tests/pdw_cases.py), a pfb_dwell_analyze MEAN result against tests/dwell_ref.py (check_mean; its bounds are derived in
tests/test_gpu_dwell.py's header), and the synthetic channelized matrix.  Plain numpy, imported by basename."""
import math

import numpy as np
import pytest

import dwell_ref
import pdw_cases as pc

EPS = 2.0 ** -52
FS, FC = pc.FS_RAW, pc.FC


def compare(got, want, fs, phase_col=None):
    """phase_col(i) -> the complex samples pulse i's phase steps are taken over: lets the caller's data excuse the one
    ill-conditioned point of the reference algorithm (see antipodal_slack)."""
    assert len(got) == len(want), (len(got), len(want))
    w = {k: np.array([p[k] for p in want]) for k in ("toa", "freq", "pw", "snr", "sat", "bin")}
    assert np.array_equal(got["bin"], w["bin"])
    assert np.array_equal(got["sat"] != 0, w["sat"].astype(bool))
    assert np.allclose(got["toa"], w["toa"], rtol=0, atol=1e-9 / fs + 1e-12 * np.abs(w["toa"]).max(initial=1.0))
    assert np.allclose(got["pw"], w["pw"], rtol=1e-12, atol=0)
    assert np.allclose(got["snr"], w["snr"], rtol=1e-9, atol=1e-9, equal_nan=True)
    bad = ~np.isclose(got["freq"], w["freq"], rtol=1e-9, atol=1e-6, equal_nan=True)
    if phase_col is not None:
        for i in np.flatnonzero(bad):
            bad[i] = not antipodal_slack(phase_col(i), float(got["freq"][i]), float(w["freq"][i]), fs)
    assert not bad.any(), (np.flatnonzero(bad), got["freq"][bad], w["freq"][bad])
    assert np.allclose(got["mag"], np.array([p["mag"] for p in want]), rtol=1e-12, atol=0)


def check_case(case, got, nf, want, want_nf):
    """PDWs and noise floor(s) the library returned for a designed case against the oracle's and the designed pulses."""
    if case.kind == "raw":
        assert nf == pytest.approx(want_nf, rel=1e-14)
    else:
        assert np.allclose(nf, want_nf, rtol=1e-12, atol=0)
    assert len(got) == case.count, (len(got), case.count)
    compare(got, want, case.fs)
    assert pc.triples(got, case.fs) == case.pulses


def antipodal_slack(col, got_freq, want_freq, fs):
    """create_pdws_channelized.m:114-117 wraps each phase step at +-180 degrees and takes the median.  Two consecutive
    samples that are exact negative multiples of each other (quantised data has them) step by 180 +- 1 ulp, so the
    last bit of atan2 decides between +180 and -180 there; the device's libm, this host's (the oracle) and numpy's all
    differ in that bit (so would MATLAB's).  Every assignment of +-180 to those steps gives one legitimate median:
    accept a device result whose distance from the oracle's is the distance between two of them, and nothing else."""
    c = np.asarray(col, np.complex128)
    d = np.diff(np.arctan2(c.imag, c.real) * (180.0 / np.pi))
    anti = np.flatnonzero(np.abs(np.abs(d) - 180.0) < 1e-9)
    if len(anti) == 0:
        return False
    d[d < -180.0] += 360.0
    d[d > 180.0] -= 360.0
    delta = 360.0 * (got_freq - want_freq) / fs   # freq = base + fs * med / 360
    tol = 360.0 * (1e-9 * abs(want_freq) + 1e-6) / fs
    if len(anti) > 10:  # too many assignments to list: the median is monotone in every step, so bound it
        lo, hi = d.copy(), d.copy()
        lo[anti], hi[anti] = -180.0, 180.0
        return abs(delta) <= np.median(hi) - np.median(lo) + tol
    meds = []
    for bits in range(1 << len(anti)):
        e = d.copy()
        e[anti] = [180.0 if (bits >> j) & 1 else -180.0 for j in range(len(anti))]
        meds.append(np.median(e))
    meds = np.array(meds)
    return bool((np.abs((meds[:, None] - meds[None, :]) - delta) <= tol).any())


def synthetic_matrix(F=6000, M=16, seed=0):
    rng = np.random.default_rng(seed)
    y = 0.01 * (rng.standard_normal((F, M)) + 1j * rng.standard_normal((F, M)))
    def pulse(b, a, n, amp=0.5, dphi=25.0):
        y[a:a + n, b] += amp * np.exp(1j * np.deg2rad(dphi) * np.arange(n))
    pulse(3, 100, 51)
    pulse(3, 400, 7, dphi=-140.0)        # wraps past +-180 degrees
    pulse(3, 500, 1)                     # single-frame pulse
    pulse(5, 480, 80)                    # crosses the 512-frame tile boundary
    pulse(5, 1000, 1500, amp=0.3)        # longer than the LDS cache, crosses several tiles
    pulse(0, 2000, 40, amp=1.2)          # saturates (|re| or |im| >= 0.9999 inside)
    pulse(M - 1, 0, 30)                  # starts on the very first frame
    pulse(M - 1, F - 20, 20)             # still active at the end of the data: no PDW
    pulse(9, 3000, 64); pulse(9, 3064 + 1, 10)  # one-frame gap between pulses
    return y.astype(np.complex64)


def threshold_db(data, bit_width, level=0.15):
    """the snr_threshold_db that puts the MEAN threshold near `level`, to a tenth of a dB"""
    return round(10.0 * math.log10(level / dwell_ref.stats(data, bit_width)["mean_mag"]), 1)


def check_mean(got, stats, data, bit_width, snr_db, fs=FS, fc=FC, t0=0.0, skip_freq=False, min_pulses=0, sat_fraction=0.98):
    """(pdws, stats) of a MEAN call against the reference on the same samples; returns the reference"""
    want = dwell_ref.analyze(data, fs, fc, t0, statistic="mean", bit_width=bit_width, snr_threshold_db=snr_db,
                             skip_freq=skip_freq)
    ws = dwell_ref.stats(data, bit_width, sat_fraction)
    n = want["n"]
    assert want["clearance"] >= 1e-9, want["clearance"]       # a condition on the input
    assert len(want["i0"]) >= min_pulses
    rel = (n + 4) * EPS
    print(f"n={n} pulses={stats.pulses} nf={stats.noise_floor!r} want={want['noise_floor']!r} "
          f"rel={abs(stats.noise_floor / want['noise_floor'] - 1) if want['noise_floor'] else 0:.3g} bound={rel:.3g}")
    assert stats.num_samples == n and stats.pulses == len(want["i0"])
    assert stats.peak_mag == ws["peak_mag"] and stats.peak_component == ws["peak_component"]
    assert stats.saturated_components == ws["saturated_components"]
    assert abs(stats.noise_floor - want["noise_floor"]) <= rel * want["noise_floor"]
    assert abs(stats.mean_mag - ws["mean_mag"]) <= rel * ws["mean_mag"] and stats.noise_floor == stats.mean_mag
    assert abs(stats.threshold - want["threshold"]) <= 2 * rel * want["threshold"]
    k = len(got)
    assert k == min(stats.pulses, k)
    i0 = np.rint((got["toa"] - t0) * fs).astype(np.int64)
    j = i0 + np.rint(got["pw"] * fs).astype(np.int64)
    assert np.array_equal(i0, want["i0"][:k]) and np.array_equal(j, want["j"][:k])
    assert np.array_equal(got["sat"], want["sat"][:k]) and (got["bin"] == 0).all()
    assert stats.any_pulse_saturated == bool(want["sat"][:k].any())
    assert np.allclose(got["toa"], want["toa"][:k], rtol=0, atol=1e-9 / fs + 1e-12 * abs(t0))
    assert np.allclose(got["pw"], want["pw"][:k], rtol=1e-12, atol=0)
    m = (want["j"] - want["i0"])[:k]
    mag_err = np.abs(got["mag"] - want["mag"][:k])
    assert (mag_err <= (m + 4) * EPS * want["mag"][:k]).all(), (mag_err / want["mag"][:k]).max()
    snr_err = np.abs(got["snr"] - want["snr"][:k])
    snr_bound = (20.0 / math.log(10.0)) * rel
    finite = np.isfinite(want["snr"][:k])
    print(f"snr err max={snr_err[finite].max(initial=0.0):.3g} bound={snr_bound:.3g}  "
          f"mag rel err max={(mag_err / np.maximum(want['mag'][:k], 1e-300)).max(initial=0.0):.3g}")
    assert (snr_err[finite] <= snr_bound).all(), snr_err[finite].max()
    assert np.array_equal(np.isnan(got["snr"]), np.isnan(want["snr"][:k]))
    if skip_freq:
        assert np.isnan(got["freq"]).all()
    else:
        bad = ~np.isclose(got["freq"], want["freq"][:k], rtol=1e-9, atol=1e-6, equal_nan=True)
        re, im = dwell_ref.components(data, bit_width)
        for i in np.flatnonzero(bad):
            col = re[i0[i]:j[i] + 1] + 1j * im[i0[i]:j[i] + 1]
            bad[i] = not antipodal_slack(col, float(got["freq"][i]), float(want["freq"][i]), fs)
        assert not bad.any(), (np.flatnonzero(bad), got["freq"][bad], want["freq"][:k][bad])
    return want
