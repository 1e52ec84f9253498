"""Dwell analysis and event prediction without a GPU: the ABI's new section is declared and exported, pfb_dwell_analyze
and pfb_dwell_from_iq_file check their arguments before they look for a device, the host-only fit and next-event rule
match numpy, and tests/dwell_ref.py -- the reference the GPU tests compare with -- is itself checked on streams small
enough to work out by hand."""
import ctypes as C
import math
import os

import numpy as np
import pytest

import dwell_ref
import sdr_channelizer_amd as pkg
from abi_symbols import declared_symbols
from sdr_channelizer_amd import _lib as L
from sdr_channelizer_amd.pdw import PDW_DTYPE

NEW = ("pfb_dwell_analyze", "pfb_dwell_from_iq_file", "pfb_event_fit", "pfb_event_next")


def test_header_declares_and_library_exports_the_new_functions():
    lib = L.load()
    declared = declared_symbols()
    for name in NEW:
        assert name in declared and name in L.EXPORTS and hasattr(lib, name), name
    assert lib.pfb_abi_version() == 2                      # additive change
    assert C.sizeof(L.PfbDwellConfig) == 72 and C.sizeof(L.PfbDwellStats) == 72
    for name in ("analyze_dwell", "dwell_from_iq_file", "fit_event", "next_event", "EventPredictor"):
        assert hasattr(pkg, name), name


def dwell_config(**kw):
    d = dict(struct_size=C.sizeof(L.PfbDwellConfig), sample_format=L.PFB_FMT_INT16_IQ, bit_width=12,
             statistic=L.PFB_DWELL_STAT_MEAN, flags=0, mem=L.PFB_MEM_HOST, device_id=-1, fs=56e6, fc=915e6,
             sample_start_time=0.0, snr_threshold_db=20.0, sat_fraction=0.98)
    d.update(kw)
    return L.PfbDwellConfig(**d)


BAD_CONFIGS = [dict(struct_size=64), dict(bit_width=0), dict(bit_width=17), dict(sample_format=3), dict(statistic=2),
               dict(flags=2), dict(mem=2), dict(sat_fraction=-0.1), dict(sat_fraction=1.5), dict(sat_fraction=math.nan),
               dict(fs=math.inf), dict(fs=math.nan), dict(snr_threshold_db=math.nan), dict(snr_threshold_db=math.inf),
               dict(snr_threshold_db=4000.0)]   # 10^400 is not finite


def test_dwell_analyze_validates_before_it_looks_for_a_device():
    lib = L.load()
    iq = np.zeros((16, 2), np.int16)
    out = np.zeros(4, PDW_DTYPE)
    count, stats = C.c_uint64(), L.PfbDwellStats()
    p_iq, p_out = C.c_void_p(iq.ctypes.data), out.ctypes.data_as(C.POINTER(L.PfbPdw))

    def call(cfg, iq=p_iq, n=16, out=p_out, cap=4, count=C.byref(count), stats=C.byref(stats)):
        return lib.pfb_dwell_analyze(cfg, iq, n, out, cap, count, stats, None)

    good = dwell_config()
    assert call(None) == L.PFB_ERR_BAD_ARG
    assert call(C.byref(good), iq=None) == L.PFB_ERR_BAD_ARG
    assert call(C.byref(good), count=None) == L.PFB_ERR_BAD_ARG
    assert call(C.byref(good), stats=None) == L.PFB_ERR_BAD_ARG
    assert call(C.byref(good), out=None) == L.PFB_ERR_BAD_ARG          # capacity 4 needs somewhere to write
    assert call(C.byref(good), n=1) == L.PFB_ERR_BAD_ARG and call(C.byref(good), n=0) == L.PFB_ERR_BAD_ARG
    for kw in BAD_CONFIGS:
        assert call(C.byref(dwell_config(**kw))) == L.PFB_ERR_BAD_ARG, kw
    # a bit width is only read for the integer formats; sat_fraction's ends are legal
    ok = [good, dwell_config(sample_format=L.PFB_FMT_CF32, bit_width=0), dwell_config(sat_fraction=0.0),
          dwell_config(sat_fraction=1.0), dwell_config(statistic=L.PFB_DWELL_STAT_MEDIAN, flags=L.PFB_DWELL_SKIP_FREQ)]
    if lib.pfb_device_count() == 0:
        for cfg in ok:
            assert call(C.byref(cfg)) == L.PFB_ERR_NO_DEVICE
        assert call(C.byref(good), out=None, cap=0) == L.PFB_ERR_NO_DEVICE
        with pytest.raises(pkg.PfbError) as e:
            pkg.analyze_dwell(iq, 56e6, 915e6, 0.0)
        assert e.value.status == L.PFB_ERR_NO_DEVICE


def test_dwell_from_iq_file_validates_before_it_looks_for_a_device(tmp_path):
    lib = L.load()
    out = np.zeros(4, PDW_DTYPE)
    count, stats, info = C.c_uint64(), L.PfbDwellStats(), L.PfbIqInfo()
    p_out = out.ctypes.data_as(C.POINTER(L.PfbPdw))
    path = os.path.join(tmp_path, "no_such_record.iq").encode()
    good = dwell_config()
    f = lib.pfb_dwell_from_iq_file
    assert f(None, C.byref(good), p_out, 4, C.byref(count), C.byref(stats), C.byref(info)) == L.PFB_ERR_BAD_ARG
    assert f(path, None, p_out, 4, C.byref(count), C.byref(stats), C.byref(info)) == L.PFB_ERR_BAD_ARG
    assert f(path, C.byref(good), None, 4, C.byref(count), C.byref(stats), C.byref(info)) == L.PFB_ERR_BAD_ARG
    assert f(path, C.byref(good), p_out, 4, None, C.byref(stats), C.byref(info)) == L.PFB_ERR_BAD_ARG
    assert f(path, C.byref(good), p_out, 4, C.byref(count), None, C.byref(info)) == L.PFB_ERR_BAD_ARG
    for kw in (dict(struct_size=8), dict(statistic=7), dict(flags=4), dict(sat_fraction=2.0), dict(snr_threshold_db=math.nan)):
        assert f(path, C.byref(dwell_config(**kw)), p_out, 4, C.byref(count), C.byref(stats), None) == L.PFB_ERR_BAD_ARG, kw
    if lib.pfb_device_count() == 0:
        # format, bit width, fs and mem are the record's: the config's are not looked at
        for cfg in (good, dwell_config(sample_format=9, bit_width=99, fs=math.nan, mem=5)):
            assert f(path, C.byref(cfg), p_out, 4, C.byref(count), C.byref(stats), None) == L.PFB_ERR_NO_DEVICE


# ---- pfb_event_fit ---------------------------------------------------------------------------------------------------

def pdws_of(toa, snr):
    a = np.zeros(len(toa), PDW_DTYPE)
    a["toa"], a["snr"] = toa, snr
    return a


def fit_raw(a):
    t, s, coef = C.c_double(), C.c_double(), (C.c_double * 3)()
    rc = L.load().pfb_event_fit(a.ctypes.data_as(C.POINTER(L.PfbPdw)), len(a), C.byref(t), C.byref(s), coef)
    return rc, t.value, s.value, np.array(coef[:])


def polyfit_on_centred(toa, snr):
    """numpy's least squares on the abscissae the library uses; the design's conditioning is part of the test"""
    tau = np.asarray(toa) - toa[0]
    V = np.vander(tau, 3, increasing=True)
    assert np.linalg.cond(V) < 1e4
    p2, p1, p0 = np.polyfit(tau, snr, 2)
    return np.array([p0, p1, p2])


def check_fit(toa, snr):
    rc, t_peak, snr_peak, coef = fit_raw(pdws_of(toa, snr))
    want = polyfit_on_centred(toa, snr)
    span = toa.max() - toa.min()
    print("coef", coef, "numpy", want, "t_peak", t_peak)
    assert np.allclose(coef, want, rtol=1e-9, atol=0)
    want_peak = toa[0] - want[1] / (2 * want[2])
    assert abs(t_peak - want_peak) <= 1e-9 * span
    tau = t_peak - toa[0]
    assert snr_peak == pytest.approx(want[0] + want[1] * tau + want[2] * tau * tau, rel=1e-9)
    return rc, t_peak, snr_peak, coef


def test_event_fit_matches_polyfit():
    rng = np.random.default_rng(5)
    toa = np.sort(rng.uniform(0.0, 2.0, 40))
    # an exact parabola is recovered to rounding
    snr = 30.0 - 4.0 * (toa - 1.1) ** 2
    rc, t_peak, snr_peak, coef = check_fit(toa, snr)
    assert rc == L.PFB_OK and t_peak == pytest.approx(1.1, abs=1e-12) and snr_peak == pytest.approx(30.0, abs=1e-12)
    assert coef[2] == pytest.approx(-4.0, rel=1e-12)
    # noisy concave data
    rc, t_noisy, _, _ = check_fit(toa, snr + 0.3 * rng.standard_normal(40))
    assert rc == L.PFB_OK and abs(t_noisy - 1.1) < 0.2
    # UTC seconds: the same peak, moved by the offset (the fit runs on toa - toa[0]; 1.7e9 + toa rounds toa to 2.4e-7 s)
    off = 1.7e9
    rc, t_off, snr_off, _ = check_fit(toa + off, snr)
    assert rc == L.PFB_OK and abs((t_off - off) - 1.1) < 1e-6 and snr_off == pytest.approx(30.0, abs=1e-6)
    # three points: the interpolating parabola
    rc, t3, s3, c3 = check_fit(np.array([0.0, 1.0, 2.0]), np.array([1.0, 3.0, 1.0]))
    assert rc == L.PFB_OK and t3 == pytest.approx(1.0, abs=1e-12) and s3 == pytest.approx(3.0, abs=1e-12)
    # a parabola that opens upwards has no peak: PFB_ERR_UNSUPPORTED, coefficients still reported
    rc, _, _, cu = check_fit(toa, 10.0 + 2.0 * (toa - 0.7) ** 2)
    assert rc == L.PFB_ERR_UNSUPPORTED and cu[2] == pytest.approx(2.0, rel=1e-9)
    assert pkg.fit_event(pdws_of(toa, 10.0 + 2.0 * (toa - 0.7) ** 2)) is None
    # degenerate abscissae and too few points
    assert fit_raw(pdws_of(np.full(5, 3.0), np.arange(5.0)))[0] == L.PFB_ERR_UNSUPPORTED
    assert fit_raw(pdws_of(np.array([0.0, 1.0]), np.array([1.0, 2.0])))[0] == L.PFB_ERR_BAD_ARG
    t = C.c_double()
    assert L.load().pfb_event_fit(None, 5, C.byref(t), C.byref(t), (C.c_double * 3)()) == L.PFB_ERR_BAD_ARG
    t_peak, snr_peak, coef = pkg.fit_event(pdws_of(toa, snr))
    assert t_peak == pytest.approx(1.1, abs=1e-12) and len(coef) == 3


# ---- pfb_event_next --------------------------------------------------------------------------------------------------

def test_event_next_in_both_conventions():
    ev = [10.0, 14.0, 19.0, 21.0, 28.0, 30.0, 39.0]          # diffs 4 5 2 7 2 9
    # MATLAB (predict_event.m:134-138): from two events on, median() of the differences
    assert pkg.next_event(ev[:0]) is None and pkg.next_event(ev[:1]) is None
    assert pkg.next_event(ev[:2]) == 14.0 + 4.0                # one difference
    assert pkg.next_event(ev[:3]) == 19.0 + 4.5                # even count: mean of the middle two
    assert pkg.next_event(ev[:4]) == 21.0 + 4.0                # odd count
    assert pkg.next_event(ev) == 39.0 + 4.5                    # sorted 2 2 4 5 7 9
    # C++ (usrp_predict_event.cpp:354-372): only with more than five events, sorted[size / 2]
    for k in range(6):
        assert pkg.next_event(ev[:k], "cpp") is None
    assert pkg.next_event(ev[:6], "cpp") == 30.0 + 4.0         # five differences 2 2 4 5 7: sorted[2]
    assert pkg.next_event(ev, "cpp") == 39.0 + 5.0             # six differences: sorted[3], the upper middle
    nxt, have = C.c_double(), C.c_int32()
    t = (C.c_double * 7)(*ev)
    lib = L.load()
    assert lib.pfb_event_next(t, 7, 2, C.byref(nxt), C.byref(have)) == L.PFB_ERR_BAD_ARG
    assert lib.pfb_event_next(None, 7, 0, C.byref(nxt), C.byref(have)) == L.PFB_ERR_BAD_ARG
    assert lib.pfb_event_next(t, 7, 0, None, C.byref(have)) == L.PFB_ERR_BAD_ARG
    assert lib.pfb_event_next(None, 0, 0, C.byref(nxt), C.byref(have)) == L.PFB_OK and have.value == 0


# ---- tests/dwell_ref.py on streams worked out by hand ---------------------------------------------------------------

FS = 4.0   # toa and pw in quarters


def stream12(levels):
    """12 int16 samples at bit width 12 with |x| = levels / 2048 exactly (I = level, Q = 0)"""
    return np.stack([np.array(levels, np.int16), np.zeros(12, np.int16)], axis=1)


def test_dwell_ref_one_sample_wide_pulse_and_the_two_toa_conventions():
    # mean = (11 * 2 + 1000) / 12 = 85.1667 LSB; at 3 dB the threshold is 169.9 LSB: sample 5 alone is above it
    iq = stream12([2, 2, 2, 2, 2, 1000, 2, 2, 2, 2, 2, 2])
    r = dwell_ref.analyze(iq, FS, 0.0, 100.0, statistic="mean", snr_threshold_db=3.0)
    nf = (11 * 2 + 1000) / 12 / 2048
    assert r["noise_floor"] == pytest.approx(nf, rel=1e-15) and r["threshold"] == pytest.approx(nf * 10 ** 0.3, rel=1e-15)
    assert r["i0"].tolist() == [5] and r["j"].tolist() == [6]
    assert r["mag"][0] == 1000 / 2048                          # j = i0 + 1: amp = mag(i0) / 1
    assert r["toa"][0] == 100.0 + 5 / FS                       # 0-based (cpp:321)
    assert r["pw"][0] == 1 / FS and r["sat"][0] == 0
    assert r["snr"][0] == pytest.approx(10 * math.log10((1000 / 2048) / nf), rel=1e-15)
    # the median of the same stream is 2 LSB; threshold 3.99 LSB; same edges, toa one sample later (m:86), amp the
    # median of samples 5 and 6
    m = dwell_ref.analyze(iq, FS, 0.0, 100.0, statistic="median", snr_threshold_db=3.0)
    assert m["noise_floor"] == 2 / 2048 and m["i0"].tolist() == [5] and m["j"].tolist() == [6]
    assert m["toa"][0] == 100.0 + 6 / FS and m["mag"][0] == (1000 + 2) / 2 / 2048


def test_dwell_ref_end_sample_is_not_in_the_mean():
    # pulse 3 .. 6 (600, 800, 700 above; sample 6 = 100 is the trailing one, below the threshold but far above the
    # background): mean = 2209 / 12 = 184.08 LSB, at 1 dB the threshold is 231.7 LSB
    iq = stream12([1, 1, 1, 600, 800, 700, 100, 1, 1, 1, 1, 2])
    r = dwell_ref.analyze(iq, FS, 0.0, 0.0, statistic="mean", snr_threshold_db=1.0)
    assert r["i0"].tolist() == [3] and r["j"].tolist() == [6]
    assert r["mag"][0] == pytest.approx((600 + 800 + 700) / 3 / 2048, rel=1e-15)   # not (.. + 100) / 4
    assert r["pw"][0] == 3 / FS
    assert r["clearance"] > 0.1
    # the literal loop and the closed form agree
    mag = dwell_ref.magnitudes(iq, 12)
    assert dwell_ref.edges_loop(mag, r["threshold"]) == [(3, 6)] == dwell_ref.edges(mag, r["threshold"])


def test_dwell_ref_open_pulse_is_dropped_and_saturation_is_interior():
    # two pulses: 1 .. 4 with full-scale samples at 1 (leading: not counted), 2 (inside: counted); and 9 .. end, open
    iq = stream12([1, 2047, 2047, 1500, 1, 1, 1, 1, 1, 1800, 1800, 1800])
    iq[1, 1] = -2048                                            # Q of the leading sample at -full scale
    r = dwell_ref.analyze(iq, FS, 0.0, 0.0, statistic="mean", snr_threshold_db=0.5)
    assert r["i0"].tolist() == [1] and r["j"].tolist() == [4]   # the pulse from 9 on never ends: no PDW
    assert r["sat"].tolist() == [0]                             # 2047 / 2048 = 0.99951 < 0.9999 inside, -2048 only on the edge
    iq[2, 1] = -2048
    r = dwell_ref.analyze(iq, FS, 0.0, 0.0, statistic="mean", snr_threshold_db=0.5)
    assert r["i0"].tolist() == [1] and r["j"].tolist() == [4] and r["sat"].tolist() == [1]
    s = dwell_ref.stats(iq, 12)
    # 0.98 limits at 12 bits: c <= -2007.04 or c >= 2006.06 -- the two 2047s and the two -2048s
    assert s["saturated_components"] == 4 and s["peak_component"] == 1.0
    assert s["peak_mag"] == math.sqrt(2047 ** 2 + 2048 ** 2) / 2048
    assert s["mean_mag"] == pytest.approx(r["noise_floor"], rel=1e-15)


def test_dwell_ref_loop_and_closed_form_agree_on_random_streams():
    rng = np.random.default_rng(9)
    for trial in range(50):
        mag = rng.integers(0, 6, size=200).astype(np.float64)
        thr = float(rng.integers(1, 5)) + (0.5 if trial % 2 else 0.0)   # every other trial has samples on the threshold
        assert dwell_ref.edges(mag, thr) == dwell_ref.edges_loop(mag, thr)
        s = np.concatenate([[False], mag > thr])
        if not (mag == thr).any():
            assert len(dwell_ref.edges(mag, thr)) == np.count_nonzero(~s[1:] & s[:-1])
    # silence: threshold 0, every sample both starts and ends a pulse (0 >= 0, 0 <= 0)
    assert dwell_ref.edges(np.zeros(10), 0.0) == [(0, 1), (2, 3), (4, 5), (6, 7), (8, 9)]
