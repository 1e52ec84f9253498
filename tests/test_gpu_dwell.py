"""pfb_dwell_analyze on the GPU.  MEDIAN must be pfb_pdw_extract_raw with equal thresholds, bit for bit.  MEAN is
compared with tests/dwell_ref.py (float64, math.fsum) on the same samples:

  exact      pulse count, leading / trailing sample (recovered from toa and pw), sat, peak_mag, peak_component,
             saturated_components -- max and the comparisons are exact statements about I^2 + Q^2
  sums       noise_floor, mean_mag: relative (n + 4) * 2^-52, the worst case of any summation order of n non-negative
             doubles plus one rounding of |x|; a pulse's mag the same with its own length
  snr        (20 / ln 10) * (n + 4) * 2^-52 dB: the same bound through the logarithm, twice (a ratio of two sums)
  freq       as compare of tests/pdw_checks.py holds it (rtol 1e-9, atol 1e-6, the antipodal-step slack)

Every design keeps each |x| at least 1e-9 (relative) away from the threshold, asserted on the reference side, so that
no rounding of the noise floor can move an edge.  The thresholds are chosen from the data (threshold_db: the level
0.15 sits between every background and every pulse sample), since a mean noise floor rises with the duty cycle."""
import dataclasses
import math
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import dwell_ref  # noqa: E402
import pdw_cases as pc  # noqa: E402
from gpu_support import Busy, cuda_torch  # noqa: E402
from pdw_checks import FC, FS, check_mean, threshold_db  # noqa: E402
from sdr_channelizer_amd import EventPredictor, analyze_dwell, dwell_from_iq_file, iqfile  # noqa: E402
from sdr_channelizer_amd.pdw import extract_pdws_raw  # noqa: E402


@pytest.fixture(scope="module")
def torch():
    return cuda_torch()


def to_device(torch, data):
    return torch.from_numpy(np.ascontiguousarray(data)).cuda()


def run_mean(data, bit_width, *, min_pulses=1, **kw):
    snr_db = threshold_db(data if isinstance(data, np.ndarray) else data.cpu().numpy(), bit_width)
    host = data if isinstance(data, np.ndarray) else data.cpu().numpy()
    got, stats = analyze_dwell(data, FS, FC, 0.0, statistic="mean", bit_width=bit_width, snr_threshold_db=snr_db, **kw)
    want = check_mean(got, stats, host, bit_width, snr_db, skip_freq=kw.get("skip_freq", False), min_pulses=min_pulses)
    return got, stats, want, snr_db


# ---- MEDIAN: the raw extractor ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("where", ["host", "device"])
@pytest.mark.parametrize("source", ["int8", "int16_12", "cf32"])
def test_median_is_the_raw_extractor_with_equal_thresholds(torch, source, where):
    case = pc.median_routes_raw("distinct", source)
    a = case.args
    data = case.data if where == "host" else to_device(torch, case.data)
    got, stats = analyze_dwell(data, a["fs"], a["fc"], 1.7e9, statistic="median", bit_width=a["bit_width"],
                               snr_threshold_db=a["snr_db"])
    want, nf = extract_pdws_raw(data, a["fs"], a["fc"], 1.7e9, bit_width=a["bit_width"], snr_threshold_db=a["snr_db"],
                                trailing_threshold_db=a["snr_db"], return_noise_floor=True)
    assert len(want) == case.count and got.tobytes() == want.tobytes()
    assert stats.noise_floor == nf and stats.threshold == nf * 10.0 ** (a["snr_db"] / 10.0) and stats.pulses == len(want)
    ws = dwell_ref.stats(case.data, a["bit_width"])
    assert stats.peak_mag == ws["peak_mag"] and stats.saturated_components == ws["saturated_components"]
    # predict_event.m's toa is 1-based (:86), and skip_freq is a MEAN option: ignored here
    again, _ = analyze_dwell(data, a["fs"], a["fc"], 1.7e9, statistic="median", bit_width=a["bit_width"],
                             snr_threshold_db=a["snr_db"], skip_freq=True)
    assert again.tobytes() == want.tobytes()


# ---- MEAN: lengths, formats, alignment -------------------------------------------------------------------------------

def short_stream(n, source, seed=1):
    """background with, where they fit: a pulse starting on sample 0, a one-sample pulse (j = i0 + 1), a pulse whose
    trailing sample is the last one; n = 2 and 3 hold the one pulse they can"""
    s = pc._Raw(n, source, seed)
    if n == 2:
        s.pulse(0, pc._tone(1, 0.5))
    elif n == 3:
        s.pulse(1, pc._tone(1, 0.5))
    else:
        s.pulse(0, pc._tone(5, 0.45))
        s.pulse(100, pc._tone(1, 0.6))
        s.pulse(150, pc.body("distinct", 40, s.rng, s.integer_full))
        s.pulse(n - 31, pc._tone(30, 0.5))
        for a in range(1000, n - 400, 3001):
            s.pulse(a, pc.body("distinct", 200 + a % 97, s.rng, s.integer_full))
    return s.case(f"short-{n}-{source}")


LENGTHS = (2, 3, 255, 256, 257, 4 * 256 + 1, (1 << 16) + 3)   # 1024: one step of a stats workgroup


@pytest.mark.parametrize("source", list(pc.RAW_SOURCES))
@pytest.mark.parametrize("n", LENGTHS)
def test_mean_matches_the_reference(torch, n, source):
    case = short_stream(n, source)
    bw = case.args["bit_width"]
    got, stats, want, _ = run_mean(case.data, bw)
    assert len(got) == case.count, (len(got), case.pulses)
    dev, _ = analyze_dwell(to_device(torch, case.data), FS, FC, 0.0, bit_width=bw, snr_threshold_db=threshold_db(case.data, bw))
    assert dev.tobytes() == got.tobytes()    # a host buffer is staged at an aligned address: the same route


@pytest.mark.parametrize("offset", [1, 3])
@pytest.mark.parametrize("source", ["int8", "int16_12", "cf32"])
def test_mean_on_a_misaligned_device_pointer(torch, source, offset):
    """a device pointer 1 or 3 samples past a 16-byte boundary: one sample per load in every pass, ragged tail included"""
    case = short_stream((1 << 16) + 3 + offset, source, seed=2)
    d = to_device(torch, case.data)
    assert d.data_ptr() % 16 == 0 and d[offset:].data_ptr() % 16 != 0
    got, stats, want, _ = run_mean(d[offset:], case.args["bit_width"], min_pulses=15)
    host = case.data[offset:]
    aligned, astats = analyze_dwell(host, FS, FC, 0.0, bit_width=case.args["bit_width"],
                                    snr_threshold_db=threshold_db(host, case.args["bit_width"]))
    assert len(aligned) == len(got) and np.array_equal(aligned["toa"], got["toa"]) and astats.peak_mag == stats.peak_mag


@pytest.mark.parametrize("source", ["int16_12", "cf32"])
def test_mean_pulse_lengths_around_the_workgroup_and_the_cache(torch, source):
    """pulses of n = j - i0 + 1 samples around the pulse kernel's 512 threads and its kPulseCacheRaw-sample cache, one
    of 40 000 (many strides per thread, far longer than any cache) and one of 2 (a single sample above the threshold)"""
    lengths = (2, 511, 512, 513, 514, pc.kPulseCacheRaw - 1, pc.kPulseCacheRaw, pc.kPulseCacheRaw + 1,
               pc.kPulseCacheRaw + 2, 40000)
    s = pc._Raw(6 * sum(lengths), source, seed=31)
    cursor = 77
    for n in lengths:
        s.pulse(cursor, pc.body("distinct", n, s.rng, s.integer_full))
        cursor += n + 64 + int(s.rng.integers(0, 150))
    case = s.case(f"lengths-{source}")
    got, stats, want, _ = run_mean(to_device(torch, case.data), case.args["bit_width"])
    assert (want["j"] - want["i0"] + 1).tolist() == list(lengths)
    skip, sstats, _, _ = run_mean(to_device(torch, case.data), case.args["bit_width"], skip_freq=True)
    # SKIP_FREQ: freq is NaN and nothing else moves
    assert np.isnan(skip["freq"]).all() and not np.isnan(got["freq"]).any()
    a, b = got.copy(), skip.copy()
    a["freq"] = b["freq"] = 0.0
    assert a.tobytes() == b.tobytes() and sstats == stats


def test_mean_near_2_22_samples(torch):
    """more chunks than the stats pass has workgroups, so a workgroup takes more than one, and a ragged end"""
    n = (1 << 22) - 5
    s = pc._Raw(n, "int16_12", seed=8)
    for a in range(40000, n - 5000, 131071):
        s.pulse(a, pc.body("distinct", 1500 + a % 1000, s.rng, s.integer_full))
    case = s.case("near-2^22")
    got, stats, want, _ = run_mean(to_device(torch, case.data), 12, min_pulses=30)
    assert len(got) == case.count


@pytest.mark.parametrize("end", ["terminated", "unterminated"])
def test_mean_edges_on_word_and_tile_boundaries(torch, end):
    """tests/pdw_cases.py family C: edges at 64 k + o and 512 k + o, a pulse from sample 0, a last pulse that ends on
    the last sample (one PDW) or is still open there (none)"""
    case = pc.edges_raw(end)
    got, stats, want, _ = run_mean(to_device(torch, case.data), case.args["bit_width"])
    assert [(0, int(a), int(b - a + 1)) for a, b in zip(want["i0"], want["j"])] == case.pulses
    assert want["i0"][0] == 0 and (want["j"][-1] == len(case.data) - 1) == (end == "terminated")


# ---- capacity, silence, saturation -----------------------------------------------------------------------------------

def test_capacity_smaller_than_the_count(torch):
    case = pc.edges_raw("terminated")
    d = to_device(torch, case.data)
    snr_db = threshold_db(case.data, 12)
    full, fstats = analyze_dwell(d, FS, FC, 0.0, snr_threshold_db=snr_db)
    assert len(full) == case.count > 3
    for cap in (0, 3):
        got, stats = analyze_dwell(d, FS, FC, 0.0, snr_threshold_db=snr_db, capacity=cap)
        assert len(got) == cap and got.tobytes() == full[:cap].tobytes()
        assert stats.pulses == case.count
        assert dataclasses.replace(stats, any_pulse_saturated=fstats.any_pulse_saturated) == fstats


@pytest.mark.parametrize("source", ["int16_12", "cf32"])
def test_silence(torch, source):
    """An all-zero dwell: noise floor 0, threshold 0, so every sample both starts (0 >= 0) and ends (0 <= 0) a pulse --
    n / 2 two-sample pulses with NaN snr, as both sources' loops produce and as the raw extractor's silence test
    (tests/test_gpu_pdw.py::test_raw_stream_argument_checks_and_silence) shows; reproduced, not patched.  The distance
    from the threshold is 0 here by construction: 0 == 0 is exact in any arithmetic."""
    n = 1000
    data = np.zeros(n, np.complex64) if source == "cf32" else np.zeros((n, 2), np.int16)
    got, stats = analyze_dwell(data, 1e6, 0.0, 0.0, statistic="mean")
    want = dwell_ref.analyze(data, 1e6, 0.0, 0.0, statistic="mean")
    assert stats.noise_floor == 0.0 and stats.threshold == 0.0 and stats.peak_mag == 0.0 and stats.saturated_components == 0
    assert stats.pulses == len(got) == n // 2 == len(want["i0"])
    assert np.array_equal(np.rint(got["toa"] * 1e6).astype(int), want["i0"]) and np.allclose(got["pw"], 1e-6, rtol=1e-12)
    assert np.isnan(got["snr"]).all() and np.isnan(want["snr"]).all() and not got["sat"].any()
    med, mstats = analyze_dwell(data, 1e6, 0.0, 0.0, statistic="median")
    assert med.tobytes() == extract_pdws_raw(data, 1e6, 0.0, 0.0, snr_threshold_db=20.0, trailing_threshold_db=20.0).tobytes()
    assert mstats.pulses == n // 2 and mstats.noise_floor == 0.0


@pytest.mark.parametrize("sat_fraction", [0.98, 0.5, 1.0])
@pytest.mark.parametrize("source", ["int8", "int16_12", "int16_16", "cf32"])
def test_saturated_components_at_the_limits(torch, source, sat_fraction):
    """components on, one below and one above both of the gain finders' limits sat_fraction * (-full) and
    sat_fraction * (full - 1) (0.5 and 1.0 make them integers; 0.98 does not), +-sat_fraction for complex64"""
    src = pc.RAW_SOURCES[source]
    full = src["full"]
    s = pc._Raw(5000, source, seed=3)
    case = s.case("limits")
    data = case.data.copy()
    if source == "cf32":
        f = np.float32(sat_fraction)
        vals = [np.nextafter(f, np.float32(0)), f, np.nextafter(f, np.float32(2)), np.float32(sat_fraction - 1e-3)]
        vals = np.array(vals + [-v for v in vals], np.float32)
        for k, v in enumerate(vals):
            data[100 + 10 * k] = complex(v, 0.001)
            data[105 + 10 * k] = complex(0.001, v)
    else:
        lo, hi = sat_fraction * -full, sat_fraction * (full - 1)
        vals = sorted({int(v) for L in (lo, hi) for v in (math.floor(L) - 1, math.floor(L), math.ceil(L), math.ceil(L) + 1)
                       if -full <= v <= full - 1})
        for k, v in enumerate(vals):
            data[100 + 10 * k] = (v, 1)
            data[105 + 10 * k] = (-1, v)
    want = dwell_ref.stats(data, src["bit_width"], sat_fraction)
    assert 0 < want["saturated_components"] < 2 * len(vals)
    for where in (data, to_device(torch, data), to_device(torch, data)[1:]):
        host = data if where is data else where.cpu().numpy()
        _, stats = analyze_dwell(where, FS, FC, 0.0, bit_width=src["bit_width"], snr_threshold_db=30.0, sat_fraction=sat_fraction)
        w = dwell_ref.stats(host, src["bit_width"], sat_fraction)
        assert stats.saturated_components == w["saturated_components"]
        assert stats.peak_component == w["peak_component"] and stats.peak_mag == w["peak_mag"]
    # 0 stands for the gain finders' 0.98
    _, s0 = analyze_dwell(data, FS, FC, 0.0, bit_width=src["bit_width"], snr_threshold_db=30.0, sat_fraction=0.0)
    assert s0.saturated_components == dwell_ref.stats(data, src["bit_width"], 0.98)["saturated_components"]


def test_pulse_saturation_is_interior(torch):
    """tests/pdw_cases.py family B: one -full-scale sample per pulse at designed offsets from the leading sample; offset 0
    is the leading sample itself and does not count (cpp:332-340), every other one does"""
    case = pc.saturation_raw()
    got, stats, want, _ = run_mean(to_device(torch, case.data), 12)
    assert got["sat"].tolist() == case.facts["sat"] and stats.any_pulse_saturated
    ep = EventPredictor("cpp", snr_threshold_db=threshold_db(case.data, 12))
    ep.update(to_device(torch, case.data), FS, FC, 0.0)
    assert ep.saturated and ep.gain_step_db() == -1.0        # cpp:211-214


# ---- determinism, streams, files -------------------------------------------------------------------------------------

@pytest.mark.parametrize("source", ["int16_12", "cf32"])
def test_same_buffer_same_bits(torch, source):
    case = short_stream((1 << 20) + 77, source, seed=4)
    d = to_device(torch, case.data)
    snr_db = threshold_db(case.data, case.args["bit_width"])
    runs = [analyze_dwell(d, FS, FC, 0.0, bit_width=case.args["bit_width"], snr_threshold_db=snr_db) for _ in range(3)]
    assert len(runs[0][0]) > 100
    for pdws, stats in runs[1:]:
        assert pdws.tobytes() == runs[0][0].tobytes() and stats == runs[0][1]


def test_dwell_on_a_busy_stream(torch):
    """analyze_dwell on a device tensor while a non-default stream is current and still busy with the kernel that wrote
    the tensor (the pattern of tests/test_gpu_async.py::test_pdw_extraction_on_a_busy_stream)"""
    busy = Busy(torch)
    case = short_stream((1 << 20) + 5, "int16_12", seed=6)
    src = to_device(torch, case.data)
    snr_db = threshold_db(case.data, 12)
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        busy.queue(s)
        iq = src + 0   # written on s, behind the copies
        assert not s.query()
        got, stats = analyze_dwell(iq, FS, FC, 0.0, snr_threshold_db=snr_db)
        busy.queue(s)
        iq2 = src + 0
        assert not s.query()
        med, mstats = analyze_dwell(iq2, FS, FC, 0.0, statistic="median", snr_threshold_db=12.0)
    torch.cuda.synchronize()
    assert torch.equal(iq, src) and torch.equal(iq2, src)
    want, wstats = analyze_dwell(src, FS, FC, 0.0, snr_threshold_db=snr_db)
    wmed, wmstats = analyze_dwell(src, FS, FC, 0.0, statistic="median", snr_threshold_db=12.0)
    assert len(want) > 100 and got.tobytes() == want.tobytes() and stats == wstats
    assert len(wmed) > 100 and med.tobytes() == wmed.tobytes() and mstats == wmstats
    del busy.src, busy.dst
    torch.cuda.empty_cache()


@pytest.mark.parametrize("statistic", ["mean", "median"])
def test_record_to_dwell_in_one_call(tmp_path, statistic):
    """a format-1 record (104-byte header, 16-bit samples, 32-bit frequency 0): the header's values override the call's"""
    case = short_stream(300001, "int16_16", seed=12)
    path = os.path.join(tmp_path, "dwell.iq")
    iqfile.write_iq_fmt1(path, case.data, fs=20e6, start_time=1.7e9 + 0.25)
    snr_db = threshold_db(case.data, 16) if statistic == "mean" else 18.0
    got, stats, info = dwell_from_iq_file(path, statistic=statistic, snr_threshold_db=snr_db)
    assert info.file_format == 1 and info.packet.numSamples == len(case.data) and info.packet.bitWidth == 16
    want, wstats = analyze_dwell(case.data, 20e6, 0.0, 1.7e9 + 0.25, statistic=statistic, bit_width=16, snr_threshold_db=snr_db)
    assert len(want) == case.count and got.tobytes() == want.tobytes() and stats == wstats


# ---- end to end ------------------------------------------------------------------------------------------------------

def event_dwell(k, peak_level, fs=1e6, n=200_000, pri=0.005, width=25, period=1.0, curvature=600.0, seed=0):
    """dwell k of a scan: a pulse every `pri` seconds whose level in dB (10 log10, the scripts' convention) is a parabola
    in time, peak_level at the event and curvature * dt^2 dB below it dt seconds away; the event sits 0.1 s + a known
    offset into the dwell, and events are exactly `period` apart"""
    rng = np.random.default_rng(seed + k)
    t_event = 3.0 + k * period
    t0 = t_event - 0.1 - 0.013 * ((k * 7) % 5 - 2)      # the dwell is not centred the same way every time
    s = pc._Raw(n, "int16_12", seed=100 + k)
    step = int(round(pri * fs))
    for a in range(int(rng.integers(50, 400)), n - width - 2, step):
        dt = t0 + a / fs - t_event
        s.pulse(a, pc._tone(width, peak_level * 10.0 ** (-curvature * dt * dt / 10.0), dphi_deg=35.0))
    return s.case(f"event-{k}").data, t0, t_event


@pytest.mark.parametrize("convention", ["cpp", "matlab"])
def test_event_predictor_recovers_peaks_and_spacing(torch, convention):
    """12 dwells.  The C++ convention gates on more than ten pulses and predicts from the sixth event on, the MATLAB one
    gates on max |x| > 0.9 and predicts from the second; both must place every peak within one PRI and the spacing
    (next event minus the last) within two."""
    fs, pri, period = 1e6, 0.005, 1.0
    ep = EventPredictor(convention, snr_threshold_db=10.0)
    for k in range(12):
        data, t0, t_event = event_dwell(k, 0.95)
        found = ep.update(to_device(torch, data), fs, FC, t0)
        assert found is not None and len(ep.last_pdws) >= 30
        t_peak, snr_peak = found
        print(f"dwell {k}: peak error {t_peak - t_event:+.3e} s, snr {snr_peak:.2f} dB, next {ep.next_event_time}")
        assert abs(t_peak - t_event) < pri
        needs = 6 if convention == "cpp" else 2
        if k + 1 >= needs:
            assert abs(ep.next_event_time - (t_event + period)) < 2 * pri
            assert ep.capture_start(0.2) == ep.next_event_time - 0.1
        else:
            assert ep.next_event_time is None and ep.capture_start(0.2) is None
    assert len(ep.events) == 12 and ep.gain_step_db() == 0.0
    # a quiet dwell is gated out and leaves the events alone
    quiet = pc._Raw(50_000, "int16_12", seed=5).case("quiet").data
    assert ep.update(quiet, fs, FC, 99.0) is None and len(ep.events) == 12 and ep.next_event_time is None
