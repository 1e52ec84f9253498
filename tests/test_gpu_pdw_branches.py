"""The data-dependent branches of the PDW extractors (sdr_channelizer_amd/csrc/pfb_pdw.hip, pfb_pdw_*.hpp) on data
designed to land on them -- tests/pdw_cases.py, whose designs tests/test_pdw_cases_cpu.py proves with the oracle alone:

  A  per-pulse medians: pulse lengths on either side of kCountingMedian, kPulseCache and kPulseCacheRaw, with distinct,
     constant, two-level (both tie branches of block_median) and narrowly packed values, every source format
  B  the saturation scan: one saturated sample on the edge sample (not counted) and at chosen offsets inside
  C  the edge scan: edges round the 64-sample word and the 512-sample tile, in-band plateaus (the scan's identity)
     of a sample to several tiles, entered active and inactive, first / last sample, ragged lengths, several M
  D  the scan's segmentation: thread segments with unrolled group and remainder, empty threads, the wave boundary,
     identity over whole segments; tile_words 32 and 64 (the first wave-per-tile size)
  E  noise-floor path 4: the undecided list overflows and the device redoes the masks
  F  wide banks, short: family C's channelized edges at M = 128 .. 1024 (tests/test_gpu_pdw_wide.py)
  G  wide banks, long: the sampled-bracket route at M = 128 .. 1024 on an (F, 9) base expanded to M columns, the
     oracle's answer mapped from its run on the base (tests/test_gpu_pdw_wide.py)

Everything is an exact integer outcome or goes through pdw_checks.py's compare, unchanged and without phase_col."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import pdw_cases as pc  # noqa: E402
from pdw_checks import check_case, compare  # noqa: E402
from sdr_channelizer_amd import _lib as L, synth  # noqa: E402
from sdr_channelizer_amd.pdw import extract_pdws, extract_pdws_raw  # noqa: E402

_WANT = {}   # the oracle's answer per case, computed once and shared by the host- and device-input runs


def oracle_of(oracle, case):
    if case.name not in _WANT:
        _WANT[case.name] = pc.run_oracle(oracle, case)
    return _WANT[case.name]


def run_library(case, where):
    data = case.data
    if where == "device":
        import torch
        data = torch.from_numpy(case.data).cuda()
    a = case.args
    if case.kind == "raw":
        return extract_pdws_raw(data, a["fs"], a["fc"], a["t0"], bit_width=a["bit_width"], snr_threshold_db=a["snr_db"],
                                trailing_threshold_db=a["trail_db"], return_noise_floor=True)
    return extract_pdws(data, a["fs_in"], a["fc"], a["t0"], snr_threshold_db=a["snr_db"],
                        matlab_quirks=a["matlab_quirks"], return_noise_floor=True)


def check(oracle, case, where):
    got, nf = run_library(case, where)
    check_case(case, got, nf, *oracle_of(oracle, case))
    return got


def check_exact_fields(case, got):
    """constant and two-level pulses: nothing saturates, the column is the designed one and pw * fs + 1 is the designed n"""
    assert not got["sat"].any()
    assert [int(b) for b in got["bin"]] == [c for c, _, _ in case.pulses]
    samples = got["pw"] * case.fs
    assert np.abs(samples - np.rint(samples)).max() < 1e-6
    assert [int(s) + 1 for s in np.rint(samples)] == [n for _, _, n in case.pulses]


# ---- A: per-pulse median routes ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("where", ["host", "device"])
@pytest.mark.parametrize("source", list(pc.RAW_SOURCES))
@pytest.mark.parametrize("structure", pc.STRUCTURES)
def test_raw_median_routes(oracle, structure, source, where):
    """pulses of 2 .. 9002 samples in one stream: counting median, select over the LDS cache (from n = 513 for the
    magnitudes, n = 514 for the phase steps) and select over memory (from n = 7169)"""
    case = pc.median_routes_raw(structure, source)
    got = check(oracle, case, where)
    if structure != "distinct" and structure != "narrow":
        check_exact_fields(case, got)


@pytest.mark.parametrize("where", ["host", "device"])
@pytest.mark.parametrize("quirks", [False, True])
@pytest.mark.parametrize("structure", pc.STRUCTURES)
def test_channelized_median_routes(oracle, structure, quirks, where):
    """pulses of 2 .. 2050 frames over three columns: counting median up to 512 frames, select over memory beyond (at
    n = 513 its phase steps are exactly kCountingMedian: no digit pass, the bucket is the whole scratch)"""
    case = pc.median_routes_chan(structure, quirks)
    got = check(oracle, case, where)
    if structure != "distinct" and structure != "narrow":
        check_exact_fields(case, got)


# ---- B: saturation position ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("build", [pc.saturation_raw, pc.saturation_chan])
def test_saturated_sample_position(oracle, build):
    """one saturated sample per 1200-sample pulse: on the edge sample it does not count (the scripts take the other
    branch there), at offsets 1, 63, 64, 511, 512, 513 and n - 2 it does"""
    case = build()
    got = check(oracle, case, "device")
    assert [int(s != 0) for s in got["sat"]] == case.facts["sat"]


# ---- C: edge-scan boundaries -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("where", ["host", "device"])
@pytest.mark.parametrize("end", ["terminated", "unterminated"])
def test_raw_edges_at_word_and_tile_boundaries(oracle, end, where):
    check(oracle, pc.edges_raw(end), where)


@pytest.mark.parametrize("where", ["host", "device"])
@pytest.mark.parametrize("entered", ["active", "inactive"])
def test_raw_in_band_plateaus(oracle, entered, where):
    """stretches between the trailing and the leading threshold keep whatever state they are entered in: words, tiles
    and whole runs of tiles whose transition function is the identity"""
    check(oracle, pc.plateaus_raw(entered), where)


@pytest.mark.parametrize("where", ["host", "device"])
@pytest.mark.parametrize("M", [1, 33, 64, 65])
def test_channelized_edges_staggered_over_columns(oracle, M, where):
    check(oracle, pc.edges_chan(M), where)


# ---- D: scan segmentation --------------------------------------------------------------------------------------------

def test_raw_scan_segments(oracle):
    """9217 tiles on 1024 threads: ten tiles per thread (a group of 8 and a remainder of 2), empty trailing threads, an
    in-band plateau across the first wave boundary and over two whole thread segments, entered active and inactive"""
    case = pc.segments_raw()
    try:
        check(oracle, case, "device")
    finally:
        L.load().pfb_pdw_release_workspace(-1)


def test_channelized_scan_segments(oracle):
    """579 tiles on one wave per column (M = 33): ten tiles per thread, the last thread's segment short and ragged"""
    case = pc.segments_chan()
    try:
        check(oracle, case, "device")
    finally:
        L.load().pfb_pdw_release_workspace(-1)
        pc.segments_chan.cache_clear()
        _WANT.pop(case.name, None)


@pytest.mark.parametrize("n,tile_words", [((1 << 25) - 777, 32), ((1 << 26) - 999, 64)])
def test_raw_int8_tile_words_32_and_64(oracle, n, tile_words):
    """the pulse train of synth.pulsed_iq_torch as int8, thresholds 4 dB / 2 dB as in test_raw_stream_long_tiles: tiles of
    32 words (a thread per tile) and of 64 (the first size handed to a wave per tile)"""
    import torch
    assert pc.tile_words_for(n, 1) == tile_words
    iq = synth.pulsed_iq_torch(n, 8, dtype=torch.int8, device="cuda")
    try:
        got, nf = extract_pdws_raw(iq, 56e6, 915e6, 0.0, bit_width=8, snr_threshold_db=4.0, trailing_threshold_db=2.0,
                                   return_noise_floor=True)
        h = iq.cpu().numpy()
        del iq
        x = (h[:, 0].astype(np.float64) + 1j * h[:, 1].astype(np.float64)) / 128.0
        want, want_nf = oracle.extract_pdws_raw(x, 56e6, 915e6, 0.0, snr_db=4.0, trail_db=2.0, max_out=1 << 18)
        assert nf == pytest.approx(want_nf, rel=1e-14)
        assert len(want) >= 10000          # the train's pulses (one per ms) and the noise's short detections
        compare(got, want, 56e6)
    finally:
        L.load().pfb_pdw_release_workspace(-1)


# ---- E: noise-floor path 4 -------------------------------------------------------------------------------------------

def test_undecided_list_overflow_takes_path_4(oracle):
    """1.2 M samples 0.3 % above their column's threshold (pdw_cases.PATH4_OFFSET: well inside the zone the sampled
    bracket leaves open, about +-1.4 % for this data): more than kUndecided, so flag 4 is raised and pdw_mask_kernel
    redoes the masks on the device; medians exact, PDWs the oracle's"""
    case = pc.path4()
    try:
        got, nf = run_library(case, "device")
        assert L.load().pfb_pdw_last_noise_floor_path() == 4
        assert np.allclose(nf, case.facts["med"], rtol=1e-12, atol=0)
        want, want_nf = pc.run_oracle(oracle, case)
        assert np.allclose(nf, want_nf, rtol=1e-12, atol=0)
        assert len(got) == case.count
        compare(got, want, case.fs)
        assert pc.triples(got, case.fs) == case.pulses
    finally:
        L.load().pfb_pdw_release_workspace(-1)
        pc.path4.cache_clear()
