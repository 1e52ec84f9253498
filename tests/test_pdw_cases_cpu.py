"""The designs of tests/pdw_cases.py, proven with the oracle alone (no GPU): the oracle's restatement of
create_pdws.m / create_pdws_channelized.m finds exactly the designed pulses on every designed input, the tie structures
are what they claim to be, no phase step sits on the +-180 degree wrap, and the kernel constants the lengths were chosen
around are still the ones in pfb_pdw.hip and its headers.  tests/test_gpu_pdw_branches.py then holds the library to the same
answers."""
import os
import re

import numpy as np
import pytest

import pdw_cases as pc


def check_design(oracle, case):
    """the designed (column, toa0, n) triples are exactly the oracle's pulses; returns the oracle's PDWs"""
    want, _ = pc.run_oracle(oracle, case)
    assert pc.triples(want, case.fs) == case.pulses
    assert len(want) == case.count == len(case.pulses)
    return want


def phase_source(case):
    x = case.normalised()
    if case.kind == "raw":
        return lambda c: x
    return lambda c: x[:, 0 if case.args["matlab_quirks"] else c]


def check_no_antipodal_steps(case):
    """compare() is called without phase_col, so no pulse may hold a phase step within 1e-9 of +-180 degrees"""
    col = phase_source(case)
    for c, a, n in case.pulses:
        d = pc.phase_steps(col(c)[a:a + n])
        assert np.abs(np.abs(d) - 180.0).min() > 1e-6, (case.name, c, a, n)


def check_two_level(case, want):
    """numpy's sort of the float64 magnitudes: the upper middle value is the smallest member of its tie group, the lower
    middle a different value; the oracle's amplitude is their mean (even n) or the upper one (odd n)"""
    x = case.normalised()
    for (c, a, n), p in zip(case.pulses, want):
        mags = np.sort(np.abs(x[a:a + n] if case.kind == "raw" else x[a:a + n, c]))
        hi, lo = mags[n // 2], mags[n // 2 - 1]
        assert lo < hi, (case.name, n)
        assert mags[-1] == hi                      # the tie group is everything from the upper middle up
        if n >= 4:
            assert mags[1] == lo and mags[0] < lo  # the lower group, above the one background sample
        assert p["mag"] == pytest.approx(hi if n & 1 else 0.5 * (lo + hi), rel=1e-15)


def test_kernel_constants_are_the_ones_designed_around():
    csrc = os.path.join(os.path.dirname(__file__), "..", "sdr_channelizer_amd", "csrc")
    src = open(os.path.join(csrc, "pfb_pdw.hip")).read()   # the umbrella, then the stage headers it includes
    src += "".join(open(os.path.join(csrc, h)).read() for h in re.findall(r'^#include "(pfb_(?:pdw_\w+|dwell)\.hpp)"', src, re.M))
    for name in ("kTile", "kPulseCache", "kPulseCacheRaw", "kCountingMedian", "kUndecided"):
        m = re.search(r"constexpr\s+int\s+" + name + r"\s*=\s*([^;]+);", src)
        assert m, name
        expr = m.group(1).strip()
        assert re.fullmatch(r"[0-9<\s]+", expr), (name, expr)
        assert eval(expr) == getattr(pc, name), (name, expr)
    # the lengths of family A straddle every threshold between two routes
    for edge, lengths in ((pc.kCountingMedian, pc.CHAN_LENGTHS), (pc.kPulseCache, pc.CHAN_LENGTHS),
                          (pc.kCountingMedian, pc.RAW_LENGTHS), (pc.kPulseCacheRaw, pc.RAW_LENGTHS)):
        assert {edge, edge + 1, edge + 2} <= set(lengths)


def test_tile_lengths_of_the_designed_streams():
    """every small stream scans 512-sample tiles; the two long int8 streams of family D take 32- and 64-word tiles"""
    assert pc.tile_words_for(40 * pc.kTile + 37, 1) == 8 and pc.tile_words_for(pc.kTile * 9216 + 300, 1) == 8
    assert pc.tile_words_for(pc.kTile * 578 + 37, 33) == 8
    assert pc.tile_words_for((1 << 25) - 777, 1) == 32 and pc.tile_words_for((1 << 26) - 999, 1) == 64
    assert pc.tile_words_for((1 << 26) + 12345, 1) == 128      # test_gpu_pdw.py::test_raw_stream_long_tiles


def test_median_routes_change_where_designed():
    assert pc.median_route("raw", 512) == ("counting", "counting")
    assert pc.median_route("raw", 513) == ("select_cached", "counting")
    assert pc.median_route("raw", 514) == ("select_cached", "select_cached")
    assert pc.median_route("raw", 7168) == ("select_cached", "select_cached")
    assert pc.median_route("raw", 7169) == ("select", "select")
    assert pc.median_route("chan", 512) == ("counting", "counting")
    assert pc.median_route("chan", 513) == ("select", "select")


@pytest.mark.parametrize("source", list(pc.RAW_SOURCES))
@pytest.mark.parametrize("structure", pc.STRUCTURES)
def test_raw_median_route_designs(oracle, structure, source):
    case = pc.median_routes_raw(structure, source)
    want = check_design(oracle, case)
    assert [n for _, _, n in case.pulses] == list(pc.RAW_LENGTHS)
    check_no_antipodal_steps(case)
    assert not any(p["sat"] for p in want)
    if structure.startswith("two_level"):
        check_two_level(case, want)
    x = case.normalised()
    if structure == "constant":
        for _, a, n in case.pulses:
            assert len(set(x[a:a + n - 1])) == 1 and (pc.phase_steps(x[a:a + n - 1]) == 0.0).all()
    if structure == "narrow":     # as closely packed as the format allows: 2^-20 relative, or +-1 LSB (and rounding) near full scale
        full = pc.RAW_SOURCES[source]["full"]
        for _, a, n in case.pulses:
            mags = np.abs(x[a:a + n - 1])
            if source == "cf32":
                # (thousands of float32 pairs inside a 2^-20 window: a few land on the same float64 magnitude)
                assert len(np.unique(mags)) >= 0.999 * (n - 1) and mags.max() / mags.min() - 1.0 < 2.0 ** -19
            else:
                assert np.abs(mags - 0.95).max() * full < 1.0 + 2.0 ** -0.5 + 1e-9
    if structure == "distinct" and source == "cf32":
        assert all(len(np.unique(np.abs(x[a:a + n - 1]))) == n - 1 for _, a, n in case.pulses)


@pytest.mark.parametrize("quirks", [False, True])
@pytest.mark.parametrize("structure", pc.STRUCTURES)
def test_channelized_median_route_designs(oracle, structure, quirks):
    case = pc.median_routes_chan(structure, quirks)
    want = check_design(oracle, case)
    assert sorted(n for _, _, n in case.pulses) == sorted(pc.CHAN_LENGTHS)
    assert {c for c, _, _ in case.pulses} == {0, 1, 2}
    check_no_antipodal_steps(case)
    assert not any(p["sat"] for p in want)
    if structure.startswith("two_level"):
        check_two_level(case, want)
    if structure in ("distinct", "narrow"):
        x = case.normalised()
        for c, a, n in case.pulses:
            mags = np.abs(x[a:a + n - 1, c])
            assert len(np.unique(mags)) == n - 1
            if structure == "narrow":
                assert mags.max() / mags.min() - 1.0 < 2.0 ** -19


@pytest.mark.parametrize("build", [pc.saturation_raw, pc.saturation_chan])
def test_saturation_designs(oracle, build):
    case = build()
    want = check_design(oracle, case)
    check_no_antipodal_steps(case)
    assert [int(p["sat"]) for p in want] == case.facts["sat"]
    assert sorted(case.facts["sat"]) == [0] + [1] * 7 and all(n == pc.SAT_N for _, _, n in case.pulses)


@pytest.mark.parametrize("end,count", [("terminated", 12), ("unterminated", 11)])
def test_raw_edge_designs(oracle, end, count):
    case = pc.edges_raw(end)
    check_design(oracle, case)
    check_no_antipodal_steps(case)
    assert case.count == count and len(case.data) % 64 != 0
    starts = {a for _, a, _ in case.pulses}
    ends = {a + n - 1 for _, a, n in case.pulses}
    for o in range(-2, 3):
        for edges in (starts, ends):
            assert any((e - o) % 64 == 0 and (e - o) % pc.kTile != 0 for e in edges), o
            assert any((e - o) % pc.kTile == 0 and e > 2 for e in edges), o
    assert 0 in starts
    assert (len(case.data) - 1 in ends) == (end == "terminated")


@pytest.mark.parametrize("entered,count", [("active", 2 + len(pc.PLATEAU_LENGTHS)), ("inactive", 2)])
def test_raw_plateau_designs(oracle, entered, count):
    case = pc.plateaus_raw(entered)
    want, nf = pc.run_oracle(oracle, case)
    assert pc.triples(want, case.fs) == case.pulses and len(want) == count == case.count
    check_no_antipodal_steps(case)
    # the plateau level lies strictly inside the band, the background below it
    a = case.args
    lead, trail = nf * 10.0 ** (a["snr_db"] / 10.0), nf * 10.0 ** (a["trail_db"] / 10.0)
    mag = np.abs(case.normalised())
    band = (mag > trail) & (mag < lead)
    assert band.sum() == sum(pc.PLATEAU_LENGTHS)
    level = case.facts["level"]
    assert trail < 0.9 * level and 1.1 * level < lead
    if entered == "active":
        assert [n - 21 for _, _, n in case.pulses[1:-1]] == list(pc.PLATEAU_LENGTHS)


@pytest.mark.parametrize("M", [1, 33, 64, 65])
def test_channelized_edge_designs(oracle, M):
    case = pc.edges_chan(M)
    check_design(oracle, case)
    check_no_antipodal_steps(case)
    assert case.count == 2 * M and case.data.shape == (pc.kTile * 6 + 37, M)
    mid = M // 2                                     # the unterminated pulse: strong to the last frame, no PDW
    assert (np.abs(case.data[-20:, mid]) > 0.4).all()
    assert all(a + n <= case.data.shape[0] - 20 for c, a, n in case.pulses if c == mid)


def test_raw_segment_design(oracle):
    case = pc.segments_raw()
    want, nf = pc.run_oracle(oracle, case)
    assert pc.triples(want, case.fs) == case.pulses and len(want) == case.count == 3
    n = len(case.data)
    assert (n + pc.kTile - 1) // pc.kTile == 9217 and -(-9217 // 1024) == 10
    wave = 64 * 10 * pc.kTile
    assert wave == 327680
    a = case.args
    lead, trail = nf * 10.0 ** (a["snr_db"] / 10.0), nf * 10.0 ** (a["trail_db"] / 10.0)
    mag = np.abs(case.normalised())
    band = (mag > trail) & (mag < lead)
    assert band[wave - 2000:wave + 2000].all()                                   # in band across the wave boundary
    seg = 10 * pc.kTile
    assert band[seg * 100 - 50:seg * 102 + 50].all() and band[seg * 300 - 50:seg * 302 + 50].all()
    assert band.sum() == 4000 + 2 * (2 * seg + 100)
    assert (mag[-500:] >= lead).all()                                            # still active at the end
    assert pc.median_route("raw", case.pulses[2][2])[0] == "select"


def test_channelized_segment_design(oracle):
    case = pc.segments_chan()
    check_design(oracle, case)
    F, M = case.data.shape
    assert (F + pc.kTile - 1) // pc.kTile == 579 and -(-579 // 64) == 10 and M >= 32
    assert case.count == 3 * M


def test_path4_design():
    """the builder's medians are the columns' medians, and more samples than the undecided list holds lie within 1 % of
    the thresholds (the sampled bracket cannot be narrower than that: rank +-642 of 65 536 samples is about +-1.4 % in
    magnitude for this data)"""
    case = pc.path4()
    mag = np.abs(case.normalised())
    assert np.array_equal(case.facts["med"], np.median(mag, axis=0))
    thr = case.facts["gain"] * case.facts["med"]
    near = np.abs(mag / thr - 1.0) <= 0.01
    assert near.sum() > pc.kUndecided
    assert (mag[near] > thr[np.nonzero(near)[1]]).all()       # every one of them above its threshold: inside the pulse
    assert case.data.shape[0] >= 8 * 65536
