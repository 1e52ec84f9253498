"""The designs of tests/pdw_cases.py, proven with the oracle alone (no GPU): the oracle's restatement of
create_pdws.m / create_pdws_channelized.m finds exactly the designed pulses on every designed input, the tie structures
are what they claim to be, no phase step sits on the +-180 degree wrap, and the kernel constants the lengths were chosen
around are still the ones in pfb_pdw.hip and its headers; for the wide banks, the rule that maps the oracle's answer on a
narrow base to the wide matrix built from it, and the routes the chosen lengths take.  tests/test_gpu_pdw_branches.py and
tests/test_gpu_pdw_wide.py then hold the library to the same answers."""
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
    for name in ("kTile", "kPulseCache", "kPulseCacheRaw", "kCountingMedian", "kUndecided", "kSampleRows", "kBracketRows"):
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


@pytest.mark.parametrize("M", (1, 33, 64, 65) + pc.WIDE_M)
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


# ---- wide banks: family F is test_channelized_edge_designs at pc.WIDE_M; family G below --------------------------------

def test_routes_of_the_wide_lengths():
    """pfb_pdw_extract's geometry at the lengths of family G, restated from pfb_pdw.hip / pfb_pdw_stage.hpp: the
    sampled route from 8 kSampleRows frames, the tile length, the tiles per column, the scan kernel on either side of
    `M >= 32 && ntiles < 2048`, and the parts per channel of the candidate select"""
    assert pc.WIDE_F1 == 8 * pc.kSampleRows + 300 == 524588 and pc.WIDE_F1 % 64 != 0
    assert all(F >= 8 * pc.kSampleRows for F in pc.WIDE_FS)
    assert [pc.tile_words_for(F, 128) for F in pc.WIDE_FS] == [8, 8, 8, 16]
    assert [-(-F // (64 * pc.tile_words_for(F, 128))) for F in pc.WIDE_FS] == [1025, 2047, 2048, 1025]
    assert [pc.scan_kernel_for(F, 128) for F in pc.WIDE_FS] == ["pdw_tilescan_kernel<64>"] * 2 + \
        ["pdw_tilescan_kernel<1024>", "pdw_tilescan_kernel<64>"]
    assert -(-2047 // 64) == 32                       # tiles per thread of the one-wave scan at F2
    for M in pc.WIDE_M:                               # one tile length for every wide bank: max_tiles is 2048 from M = 128 up
        assert [pc.tile_words_for(F, M) for F in pc.WIDE_FS] == [8, 8, 8, 16]
        assert pc.scan_kernel_for(pc.WIDE_F1, M) == "pdw_tilescan_kernel<64>"

    def parts(F, M):
        stride = F // pc.kSampleRows
        ns = F // stride
        delta = int(np.ceil(2.5 * np.sqrt(ns))) + 2
        expect = int((2 * delta + 1) / ns * F)
        return max(1, min(16, 512 // M + 1, expect // 8192))
    assert [parts(pc.WIDE_F1, M) for M in pc.WIDE_M] == [1] * 5
    assert [parts(F, 128) for F in pc.WIDE_FS] == [1, 2, 2, 2] and parts(pc.WIDE_F4, 560) == 1
    # column groups of 64 and the last one's live lanes: full groups only, and a full group followed by a partial one
    assert [(-(-M // 64), M % 64) for M in pc.WIDE_M] == [(2, 0), (3, 2), (4, 0), (9, 48), (16, 0)]
    assert pc.WIDE_M0 % 2 == 1 and len({(64 * g) % pc.WIDE_M0 for g in range(9)}) == 9   # every group starts on another base column


WIDE_BASES = [(pc.WIDE_F1, False, True), (pc.WIDE_F1, False, False), (pc.WIDE_F1, True, False),
              (pc.WIDE_F2, False, True), (pc.WIDE_F3, False, True), (pc.WIDE_F4, False, True)]


@pytest.mark.parametrize("F,tied,quirks", WIDE_BASES)
def test_wide_base_designs(oracle, F, tied, quirks):
    case = pc.wide_base(F, tied, quirks)
    check_design(oracle, case)
    check_no_antipodal_steps(case)
    M0 = pc.WIDE_M0
    assert case.data.shape == (F, M0) and case.count == 3 * M0 + 2
    T, R = case.facts["T"], case.facts["R"]
    assert T == 64 * pc.tile_words_for(F, 128) and R % pc.kBracketRows == 0 and F - pc.kBracketRows <= R < F
    starts = {(c, a) for c, a, _ in case.pulses}
    ends = {(c, a + n - 1) for c, a, n in case.pulses}
    near = lambda x: (x + T // 2) % T - T // 2         # signed distance from the nearest tile boundary
    tile_offsets = set()
    for c in range(M0):
        per = [(a, a + n - 1) for cc, a, n in case.pulses if cc == c]
        assert sum(e - a for a, e in per) < F // 4
        assert any(e < 64 * 8 for _, e in per)                                        # a) early
        b = [(a, e) for a, e in per if a > T and abs(near(a)) <= 2 and abs(near(e)) <= 2 and abs(e - a - T) <= 4]
        assert len(b) == 1                                                            # b) tile boundary to tile boundary
        tile_offsets.add((near(b[0][0]), near(b[0][1])))
        assert any(a < R < e for a, e in per)                                         # c) across the last row-group boundary
    assert len(tile_offsets) == M0 and all({o[k] for o in tile_offsets} == {-2, -1, 0, 1, 2} for k in (0, 1))
    assert (pc.WIDE_START0, 0) in starts and (pc.WIDE_ENDS_LAST, F - 1) in ends
    mag = np.abs(case.data[-20:, pc.WIDE_OPEN])
    assert (mag > 0.5).all() and all(a + n <= F - 20 for c, a, n in case.pulses if c == pc.WIDE_OPEN)
    nf = np.median(np.abs(case.normalised()), axis=0)
    if tied:   # most magnitudes tied: a handful of values hold the bulk of every column, the median among them
        col = np.abs(case.normalised()[:, 0])
        assert len(np.unique(col[col < 0.1])) < 200 and np.count_nonzero(col == nf[0]) > F // 50
    else:      # neighbouring base columns' floors are further apart than the sampled bracket is wide (about +-1.4 %)
        assert (nf[1:] / nf[:-1] > 1.05).all()


@pytest.mark.parametrize("tied,quirks", [(False, False), (False, True), (True, False)])
def test_widening_rule_with_the_oracle_alone(oracle, tied, quirks):
    """oracle(explicit wide matrix) == widen_expected(oracle(base)): bit-equal but for freq, which moves by one
    reassociated addition at 1e9 Hz (a few ulp: 1e-6 Hz).  Same builder at a small F (the sampled route is the
    library's business, not the oracle's)."""
    F = 6 * pc.kBracketRows + 300
    base = pc.wide_base(F, tied, quirks)
    a, M0 = base.args, pc.WIDE_M0
    want_base, _ = pc.run_oracle(oracle, base)
    assert pc.triples(want_base, base.fs) == base.pulses
    for M in (65, 130, 560):
        wide = oracle.extract_pdws(pc.widen(base.data, M).astype(np.complex128), a["fs_in"], a["fc"], a["t0"], a["snr_db"],
                                   matlab_quirks=quirks, decim=M0)
        mapped = pc.widen_expected(oracle, want_base, M, M0, a["fs_in"])
        assert len(wide) == len(mapped) == len(pc.widen_pulses(base.pulses, M, M0))
        assert pc.triples(wide, base.fs) == pc.widen_pulses(base.pulses, M, M0)
        for k in ("toa", "pw", "snr", "mag", "sat", "bin"):
            assert [p[k] for p in wide] == [p[k] for p in mapped], k
        assert np.abs(np.array([p["freq"] for p in wide]) - np.array([p["freq"] for p in mapped])).max() <= 1e-6
    pc._wide_data.cache_clear()
