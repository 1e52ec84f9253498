"""The three PDW entry points (pfb_pdw_extract, pfb_pdw_extract_raw, pfb_dwell_analyze) share one grow-only pair of
scratch arenas per device.  Five calls of different kinds and sizes -- the smallest that reach each path: the sampled
bracket needs F >= 8 * kSampleRows, the raw digit prediction n >= 2^22 --

  A  raw          int16, n = 40 * 512 + 37, host memory                    (staging)
  B  channelized  M = 8, F = 8 * 65536 + 300, device memory                (sampled bracket: noise-floor path 1)
  C  channelized  M = 65, F = 4096 + 37, channel-major, host memory        (full select: path 2; transpose, staging)
  D  dwell MEAN   int8, n = 2^22 + 5, a device pointer offset by 2 bytes   (one sample per load in every pass)
  E  dwell MEDIAN complex64, n = 2^22 + 12345, host memory                 (digit prediction; staging)

run each alone on a released workspace, where A, B, C are held to the oracle as tests/test_gpu_pdw_branches.py holds
its cases and D, E to tests/dwell_ref.py as tests/test_gpu_dwell.py does; then A B C D E A C B E D with no release in
between must return, call by call, the bytes of the run alone: PDWs, count, noise floors, path number, dwell figures.

What this cannot see: a layout that reserves less than its buffers take by under the arena's 1/8 growth slack.  The
layout is written once and measured by running it (pfb_pdw_scratch.hpp, arena_layout), which rules that out by
construction; this test guards the reuse, regrow and staging paths around it."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import dwell_ref  # noqa: E402
import pdw_cases as pc  # noqa: E402
from gpu_support import cuda_torch  # noqa: E402
from pdw_checks import FC, FS, check_case, check_mean, threshold_db  # noqa: E402
from sdr_channelizer_amd import _lib as L, analyze_dwell  # noqa: E402
from sdr_channelizer_amd.pdw import extract_pdws, extract_pdws_raw  # noqa: E402

ORDER = "ABCDEACBED"


def release():
    assert L.load().pfb_pdw_release_workspace(-1) == L.PFB_OK


def chan_case(name, M, F, seed, pulses_of):
    y, _ = pc._chan_background(F, M, seed)
    pulses = []
    for c in range(M):
        for a, jj in pulses_of(c):
            pc._chan_pulse(y, pulses, c, a, pc._tone(jj - a, 0.5))
    pc._chan_pulse(y, pulses, M // 2, F - 20, pc._tone(20, 0.5), terminated=False)   # still active at the end: no PDW
    return pc._chan_case(name, y, pulses)


def case_b():
    """edges at tile and word boundaries plus family C's staggered offsets, spread over the whole matrix"""
    F = 8 * 65536 + 300

    def pulses_of(c):
        o1, o2 = pc._stagger(c)
        for k in range(6):
            a = pc.kTile * (100 + 150 * k + 11 * c) + o1
            yield a, a + 64 * (2 + k) + o2 - o1
        yield F - 5000 + 300 * c, F - 4900 + 300 * c + o2
    return chan_case("workspace-B", 8, F, 501, pulses_of)


def case_c():
    def pulses_of(c):
        o1, o2 = pc._stagger(c)
        yield 64 * (2 + c % 3) + o1, 64 * (4 + c % 3) + o2
        t = 1 + c % 6
        yield pc.kTile * t + o1, pc.kTile * (t + 1) + o2
    return chan_case("workspace-C", 65, 4096 + 37, 502, pulses_of)


def long_raw(n, source, seed):
    s = pc._Raw(n, source, seed)
    s.pulse(0, pc._tone(30, 0.5))
    for a in range(40000, n - 5000, 262139):
        s.pulse(a, pc.body("distinct", 900 + a % 700, s.rng, s.integer_full))
    s.pulse(n - 40, pc._tone(39, 0.5))
    return s.case(f"workspace-{source}-{n}")


class Calls:
    def __init__(self, torch):
        self.a = pc.edges_raw("terminated")
        assert len(self.a.data) == 40 * 512 + 37 and self.a.data.dtype == np.int16
        self.b = case_b()
        self.b_dev = torch.from_numpy(self.b.data).cuda()
        self.c = case_c()
        self.c_cm = np.ascontiguousarray(self.c.data.T)          # MATLAB's own layout
        d = long_raw((1 << 22) + 6, "int8", 503)
        self.d_dev = torch.from_numpy(d.data).cuda()[1:]
        assert self.d_dev.data_ptr() % 16 == 2 and len(self.d_dev) == (1 << 22) + 5
        self.d_host = d.data[1:]
        self.d_db = threshold_db(self.d_host, 8)
        self.e = long_raw((1 << 22) + 12345, "cf32", 504)

    def run(self, name):
        """everything the call returns, as bytes and plain numbers"""
        lib = L.load()
        if name == "A":
            a = self.a.args
            got, nf = extract_pdws_raw(self.a.data, a["fs"], a["fc"], a["t0"], bit_width=a["bit_width"],
                                       snr_threshold_db=a["snr_db"], trailing_threshold_db=a["trail_db"], return_noise_floor=True)
            return got, (nf,)
        if name in "BC":
            case, y = (self.b, self.b_dev) if name == "B" else (self.c, self.c_cm)
            a = case.args
            got, nf = extract_pdws(y, a["fs_in"], a["fc"], a["t0"], snr_threshold_db=a["snr_db"], matlab_quirks=a["matlab_quirks"],
                                   return_noise_floor=True, channel_major=name == "C")
            return got, (nf.tobytes(), lib.pfb_pdw_last_noise_floor_path())
        if name == "D":
            got, stats = analyze_dwell(self.d_dev, FS, FC, 0.0, statistic="mean", bit_width=8, snr_threshold_db=self.d_db)
            return got, (stats,)
        a = self.e.args
        got, stats = analyze_dwell(self.e.data, a["fs"], a["fc"], a["t0"], statistic="median", snr_threshold_db=a["snr_db"])
        return got, (stats,)


@pytest.fixture(scope="module")
def calls():
    return Calls(cuda_torch())


@pytest.fixture(scope="module")
def alone(calls):
    """every call on a workspace released just before it"""
    res = {}
    for name in "ABCDE":
        release()
        res[name] = calls.run(name)
    release()
    return res


def test_raw_alone_matches_the_oracle(oracle, calls, alone):
    got, (nf,) = alone["A"]
    check_case(calls.a, got, nf, *pc.run_oracle(oracle, calls.a))


@pytest.mark.parametrize("name,path", [("B", 1), ("C", 2)])
def test_channelized_alone_matches_the_oracle(oracle, calls, alone, name, path):
    got, (nf, took) = alone[name]
    assert took == path
    case = calls.b if name == "B" else calls.c
    check_case(case, got, np.frombuffer(nf, np.float64), *pc.run_oracle(oracle, case))


def test_dwell_mean_alone_matches_the_reference(calls, alone):
    got, (stats,) = alone["D"]
    check_mean(got, stats, calls.d_host, 8, calls.d_db, min_pulses=15)


def test_dwell_median_alone_is_the_raw_extractor_and_the_reference(calls, alone):
    """MEDIAN is pfb_pdw_extract_raw with equal thresholds, bit for bit (tests/test_gpu_dwell.py), and its edges are
    those of the reference's median"""
    got, (stats,) = alone["E"]
    a = calls.e.args
    want, nf = extract_pdws_raw(calls.e.data, a["fs"], a["fc"], a["t0"], snr_threshold_db=a["snr_db"],
                                trailing_threshold_db=a["snr_db"], return_noise_floor=True)
    release()
    assert len(want) == calls.e.count and got.tobytes() == want.tobytes()
    assert stats.noise_floor == nf and stats.threshold == nf * 10.0 ** (a["snr_db"] / 10.0) and stats.pulses == len(want)
    ws = dwell_ref.stats(calls.e.data, a["bit_width"])
    assert stats.peak_mag == ws["peak_mag"] and stats.saturated_components == ws["saturated_components"]
    ref = dwell_ref.analyze(calls.e.data, a["fs"], a["fc"], a["t0"], statistic="median", snr_threshold_db=a["snr_db"])
    assert stats.noise_floor == pytest.approx(ref["noise_floor"], rel=1e-14)
    assert [(0, int(i0), int(j - i0 + 1)) for i0, j in zip(ref["i0"], ref["j"])] == calls.e.pulses


def test_alternating_calls_on_one_workspace_repeat_their_bytes(calls, alone):
    release()
    try:
        for step, name in enumerate(ORDER):
            got, rest = calls.run(name)
            want, want_rest = alone[name]
            assert len(got) == len(want) and got.tobytes() == want.tobytes(), (step, name)
            assert rest == want_rest, (step, name, rest, want_rest)
    finally:
        release()
