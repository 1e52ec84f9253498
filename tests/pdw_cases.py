"""Designed inputs for the PDW extractors (plain numpy, no GPU): data built to land on the data-dependent branches of
sdr_channelizer_amd/csrc/pfb_pdw.hip and its stage headers -- the per-pulse median routes (pfb_pdw_pulse.hpp:
pdw_pulse_kernel; pfb_pdw_select.hpp: cached_median, block_median and its two tie branches), the saturation scan, the
identity elements and the word / tile / thread-segment / wave boundaries of the edge scan, the overflow of the undecided
list (noise-floor path 4), and the launch geometry of the channelized extractor on wide banks (pfb_pdw.hip: column
groups of 64 past the second, the scan kernels' switch, 16-word tiles).

Families: A per-pulse median routes, B saturation position, C edge-scan boundaries, D scan segmentation, E noise-floor
path 4 (tests/test_gpu_pdw_branches.py), F wide banks on short matrices and G on long ones (tests/test_gpu_pdw_wide.py).

Every builder returns a Case: the input, the extraction arguments, and the designed facts -- the pulses as
(column, toa0, n) with toa0 the 0-based index of the first sample at or above the leading threshold and
n = jj - toa0 + 1 counting the trailing below-threshold sample jj as the scripts do -- the PDW count and the intended
route.  tests/test_pdw_cases_cpu.py proves the designs with the oracle alone; tests/test_gpu_pdw_branches.py and
tests/test_gpu_pdw_wide.py run them through the library.

Backgrounds.  Raw streams: integer jitter of +-3 LSB per component (+-1 LSB for int8), whose magnitudes take a handful
of values, so the median is one of them whatever the pulses add: 2.83 .. 3.2 LSB (1 .. 1.42 LSB for int8).  The
background's largest magnitude (4.25 LSB, 1.42 for int8) stays below the 3 dB trailing threshold (>= 5.6 LSB, >= 1.99),
every pulse sample (>= 0.3 full scale) far above the leading one, and the in-band plateau levels (40 LSB at 12 bits,
8 LSB at 8 bits) strictly between the two, for every median in that range.  int8 has too little dynamic range for the
script's 18 dB (see test_gpu_pdw.py::test_raw_stream_pdws_match_oracle): its cases run at 12 dB.  Channelized matrices:
Gaussian noise of sigma 0.0015 per component (3 LSB at 12 bits); integer jitter would put exactly antipodal neighbours
into column 1, whose phases create_pdws_channelized.m:114 reads for every pulse, and a phase step of +-180 degrees is
decided by the last bit of atan2.  The sample that ends a designed raw pulse is set to (1, -1) LSB for the same reason.
Every designed stream keeps its pulses below a quarter of the samples, so the median stays a background value."""
from __future__ import annotations

import functools
from dataclasses import dataclass, field

import numpy as np

# constants of sdr_channelizer_amd/csrc/pfb_pdw_select.hpp (tests/test_pdw_cases_cpu.py reads them out of the source and fails
# if they move: the lengths below sit on them)
kTile = 512
kPulseCache = 512
kPulseCacheRaw = 7168
kCountingMedian = 512
kUndecided = 1 << 20
kSampleRows = 65536
kBracketRows = 1024

FS_RAW = 56e6      # create_pdws.m: the recorder's rate
FS_IN = 56e6       # create_pdws_channelized.m: rate before the bank
FC = 915e6
T0 = 0.0           # a start time of 0 leaves toa its sample resolution (compare's atol scales with the largest toa)

CHAN_LENGTHS = (2, 3, 4, 511, 512, 513, 514, 515, 1025, 1026, 2049, 2050)
RAW_LENGTHS = CHAN_LENGTHS + (7167, 7168, 7169, 7170, 9001, 9002)
STRUCTURES = ("distinct", "constant", "two_level_exponent", "two_level_ulp", "narrow")
SAT_OFFSETS = (0, 1, 63, 64, 511, 512, 513, 1198)   # 1198 = n - 2, the last strong sample of an n = 1200 pulse
SAT_N = 1200
PLATEAU_LENGTHS = (1, 63, 64, 65, 512, 1024, 1500)
PLATEAU_OFFSETS = (-2, -1, 0, 1, 2, 63, 65)          # start of each plateau relative to a 512-sample tile boundary

RAW_SOURCES = {
    "int8": dict(dtype=np.int8, bit_width=8, full=128, jitter=1, snr_db=12.0, trail_db=3.0, band=8.0 / 128),
    "int16_12": dict(dtype=np.int16, bit_width=12, full=2048, jitter=3, snr_db=18.0, trail_db=3.0, band=40.0 / 2048),
    "int16_16": dict(dtype=np.int16, bit_width=16, full=32768, jitter=3, snr_db=18.0, trail_db=3.0, band=40.0 / 32768),
    "cf32": dict(dtype=np.complex64, bit_width=12, full=2048, jitter=3, snr_db=18.0, trail_db=3.0, band=40.0 / 2048),
}
CHAN_SIGMA = 0.0015
CHAN_SNR_DB = 15.0


@dataclass
class Case:
    name: str
    kind: str                      # "raw" or "chan"
    data: np.ndarray               # (n, 2) int8 / int16, (n,) complex64, or (F, M) complex64
    args: dict                     # raw: fs, fc, t0, bit_width, snr_db, trail_db; chan: fs_in, fc, t0, snr_db, matlab_quirks
    pulses: list                   # designed (column, toa0, n), in the reference's order (columns outermost, time inside)
    count: int                     # designed PDW count (= len(pulses))
    route: dict = field(default_factory=dict)   # intended route(s), free-form per family
    facts: dict = field(default_factory=dict)   # further designed facts (saturation flags, levels, medians)

    @property
    def fs(self) -> float:
        """rate of the samples the PDWs are timed in"""
        return self.args["fs"] if self.kind == "raw" else self.args["fs_in"] / self.data.shape[1]

    def normalised(self) -> np.ndarray:
        """the complex128 samples the scripts would see"""
        if self.kind == "raw" and self.data.dtype != np.complex64:
            full = float(2 ** (self.args["bit_width"] - 1))
            return (self.data[:, 0].astype(np.float64) + 1j * self.data[:, 1].astype(np.float64)) / full
        return self.data.astype(np.complex128)


def run_oracle(oracle, case: Case, max_out: int = 1 << 16):
    """(pdws, noise floor(s)) of the oracle's restatement of the scripts on the case's data"""
    x = case.normalised()
    a = case.args
    if case.kind == "raw":
        return oracle.extract_pdws_raw(x, a["fs"], a["fc"], a["t0"], snr_db=a["snr_db"], trail_db=a["trail_db"], max_out=max_out)
    want = oracle.extract_pdws(x, a["fs_in"], a["fc"], a["t0"], a["snr_db"], matlab_quirks=a["matlab_quirks"], max_out=max_out)
    return want, np.median(np.abs(x), axis=0)


def triples(pdws, fs: float, t0: float = T0):
    """(column, toa0, n) of PDW records (the oracle's dicts or the library's structured array)"""
    if isinstance(pdws, np.ndarray):
        cols, toa, pw = pdws["bin"], pdws["toa"], pdws["pw"]
    else:
        cols, toa, pw = (np.array([p[k] for p in pdws]) for k in ("bin", "toa", "pw"))
    return [(int(c), int(round((t - t0) * fs)) - 1, int(round(w * fs)) + 1) for c, t, w in zip(cols, toa, pw)]


def median_route(kind: str, n: int):
    """(route of the magnitudes' median, route of the phase steps' median) in pdw_pulse_kernel for a pulse of n samples:
    'counting' = cached_median, 'select_cached' = block_median over the LDS cache, 'select' = block_median over memory"""
    cache = kPulseCacheRaw if kind == "raw" else kPulseCache
    if n > cache:
        return "select", "select"
    one = lambda m: "counting" if m <= kCountingMedian else "select_cached"
    return one(n), one(n - 1)


def tile_words_for(samples: int, M: int) -> int:
    """restates pfb_pdw_stage.hpp's tile_words_for: the tile length of the edge scan, in 64-sample words"""
    w = (samples + 63) // 64
    max_tiles = min(16384, max(2048, (1 << 18) // max(1, M)))
    tw = kTile // 64
    while tw < 1024 and w // tw > max_tiles:
        tw *= 2
    return tw


def phase_steps(col: np.ndarray) -> np.ndarray:
    """the wrapped phase steps (degrees) of create_pdws*.m over consecutive samples"""
    ph = np.arctan2(col.imag, col.real) * (180.0 / np.pi)
    d = np.diff(ph)
    d[d < -180.0] += 360.0
    d[d > 180.0] -= 360.0
    return d


# ---- pulse bodies: the above-threshold samples of a pulse, normalised complex128 ------------------------------------

def _tone(m: int, amp: float, dphi_deg: float = 20.0, phi0_deg: float = 10.0) -> np.ndarray:
    return amp * np.exp(1j * np.deg2rad(phi0_deg + dphi_deg * np.arange(m)))


def _random_phases(rng, m: int) -> np.ndarray:
    return np.deg2rad(np.cumsum(rng.uniform(-170.0, 170.0, m)))


def two_levels(variant: str, integer_full: int | None):
    """A, B with |A| < |B| and different phases.  'exponent': the magnitudes differ in the exponent (they part at the
    first digit of a radix select); 'ulp': in the last representable step -- adjacent integers, or adjacent float32
    values, on one component each -- so they share every digit but the last."""
    if variant == "exponent":
        return 0.35 * np.exp(1j * np.deg2rad(40.0)), 0.7 * np.exp(-1j * np.deg2rad(25.0))
    if integer_full:
        a = integer_full // 2
        return 1j * a / integer_full, (a + 1.0) / integer_full
    return 1j * 0.5, complex(np.nextafter(np.float32(0.5), np.float32(1.0)))


def body(structure: str, n: int, rng, integer_full: int | None) -> np.ndarray:
    """the n - 1 above-threshold samples of a pulse of n samples; integer_full: the integer format's full scale, None
    for complex64 data"""
    m = n - 1
    if structure == "distinct":
        return rng.permutation(np.linspace(0.3, 0.8, m)) * np.exp(1j * _random_phases(rng, m))
    if structure == "constant":
        return np.full(m, 0.5 * np.exp(1j * np.deg2rad(30.0)))
    if structure.startswith("two_level"):
        A, B = two_levels(structure.split("_")[2], integer_full)
        n_a = n // 2 - 1                       # with the background sample below them: B's smallest is the upper middle
        return rng.permutation(np.concatenate([np.full(n_a, A), np.full(m - n_a, B)]))
    if structure == "narrow":
        if integer_full:                       # near full scale, within +-1 LSB in magnitude
            mags = 0.95 + rng.uniform(-1.0, 1.0, m) / integer_full
        else:                                  # within 2^-20 relative
            mags = 0.6 * (1.0 + rng.permutation(np.linspace(0.0, 1.0, m, endpoint=False)) * 2.0 ** -20)
        return mags * np.exp(1j * _random_phases(rng, m))
    raise ValueError(structure)


# ---- raw streams -----------------------------------------------------------------------------------------------------

class _Raw:
    """a raw stream under construction, in LSB units of the source's full scale"""

    def __init__(self, n: int, source: str, seed: int):
        self.src = RAW_SOURCES[source]
        self.source = source
        self.rng = np.random.default_rng(seed)
        j = self.src["jitter"]
        self.q = self.rng.integers(-j, j + 1, size=(n, 2)).astype(np.float64)
        self.pulses = []

    @property
    def integer_full(self):
        return None if self.source == "cf32" else self.src["full"]

    def put(self, a: int, v: np.ndarray):
        full = self.src["full"]
        self.q[a:a + len(v), 0] = v.real * full
        self.q[a:a + len(v), 1] = v.imag * full

    def pulse(self, a: int, v: np.ndarray, terminated: bool = True):
        """samples v from a on; a terminated pulse ends on a (1, -1) LSB sample and is recorded as designed"""
        self.put(a, v)
        if terminated:
            self.q[a + len(v)] = (1.0, -1.0)
            self.pulses.append((0, a, len(v) + 1))

    def case(self, name: str, route=None, facts=None) -> Case:
        s = self.src
        if self.source == "cf32":
            data = ((self.q[:, 0] + 1j * self.q[:, 1]) / s["full"]).astype(np.complex64)
        else:
            lim = s["full"]
            data = np.clip(np.rint(self.q), -lim, lim - 1).astype(s["dtype"])
        args = dict(fs=FS_RAW, fc=FC, t0=T0, bit_width=s["bit_width"], snr_db=s["snr_db"], trail_db=s["trail_db"])
        return Case(name, "raw", data, args, sorted(self.pulses), len(self.pulses), route or {}, facts or {})


@functools.lru_cache(maxsize=None)
def median_routes_raw(structure: str, source: str) -> Case:
    """family A, raw: one pulse of every length in RAW_LENGTHS, quiet gaps of >= 64 samples between them"""
    total = 8 * sum(RAW_LENGTHS) + 1
    s = _Raw(total, source, seed=STRUCTURES.index(structure) * 10 + list(RAW_SOURCES).index(source))
    cursor = 101
    for n in RAW_LENGTHS:
        s.pulse(cursor, body(structure, n, s.rng, s.integer_full))
        cursor += n + 64 + int(s.rng.integers(0, 150))
    assert cursor < total
    return s.case(f"A-raw-{structure}-{source}", {n: median_route("raw", n) for n in RAW_LENGTHS})


@functools.lru_cache(maxsize=None)
def saturation_raw() -> Case:
    """family B, raw int16 at 12 bits: eight n = 1200 pulses, one sample of -full scale each at the given offset from
    toa (the positive end, 2047 / 2048, is below the scripts' 0.9999)"""
    s = _Raw(8 * len(SAT_OFFSETS) * SAT_N + 5, "int16_12", seed=77)
    for i, off in enumerate(SAT_OFFSETS):
        v = _tone(SAT_N - 1, 0.5)
        v[off] = -1.0 + 0.25j
        s.pulse(300 + i * (SAT_N + 200) + 7 * i, v)
    return s.case("B-raw", facts=dict(sat=[int(off > 0) for off in SAT_OFFSETS]))


def _raw_edge_stream(source="int16_12", tiles=40, seed=5):
    return _Raw(tiles * kTile + 37, source, seed)          # a length that is no multiple of 64


@functools.lru_cache(maxsize=None)
def edges_raw(end: str) -> Case:
    """family C, raw int16 at the default 18 dB / 3 dB: leading and trailing edges at 64 k + o and 512 k + o for
    o = -2 .. 2, a pulse starting on sample 0, and a last pulse whose final strong sample is n - 2 ('terminated': it
    ends on n - 1, one PDW) or n - 1 ('unterminated': none)"""
    s = _raw_edge_stream()
    n = len(s.q)
    s.pulse(0, _tone(30, 0.5))
    for i, o in enumerate(range(-2, 3)):
        t = 1 + 3 * i
        a, jj = kTile * t + 128 + o, kTile * (t + 1) + o          # leading edge on a word, trailing edge on a tile boundary
        s.pulse(a, _tone(jj - a, 0.5))
        a, jj = kTile * (t + 2) + o, kTile * (t + 2) + 192 + o    # leading edge on a tile, trailing edge on a word boundary
        s.pulse(a, _tone(jj - a, 0.5))
    if end == "terminated":
        s.pulse(n - 40, _tone(39, 0.5))
    else:
        s.pulse(n - 40, _tone(40, 0.5), terminated=False)
    return s.case(f"C-raw-edges-{end}")


@functools.lru_cache(maxsize=None)
def plateaus_raw(entered: str) -> Case:
    """family C, raw: stretches whose level lies strictly between the trailing and the leading threshold -- the identity
    of the scan -- of every length in PLATEAU_LENGTHS, starting at PLATEAU_OFFSETS from a tile boundary.  'active': ten
    strong samples, the plateau, ten strong samples: the pulse runs through, one PDW covers it.  'inactive': the plateau
    alone between background samples: no pulse (an ordinary pulse before the first and after the last plateau shows
    that the state crosses them unchanged)."""
    s = _raw_edge_stream(seed=6 + (entered == "active"))
    level = s.src["band"]
    s.pulse(50, _tone(100, 0.5))
    cursor = 300
    for L, o in zip(PLATEAU_LENGTHS, PLATEAU_OFFSETS):
        start = kTile * ((cursor + 80 + kTile - 1) // kTile) + o
        if entered == "active":
            s.pulse(start - 10, np.concatenate([_tone(10, 0.5), _tone(L, level), _tone(10, 0.5)]))
        else:
            s.put(start, _tone(L, level))
        cursor = start + L + 12
    s.pulse(cursor + 100, _tone(100, 0.5))
    assert cursor + 300 < len(s.q)
    return s.case(f"C-raw-plateaus-{entered}", facts=dict(level=level))


@functools.lru_cache(maxsize=None)
def segments_raw() -> Case:
    """family D, raw int8, n = 512 * 9216 + 300: 9217 tiles, pdw_tilescan_kernel<1024> with per = 10 tiles per thread
    (one unrolled group of 8, a remainder of 2, threads 922 .. 1023 empty); thread segments are 5120 samples, the
    first wave ends at sample 327 680"""
    n = kTile * 9216 + 300
    s = _Raw(n, "int8", seed=9)
    level, seg, wave = s.src["band"], 10 * kTile, 64 * 10 * kTile
    s.pulse(1000, _tone(300, 0.5))
    # a pulse whose in-band plateau crosses the wave boundary of the scan
    s.pulse(wave - 3000, np.concatenate([_tone(1000, 0.5), _tone(4000, level), _tone(100, 0.5)]))
    # inactive in-band plateau over two whole thread segments: identity functions, state 0 carried through
    s.put(seg * 100 - 50, _tone(2 * seg + 100, level))
    # the same entered active: identity functions, state 1 carried through
    s.pulse(seg * 300 - 150, np.concatenate([_tone(100, 0.5), _tone(2 * seg + 100, level), _tone(100, 0.5)]))
    s.pulse(n - 500, _tone(500, 0.5), terminated=False)   # still active at the end: no PDW
    return s.case("D-raw-segments", dict(tiles=9217, per=10, scan="pdw_tilescan_kernel<1024>"))


# ---- channelized matrices --------------------------------------------------------------------------------------------

def _chan_background(F: int, M: int, seed: int):
    rng = np.random.default_rng(seed)
    y = (CHAN_SIGMA * rng.standard_normal((F, M), dtype=np.float32)).astype(np.complex64)
    y.imag = CHAN_SIGMA * rng.standard_normal((F, M), dtype=np.float32)
    return y, rng


def _chan_case(name, y, pulses, quirks=True, route=None, facts=None) -> Case:
    args = dict(fs_in=FS_IN, fc=FC, t0=T0, snr_db=CHAN_SNR_DB, matlab_quirks=quirks)
    return Case(name, "chan", y, args, sorted(pulses), len(pulses), route or {}, facts or {})


def _chan_pulse(y, pulses, col: int, a: int, v: np.ndarray, terminated: bool = True):
    y[a:a + len(v), col] = v.astype(np.complex64)
    if terminated:
        pulses.append((col, a, len(v) + 1))


@functools.lru_cache(maxsize=None)
def median_routes_chan(structure: str, quirks: bool) -> Case:
    """family A, channelized: M = 3, the lengths of CHAN_LENGTHS dealt over the columns, gaps of >= 64 frames"""
    M = 3
    F = 8 * max(sum(CHAN_LENGTHS[c::M]) for c in range(M)) + 1001
    y, rng = _chan_background(F, M, seed=40 + STRUCTURES.index(structure))
    cursor = [101, 133, 171]
    pulses = []
    for i, n in enumerate(CHAN_LENGTHS):
        c = i % M
        _chan_pulse(y, pulses, c, cursor[c], body(structure, n, rng, None))
        cursor[c] += n + 64 + int(rng.integers(0, 150))
    assert max(cursor) < F
    return _chan_case(f"A-chan-{structure}-{'quirks' if quirks else 'plain'}", y, pulses, quirks,
                      {n: median_route("chan", n) for n in CHAN_LENGTHS})


@functools.lru_cache(maxsize=None)
def saturation_chan() -> Case:
    """family B, channelized: as saturation_raw, the pulses dealt over M = 3 columns (matlab_quirks off)"""
    M = 3
    F = 8 * 3 * SAT_N + 3
    y, _ = _chan_background(F, M, seed=78)
    pulses, sat = [], {}
    for i, off in enumerate(SAT_OFFSETS):
        v = _tone(SAT_N - 1, 0.5)
        v[off] = -1.0 + 0.25j
        c, a = i % M, 300 + (i // M) * (SAT_N + 200) + 7 * i
        _chan_pulse(y, pulses, c, a, v)
        sat[(c, a)] = int(off > 0)
    pulses.sort()
    return _chan_case("B-chan", y, pulses, False, facts=dict(sat=[sat[(c, a)] for c, a, _ in pulses]))


def _stagger(c: int):
    return c % 5 - 2, (c // 5) % 5 - 2     # start and end offsets of column c, staggered separately


@functools.lru_cache(maxsize=None)
def edges_chan(M: int) -> Case:
    """family C, channelized, F = 512 * 6 + 37: column c has a short pulse with its edges at word boundaries and a long
    one with its edges at tile boundaries, each plus (c mod 5 - 2) at the start and ((c div 5) mod 5 - 2) at the end;
    the middle column also holds a pulse still active at the end (no PDW) while later columns have theirs"""
    F = kTile * 6 + 37
    y, _ = _chan_background(F, M, seed=90 + M)
    pulses = []
    for c in range(M):
        o1, o2 = _stagger(c)
        a, jj = 64 * (2 + c % 3) + o1, 64 * (4 + c % 3) + o2
        _chan_pulse(y, pulses, c, a, _tone(jj - a, 0.5))
        t = 1 + c % 4
        a, jj = kTile * t + o1, kTile * (t + 1) + o2
        _chan_pulse(y, pulses, c, a, _tone(jj - a, 0.5))
    _chan_pulse(y, pulses, M // 2, F - 20, _tone(20, 0.5), terminated=False)
    return _chan_case(f"C-chan-edges-M{M}", y, pulses)


@functools.lru_cache(maxsize=None)
def segments_chan() -> Case:
    """family D, channelized, M = 33, F = 512 * 578 + 37: 579 tiles, pdw_tilescan_kernel<64> with per = 10 tiles per
    thread; per column a pulse from one thread-segment boundary to the next, one starting where a thread's unrolled
    group of 8 tiles hands over to its remainder, and one through the last thread's short segment into the ragged
    last tile, with the staggered offsets of family C"""
    M, F = 33, kTile * 578 + 37
    seg = 10 * kTile
    y, _ = _chan_background(F, M, seed=123)
    pulses = []
    for c in range(M):
        o1, o2 = _stagger(c)
        a, jj = seg * (1 + c % 7) + o1, seg * (2 + c % 7) + o2
        _chan_pulse(y, pulses, c, a, _tone(jj - a, 0.5))
        a, jj = seg * 20 + 8 * kTile + o1, seg * 20 + 9 * kTile + o2
        _chan_pulse(y, pulses, c, a, _tone(jj - a, 0.5))
        a, jj = kTile * 570 + o1, kTile * 578 + 10 + c % 3
        _chan_pulse(y, pulses, c, a, _tone(jj - a, 0.5))
    _chan_pulse(y, pulses, M // 2, F - 20, _tone(20, 0.5), terminated=False)
    return _chan_case("D-chan-segments", y, pulses, True, dict(tiles=579, per=10, scan="pdw_tilescan_kernel<64>"))


PATH4_OFFSET = 0.003   # the stretch stands this far (relative) above the threshold


@functools.lru_cache(maxsize=None)
def path4() -> Case:
    """family E: M = 8, F = 600 001 (the sampled route).  Each column is Gaussian background plus one stretch of 150 000
    frames of magnitude gain * med * (1 + PATH4_OFFSET), med being the column's own median: computed in float64 as the
    middle order statistic of the finished column (F is odd), which the stretch cannot move once it lies above it.
    1.2 M samples then sit inside the zone the bracket pass cannot classify before the median is known -- more than
    kUndecided -- so the device has to redo the masks (noise-floor path 4)."""
    M, F, L = 8, 600001, 150000
    rng = np.random.default_rng(2024)
    y = (0.01 * rng.standard_normal((F, M), dtype=np.float32)).astype(np.complex64)
    y.imag = 0.01 * rng.standard_normal((F, M), dtype=np.float32)
    gain = 10.0 ** (CHAN_SNR_DB / 10.0)
    pulses, med = [], np.zeros(M)
    for c in range(M):
        a = 20000 + 50000 * c
        y[a:a + L, c] = 1.0
        mag = np.abs(y[:, c].astype(np.complex128))
        med[c] = np.partition(mag, F // 2)[F // 2]
        y[a:a + L, c] = _tone(L, gain * med[c] * (1.0 + PATH4_OFFSET)).astype(np.complex64)
        pulses.append((c, a, L + 1))
    return _chan_case("E-path4", y, pulses, True, dict(noise_floor_path=4), dict(med=med, gain=gain))


# ---- wide banks ------------------------------------------------------------------------------------------------------
# Family F is edges_chan(M) at the M of WIDE_M: short (the full-select route), small enough for the oracle as it is.
#
# Family G is long as well as wide, out of the oracle's reach as a whole matrix (524 588 x 1024 is 8.6 GB of
# complex128).  The oracle treats columns independently -- noise floor, edges, amplitude, snr and sat all come from the
# column itself -- but for the bin's centre frequency, which depends on (bin, M), and, with matlab_quirks, the phase
# steps, which always come from column 0.  So a wide matrix whose column j is column j mod M0 of a narrow base has an
# exactly predictable answer from the oracle's run on the base, both runs given the same explicit decimation (WIDE_M0,
# what Case.fs assumes for the base anyway): for each wide column j, in order, the base's records of column j mod M0
# with bin = j and freq moved from the base bin's centre frequency to the wide bin's (widen_expected; column 0 of the
# wide matrix is column 0 of the base, so the rule holds with quirks on).  test_pdw_cases_cpu.py proves the rule with
# the oracle alone on explicit wide matrices.

WIDE_M = (128, 130, 256, 560, 1024)
WIDE_M0 = 9            # odd: column groups g and g + k of 64 hold different base columns unless 9 divides k
WIDE_TIED_SIGMA = 0.01     # the tied background: Gaussian of this sigma per component ...
WIDE_TIED_LEVELS = 200     # ... rounded to a grid of 1 / 200, as test_gpu_pdw.py's big_matrix(levels=200)
# the lengths of family G, each the smallest that reaches its route (test_pdw_cases_cpu.py asserts the routes)
WIDE_F1 = 8 * kSampleRows + 300   # sampled route, ragged last word: tile_words 8, 1025 tiles, pdw_tilescan_kernel<64>
WIDE_F2 = 1048000                 # 2047 tiles of 8 words: <64> with 32 tiles per thread
WIDE_F3 = 1 << 20                 # 2048 tiles: <1024>
WIDE_F4 = 1049253                 # tile_words 16, 1025 tiles; two parts per channel in the candidate select at M = 128
WIDE_FS = (WIDE_F1, WIDE_F2, WIDE_F3, WIDE_F4)
WIDE_START0, WIDE_ENDS_LAST, WIDE_OPEN = 3, 5, 7   # base columns of the pulse from frame 0 / to the last frame / left open


def scan_kernel_for(F: int, M: int) -> str:
    """restates edges_and_pulses' choice in pfb_pdw_stage.hpp"""
    tiles = -(-F // (64 * tile_words_for(F, M)))
    return "pdw_tilescan_kernel<64>" if M >= 32 and tiles < 2048 else "pdw_tilescan_kernel<1024>"


def bracket_row_groups(F: int, M: int) -> int:
    """restates pfb_pdw_extract's row_groups: the bracket pass walks whole tiles in groups of kBracketRows frames"""
    tw = tile_words_for(F, M)
    words = -(-F // (64 * tw)) * tw
    return -(-words * 64 // kBracketRows)


def _wide_tone(c: int, m: int) -> np.ndarray:
    # amplitude and phase step name the base column; 0.6 and up clears the tied background's thresholds as well (its
    # medians are sqrt(5) .. sqrt(10) grid steps of 0.005: thresholds of 0.354 .. 0.5)
    return _tone(m, 0.6 + 0.03 * c, 14.0 + 3.0 * c, 10.0 + 7.0 * c)


@functools.lru_cache(maxsize=None)
def _wide_data(F: int, tied: bool):
    M0 = WIDE_M0
    # every base column has its own background level (a sample or a histogram taken from the wrong column brackets the
    # wrong median): sigma (1 + c / 4) CHAN_SIGMA, or WIDE_TIED_SIGMA (1 + c / 32) before rounding
    if tied:   # most of a column's magnitudes tied: the bracket's count check fails, the full select runs (path 3)
        rng = np.random.default_rng(7000 + F % 1000)
        scale = (WIDE_TIED_SIGMA * WIDE_TIED_LEVELS * (1.0 + np.arange(M0) / 32.0)).astype(np.float32)
        y = np.empty((F, M0), dtype=np.complex64)
        y.real = np.round(rng.standard_normal((F, M0), dtype=np.float32) * scale) / WIDE_TIED_LEVELS
        y.imag = np.round(rng.standard_normal((F, M0), dtype=np.float32) * scale) / WIDE_TIED_LEVELS
    else:
        y, _ = _chan_background(F, M0, seed=6000 + F % 1000)
        y *= (1.0 + np.arange(M0) / 4.0).astype(np.float32)
    T = 64 * tile_words_for(F, 128)                       # the same for every M >= 128: max_tiles is 2048 there
    ntiles = -(-F // T)
    R = (bracket_row_groups(F, 128) - 1) * kBracketRows   # first frame of the last row group of the bracket pass
    assert R + 100 < F - 70
    pulses = []
    for c in range(M0):
        o1, o2 = _stagger(3 * c)                          # nine different (o1, o2), each offset from -2 to 2 on either edge
        tone = functools.partial(_wide_tone, c)
        a, jj = 64 * (2 + c % 3) + o1, 64 * (4 + c % 3) + o2            # a) short and early, edges at word boundaries
        _chan_pulse(y, pulses, c, a, tone(jj - a))
        t = ntiles * (c + 1) // (M0 + 2)                                # b) edges at tile boundaries, spread over the stream
        a, jj = T * t + o1, T * (t + 1) + o2
        _chan_pulse(y, pulses, c, a, tone(jj - a))
        a, jj = R - 70 + o1, R + 90 + o2                                # c) across the last row-group boundary
        _chan_pulse(y, pulses, c, a, tone(jj - a))
    c = WIDE_START0
    _chan_pulse(y, pulses, WIDE_START0, 0, _wide_tone(WIDE_START0, 30))                        # d) from frame 0
    _chan_pulse(y, pulses, WIDE_ENDS_LAST, F - 60, _wide_tone(WIDE_ENDS_LAST, 59))             # e) trailing sample = frame F - 1
    _chan_pulse(y, pulses, WIDE_OPEN, F - 20, _wide_tone(WIDE_OPEN, 20), terminated=False)     # f) still open: no PDW
    return y, sorted(pulses), dict(T=T, ntiles=ntiles, R=R)


def wide_base(F: int, tied: bool = False, quirks: bool = True) -> Case:
    """family G: the (F, WIDE_M0) base of a wide matrix (column j of the wide one is column j mod WIDE_M0 of this).
    Every column has a) a short pulse early on, b) one with its edges at the tile boundaries t T and (t + 1) T,
    T = 64 tile_words_for(F, 128), c) one spanning the kBracketRows boundary where the bracket pass's last row group
    starts, each with _stagger offsets on both edges; single columns have d) a pulse from frame 0, e) one whose trailing
    sample is the last frame and f) one still open there (no PDW).  Amplitude, phase step and background differ per
    column, so a record from the wrong base column is wrong in mag, snr and (quirks off) freq as well as in time, and
    a noise floor taken from the wrong column is wrong.
    tied: the background on a grid of 1 / 200 -- noise-floor path 3; its exactly antipodal neighbours would put phase
    steps of +-180 degrees into column 0, so that case runs with quirks off (pulse bodies are tones in every column)."""
    y, pulses, facts = _wide_data(F, tied)
    name = f"G-wide-F{F}-{'tied' if tied else 'gauss'}-{'quirks' if quirks else 'plain'}"
    return _chan_case(name, y, pulses, quirks, dict(noise_floor_path=3 if tied else 1), facts)


def widen(y: np.ndarray, M: int) -> np.ndarray:
    """the explicit wide matrix of a base (the GPU tests build it on the device instead)"""
    M0 = y.shape[1]
    return np.ascontiguousarray(np.tile(y, (1, -(-M // M0)))[:, :M])


def widen_expected(oracle, want_base, M: int, M0: int, fs_in: float):
    """the oracle's PDWs of the (F, M) matrix whose column j is column j mod M0 of the base, from its PDWs of the base
    (both at the same explicit decimation)"""
    def centre(m):
        cf = oracle.center_frequencies(m, fs_in)
        return lambda b: cf[(b + (m + 1) // 2) % m]
    cf0, cf = centre(M0), centre(M)
    by_col = [[p for p in want_base if p["bin"] == c] for c in range(M0)]   # time order kept
    return [dict(p, bin=j, freq=p["freq"] - cf0(j % M0) + cf(j)) for j in range(M) for p in by_col[j % M0]]


def widen_pulses(pulses, M: int, M0: int):
    by_col = [[p for p in pulses if p[0] == c] for c in range(M0)]
    return [(j, a, n) for j in range(M) for _, a, n in by_col[j % M0]]
