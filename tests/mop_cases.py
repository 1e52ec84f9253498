"""Designed inputs of the modulation-on-pulse tests (test_mop_cpu.py, test_gpu_mop.py): series, pulse lists and the
synthetic pulses of the accuracy table.  A support module, not a test."""
import numpy as np

import mf_ref as MF
import mop_ref as R
import synth_ref as S

FS = 56e6
SIGMAS = (0.0, 2.0 ** -6, 2.0 ** -4, 2.0 ** -3)
SEEDS = tuple(range(1, 9))
GROUP_MIN, SPLIT_MIN, PART, GRID_CAP, SLICE, SLOTS = 4096, 1 << 15, 1 << 14, 2048, 1 << 16, 256   # pfb_mop_plan, pinned in test_mop_cpu
# The accuracy table: synth_ref pulses, 12 bit, amplitude 0.5, fs = 56 MHz, carrier 3 MHz at the
# first sample, seeds 1 .. 8.  Per input and per sigma of SIGMAS: the largest |error| over the seeds of the mid frequency
# and of the sweep's extent, in MHz, and the least and the most negatives.  test_mop_cpu.py::test_the_accuracy_table
# measures every figure again and holds it to this table; the chain's tolerances below are taken from it.
TABLE = {
    "carrier 3 MHz, pw 1000": dict(pw=1000),
    "LFM 5 MHz, pw 1000": dict(pw=1000, extent=5e6),
    "LFM 40 MHz, pw 1000": dict(pw=1000, extent=40e6),
    "LFM -50 MHz, pw 5600": dict(pw=5600, extent=-50e6),
    "Barker-13 (degrees) on LFM 2 MHz, pw 1001": dict(pw=1001, extent=2e6, flags=S.BARKER13 | S.BARKER_DEGREES),
    "Barker-13 (radians) on LFM 2 MHz, pw 1001": dict(pw=1001, extent=2e6, flags=S.BARKER13),
}
MEASURED = {
    "carrier 3 MHz, pw 1000": [(0.0000, 0.0000, 0, 0), (0.0012, 0.0046, 0, 0), (0.0167, 0.0404, 0, 0), (0.0686, 0.1270, 11, 17)],
    "LFM 5 MHz, pw 1000": [(0.0025, 0.0000, 0, 0), (0.0053, 0.0066, 0, 0), (0.0212, 0.0464, 0, 0), (0.0664, 0.1409, 8, 23)],
    "LFM 40 MHz, pw 1000": [(0.0199, 0.0000, 0, 0), (0.0841, 0.0046, 0, 0), (0.3224, 0.0482, 0, 0), (0.7297, 0.1908, 12, 20)],
    "LFM -50 MHz, pw 5600": [(0.0041, 0.0000, 0, 0), (0.1119, 0.0019, 0, 0), (0.4685, 0.0349, 0, 0), (0.9508, 0.1356, 78, 110)],
    "Barker-13 (degrees) on LFM 2 MHz, pw 1001": [(0.0037, 0.0001, 12, 12), (0.0076, 0.0128, 12, 12), (0.0321, 0.0658, 12, 12),
                                                  (0.0946, 0.1914, 20, 29)],
    "Barker-13 (radians) on LFM 2 MHz, pw 1001": [(0.0027, 0.0581, 12, 12), (0.0059, 0.0671, 12, 12), (0.0284, 0.1200, 10, 12),
                                                  (0.0889, 0.2808, 19, 27)],
}
TABLE_SLACK = 6e-5       # MHz: the table is kept to four decimals
# The chain of test_mop_cpu.py and test_gpu_mop.py: its noise, and the leading-edge threshold that still finds its pulses.
# Its tolerances are the table's figures for "LFM 40 MHz, pw 1000" at that noise times a margin of 4, because seeds differ.
CHAIN_SIGMA, CHAIN_SNR_DB, MARGIN = SIGMAS[1], 12.0, 4
FREQ_TOL_LFM40 = MARGIN * MEASURED["LFM 40 MHz, pw 1000"][1][0] * 1e6       # 0.3364 MHz
EXTENT_TOL_LFM40 = MARGIN * MEASURED["LFM 40 MHz, pw 1000"][1][1] * 1e6     # 0.0184 MHz
BARKER_NEGS = [383, 384, 537, 538, 691, 692, 768, 769, 845, 846, 922, 923]       # pw 1001: chips of 77 samples


def synth_pulse(pw, seed, sigma, f0=3e6, extent=0.0, flags=0, bit_width=12, fmt="int16", lead=0, tail=0):
    """one pulse of the pulse-train source (synth_ref) with `lead` samples of noise before it and `tail` after:
    ((rows, 2) samples, the pulse's length after the Barker adjustment)"""
    d = S.derive(pw, 1 << 24, FS, f0, bit_width, flags, extent, 0.5, sigma)
    tab = S.cos_table(bit_width, 0.5)
    return S.stream(0, lead + d["pw"] + tail, d, tab, seed, bit_width, fmt, lead, 0, flags), d["pw"]


def chain_stream(kind, seed=3, sigma=CHAIN_SIGMA, pulses=6):
    """a train of `pulses` pulses of the source (synth_ref), 12 bit, PRI 4000, the first at sample 700: an LFM of
    40 MHz over 1000 samples, or a Barker-13 code of 1001; (samples, parameters, first sample of pulse 0)"""
    kw = dict(pw=1000, extent=40e6, flags=0) if kind == "lfm" else dict(pw=1001, extent=0.0, flags=S.BARKER13 | S.BARKER_DEGREES)
    d = S.derive(kw["pw"], 4000, FS, 3e6, 12, kw["flags"], kw["extent"], 0.5, sigma)
    first = 700
    return S.stream(0, first + pulses * 4000, d, S.cos_table(12, 0.5), seed, 12, "int16", first, 0, kw["flags"]), d, first


def replica_peak_offsets(x, replica, first=700, pulses=6, pri=4000):
    """where the float64 matched filter (mf_ref) of the 12-bit stream x against `replica` peaks within 200 samples of
    each pulse's true first sample, as the offset from that sample"""
    y = np.abs(MF.compress(MF.unpack(x, "int16", 12), replica)) ** 2
    return [int(np.argmax(y[first + pri * k - 200:first + pri * k + 200])) - 200 for k in range(pulses)]


def random_series(fmt, rows, seed, ld=1):
    rng = np.random.default_rng(seed)
    if fmt == "cf32":
        shape = (rows,) if ld == 1 else (rows, ld)
        return (rng.standard_normal(shape) + 1j * rng.standard_normal(shape)).astype(np.complex64)
    info = np.iinfo(np.int8 if fmt == "int8" else np.int16)
    return rng.integers(info.min, info.max + 1, (rows, 2)).astype(info.dtype)


def carrier(fmt, rows, flips=(), amp=1000.0, turns=0.01):
    """a noiseless carrier of `turns` cycles a sample whose sign flips in front of every sample of `flips`: each flip
    at b makes the negatives b - 2 and b - 1 (those that exist) and nothing else does"""
    i = np.arange(rows)
    sign = np.ones(rows)
    for b in flips:
        sign[b:] *= -1
    z = amp * sign * np.exp(2j * np.pi * turns * i)
    if fmt == "cf32":
        return z.astype(np.complex64)
    dt = np.int8 if fmt == "int8" else np.int16
    return np.stack([np.rint(z.real), np.rint(z.imag)], axis=1).astype(dt)


def lengths_of_interest(trim=0):
    """every length at which the unit takes another path, as n + 2 trim"""
    ns = [0, 1, 2, 3, 4, 5, 63, 64, 65, 255, 256, 257, GROUP_MIN - 1, GROUP_MIN, GROUP_MIN + 1, PART - 1, PART, PART + 1,
          SPLIT_MIN - 1, SPLIT_MIN, SPLIT_MIN + 1, 2 * PART + 1]
    return [n + 2 * trim for n in ns]


def spread(lengths, rows, seed):
    """a PULSE list of these lengths at random starts inside a series of `rows`"""
    rng = np.random.default_rng(seed)
    starts = [int(rng.integers(0, rows - n + 1)) for n in lengths]
    return R.pulses(starts, lengths)


def same_exact(got, want):
    """the integer fields of two record arrays, byte for byte"""
    return all(np.array_equal(got[name], want[name]) for name in R.EXACT)
