"""The yardstick of the pulse-train source: a numpy restatement of the stream's definition (include/pfb_channelizer.h,
"pulse-train source"), in uint64 with wrap-around, independent of the C code.  A support module, not a test."""
import math

import numpy as np

BARKER13, BARKER_DEGREES, PHASE_FROM_ZERO, ROUND_MATLAB = 1, 2, 4, 8
BARKER_13 = (+1, +1, +1, +1, +1, -1, -1, +1, +1, -1, +1, -1, +1)
FX = 20
IH_SIGMA = math.sqrt(4 * (65536.0 ** 2 - 1) / 12.0)
U32 = np.uint64(0xFFFFFFFF)


def _rint(x: float) -> int:
    return int(round(x))   # Python's round is half-even, as llrint in the default rounding mode


def derive(pw, pri, fs, f0, bit_width, flags=0, lfm_extent_hz=0.0, amplitude=0.5, noise_sigma=2.0 ** -6):
    """dict of the host-side integers: pw (adjusted), chip, fcw, dcw, gain, off."""
    chip = 0
    if flags & BARKER13:
        chip = max(_rint(pw / 13), 1)
        pw = 13 * chip
    full = float(2 ** (bit_width - 1))
    dturns = (lfm_extent_hz / (pw - 1)) / fs if pw > 1 else 0.0
    assert abs(dturns) < 0.5
    off = 0
    if flags & BARKER13:
        off = (1 << 30) if flags & BARKER_DEGREES else _rint(math.fmod(90.0 / (2.0 * math.pi), 1.0) * 2.0 ** 32)
    return dict(pw=pw, pri=pri, chip=chip, fcw=_rint(f0 / fs * 2.0 ** 32) % 2 ** 32,
                dcw=_rint(math.ldexp(dturns, 64)) % 2 ** 64,
                gain=_rint(noise_sigma * full * (1 << FX) / IH_SIGMA), off=off)


def cos_table(bit_width, amplitude=0.5):
    j = np.arange(1 << 16, dtype=np.float64)
    full = float(2 ** (bit_width - 1))
    return np.rint(amplitude * full * (1 << FX) * np.cos(2.0 * np.pi * j / 65536.0)).astype(np.int64)


def _mix32(x):
    x = x ^ (x >> np.uint64(16))
    x = (x * np.uint64(0x7FEB352D)) & U32
    x = x ^ (x >> np.uint64(15))
    x = (x * np.uint64(0x846CA68B)) & U32
    return x ^ (x >> np.uint64(16))


def on_and_phase(start, n, d, first=0, record=0, flags=0):
    """(on mask, 32-bit phase word as uint64, k) of samples start .. start + n - 1."""
    i = np.uint64(start) + np.arange(n, dtype=np.uint64)
    after = i >= np.uint64(first)
    rel = np.where(after, i - np.uint64(first), np.uint64(0))
    k = rel % np.uint64(d["pri"])
    s = np.where(after, i - k, np.uint64(0))
    on = after & (k < np.uint64(d["pw"]))
    if record:
        on &= s + np.uint64(1 + d["pw"]) < np.uint64(record)
    kk = k if flags & PHASE_FROM_ZERO else k + np.uint64(1)
    with np.errstate(over="ignore"):
        T = k * (k + np.uint64(1)) // np.uint64(2)
        ph = kk * np.uint64(d["fcw"]) + ((T * np.uint64(d["dcw"])) >> np.uint64(32))   # uint64 products wrap mod 2^64
        if flags & BARKER13:
            c = np.minimum(k // np.uint64(d["chip"]), np.uint64(12)).astype(np.int64)
            plus = np.asarray(BARKER_13)[c] > 0
            ph = ph + np.where(plus, np.uint64(d["off"]), np.uint64(2 ** 32 - d["off"]))
    return on, ph & U32, k


def stream(start, n, d, tab, seed, bit_width, fmt="int16", first=0, record=0, flags=0):
    """(n, 2) samples start .. start + n - 1: int8 / int16 / float32 by fmt.  d = derive(...), tab = the cos table."""
    i = np.uint64(start) + np.arange(n, dtype=np.uint64)
    on, ph, _ = on_and_phase(start, n, d, first, record, flags)
    ci = (ph >> np.uint64(16)).astype(np.int64)
    si = (ci - 16384) & 65535
    lo, hi = i & U32, i >> np.uint64(32)
    base = lo ^ ((hi * np.uint64(0x9E3779B1)) & U32) ^ np.uint64(seed & 0xFFFFFFFF)
    full = 1 << (bit_width - 1)
    out = []
    for lane, ti in ((0, ci), (1, si)):
        a = _mix32(base ^ np.uint64((0x68E31DA4 * (2 * lane + 1)) & 0xFFFFFFFF))
        b = _mix32(a ^ np.uint64(0x5BD1E995))
        noise = ((a & np.uint64(0xFFFF)) + (a >> np.uint64(16)) + (b & np.uint64(0xFFFF)) + (b >> np.uint64(16))
                 ).astype(np.int64) - 2 * 65535
        v = tab[ti] * on + noise * d["gain"]
        if fmt == "cf32":
            out.append((v.astype(np.float64) * 2.0 ** -(FX + bit_width - 1)).astype(np.float32))
            continue
        r = (v + (1 << (FX - 1))) >> FX
        if flags & ROUND_MATLAB:
            r = np.where(v < 0, -((-v + (1 << (FX - 1))) >> FX), r)
        out.append(np.clip(r, -full, full - 1).astype(np.int8 if fmt == "int8" else np.int16))
    return np.stack(out, axis=1)
