"""The numpy restatement of the trace / envelope contract (include/pfb_channelizer.h, "magnitude / phase traces and plot
envelopes"): what the GPU tests compare the library against, itself checked against the script's lines by
test_trace_cpu.py.  Imported by basename like synth_ref."""
import numpy as np

BIN_DTYPE = np.dtype([("peak_sample", "<u8"), ("power_min", "<f8"), ("power_max", "<f8"), ("power_mean", "<f8"),
                      ("peak_i", "<f4"), ("peak_q", "<f4"), ("count", "<u4"), ("reserved", "<u4")])
FORMATS = [("int8", 8), ("int16", 12), ("int16", 16), ("cf32", 12)]
NP_DTYPE = {"int8": np.int8, "int16": np.int16, "cf32": np.float32}

# Allowed |phase_deg - float64 restatement| (modulo 360) of pfb_trace_samples, in degrees.  No bound for the device's
# atan2f is recorded in this project and the device math library's own documentation was not at hand, so the bound is
# four times the worst error of numpy's float32 route, np.arctan2(q, i) * np.float32(180 / pi) against float64, taken
# on the CPU over the inputs of test_gpu_trace.py's full-rate tests (phase_inputs below: random int16, int8 and cf32
# data, small magnitudes, full-scale corners and the axes): 2.64e-5 degrees (float32_phase_error recomputes it; the
# CPU test pins it).  The factor 4 is for a different implementation of comparable accuracy plus the float32 multiply.
NUMPY_F32_PHASE_ERR_DEG = 2.64e-5
PHASE_TOL_DEG = 4 * NUMPY_F32_PHASE_ERR_DEG


def random_iq(fmt, bw, n, seed):
    """(n, 2) samples of the format: integers over the whole range of the bit width, floats in [-1, 1)."""
    rng = np.random.default_rng(seed)
    if fmt == "cf32":
        return (rng.random((n, 2), dtype=np.float32) * 2 - 1).astype(np.float32)
    full = 1 << (bw - 1)
    return rng.integers(-full, full, size=(n, 2)).astype(NP_DTYPE[fmt])


def powers(iq, fmt, bw):
    """Per sample: u = I^2 + Q^2 as uint64 (integer formats) or p as float64 (cf32); and the scale that makes u a
    power, 2^-(2(bw-1)) (1 for cf32)."""
    iq = np.asarray(iq).reshape(-1, 2)
    if fmt == "cf32":
        x = iq.astype(np.float64)
        return x[:, 0] * x[:, 0] + x[:, 1] * x[:, 1], 1.0
    x = iq.astype(np.int64)
    return (x[:, 0] * x[:, 0] + x[:, 1] * x[:, 1]).astype(np.uint64), 2.0 ** (-2 * (bw - 1))


def fold(parts, fmt, bw):
    """One record from the figures of consecutive pieces of a bin: (u_min, u_max, first global argmax, sum, count,
    peak I, peak Q) each.  Integer formats: exact, so any cutting gives the same record."""
    parts = [p for p in parts if p[4] > 0]
    rec = np.zeros(1, BIN_DTYPE)[0]
    lo = min(p[0] for p in parts)
    hi = max(p[1] for p in parts)
    first = min((p for p in parts if p[1] == hi), key=lambda p: p[2])  # lexicographic: largest power, lowest index
    count = sum(int(p[4]) for p in parts)
    if fmt == "cf32":
        s = 0.0
        for p in parts:
            s += float(p[3])
        rec["power_min"], rec["power_max"], rec["power_mean"] = lo, hi, s / count
        rec["peak_i"], rec["peak_q"] = first[5], first[6]
    else:
        scale = 2.0 ** (-2 * (bw - 1))
        s = sum(int(p[3]) for p in parts)
        rec["power_min"], rec["power_max"] = float(int(lo)) * scale, float(int(hi)) * scale
        rec["power_mean"] = (float(np.float64(np.uint64(s))) / float(count)) * scale
        comp = np.float32(2.0 ** -(bw - 1))
        rec["peak_i"], rec["peak_q"] = np.float32(first[5]) * comp, np.float32(first[6]) * comp
    rec["peak_sample"], rec["count"] = first[2], count
    return rec


def piece(iq, fmt, bw, first_index):
    """The figures of one piece of a bin, whose first sample has global index first_index."""
    iq = np.asarray(iq).reshape(-1, 2)
    if len(iq) == 0:
        return (0, 0, 0, 0, 0, 0, 0)
    u, _ = powers(iq, fmt, bw)
    k = int(np.argmax(u))
    s = u.sum(dtype=np.uint64) if fmt != "cf32" else float(np.sum(u))
    return (u.min(), u.max(), first_index + k, s, len(iq), iq[k, 0], iq[k, 1])


def envelope(iq, fmt, bw, B, origin=0, partial=True):
    """The records of a stream whose first sample has global index `origin` and starts a bin; partial: the final short
    bin is included (what flush returns)."""
    iq = np.asarray(iq).reshape(-1, 2)
    n = len(iq)
    bins = -(-n // B) if partial else n // B
    out = np.zeros(bins, BIN_DTYPE)
    for k in range(bins):
        out[k] = fold([piece(iq[k * B:(k + 1) * B], fmt, bw, origin + k * B)], fmt, bw)
    return out


def envelope_fast(iq, fmt, bw, B, origin=0, partial=True):
    """envelope() without a Python loop over the full bins: the same records (test_trace_cpu.py compares the two)."""
    iq = np.asarray(iq).reshape(-1, 2)
    n = len(iq)
    full = n // B
    out = np.zeros(full, BIN_DTYPE)
    if full:
        u, scale = powers(iq[:full * B], fmt, bw)
        u = u.reshape(full, B)
        k = np.argmax(u, axis=1)
        at = np.arange(full) * B + k
        out["peak_sample"] = (origin + at).astype(np.uint64)
        out["count"] = B
        if fmt == "cf32":
            out["power_min"], out["power_max"] = u.min(axis=1), u.max(axis=1)
            out["power_mean"] = u.sum(axis=1) / float(B)
            out["peak_i"], out["peak_q"] = iq[at, 0], iq[at, 1]
        else:
            out["power_min"] = u.min(axis=1).astype(np.float64) * scale
            out["power_max"] = u.max(axis=1).astype(np.float64) * scale
            out["power_mean"] = (u.sum(axis=1, dtype=np.uint64).astype(np.float64) / float(B)) * scale
            comp = np.float32(2.0 ** -(bw - 1))
            out["peak_i"] = iq[at, 0].astype(np.float32) * comp
            out["peak_q"] = iq[at, 1].astype(np.float32) * comp
    if partial and n % B:
        out = np.concatenate([out, envelope(iq[full * B:], fmt, bw, B, origin + full * B)])
    return out


def mean_close(got, want, rtol_per_sample=2.0 ** -52):
    """cf32 power_mean: within count * 2^-52 relative, the bound for any summation order of `count` non-negative
    doubles plus the division; every other field bit for bit."""
    a, b = got.copy(), want.copy()
    ok = np.all(np.abs(a["power_mean"] - b["power_mean"]) <= b["count"] * rtol_per_sample * np.abs(b["power_mean"]))
    a["power_mean"] = b["power_mean"] = 0
    return bool(ok) and a.tobytes() == b.tobytes()


def mag_phase64(iq, fmt, bw):
    """abs((I + jQ)/full) and rad2deg(angle()) in float64 (plot_my_iq.m:105-111)."""
    x = np.asarray(iq).reshape(-1, 2).astype(np.float64)
    full = 1.0 if fmt == "cf32" else 2.0 ** (bw - 1)
    return np.hypot(x[:, 0], x[:, 1]) / full, np.degrees(np.arctan2(x[:, 1], x[:, 0]))


def phase_inputs(fmt, bw, n, seed):
    """The samples of the full-rate tests: random data, then small magnitudes, the full-scale corners and the axes."""
    iq = random_iq(fmt, bw, n, seed)
    if fmt == "cf32":
        edge = np.array([[1e-6, -2e-6], [1, 1], [-1, 1], [-1, -1], [1, -1], [1, 0], [0, 1], [-1, 0], [0, -1], [0, 0],
                         [3e-3, 1], [-1, 1e-4]], np.float32)
    else:
        full = 1 << (bw - 1)
        edge = np.array([[1, 0], [0, 1], [-1, 0], [0, -1], [1, 1], [-1, 2], [2, -3], [0, 0], [-full, -full],
                         [full - 1, full - 1], [-full, full - 1], [full - 1, -full], [-full, 0], [0, -full], [-full, 1],
                         [1, -full]]).astype(NP_DTYPE[fmt])
    iq[:len(edge)] = edge
    small = slice(len(edge), len(edge) + n // 8)
    iq[small] = iq[small] * np.float32(1e-3) if fmt == "cf32" else iq[small] % 4 - 2
    return iq


SAMPLES_PER_VECTOR = {"int8": 8, "int16": 4, "cf32": 2}   # one 16-byte load of trace_samples_kernel


def grid_pass(fmt, cus):
    """(pass_, n): the samples one pass of pfb_trace_samples' grid covers on a device of `cus` compute units (8
    workgroups per unit, 256 lanes, one vector per lane), and a call of two whole passes, half a workgroup of vectors
    of a third, and a scalar tail of three samples."""
    S = SAMPLES_PER_VECTOR[fmt]
    pass_ = 8 * cus * 256 * S
    return pass_, 2 * pass_ + 128 * S + 3


def bins_holding(indices, B, origin, n):
    """The bins (sorted, each once) that hold the samples with the given global indices, for a stream of n samples
    whose first sample has global index `origin` and starts bin 0; indices outside the stream hold no bin."""
    i = np.asarray(indices, dtype=np.int64).reshape(-1) - origin
    return np.unique(i[(i >= 0) & (i < n)] // B)


def call_segments(n, B, open_, tile=4096):
    """The segments an envelope call of n > 0 samples is cut into when its first bin already holds open_ < B samples:
    one per started tile of each bin (bins of 1024 samples and more; the partials a bin longer than a tile needs)."""
    last = open_ + n - 1
    return (last // B) * (-(-B // tile)) + (last % B) // tile + 1 - open_ // tile


def wide_iq(fmt, n, seed):
    """Integers over the whole range of the container, whatever the handle's bit width says, with the container's
    largest power (-full, -full) at sample 3."""
    bits = {"int8": 8, "int16": 16}[fmt]
    iq = random_iq(fmt, bits, n, seed)
    iq[3] = -(1 << (bits - 1))
    return iq


def planted_fold_stream(fmt, bw, B, seed, tile=4096):
    """Two streams of 3 B + 5000 samples for a bin of 67 partials (B = 66 tiles + 3): random data at half scale without
    a zero sample; in bin 1 the same full-scale sample twice -- in partials 2 and 66, which one lane of the fold takes
    in two rounds, or (second stream) in partials 10 and 50, two lanes -- and the bin's only zero sample in partial 65."""
    assert (B - 1) // tile == 66 and B % tile >= 2
    n = 3 * B + 5000
    rng = np.random.default_rng(seed)
    if fmt == "cf32":
        iq = rng.random((n, 2), dtype=np.float32) - np.float32(0.5)
        big, floor = (1.0, -1.0), (2.0 ** -10, 0.0)
    else:
        full = 1 << (bw - 1)
        iq = rng.integers(-(full // 2), full // 2, size=(n, 2)).astype(NP_DTYPE[fmt])
        big, floor = (-full, -full), (1, 1)
    iq[~iq.any(axis=1)] = floor
    out = []
    for first, second in ((2, 66), (10, 50)):
        v = iq.copy()
        v[B + first * tile + 17] = v[B + second * tile + 1] = big
        v[B + 65 * tile + 4000] = 0
        out.append(v)
    return tuple(out)


def phase_diff(a, b):
    """|a - b| modulo 360 degrees"""
    d = np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)) % 360.0
    return np.minimum(d, 360.0 - d)


def float32_phase_error(iq):
    """worst error in degrees of numpy's float32 arctan2(q, i) * (180/pi) against float64 on these samples"""
    x = np.asarray(iq).reshape(-1, 2)
    f = x.astype(np.float32)
    got = np.arctan2(f[:, 1], f[:, 0]) * np.float32(180.0 / np.pi)
    assert got.dtype == np.float32
    return float(phase_diff(got, np.degrees(np.arctan2(x[:, 1].astype(np.float64), x[:, 0].astype(np.float64)))).max())


def ulp32(x):
    return np.spacing(np.abs(np.asarray(x, np.float64)).astype(np.float32)).astype(np.float64)
