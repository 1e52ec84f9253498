"""The trace / envelope contract without a GPU: the numpy restatement (trace_ref) against the script's own lines, the
record layout, the host-only entry points and every argument check that comes before the device."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import trace_ref as R
from sdr_channelizer_amd import _lib as L
from sdr_channelizer_amd import trace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def ulps64(a, b):
    return np.abs(a - b) / np.spacing(np.maximum(np.abs(a), np.abs(b)))


@pytest.mark.parametrize("fmt,bw", R.FORMATS)
@pytest.mark.parametrize("B", [5, 64, 1000])
def test_restatement_is_the_script(fmt, bw, B):
    """plot_my_iq.m:105-111 on a small record: iq/2^(bitWidth-1), abs; the records' figures are its min / max / mean
    square per bin, the peak is numpy's first argmax.  The script's mean(abs(x)**2) carries up to 2.5 * 2^-52 of its
    own per term (hypot, then the squaring) besides the (count - 1) * 2^-53 of its sum, so count * 2^-52 holds it from
    4 samples per bin on: the record's length leaves no shorter final bin.  abs() is np.hypot(real, imag), within 1 ulp
    of the correctly rounded magnitude; numpy's vectorised abs of a complex128 array is itself up to 2 ulp away from it on
    these records (measured against math.hypot), which would charge the script's own rounding to the restatement."""
    N = 3005
    iq = R.random_iq(fmt, bw, N, seed=B)
    iq[10:13] = iq[11]          # equal powers: the first wins
    full = 1.0 if fmt == "cf32" else 2.0 ** (bw - 1)
    x = (iq[:, 0].astype(np.float64) + 1j * iq[:, 1].astype(np.float64)) / full
    mag = np.hypot(x.real, x.imag)
    rec = R.envelope(iq, fmt, bw, B, origin=100)
    assert rec.size == -(-N // B) and N % B in (0, 5, 61) and rec.dtype == R.BIN_DTYPE
    for k, r in enumerate(rec):
        m = mag[k * B:(k + 1) * B]
        assert r["count"] == m.size and r["reserved"] == 0
        assert ulps64(np.sqrt(r["power_max"]), m.max()) <= 1 and ulps64(np.sqrt(r["power_min"]), m.min()) <= 1
        mean = np.mean(m ** 2)
        assert abs(r["power_mean"] - mean) <= m.size * 2.0 ** -52 * mean
        u, _ = R.powers(iq[k * B:(k + 1) * B], fmt, bw)
        at = int(np.argmax(u))
        assert r["peak_sample"] == 100 + k * B + at
        assert r["peak_i"] == np.float32(x[k * B + at].real) and r["peak_q"] == np.float32(x[k * B + at].imag)
    assert R.envelope_fast(iq, fmt, bw, B, origin=100).tobytes() == rec.tobytes() or \
        (fmt == "cf32" and R.mean_close(R.envelope_fast(iq, fmt, bw, B, origin=100), rec))
    m64, p64 = R.mag_phase64(iq, fmt, bw)
    assert np.array_equal(m64, mag) or np.max(ulps64(m64, mag)) <= 1
    assert R.phase_diff(p64, np.degrees(np.angle(x))).max() < 1e-12


@pytest.mark.parametrize("fmt,bw", [f for f in R.FORMATS if f[0] != "cf32"])
def test_restatement_does_not_depend_on_the_cutting(fmt, bw):
    """integer formats: fold the figures of the two halves of a bin, split anywhere -- the same bits"""
    iq = R.random_iq(fmt, bw, 777, seed=9)
    iq[300:500] = iq[0]  # the largest power may sit on both sides of a cut
    if bw == 16:
        iq[5] = iq[600] = (-32768, -32768)
    whole = R.fold([R.piece(iq, fmt, bw, 40)], fmt, bw)
    for cut in (0, 1, 5, 6, 299, 300, 301, 499, 500, 600, 601, 776, 777):
        halves = [R.piece(iq[:cut], fmt, bw, 40), R.piece(iq[cut:], fmt, bw, 40 + cut)]
        assert R.fold(halves, fmt, bw).tobytes() == whole.tobytes(), cut
        assert R.fold(halves[::-1], fmt, bw).tobytes() == whole.tobytes(), cut


def test_extreme_powers_do_not_fit_32_bits():
    iq = np.full((1 << 12, 2), -32768, np.int16)
    u, scale = R.powers(iq, "int16", 16)
    assert u.dtype == np.uint64 and int(u[0]) == 2 ** 31 and int(u.sum(dtype=np.uint64)) == 2 ** 43
    r = R.envelope(iq, "int16", 16, 1 << 12)[0]
    assert r["power_min"] == r["power_max"] == r["power_mean"] == 2.0 and r["peak_sample"] == 0
    assert r["peak_i"] == r["peak_q"] == -1.0


def test_record_layout():
    assert C.sizeof(L.PfbTraceBin) == 48 == R.BIN_DTYPE.itemsize == trace.BIN_DTYPE.itemsize
    assert R.BIN_DTYPE == trace.BIN_DTYPE
    for name, _ in L.PfbTraceBin._fields_:
        assert getattr(L.PfbTraceBin, name).offset == R.BIN_DTYPE.fields[name][1], name
        assert getattr(L.PfbTraceBin, name).size == R.BIN_DTYPE.fields[name][0].itemsize, name
    assert [n for n, _ in L.PfbTraceBin._fields_] == list(R.BIN_DTYPE.names)
    assert C.sizeof(L.PfbTraceConfig) == 24
    hdr = open(os.path.join(ROOT, "include", "pfb_channelizer.h")).read()
    assert "#define PFB_ABI_VERSION 2" in hdr or L.load().pfb_abi_version() == 2


def test_choose_bin():
    lib = L.load()
    b = C.c_uint32(77)
    for max_bins in (1, 7, 4096, 2 ** 32 - 1):
        for n in (0, 1, max_bins, max_bins + 1, 2 ** 32 + 5):
            want = max(1, -(-n // max_bins))
            if want > 2 ** 31:
                assert lib.pfb_trace_choose_bin(n, max_bins, C.byref(b)) == L.PFB_ERR_BAD_ARG, (n, max_bins)
                continue
            assert lib.pfb_trace_choose_bin(n, max_bins, C.byref(b)) == L.PFB_OK and b.value == want, (n, max_bins)
            assert trace.choose_bin(n, max_bins) == want
    assert lib.pfb_trace_choose_bin(2 ** 31, 1, C.byref(b)) == L.PFB_OK and b.value == 2 ** 31
    assert lib.pfb_trace_choose_bin(2 ** 31 + 1, 1, C.byref(b)) == L.PFB_ERR_BAD_ARG
    assert lib.pfb_trace_choose_bin(2 ** 64 - 1, 2 ** 32 - 1, C.byref(b)) == L.PFB_ERR_BAD_ARG   # B = 2^32 + 1
    assert lib.pfb_trace_choose_bin(100, 0, C.byref(b)) == L.PFB_ERR_BAD_ARG
    assert lib.pfb_trace_choose_bin(100, 10, None) == L.PFB_ERR_BAD_ARG


def config(fmt=L.PFB_FMT_INT16_IQ, bw=12, B=64, flags=0, size=None, device=-1):
    return L.PfbTraceConfig(C.sizeof(L.PfbTraceConfig) if size is None else size, fmt, bw, B, flags, device)


def test_arguments_are_checked_before_the_device():
    lib = L.load()
    h = C.c_void_p()

    def create(**kw):
        cfg = config(**kw)
        return lib.pfb_trace_create(C.byref(cfg), C.byref(h))

    assert lib.pfb_trace_create(None, C.byref(h)) == L.PFB_ERR_BAD_ARG
    cfg = config()
    assert lib.pfb_trace_create(C.byref(cfg), None) == L.PFB_ERR_BAD_ARG
    assert create(size=20) == L.PFB_ERR_BAD_ARG
    assert create(B=0) == L.PFB_ERR_BAD_ARG and create(B=2 ** 31 + 1) == L.PFB_ERR_BAD_ARG
    for bit in (1, 2, 1 << 31):
        assert create(flags=bit) == L.PFB_ERR_BAD_ARG
    assert create(fmt=3) == L.PFB_ERR_BAD_FORMAT
    for fmt, bad in ((L.PFB_FMT_INT8_IQ, (0, 9)), (L.PFB_FMT_INT16_IQ, (0, 17))):
        for bw in bad:
            assert create(fmt=fmt, bw=bw) == L.PFB_ERR_BAD_FORMAT, (fmt, bw)
    assert create(B=0, fmt=3) == L.PFB_ERR_BAD_ARG          # the order of the list: arguments, then formats
    assert not h.value
    # null handles and pointers
    u, i, b = C.c_uint64(), C.c_int32(), C.c_uint32()
    rec = L.PfbTraceBin()
    buf = np.zeros(64, np.int16)
    p = C.c_void_p(buf.ctypes.data)
    assert lib.pfb_trace_destroy(None) == lib.pfb_trace_reset(None) == lib.pfb_trace_sync(None) == L.PFB_ERR_BAD_ARG
    assert lib.pfb_trace_set_stream(None, None) == lib.pfb_trace_get_device(None, None) == L.PFB_ERR_BAD_ARG
    assert lib.pfb_trace_bins_for(None, 5, C.byref(u)) == L.PFB_ERR_BAD_ARG
    assert lib.pfb_trace_envelope(None, p, 32, p, 1, C.byref(u), L.PFB_MEM_HOST) == L.PFB_ERR_BAD_ARG
    assert lib.pfb_trace_envelope_async(None, p, 32, p, 1, C.byref(u)) == L.PFB_ERR_BAD_ARG
    assert lib.pfb_trace_flush(None, C.byref(rec), C.byref(i)) == L.PFB_ERR_BAD_ARG
    assert lib.pfb_trace_samples(None, p, 32, p, p, L.PFB_MEM_HOST) == L.PFB_ERR_BAD_ARG
    info = L.PfbIqInfo()
    file_call = lib.pfb_trace_envelope_from_iq_file
    assert file_call(None, 16, p, 1, C.byref(u), C.byref(b), C.byref(info), -1) == L.PFB_ERR_BAD_ARG
    assert file_call(b"x.iq", 0, p, 1, C.byref(u), C.byref(b), C.byref(info), -1) == L.PFB_ERR_BAD_ARG
    assert file_call(b"x.iq", 16, None, 1, C.byref(u), C.byref(b), C.byref(info), -1) == L.PFB_ERR_BAD_ARG
    assert file_call(b"x.iq", 16, p, 1, None, C.byref(b), C.byref(info), -1) == L.PFB_ERR_BAD_ARG
    assert file_call(b"x.iq", 16, p, 1, C.byref(u), None, C.byref(info), -1) == L.PFB_ERR_BAD_ARG
    assert file_call(b"x.iq", 16, C.c_void_p(buf.ctypes.data + 2), 1, C.byref(u), C.byref(b), None, -1) == L.PFB_ERR_BAD_ARG


def test_a_valid_config_needs_a_device():
    lib = L.load()
    if lib.pfb_device_count() > 0:
        pytest.skip("a GPU is present")
    h = C.c_void_p()
    for fmt, bw in ((L.PFB_FMT_INT8_IQ, 1), (L.PFB_FMT_INT8_IQ, 8), (L.PFB_FMT_INT16_IQ, 16), (L.PFB_FMT_CF32, 99)):
        for B in (1, 2 ** 31):
            cfg = config(fmt=fmt, bw=bw, B=B)
            assert lib.pfb_trace_create(C.byref(cfg), C.byref(h)) == L.PFB_ERR_NO_DEVICE and not h.value
    with pytest.raises(L.PfbError) as e:
        trace.Trace(64)
    assert e.value.status == L.PFB_ERR_NO_DEVICE
    u, b = C.c_uint64(), C.c_uint32()
    rec = L.PfbTraceBin()
    assert lib.pfb_trace_envelope_from_iq_file(b"no_such.iq", 16, C.byref(rec), 1, C.byref(u), C.byref(b), None, -1) \
        == L.PFB_ERR_NO_DEVICE


def test_phase_bound_is_the_measured_one():
    """PHASE_TOL_DEG is four times what numpy's float32 route loses on the inputs the GPU test uses."""
    worst = max(R.float32_phase_error(R.phase_inputs(fmt, bw, 200003, seed=5)) for fmt, bw in R.FORMATS)
    assert 0.9 * R.NUMPY_F32_PHASE_ERR_DEG <= worst <= R.NUMPY_F32_PHASE_ERR_DEG, worst
    assert R.PHASE_TOL_DEG == 4 * R.NUMPY_F32_PHASE_ERR_DEG


def test_trace_entry_points_sit_under_the_abi_guard():
    src = open(os.path.join(ROOT, "sdr_channelizer_amd", "csrc", "pfb_trace.hip")).read()
    found = {}
    for m in re.finditer(r'^extern "C" int (\w+)\(', src, re.M):
        rest = src[m.start():]
        found[m.group(1)] = rest[: rest.index("\n}\n")]
    assert set(found) == {n for n in L.EXPORTS if n.startswith("pfb_trace_")} and len(found) == 13
    for name, body in found.items():
        assert "abi_guard" in body.split("{", 1)[1][:80], name
    assert src.count('extern "C"') == len(found)


# ---- what tests/test_gpu_trace_reach.py builds on: its helpers, and the conditions its bounds need, on the CPU ----

def test_bins_holding():
    assert R.bins_holding([], 5, 0, 41).size == 0
    assert R.bins_holding([0, 4, 5, 5, 39, 40], 5, 0, 41).tolist() == [0, 1, 7, 8]
    assert R.bins_holding([40, 41, -1], 5, 0, 41).tolist() == [8]                 # 41 and -1 are outside the stream
    assert R.bins_holding([99, 100, 104, 105, 140], 5, 100, 41).tolist() == [0, 1, 8]
    assert R.bins_holding(np.array([7, 3]), 1, 0, 8).tolist() == [3, 7]
    got = R.bins_holding([2 ** 33 + 5], 2 ** 31, 0, 2 ** 34)
    assert got.tolist() == [4] and got.dtype == np.int64


def test_call_segments_counts_the_cuts():
    """against a walk over every sample: a new segment at each bin start and each multiple of the tile inside a bin"""
    tile = 8
    for B in (8, 9, 16, 17, 30):
        for open_ in range(B):
            for n in (1, 2, 7, 8, 9, B - 1, B, B + 1, 3 * B + 5):
                if n < 1:
                    continue
                g = np.arange(open_, open_ + n)
                want = len(set(zip((g // B).tolist(), ((g % B) // tile).tolist())))
                assert R.call_segments(n, B, open_, tile) == want, (B, open_, n)
    assert R.call_segments(2 * 70001, 70001, 4) == 18 + 18 + 1 and R.call_segments(1, 5000, 4999) == 1


@pytest.mark.parametrize("fmt,bw", R.FORMATS)
def test_phase_bound_holds_over_several_grid_passes(fmt, bw):
    """The inputs of the multi-pass full-rate test on a device of 256 compute units: numpy's float32 route stays below
    half of PHASE_TOL_DEG on exactly these samples, so the bound taken on 200 003 samples needs no widening for 8.4
    million.  Measured: 2.42e-5 (int8), 2.71e-5 (int16), 2.70e-5 (cf32) degrees."""
    pass_, n = R.grid_pass(fmt, 256)
    assert pass_ == 2048 * 256 * R.SAMPLES_PER_VECTOR[fmt] and n > 2 * pass_
    assert (fmt != "int8" or n == 8389635) and (n - 3) % R.SAMPLES_PER_VECTOR[fmt] == 0
    worst = R.float32_phase_error(R.phase_inputs(fmt, bw, n + 1, seed=21))
    print(f"{fmt}/{bw}: {worst:.3e} degrees over {n + 1} samples")
    assert worst < R.PHASE_TOL_DEG / 2, worst


def test_phase_bound_holds_wide_and_scaled_inputs():
    """The other full-rate inputs of the reach module: integers over the whole container (measured 2.4e-5 and 2.5e-5
    degrees) and the cf32 inputs times 2^40 and 2^-40 (2.63e-5 at both: the scaling is exact)."""
    for fmt in ("int8", "int16"):
        iq = R.wide_iq(fmt, 5 * (trace.TILE + 1) + 3, seed=6)[:20003]
        full = 128 if fmt == "int8" else 32768
        assert iq.min() == -full and iq.max() == full - 1 and tuple(iq[3]) == (-full, -full)
        assert R.float32_phase_error(iq) < R.PHASE_TOL_DEG / 2
    base = R.phase_inputs("cf32", 12, 20003, seed=8)
    for e in (40, -40):
        iq = base * np.float32(2.0 ** e)
        assert iq.dtype == np.float32 and np.array_equal(iq.astype(np.float64), base.astype(np.float64) * 2.0 ** e)
        u, _ = R.powers(iq, "cf32", 12)
        assert np.all((u == 0) | (u > 2.0 ** -1000)) and np.all(u < 2.0 ** 1000)     # normal doubles
        assert np.all((iq == 0) | (np.abs(iq) >= np.finfo(np.float32).tiny))            # normal floats
        assert R.float32_phase_error(iq) < R.PHASE_TOL_DEG / 2


def test_reference_mean_against_a_sequential_sum():
    """cf32: the restatement sums a bin pairwise (numpy); a plain sequential sum of the same doubles stays inside the
    count * 2^-52 that mean_close allows, with room for the device's own order.  Measured at B = 70 001: 5.7e-14
    against an allowance of 1.6e-11."""
    iq = R.random_iq("cf32", 12, 8 * 100003 + 4, seed=16)[:200000]
    for B in (3, 4096, 70001):
        want = R.envelope_fast(iq, "cf32", 12, B, partial=False)
        u, _ = R.powers(iq[:want.size * B], "cf32", 12)
        seq = np.cumsum(u.reshape(want.size, B), axis=1)[:, -1] / float(B)
        rel = np.abs(seq - want["power_mean"]) / want["power_mean"]
        print(f"B = {B}: {rel.max():.2e} of an allowed {B * 2.0 ** -52:.2e}")
        assert np.all(rel <= B * 2.0 ** -52)
        if B == 70001:
            assert rel.max() < 0.05 * B * 2.0 ** -52


@pytest.mark.parametrize("fmt,bw", [("int8", 8), ("int16", 12), ("cf32", 12)])
def test_planted_fold_stream(fmt, bw):
    T = trace.TILE
    B = 66 * T + 3
    streams = R.planted_fold_stream(fmt, bw, B, seed=7)
    assert len(streams) == 2 and -(-B // T) == 67
    for iq, (first, second) in zip(streams, ((2, 66), (10, 50))):
        assert iq.shape == (3 * B + 5000, 2) and iq.dtype == R.NP_DTYPE[fmt]
        u, _ = R.powers(iq, fmt, bw)
        in_bin = u[B:2 * B]
        top = np.flatnonzero(in_bin == in_bin.max())
        assert top.tolist() == [first * T + 17, second * T + 1]                  # the planted pair, and nowhere larger
        assert np.flatnonzero(in_bin == 0).tolist() == [65 * T + 4000] and np.count_nonzero(u == 0) == 1
        assert first % 64 == second % 64 or (first, second) == (10, 50)       # one lane of the fold in two rounds, or two
        assert u.max() == in_bin.max() and np.sort(u)[-3] <= in_bin.max() / 4 + 1e-30   # half scale elsewhere
        rec = R.envelope_fast(iq, fmt, bw, B)
        assert rec.size == 4 and rec["count"].tolist() == [B, B, B, 5000]
        assert rec["peak_sample"][1] == B + first * T + 17 and rec["power_min"][1] == 0 and np.all(rec["power_min"][[0, 2, 3]] > 0)
        big = (1.0, -1.0) if fmt == "cf32" else (-1.0, -1.0)
        assert (rec["peak_i"][1], rec["peak_q"][1]) == big
