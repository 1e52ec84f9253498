"""Envelopes and full-rate traces on the MI355X against the numpy restatement (trace_ref).  Integer formats and every
selection of cf32 bit for bit; cf32 power_mean to count * 2^-52 relative; mag to 1 float32 ulp; phase to
trace_ref.PHASE_TOL_DEG.  The shapes sit where the kernels change path: lane groups below 1024 samples per bin, one
workgroup per bin up to the tile, partials and a fold above it."""
import ctypes as C
import os

import numpy as np
import pytest

import trace_ref as R
from gpu_support import cuda_torch
from sdr_channelizer_amd import _lib as L
from sdr_channelizer_amd import PulseTrain, Trace, envelope, envelope_from_iq_file, iqfile, synth, trace
from trace_support import same, stream

pytestmark = pytest.mark.gpu
T = trace.TILE
BINS = [1, 2, 3, 7, 63, 64, 65, 255, 256, 257, 1000, T - 1, T, T + 1, 3 * T + 5, 100003]
INTEGER = [f for f in R.FORMATS if f[0] != "cf32"]


@pytest.fixture(scope="module")
def torch():
    return cuda_torch()


@pytest.mark.parametrize("fmt,bw", R.FORMATS)
def test_bin_sizes_and_call_lengths(torch, fmt, bw):
    iq, d = stream(torch, fmt, bw)
    for B in BINS:
        lengths = [0, 1, B - 1, B, B + 1, 5 * B + 3]
        with Trace(B, fmt, bw) as tr:
            # each length as the first call of a stream, from a pointer that moves with B
            for n in lengths + [300007]:
                tr.reset()
                assert tr.bins_for(n) == n // B
                got = tr.envelope(d[B:B + n])
                assert got.shape == (n // B, 48)
                assert same(np.concatenate([trace.as_records(got), tr.flush()]), R.envelope_fast(iq[B:B + n], fmt, bw, B), fmt), (B, n)
                assert tr.flush().size == 0
            # and one after the other: every call but the first meets an open bin
            tr.reset()
            got, at = [], 0
            for n in lengths:
                got.append(trace.as_records(tr.envelope(d[at:at + n])))
                at += n
            got.append(tr.flush())
            assert same(np.concatenate(got), R.envelope_fast(iq[:at], fmt, bw, B), fmt), B


@pytest.mark.parametrize("fmt,bw", [("int16", 12), ("int8", 8), ("cf32", 12)])
def test_vector_edges(torch, fmt, bw):
    """Every n from 0 to 70 with bins of 1, 5 and 64 samples, from a 16-byte aligned pointer and from one a sample past
    it: the peeled head and tail, nothing read past the call (a sample of full scale waits there) and nothing written
    outside the records."""
    row, slot = 80, 72 * 48
    cases = [(n, B, off) for n in range(71) for B in (1, 5, 64) for off in (0, 1)]
    iq = R.random_iq(fmt, bw, row, seed=3)
    iq = np.clip(iq // 2, -60, 60).astype(iq.dtype) if fmt != "cf32" else iq * np.float32(0.5)
    rows = np.empty((len(cases), row, 2), iq.dtype)
    big = 1.0 if fmt == "cf32" else (1 << (bw - 1)) - 1
    for r, (n, B, off) in enumerate(cases):
        rows[r] = big                      # whatever the call must not read would win every comparison
        rows[r, off:off + n] = iq[:n]
    d = torch.from_numpy(rows).cuda()
    assert d.data_ptr() % 16 == 0 and (row * iq.itemsize * 2) % 16 == 0
    out = torch.full((len(cases), slot), 0xA5, dtype=torch.uint8, device="cuda")
    last = {}
    handles = {B: Trace(B, fmt, bw) for B in (1, 5, 64)}
    try:
        for r, (n, B, off) in enumerate(cases):
            tr = handles[B]
            tr.reset()
            tr.envelope(d[r, off:off + n], out=out[r, 48:48 + (n // B) * 48], sync=False)
            last[r] = tr.flush()
    finally:
        for tr in handles.values():
            tr.close()
    got = out.cpu().numpy()
    for r, (n, B, off) in enumerate(cases):
        f = n // B
        want = R.envelope_fast(iq[:n], fmt, bw, B)
        recs = np.concatenate([got[r, 48:48 + f * 48].copy().view(R.BIN_DTYPE), last[r]])
        assert same(recs, want, fmt), (n, B, off)
        assert np.all(got[r, :48] == 0xA5) and np.all(got[r, 48 + f * 48:] == 0xA5), (n, B, off)


def test_extremes(torch):
    # u = 2^31 per sample: a 32-bit sum overflows at the second sample, a bin of 2^20 of them sums to 2^51
    n = (1 << 20) + 3 * T + 7
    iq = np.full((n, 2), -32768, np.int16)
    d = torch.from_numpy(iq).cuda()
    for B in (1, 2, 3, 4, 64, 1000, T, 3 * T + 5, 1 << 20):
        with Trace(B, "int16", 16) as tr:
            got = np.concatenate([trace.as_records(tr.envelope(d)), tr.flush()])
        assert np.array_equal(got.view(np.uint8), R.envelope_fast(iq, "int16", 16, B).view(np.uint8)), B
        assert np.all(got["power_max"] == 2.0) and np.all(got["power_mean"] == 2.0) and np.all(got["power_min"] == 2.0)
        assert np.array_equal(got["peak_sample"], np.arange(got.size, dtype=np.uint64) * B), B   # constant: the first index
        assert np.all(got["peak_i"] == -1.0) and np.all(got["peak_q"] == -1.0)
    # all zeros, every format
    for fmt, bw in R.FORMATS:
        z = np.zeros((3 * T + 100, 2), R.NP_DTYPE[fmt])
        for B in (1, 7, 300, T + 1):
            with Trace(B, fmt, bw) as tr:
                got = np.concatenate([trace.as_records(tr.envelope(torch.from_numpy(z).cuda())), tr.flush()])
            assert np.array_equal(got.view(np.uint8), R.envelope_fast(z, fmt, bw, B).view(np.uint8)), (fmt, B)
            assert not got["power_max"].any() and np.array_equal(got["peak_sample"], np.arange(got.size, dtype=np.uint64) * B)


@pytest.mark.parametrize("fmt,bw", R.FORMATS)
def test_single_spike(torch, fmt, bw):
    """One sample above a constant floor, at the first and the last sample of a bin, of a tile and of a call."""
    n = 4 * T + 11
    spike = (0.75, -0.5) if fmt == "cf32" else ((1 << (bw - 1)) - 1, -(1 << (bw - 1)))
    for B in (5, 300, T, 2 * T + 3, n + 100):
        places = sorted({0, n - 1, B - 1 if B <= n else n // 2, min(B, n - 1), T - 1, T, 2 * T - 1, 2 * T, (n // B) * B - 1 if n >= B else 1})
        with Trace(B, fmt, bw) as tr:
            for at in places:
                iq = np.full((n, 2), 0.25 if fmt == "cf32" else 1, R.NP_DTYPE[fmt])
                iq[at] = spike
                tr.reset()
                got = np.concatenate([trace.as_records(tr.envelope(torch.from_numpy(iq).cuda())), tr.flush()])
                assert same(got, R.envelope_fast(iq, fmt, bw, B), fmt), (B, at)
                assert got["peak_sample"][at // B] == at and got["peak_sample"][0] == (at if at < B else 0)


@pytest.mark.parametrize("fmt,bw", INTEGER)
@pytest.mark.parametrize("B", [3, 4096, 70001])
def test_any_cutting_gives_the_same_bits(torch, fmt, bw, B):
    n = 200000
    iq, d = stream(torch, fmt, bw)
    iq, d = iq[:n], d[:n]
    want = R.envelope_fast(iq, fmt, bw, B)
    rng = np.random.default_rng(B)
    with Trace(B, fmt, bw) as tr:
        whole = np.concatenate([trace.as_records(tr.envelope(d)), tr.flush()])
        assert np.array_equal(whole.view(np.uint8), want.view(np.uint8))
        # reset: the origin is back at 0 and nothing is carried
        tr.envelope(d[:B + 1])
        tr.reset()
        pieces, at, calls_in_bin, first = [], 0, {}, [1, 0, 1, 1, 2, 5]
        while at < n:
            m = first.pop(0) if first else int(rng.choice([0, 1, 2, 5, 97, 1023, 1024, T, T + 1, 9973, 30011]))
            m = min(m, n - at)
            f = tr.bins_for(m)
            if f > 0 and rng.random() < 0.3:   # too little room: the number needed, and no state change
                got = C.c_uint64()
                rc = tr._lib.pfb_trace_envelope(tr._h, C.c_void_p(d[at:].data_ptr()), m, C.c_void_p(d.data_ptr()), f - 1,
                                                C.byref(got), L.PFB_MEM_DEVICE)
                assert rc == L.PFB_ERR_CAPACITY and got.value == f and tr.bins_for(m) == f
            pieces.append(trace.as_records(tr.envelope(d[at:at + m], sync=bool(rng.integers(2)))))
            tr.sync()
            for b in range(at // B, (at + max(m, 1) - 1) // B + 1):
                calls_in_bin[b] = calls_in_bin.get(b, 0) + 1
            at += m
        pieces.append(tr.flush())
        assert max(calls_in_bin.values()) >= 3                    # a bin that straddles three calls and more
        got = np.concatenate(pieces)
        assert np.array_equal(got.view(np.uint8), want.view(np.uint8))
        # after the flush a new grid starts at the next sample, with the stream's indices going on
        again = np.concatenate([trace.as_records(tr.envelope(d[:B + 2])), tr.flush()])
        assert np.array_equal(again.view(np.uint8), R.envelope_fast(iq[:B + 2], fmt, bw, B, origin=n).view(np.uint8))


@pytest.mark.parametrize("fmt,bw", R.FORMATS)
def test_host_pointers_equal_device_pointers(torch, fmt, bw):
    iq, d = stream(torch, fmt, bw)
    n = 300007
    side = torch.cuda.Stream()
    for B in (5, 1000, T + 1, 100003):
        with Trace(B, fmt, bw) as tr:
            dev = np.concatenate([trace.as_records(tr.envelope(d[:n])), tr.flush()])
            tr.reset()
            host_recs = tr.envelope(iq[:n])
            assert host_recs.dtype == R.BIN_DTYPE
            host = np.concatenate([host_recs, tr.flush()])
            assert np.array_equal(host.view(np.uint8), dev.view(np.uint8)), B   # cf32 too: the same cutting, aligned pointers
            assert same(dev, R.envelope_fast(iq[:n], fmt, bw, B), fmt)
            # enqueue only, on a stream of the caller's, then sync
            tr.reset()
            tr.set_stream(side.cuda_stream)
            out = tr.envelope(d[:n], sync=False)
            tr.sync()
            assert np.array_equal(np.concatenate([trace.as_records(out), tr.flush()]).view(np.uint8), dev.view(np.uint8)), B
            tr.set_stream(0)


def test_host_call_crosses_a_staging_chunk(torch):
    n, B = (1 << 25) + 4099, 100003        # int8: 2 bytes per sample, just over 64 MiB
    rng = np.random.default_rng(11)
    iq = rng.integers(-128, 128, size=(n, 2), dtype=np.int8)
    with Trace(B, "int8", 8) as tr:
        host = np.concatenate([tr.envelope(iq), tr.flush()])
        tr.reset()
        dev = np.concatenate([trace.as_records(tr.envelope(torch.from_numpy(iq).cuda())), tr.flush()])
    assert host.size == -(-n // B) and np.array_equal(host.view(np.uint8), dev.view(np.uint8))
    k = (1 << 25) // B                      # the bin the chunk boundary cuts, and the last ones
    for b in (0, k, host.size - 2, host.size - 1):
        assert np.array_equal(host[b:b + 1].view(np.uint8), R.envelope(iq[b * B:(b + 1) * B], "int8", 8, B, origin=b * B).view(np.uint8)), b


def test_records_from_files(torch, tmp_path):
    one, three, eight, long_ = (os.path.join(tmp_path, f) for f in ("one.iq", "three.iq", "eight.iq", "long.iq"))
    n = 300001
    with PulseTrain(bit_width=16, amplitude=1.0) as pt:
        pt.write_iq(one, n, 4242, file_format=1)
    with PulseTrain() as pt:
        pt.write_iq(three, n, 4242, file_format=3)
        pt.write_iq(long_, (1 << 24) + 5, 0, file_format=3)     # just past the reader's chunk of 2^24 samples
    iq8 = R.random_iq("int8", 8, 70001, seed=2)
    iqfile.write_iq(eight, iq8, 56e6, 0.0, 8)
    for path, fmt, bw, max_bins in ((one, "int16", 16, 4096), (three, "int16", 12, 1000), (eight, "int8", 8, 70001),
                                    (eight, "int8", 8, 7), (long_, "int16", 12, 4096)):
        rec = iqfile.read_iq(path)
        env = envelope_from_iq_file(path, max_bins)
        B = max(1, -(-len(rec.iq) // max_bins))
        want = R.envelope_fast(rec.iq, fmt, bw, B)
        assert env.bin_samples == B and env.count.size == want.size == -(-len(rec.iq) // B) and want["count"][-1] == (len(rec.iq) - 1) % B + 1
        assert np.array_equal(env.peak_sample, want["peak_sample"]) and np.array_equal(env.count, want["count"])
        assert np.array_equal(env.mag_max, np.sqrt(want["power_max"])) and np.array_equal(env.mag_min, np.sqrt(want["power_min"]))
        assert np.array_equal(env.rms, np.sqrt(want["power_mean"]))
        assert np.array_equal(env.t, np.arange(want.size) * B / 56e6) and env.info.packet.numSamples == len(rec.iq)
        assert np.array_equal(env.peak_phase_deg, np.degrees(np.arctan2(want["peak_q"].astype(np.float64), want["peak_i"].astype(np.float64))))
        # the raw call: too little room names the number needed
        f, b = C.c_uint64(), C.c_uint32()
        recs = np.zeros(want.size, R.BIN_DTYPE)
        call = L.load().pfb_trace_envelope_from_iq_file
        assert call(path.encode(), max_bins, C.c_void_p(recs.ctypes.data), want.size - 1, C.byref(f), C.byref(b), None, -1) == L.PFB_ERR_CAPACITY
        assert f.value == want.size and b.value == B
        assert call(path.encode(), max_bins, C.c_void_p(recs.ctypes.data), want.size, C.byref(f), C.byref(b), None, -1) == L.PFB_OK
        assert f.value == want.size and np.array_equal(recs.view(np.uint8), want.view(np.uint8))
    # the one-shot on a buffer is the same view
    rec = iqfile.read_iq(three)
    env = envelope(rec.iq, max_bins=1000, bit_width=12, fs=56e6)
    by_file = envelope_from_iq_file(three, 1000)
    for a, b in zip(env[:8], by_file[:8]):
        assert np.array_equal(a, b)
    env = envelope(torch.from_numpy(np.array(rec.iq)).cuda(), bin_samples=301, bit_width=12)
    assert np.array_equal(env.t, np.arange(-(-n // 301)) * 301.0) and env.count[-1] == n % 301


@pytest.mark.parametrize("fmt,bw", R.FORMATS)
def test_full_rate_trace(torch, fmt, bw):
    n = 200003
    iq = R.phase_inputs(fmt, bw, n, seed=5)
    d = torch.from_numpy(iq).cuda()
    mag64, ph64 = R.mag_phase64(iq, fmt, bw)
    with Trace(64, fmt, bw) as tr:
        tr.envelope(d[:100])                         # an open bin of 36 samples
        mag, ph = tr.mag_phase(d)
        mag, ph = mag.cpu().numpy(), ph.cpu().numpy()
        assert mag.dtype == ph.dtype == np.float32
        err = np.abs(mag.astype(np.float64) - mag64) / R.ulp32(mag64)
        print(f"{fmt}/{bw}: mag {err.max():.3f} ulp, phase {R.phase_diff(ph, ph64).max():.3e} deg (bound {R.PHASE_TOL_DEG:.3e})")
        assert err.max() <= 1.0
        assert R.phase_diff(ph, ph64).max() <= R.PHASE_TOL_DEG
        # one output alone; the other pointer is NULL
        only, none = tr.mag_phase(d, phase=False)
        assert none is None and np.array_equal(only.cpu().numpy(), mag)
        guard = torch.full((n + 2,), 7.0, dtype=torch.float32, device="cuda")
        L.check(tr._lib.pfb_trace_samples(tr._h, C.c_void_p(d.data_ptr()), n, None, C.c_void_p(guard.data_ptr() + 4),
                                          L.PFB_MEM_DEVICE), "pfb_trace_samples")
        g = guard.cpu().numpy()
        assert g[0] == 7.0 and g[-1] == 7.0 and np.array_equal(g[1:-1], ph)
        # host pointers: the same bits
        hm, hp = tr.mag_phase(iq)
        assert np.array_equal(hm, mag) and np.array_equal(hp, ph)
        assert np.array_equal(tr.mag_phase(iq[:1000], phase=False)[0], mag[:1000])
        # the envelope's state is where it was: 28 more samples close the bin that holds samples 64 .. 127
        rest = trace.as_records(tr.envelope(d[100:128]))
        assert rest.size == 1 and same(rest, R.envelope_fast(iq[:128], fmt, bw, 64)[1:], fmt)


@pytest.mark.parametrize("fmt,bw", [("int16", 12), ("int8", 8), ("cf32", 12)])
def test_full_rate_vector_edges(torch, fmt, bw):
    """Every n from 0 to 70 from an aligned input pointer and from one a sample past it, into outputs that start on a
    16-byte boundary and one float past it: nothing written outside [out, out + n)."""
    row = 80
    cases = [(n, off, ooff) for n in range(71) for off in (0, 1) for ooff in (0, 1)]
    iq = R.phase_inputs(fmt, bw, row, seed=8)
    m64, p64 = R.mag_phase64(iq, fmt, bw)
    d = torch.from_numpy(np.broadcast_to(iq, (2, row, 2)).copy()).cuda()
    assert d.data_ptr() % 16 == 0
    mag = torch.full((len(cases), row), 7.0, dtype=torch.float32, device="cuda")
    ph = torch.full((len(cases), row), 7.0, dtype=torch.float32, device="cuda")
    with Trace(64, fmt, bw) as tr:
        for r, (n, off, ooff) in enumerate(cases):
            src = d[0, off:off + n]
            rc = tr._lib.pfb_trace_samples(tr._h, C.c_void_p(src.data_ptr()), n, C.c_void_p(mag[r, ooff:].data_ptr()),
                                           C.c_void_p(ph[r, ooff:].data_ptr()), L.PFB_MEM_DEVICE)
            assert rc == L.PFB_OK
    mag, ph = mag.cpu().numpy(), ph.cpu().numpy()
    for r, (n, off, ooff) in enumerate(cases):
        sl = slice(ooff, ooff + n)
        assert np.all(np.abs(mag[r, sl].astype(np.float64) - m64[off:off + n]) <= R.ulp32(m64[off:off + n])), (n, off, ooff)
        assert np.all(R.phase_diff(ph[r, sl], p64[off:off + n]) <= R.PHASE_TOL_DEG), (n, off, ooff)
        for a in (mag, ph):
            assert np.all(a[r, :ooff] == 7.0) and np.all(a[r, ooff + n:] == 7.0), (n, off, ooff)


def test_call_arguments(torch):
    lib = L.load()
    with Trace(64, "int16", 12) as tr:
        d = torch.zeros((256, 2), dtype=torch.int16, device="cuda")
        out = torch.zeros(8 * 48, dtype=torch.uint8, device="cuda")
        f = C.c_uint64()
        p, o = d.data_ptr(), out.data_ptr()
        assert lib.pfb_trace_envelope(tr._h, C.c_void_p(p), 256, C.c_void_p(o), 8, C.byref(f), 2) == L.PFB_ERR_BAD_ARG
        assert lib.pfb_trace_envelope(tr._h, C.c_void_p(p + 2), 128, C.c_void_p(o), 8, C.byref(f), L.PFB_MEM_DEVICE) == L.PFB_ERR_BAD_ARG
        assert lib.pfb_trace_envelope(tr._h, C.c_void_p(p), 128, C.c_void_p(o + 4), 8, C.byref(f), L.PFB_MEM_DEVICE) == L.PFB_ERR_BAD_ARG
        assert lib.pfb_trace_envelope(tr._h, None, 128, C.c_void_p(o), 8, C.byref(f), L.PFB_MEM_DEVICE) == L.PFB_ERR_BAD_ARG
        assert lib.pfb_trace_envelope(tr._h, C.c_void_p(p), 128, None, 8, C.byref(f), L.PFB_MEM_DEVICE) == L.PFB_ERR_BAD_ARG
        assert lib.pfb_trace_envelope_async(tr._h, C.c_void_p(p), 256, C.c_void_p(o), 3, C.byref(f)) == L.PFB_ERR_CAPACITY and f.value == 4
        assert lib.pfb_trace_samples(tr._h, C.c_void_p(p), 16, C.c_void_p(o + 2), None, L.PFB_MEM_DEVICE) == L.PFB_ERR_BAD_ARG
        assert lib.pfb_trace_samples(tr._h, C.c_void_p(p), 16, C.c_void_p(o), None, 7) == L.PFB_ERR_BAD_ARG
        assert tr.bins_for(64) == 1 and tr.flush().size == 0       # none of them moved the stream
        assert tr.device_index == torch.cuda.current_device()
    with pytest.raises(TypeError):
        with Trace(64, "int8", 8) as tr:
            tr.envelope(d)


def test_pulse_train_envelope(torch):
    """The product as a user meets it: the pulse source's stream in bins of one pulse period.  Without noise every full
    bin's largest magnitude is the amplitude to one LSB (each component is rounded to the nearest integer: at most
    sqrt(2)/2 LSB), and it sits inside that period's pulse.  The default stream carries noise of at most 131070 *
    noise_gain * 2^-20 LSB per component (four 16-bit uniforms, the header's definition): its peaks are held to that."""
    pri, pw, full = int(round(synth.FS * synth.PRI_S)), int(round(synth.FS * synth.PW_S)), 2048
    n = 6 * pri + 1234
    for kw in (dict(noise_sigma=0.0), dict()):
        with PulseTrain(**kw) as pt, Trace(pri) as tr:
            iq = pt.generate(n)
            recs = trace.as_records(tr.envelope(iq))
            slack = 1.0 + np.sqrt(2.0) * 131070 * pt.params.noise_gain / 2.0 ** 20
        assert recs.size == 6 and np.all(recs["count"] == pri)
        assert np.array_equal(recs.view(np.uint8), R.envelope_fast(iq.cpu().numpy(), "int16", 12, pri, partial=False).view(np.uint8))
        lsb = np.sqrt(recs["power_max"]) * full
        assert np.all(np.abs(lsb - synth.AMPLITUDE * full) <= slack), (kw, lsb)
        if not kw:
            assert slack < synth.AMPLITUDE * full / 2      # off samples cannot outgrow the pulse
        at = recs["peak_sample"].astype(np.int64) - np.arange(6) * pri
        assert np.all((0 <= at) & (at < pw)), at
