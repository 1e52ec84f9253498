"""The matched filter on the MI355X (pfb_mf_*): both routes against the float64 restatement (tests/mf_ref.py) within
1e-5 * g * Bnd, the block seams on designed data, exact peak positions of PulseTrain pulses, cuttings of a stream, the
host / async / file routes and the TX / RX record pair."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import mf_ref as R  # noqa: E402
from gpu_support import cuda_torch  # noqa: E402
from mf_support import WORST, check, on_device, reset_worst, run_guarded  # noqa: E402
from sdr_channelizer_amd import (MatchedFilter, PulseTrain, compress, compress_iq_file, iqfile, pinned_empty,  # noqa: E402
                                 pulse_delay_from_iq_files, replica_from_pulse_train)
from sdr_channelizer_amd import _lib as L  # noqa: E402
from sdr_channelizer_amd.pdw import extract_pdws_raw  # noqa: E402


@pytest.fixture(scope="module")
def torch():
    t = cuda_torch()
    reset_worst()
    yield t
    # the largest error the module saw, in units of g * Bnd (the allowance is 1e-5): DESIGN.md section 15 quotes it
    print(f"\nmf worst error / (g Bnd) = {WORST['of_bound']:.3e} ({WORST['ratio']:.3f} of the allowance) at {WORST['where']}")


@pytest.mark.parametrize("nfft", [1024, 2048, 4096])
@pytest.mark.parametrize("fmt,bw", R.FORMATS)
def test_fused_against_the_restatement_on_short_streams(torch, fmt, bw, nfft):
    for K in (1, 2, 13, nfft // 2 - 1, nfft // 2):
        V = nfft - K + 1
        r = R.random_replica(K, K + nfft)
        counts = (0, 1, V - 1, V, V + 1, 2 * V + 3)
        raw = R.random_raw(fmt, bw, K - 1 + counts[-1], K + bw)
        x = R.unpack(raw, fmt, bw)
        for normalize in (False, True):
            ref = R.compress(x, r, normalize)
            for output in ("complex", "power"):
                with MatchedFilter(r, fmt, bw, output, normalize, fft_length=nfft, route="fused") as mf:
                    assert mf.plan.block_outputs == V and mf.plan.route == L.PFB_MF_ROUTE_FUSED
                    for i, outs in enumerate(counts):
                        n = K - 1 + outs
                        for misalign in (False, True):
                            mf.reset()
                            assert mf.outputs_for(n) == outs
                            y = run_guarded(torch, mf, on_device(torch, raw[: 2 * n], misalign), outs, output,
                                            misalign ^ (i % 2 == 1))
                            check(y, ref[:outs], x[:n], r, normalize, output, (fmt, nfft, K, n, output, normalize))
                            assert mf.next_index == outs
                            if outs:
                                assert mf.last_kernel == f"pfb_mf_fused<N{nfft},{fmt}>"


@pytest.mark.parametrize("K", [1, 512, 513, 1024, 1025, 2567])
def test_partitioned_route(torch, K):
    B = 512
    n = K + 3 * B + 5
    for fmt, bw in R.FORMATS if K in (1, 513) else R.FORMATS[1:2]:
        raw = R.random_raw(fmt, bw, n, K)
        x = R.unpack(raw, fmt, bw)
        r = R.random_replica(K, K + 1)
        for normalize, output in ((False, "complex"), (True, "power")):
            ref = R.compress(x, r, normalize)
            with MatchedFilter(r, fmt, bw, output, normalize, fft_length=1024, route="partitioned") as mf:
                assert mf.plan.partitions == -(-K // B) and mf.plan.block_outputs == B
                for m in (K - 1, K, n):
                    mf.reset()
                    y = run_guarded(torch, mf, on_device(torch, raw[: 2 * m], m == K), m - K + 1, output, m == n)
                    check(y, ref[: m - K + 1], x[:m], r, normalize, output, ("partitioned", fmt, K, m, output))
                assert mf.last_kernel == f"pfb_mf_partitioned<N1024,{fmt}>"
            if K <= B:   # the two routes on the same replica
                with MatchedFilter(r, fmt, bw, output, normalize, fft_length=1024, route="fused") as mf:
                    z = mf.process(torch.from_numpy(raw).cuda()).cpu().numpy()
                check(z, ref, x, r, normalize, output, ("fused next to partitioned", fmt, K))
                e = R.tolerance(x, r, normalize)
                if output == "complex":
                    assert np.abs(z - y).max() <= 2 * e


@pytest.mark.parametrize("K,fmt,bw", [(5600, "int16", 12), (65536, "int16", 16), (56000, "cf32", 1)])
def test_partitioned_long_replicas(torch, K, fmt, bw):
    n = K + 3 * 2048 + 5
    raw = R.random_raw(fmt, bw, n, K)
    x = R.unpack(raw, fmt, bw)
    r = R.random_replica(K, 3)
    for normalize, output in ((True, "complex"), (False, "power")):
        with MatchedFilter(r, fmt, bw, output, normalize) as mf:
            assert mf.plan.fft_length == 4096 and mf.plan.partitions == -(-K // 2048)
            y = mf.process(torch.from_numpy(raw).cuda()).cpu().numpy()
            assert mf.last_kernel == f"pfb_mf_partitioned<N4096,{fmt}>"
        check(y, R.compress(x, r, normalize), x, r, normalize, output, ("long", fmt, K, output))


def test_partitioned_call_longer_than_the_workspace(torch):
    """more output blocks than 64 MiB of spectra hold (8192 at 1024 points): the call is walked in chunks"""
    K, B = 600, 512
    n = 8192 * B + 2000
    raw = R.random_raw("int8", 8, n, 11)
    x = R.unpack(raw, "int8", 8)
    r = R.random_replica(K, 12)
    with MatchedFilter(r, "int8", 8, "power", True, fft_length=1024, route="partitioned") as mf:
        assert -(-(n - K + 1) // B) > mf.plan.workspace_bytes // (8 * 1024) - (mf.plan.partitions - 1)
        y = mf.process(torch.from_numpy(raw).cuda()).cpu().numpy()
    check(y, R.compress(x, r, True), x, r, True, "power", "chunk walk")


@pytest.mark.parametrize("route,K", [("fused", 300), ("partitioned", 700)])
@pytest.mark.parametrize("fmt,bw", R.FORMATS)
def test_one_sample_across_the_seams(torch, fmt, bw, route, K):
    """a single nonzero sample at s gives y[m] = g conj(r[s-m]) x[s] on s-K < m <= s and zero elsewhere: a reversed,
    shifted or unconjugated index shows against the random replica"""
    nfft = 1024
    V = nfft - K + 1 if route == "fused" else nfft // 2
    n = 2 * nfft + 77
    r = R.random_replica(K, 5)
    full = 1.0 if fmt == "cf32" else 2.0 ** (bw - 1)
    value = (0.75, -1.25) if fmt == "cf32" else (int(full) - 1, -int(full))   # cf32: float32 holds them exactly
    with MatchedFilter(r, fmt, bw, "complex", True, fft_length=nfft, route=route) as mf:
        assert mf.plan.block_outputs == V
        for s in (0, K - 1, V - 1, V, nfft - 1, nfft, n - 1):
            raw = np.zeros(2 * n, dtype=R.random_raw(fmt, bw, 1, 0).dtype)
            raw[2 * s], raw[2 * s + 1] = value
            xs = complex(value[0], value[1]) / full
            g = R.gain(r, True)
            want = np.zeros(n - K + 1, np.complex128)
            for m in range(max(0, s - K + 1), min(s, n - K) + 1):
                want[m] = g * np.conj(np.complex128(r[s - m])) * xs
            mf.reset()
            y = mf.process(torch.from_numpy(raw).cuda()).cpu().numpy()
            x = R.unpack(raw, fmt, bw)
            assert np.abs(want - R.compress(x, r, True)).max() <= 1e-12 * g * R.bound(x, r)
            check(y, want, x, r, True, "complex", ("seam", fmt, route, s))


@pytest.mark.parametrize("fmt,bw,low", [("int16", 16, -32768), ("int8", 8, -128)])
def test_full_scale_integers(torch, fmt, bw, low):
    n = 3000
    raw = np.full(2 * n, low, dtype=np.int16 if bw == 16 else np.int8)
    x = R.unpack(raw, fmt, bw)
    assert x[0] == -1 - 1j
    for route, K in (("fused", 500), ("partitioned", 900)):
        r = R.random_replica(K, 8)
        for output in ("complex", "power"):
            y = compress(torch.from_numpy(raw).cuda(), r, bit_width=bw, output=output, fft_length=1024, route=route)
            check(y.cpu().numpy(), R.compress(x, r), x, r, False, output, ("full scale", fmt, route, output))


PULSES = {
    "barker13": dict(pw=13 * 8, barker13=True, f0=3e6),
    "lfm": dict(pw=1000, lfm_extent_hz=40e6, f0=-20e6),
    "plain": dict(pw=200, f0=5e6),
}


@pytest.mark.parametrize("kind", list(PULSES))
def test_peak_position_is_exact(torch, kind):
    offset, n = 1234, 6000
    kw = dict(PULSES[kind], sample_format="int16", bit_width=12, fs=56e6, pri=1 << 20, amplitude=0.9, noise_sigma=0.0)
    r = replica_from_pulse_train(**kw)
    assert r.size == kw["pw"] and r.dtype == np.complex64 and np.abs(r).max() <= 1.0
    with PulseTrain(first_pulse=offset, **kw) as pt:
        iq = pt.generate(n)
    host = iq.cpu().numpy()
    assert not host[:offset].any() and not host[offset + r.size:].any() and host[offset: offset + r.size].any()
    for route in ("fused", "partitioned"):
        with MatchedFilter(r, "int16", 12, "power", True, fft_length=4096 if kind == "lfm" else 1024, route=route) as mf:
            p = mf.process(iq)
            assert int(torch.argmax(p).item()) == offset, (kind, route)
            # normalised: the match is the pulse's own amplitude, 1 (the replica holds the same integers)
            assert abs(float(p[offset].item()) - 1.0) < 1e-4


def test_a_pulse_under_the_envelope_threshold_is_found(torch):
    """an LFM pulse 3 dB under the noise per sample: the envelope extractor sees nothing at 15 dB, the compressed peak
    stands 27 dB over the noise and lands on the pulse's first sample"""
    offset, n, fs = 2345, 8000, 56e6
    kw = dict(PULSES["lfm"], sample_format="int16", bit_width=12, fs=fs, pri=1 << 20, amplitude=0.1)
    r = replica_from_pulse_train(**kw)
    with PulseTrain(first_pulse=offset, noise_sigma=0.1, seed=7, **kw) as pt:
        iq = pt.generate(n)
    with MatchedFilter(r, "int16", 12, "power", True) as mf:
        p = mf.process(iq)
    assert int(torch.argmax(p).item()) == offset
    pdws = extract_pdws_raw(iq, fs, 0.0, 0.0, bit_width=12, snr_threshold_db=15.0)
    assert len(pdws) == 0, pdws


def cuttings(n, K, seed):
    """edges of one cutting: a zero-length call, a cut inside the first K-1 samples, then random cuts"""
    rng = np.random.default_rng(seed)
    first = int(rng.integers(1, max(2, K - 1)))
    cuts = sorted({first, *rng.integers(1, n + 1, size=6).tolist()})
    k = int(rng.integers(0, len(cuts)))
    return [0] + cuts[:k] + [cuts[k]] + cuts[k:] + [n]   # cuts[k] twice: a call of length 0


@pytest.mark.parametrize("route,K", [("fused", 300), ("partitioned", 700)])
@pytest.mark.parametrize("fmt,bw", R.FORMATS)
def test_cuttings(torch, fmt, bw, route, K):
    n = 6000
    raw = R.random_raw(fmt, bw, n, 21)
    x = R.unpack(raw, fmt, bw)
    r = R.random_replica(K, 22)
    ref = R.compress(x, r)
    d = torch.from_numpy(raw).cuda()
    with MatchedFilter(r, fmt, bw, "complex", fft_length=1024, route=route) as mf:
        for c in range(12):
            edges = cuttings(n, K, 100 * c + K)
            assert any(a == b for a, b in zip(edges[:-1], edges[1:])) and 0 < edges[1] < K
            runs = []
            for _ in range(2):
                mf.reset()
                assert mf.next_index == 0
                parts, fed = [], 0
                for a, b in zip(edges[:-1], edges[1:]):
                    want = mf.outputs_for(b - a)
                    y = mf.process(d[2 * a: 2 * b])
                    fed = b
                    assert y.numel() == want == max(0, fed - K + 1) - sum(p.numel() for p in parts)
                    parts.append(y)
                    assert mf.next_index == max(0, fed - K + 1)
                runs.append(torch.cat(parts).cpu().numpy())
            assert runs[0].size == n - K + 1 and runs[0].tobytes() == runs[1].tobytes()
            check(runs[0], ref, x, r, False, "complex", ("cutting", fmt, route, c))


def test_host_pointers_and_tensors(torch):
    K, n = 777, 40000
    raw = R.random_raw("int16", 12, n, 31)
    x = R.unpack(raw, "int16", 12)
    r = R.random_replica(K, 32)
    ref = R.compress(x, r)
    with MatchedFilter(r, "int16", 12, "complex") as mf:
        y = mf.process(raw)                                  # pageable
        assert isinstance(y, np.ndarray)
        check(y, ref, x, r, False, "complex", "pageable")
        mf.reset()
        pin_in, pin_out = pinned_empty((n, 2), np.int16), pinned_empty((n - K + 1,), np.complex64)
        pin_in[:] = raw.reshape(-1, 2)
        z = mf.process(pin_in, out=pin_out)                  # page-locked, the caller's output buffer
        assert z.ctypes.data == pin_out.ctypes.data
        check(z, ref, x, r, False, "complex", "page-locked")
        mf.reset()
        t = mf.process(torch.from_numpy(raw).cuda().reshape(-1, 2))   # CUDA tensor in, CUDA tensor out
        assert t.is_cuda and t.dtype == torch.complex64 and t.shape == (n - K + 1,)
        check(t.cpu().numpy(), ref, x, r, False, "complex", "tensor")
        first = t.cpu().numpy().tobytes()
        mf.reset()                                           # after reset the first call's outputs come again
        assert mf.process(torch.from_numpy(raw).cuda()).cpu().numpy().tobytes() == first
    zc = compress(x.astype(np.complex64), r)                 # complex numpy in: cf32
    check(zc, ref, x.astype(np.complex64).astype(np.complex128), r, False, "complex", "complex64 numpy")


def test_async_on_a_caller_stream(torch):
    K, n = 1500, 50000
    raw = R.random_raw("int8", 8, n, 41)
    x = R.unpack(raw, "int8", 8)
    r = R.random_replica(K, 42)
    d = torch.from_numpy(raw).cuda()
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with MatchedFilter(r, "int8", 8, "power") as mf:
        mf.set_stream(s.cuda_stream)
        with torch.cuda.stream(s):
            halves = [mf.process(d[: 2 * 20001], sync=False), mf.process(d[2 * 20001:], sync=False)]
        mf.sync()
        y = torch.cat(halves).cpu().numpy()
        mf.set_stream(0)
    check(y, R.compress(x, r), x, r, False, "power", "async")


def test_capacity_leaves_the_state_untouched(torch):
    K, n = 100, 5000
    raw = R.random_raw("int16", 12, n, 51)
    r = R.random_replica(K, 52)
    d = torch.from_numpy(raw).cuda()
    lib = L.load()
    with MatchedFilter(r, "int16", 12, "complex") as mf:
        head = mf.process(d[: 2 * 1000]).cpu().numpy()
        out = torch.full((4000,), -5.0, dtype=torch.complex64, device="cuda")
        need = C.c_uint64()
        for call in (lambda: lib.pfb_mf_process(mf._h, C.c_void_p(d.data_ptr() + 4000), 4000, C.c_void_p(out.data_ptr()),
                                                3999, C.byref(need), L.PFB_MEM_DEVICE),
                     lambda: lib.pfb_mf_process_async(mf._h, C.c_void_p(d.data_ptr() + 4000), 4000,
                                                      C.c_void_p(out.data_ptr()), 0, C.byref(need))):
            assert call() == L.PFB_ERR_CAPACITY and need.value == 4000
            assert mf.next_index == 1000 - K + 1 and mf.outputs_for(4000) == 4000
        torch.cuda.synchronize()
        assert bool((out == -5.0).all())
        # device pointers off a sample / an output element
        assert lib.pfb_mf_process(mf._h, C.c_void_p(d.data_ptr() + 4002), 10, C.c_void_p(out.data_ptr()), 4000,
                                  C.byref(need), L.PFB_MEM_DEVICE) == L.PFB_ERR_BAD_ARG
        assert lib.pfb_mf_process_async(mf._h, C.c_void_p(d.data_ptr() + 4000), 10, C.c_void_p(out.data_ptr() + 4), 4000,
                                        C.byref(need)) == L.PFB_ERR_BAD_ARG
        assert lib.pfb_mf_process(mf._h, C.c_void_p(d.data_ptr()), 10, C.c_void_p(out.data_ptr()), 4000, C.byref(need),
                                  2) == L.PFB_ERR_BAD_ARG
        tail = mf.process(d[2 * 1000:]).cpu().numpy()
    x = R.unpack(raw, "int16", 12)
    check(np.concatenate([head, tail]), R.compress(x, r), x, r, False, "complex", "capacity")


@pytest.mark.parametrize("file_format", [1, 3])
def test_iq_file_route(torch, tmp_path, file_format):
    K, n = 400, 30000
    bw = 16 if file_format == 1 else 12
    raw = R.random_raw("int16", bw, n, 61)
    r = R.random_replica(K, 62)
    path = str(tmp_path / "dwell.iq")
    if file_format == 1:
        iqfile.write_iq_fmt1(path, raw.reshape(-1, 2), 56e6, start_time=3.5)
    else:
        iqfile.write_iq(path, raw.reshape(-1, 2), 56e6, 1e9, bw, start_time=3.5)
    x = R.unpack(raw, "int16", bw)
    for output in ("complex", "power"):
        y, info = compress_iq_file(path, r, output=output, normalize=True)
        assert info.file_format == file_format and info.packet.numSamples == n and info.packet.sampleStartTime == 3.5
        check(y, R.compress(x, r, True), x, r, True, output, ("file", file_format, output))
    with MatchedFilter(r, "int16", 12 if bw == 16 else 16) as mf:   # the record's bit width against the handle's
        with pytest.raises(L.PfbError) as e:
            mf.process_iq_file(path)
        assert e.value.status == L.PFB_ERR_BAD_FORMAT


def test_pulse_delay_from_iq_files(torch, tmp_path):
    """the pair tx_rx_pulses_usrp.cpp writes: a 13-chip burst of 8 samples per chip, and a dwell that holds it delayed"""
    code = np.array([1, 1, 1, 1, 1, -1, -1, 1, 1, -1, 1, -1, 1])
    burst = np.repeat(code, 8)
    tx = np.stack([16000 * burst, 4000 * burst], axis=1).astype(np.int16)
    lag, n, fs = 3777, 20000, 25e6
    rng = np.random.default_rng(71)
    rx = rng.normal(0.0, 200.0, size=(n, 2))
    rx[lag: lag + burst.size] += 0.05 * tx
    rx = np.rint(rx).astype(np.int16)
    tx_path, rx_path = str(tmp_path / "tx.iq"), str(tmp_path / "rx.iq")
    iqfile.write_iq_fmt1(tx_path, tx, fs, start_time=100.0)
    iqfile.write_iq_fmt1(rx_path, rx, fs, start_time=100.25)
    d = pulse_delay_from_iq_files(tx_path, rx_path)
    assert d["lag_samples"] == lag and d["lag_seconds"] == lag / fs and d["start_time_offset"] == 0.25
    x, r = R.unpack(rx.reshape(-1), "int16", 16), R.unpack(tx.reshape(-1), "int16", 16)
    ref = np.abs(R.compress(x, r)) ** 2
    assert int(np.argmax(ref)) == lag and abs(d["peak_power"] - ref[lag]) <= 1e-4 * ref[lag]
    long_tx = str(tmp_path / "long.iq")
    iqfile.write_iq_fmt1(long_tx, np.zeros((65537, 2), np.int16), fs)
    with pytest.raises(ValueError, match="65536"):
        pulse_delay_from_iq_files(long_tx, rx_path)
