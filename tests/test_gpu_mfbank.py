"""The matched-filter bank on the MI355X (pfb_mfbank_*): both outputs against the float64 restatement
(tests/mfbank_ref.py) within the matched filter's own allowance, 1e-5 * g * Bnd, on the smallest shapes where the kernel
can go wrong; a pulse on a carrier of whole bins, a designed tie, the motivating case, cuttings of a stream, the host /
async / file routes, samples that are not finite and the TX / RX record pair."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import mf_ref as R  # noqa: E402
import mfbank_ref as B  # noqa: E402
from gpu_support import cuda_torch  # noqa: E402
from mf_support import on_device  # noqa: E402
from sdr_channelizer_amd import (MatchedFilter, MatchedFilterBank, PulseTrain, compress_bank, iqfile, pinned_empty,  # noqa: E402
                                 pulse_delay_and_offset_from_iq_files, replica_from_pulse_train)
from sdr_channelizer_amd import _lib as L  # noqa: E402

GUARD = 5


@pytest.fixture(scope="module")
def torch():
    t = cuda_torch()
    B.reset_worst()
    yield t
    # the largest error the module saw, in units of g * Bnd (the allowance is 1e-5): DESIGN.md section 18 quotes it
    print(f"\nmfbank worst error / (g Bnd) = {B.WORST['of_bound']:.3e} ({B.WORST['ratio']:.3f} of the allowance) "
          f"at {B.WORST['where']}")


def run_guarded(torch, bank, d_in, outputs, misalign):
    """process into a caller's buffer with guard elements around it (and between the rows of a surface, whose pitch is
    larger than the row) that must survive; returns what process returns, on the host"""
    H = bank.num_hypotheses
    if bank.output == "best":
        lead = GUARD if misalign else GUARD + 1   # cells: 40 bytes (off a 16-byte boundary) or 48
        buf = torch.full((lead + outputs + GUARD, 2), -77.0, dtype=torch.float32, device="cuda")
        power, hyp = bank.process(d_in, out=buf[lead: lead + outputs])
        assert power.numel() == hyp.numel() == outputs and (outputs == 0 or power.data_ptr() == buf[lead].data_ptr())
        host = buf.cpu().numpy()
        assert np.all(host[:lead] == -77.0) and np.all(host[lead + outputs:] == -77.0)
        return host[lead: lead + outputs, 0].copy(), host[lead: lead + outputs, 1].copy().view(np.int32)
    lead = GUARD if misalign else GUARD + 3       # floats: 20 bytes or 32
    pitch = outputs + (3 if misalign else 4)       # odd pitch: the rows start at every phase of 16 bytes
    buf = torch.full((lead + H * pitch + GUARD,), -77.0, dtype=torch.float32, device="cuda")
    rows = buf[lead: lead + H * pitch].view(H, pitch)
    p = bank.process(d_in, out=rows)
    assert tuple(p.shape) == (H, outputs) and (outputs == 0 or p.data_ptr() == rows.data_ptr())
    host = buf.cpu().numpy()
    body = host[lead: lead + H * pitch].reshape(H, pitch)
    assert np.all(host[:lead] == -77.0) and np.all(host[lead + H * pitch:] == -77.0) and np.all(body[:, outputs:] == -77.0)
    return body[:, :outputs].copy()


def check(got, output, yref, e, where, keep=None):
    if output == "best":
        B.check_best(got[0], got[1], yref, e, where, keep)
    else:
        B.check_surface(got, yref, e, where, keep)


def host(got):
    return tuple(g.cpu().numpy() for g in got) if isinstance(got, tuple) else got.cpu().numpy()


@pytest.mark.parametrize("nfft", [1024, 2048, 4096])
@pytest.mark.parametrize("fmt,bw", R.FORMATS)
def test_against_the_restatement_on_short_streams(torch, fmt, bw, nfft):
    Hs, steps = (1, 2, 3, 17), (1, 3)
    seen = set()
    for k, K in enumerate((1, 2, 13, nfft // 2 - 1, nfft // 2)):
        V = nfft - K + 1
        r = R.random_replica(K, K + nfft)
        counts = (0, 1, V - 1, V, V + 1, 2 * V + 3)
        raw = R.random_raw(fmt, bw, K - 1 + counts[-1], K + bw)
        x = R.unpack(raw, fmt, bw)
        for i, H in enumerate(Hs):
            step = steps[(i + k) % 2]
            # 0, -1, -8, and banks whose q_h pass +nfft/2 and -nfft/2 on the way
            first_bin = (0, -1, -8, nfft // 2 // step - 1, -(nfft // 2 // step) - 1)[(i + k) % 5]
            normalize = (i + k) % 2 == 1
            seen.add((H, step, (i + k) % 5))
            yref = B.surface(x, r, first_bin, H, step, nfft, normalize)
            for output in ("best", "surface"):
                with MatchedFilterBank(r, fmt, bw, first_bin=first_bin, num_hypotheses=H, bin_step=step, output=output,
                                       normalize=normalize, fft_length=nfft) as bank:
                    assert (bank.plan.block_outputs, bank.plan.num_hypotheses, bank.plan.fft_length) == (V, H, nfft)
                    for j, outs in enumerate(counts):
                        n = K - 1 + outs
                        misalign = (i + j) % 2 == 1
                        bank.reset()
                        assert bank.outputs_for(n) == outs
                        got = run_guarded(torch, bank, on_device(torch, raw[: 2 * n], misalign), outs, misalign ^ (j % 2 == 1))
                        check(got, output, yref[:, :outs], R.tolerance(x[:n], r, normalize),
                              (fmt, nfft, K, H, step, first_bin, n, output))
                        assert bank.next_index == outs
                        if outs:
                            assert bank.last_kernel == f"pfb_mfbank_fused<N{nfft},{fmt},{output}>"
    assert {s[0] for s in seen} == set(Hs) and {s[1] for s in seen} == {1, 3} and {s[2] for s in seen} == set(range(5))


@pytest.mark.parametrize("nfft,K", [(1024, 300), (4096, 2048)])
def test_one_hypothesis_at_bin_zero_is_the_matched_filter(torch, nfft, K):
    n = 3 * nfft
    for fmt, bw in R.FORMATS:
        raw = R.random_raw(fmt, bw, n, 7)
        x = R.unpack(raw, fmt, bw)
        r = R.random_replica(K, 8)
        d = torch.from_numpy(raw).cuda()
        yref = R.compress(x, r)
        e = R.tolerance(x, r)
        with MatchedFilter(r, fmt, bw, "power", fft_length=nfft, route="fused") as mf:
            want = mf.process(d).cpu().numpy().astype(np.float64)
        for output in ("best", "surface"):
            got = host(compress_bank(d, r, first_bin=0, num_hypotheses=1, bit_width=bw, output=output, fft_length=nfft))
            p = got[0]   # the powers of the cells, or row 0 of the surface
            assert output == "surface" or not got[1].any()
            assert np.all(np.abs(p.astype(np.float64) - want) <= 2 * e * (2 * np.abs(yref) + e)), (fmt, output)


def barker_pulse(offset, n, bins_off, nfft, fs=56e6):
    """a noise-free Barker-13 pulse of 13 x 39 samples that starts at `offset`, on a carrier of exactly bins_off bins of
    an nfft-point FFT, and its replica at carrier 0"""
    kw = dict(pw=13 * 39, barker13=True, sample_format="int16", bit_width=12, fs=fs, pri=1 << 20, amplitude=0.9,
              noise_sigma=0.0)
    r = replica_from_pulse_train(f0=0.0, **kw)
    with PulseTrain(first_pulse=offset, f0=bins_off * fs / nfft, **kw) as pt:
        iq = pt.generate(n)
    return iq, r


def test_a_pulse_on_a_carrier_of_whole_bins(torch):
    nfft, offset, n = 1024, 1234, 4000
    # q, first_bin, H, bin_step, the h with q_h = q; the bank around 511 passes nfft/2
    for q, first_bin, H, step, h in ((37, 33, 9, 1, 4), (-200, -204, 9, 1, 4), (511, 507, 9, 1, 4), (36, 10, 5, 3, 2),
                                     (-201, -69, 5, 3, 2)):
        iq, r = barker_pulse(offset, n, q, nfft)
        assert r.size == 13 * 39 and (first_bin + h) * step == q
        with MatchedFilterBank(r, "int16", 12, first_bin=first_bin, num_hypotheses=H, bin_step=step, normalize=True,
                               fft_length=nfft) as bank:
            power, hyp = bank.process(iq)
            at = int(torch.argmax(power).item())
            assert at == offset and int(hyp[at].item()) == h, (q, first_bin, step)
            # normalised: the pulse's own amplitude, 1.  I and Q are each rounded to an integer of 0.9 * 2048 = 1843, at
            # most 0.5 * sqrt(2) / 1843 = 3.9e-4 of the amplitude even if every sample erred the same way: 7.7e-4 in power
            assert abs(float(power[at].item()) - 1.0) < 1e-3
            assert bank.frequencies(56e6)[h] == q * 56e6 / nfft


def test_a_tie_goes_to_the_lowest_hypothesis(torch):
    """a replica that is zero outside its first sample has a flat spectrum: the rotated reads fetch the same values, every
    hypothesis computes the same bits, and the strict comparison keeps h = 0"""
    r = np.zeros(5, np.complex64)
    r[0] = 0.5 - 0.25j
    raw = R.random_raw("int16", 12, 3000, 3)
    x = R.unpack(raw, "int16", 12)
    d = torch.from_numpy(raw).cuda()
    for nfft in (1024, 2048, 4096):
        power, hyp = host(compress_bank(d, r, first_bin=-3, num_hypotheses=7, fft_length=nfft))
        assert not hyp.any() and power.any()
        surf = host(compress_bank(d, r, first_bin=-3, num_hypotheses=7, output="surface", fft_length=nfft))
        assert all(surf[h].tobytes() == surf[0].tobytes() for h in range(7))
        yref = B.surface(x, r, -3, 7, 1, nfft)
        B.check_surface(surf, yref, R.tolerance(x, r), ("tie", nfft))
        B.check_best(power, hyp, yref, R.tolerance(x, r), ("tie", nfft))


def test_a_pulse_37_bins_off_its_replica(torch):
    """the case the bank is for: the plain matched filter puts the pulse at a wrong sample, the bank at the right one"""
    nfft, offset, n = 1024, 2000, 5000
    iq, r = barker_pulse(offset, n, 37, nfft)
    with MatchedFilter(r, "int16", 12, "power", True, fft_length=nfft) as mf:
        p = mf.process(iq)
    assert int(torch.argmax(p).item()) != offset and float(p.max().item()) < 0.02
    power, hyp = compress_bank(iq, r, first_bin=30, num_hypotheses=10, normalize=True, fft_length=nfft)
    at = int(torch.argmax(power).item())
    assert at == offset and int(hyp[at].item()) == 7 and float(power[at].item()) > 0.99


def cuttings(n, K, seed):
    """edges of one cutting: a zero-length call, a cut inside the first K-1 samples, then random cuts"""
    rng = np.random.default_rng(seed)
    first = int(rng.integers(1, max(2, K - 1)))
    cuts = sorted({first, *rng.integers(1, n + 1, size=6).tolist()})
    k = int(rng.integers(0, len(cuts)))
    return [0] + cuts[:k] + [cuts[k]] + cuts[k:] + [n]   # cuts[k] twice: a call of length 0


@pytest.mark.parametrize("fmt,bw", R.FORMATS)
def test_cuttings(torch, fmt, bw):
    K, n, nfft, H = 300, 5000, 1024, 6
    raw = R.random_raw(fmt, bw, n, 21)
    x = R.unpack(raw, fmt, bw)
    r = R.random_replica(K, 22)
    yref = B.surface(x, r, -2, H, 3, nfft)
    e = R.tolerance(x, r)
    d = torch.from_numpy(raw).cuda()
    for output in ("best", "surface"):
        with MatchedFilterBank(r, fmt, bw, first_bin=-2, num_hypotheses=H, bin_step=3, output=output,
                               fft_length=nfft) as bank:
            whole = host(bank.process(d))
            check(whole, output, yref, e, ("one call", fmt, output))
            for c in range(6):
                edges = cuttings(n, K, 100 * c + K)
                runs = []
                for _ in range(2):
                    bank.reset()
                    assert bank.next_index == 0
                    parts = []
                    for a, b in zip(edges[:-1], edges[1:]):
                        want = bank.outputs_for(b - a)
                        got = host(bank.process(d[2 * a: 2 * b]))
                        assert (got[0].shape[-1] if output == "best" else got.shape[1]) == want
                        parts.append(got)
                        assert bank.next_index == max(0, b - K + 1)
                    if output == "best":
                        runs.append((np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])))
                    else:
                        runs.append(np.concatenate(parts, axis=1))
                check(runs[0], output, yref, e, ("cutting", fmt, output, c))
                if output == "best":   # the same cutting twice: the same bytes
                    assert runs[0][0].tobytes() == runs[1][0].tobytes() and runs[0][1].tobytes() == runs[1][1].tobytes()
                else:                  # and every power of the cutting within twice the allowance of the one call's
                    assert runs[0].tobytes() == runs[1].tobytes()
                    diff = np.abs(runs[0].astype(np.float64) - whole.astype(np.float64))
                    assert np.all(diff <= 2 * e * (2 * np.abs(yref) + e)), (fmt, c)


def test_host_pointers_and_a_surface_in_several_staging_steps(torch):
    """numpy in, numpy out.  H = 1024 rows leave 2^24 / 1024 = 16384 samples per staging step, so this call takes two;
    blocks start where a step starts, so device calls cut at the same sample give the same bytes -- every row and every
    output of the host route is compared with them, and six rows with the restatement"""
    K, nfft, H, step_samples = 40, 1024, 1024, 16384
    n = step_samples + 500
    F = n - K + 1
    raw = R.random_raw("int16", 12, n, 31)
    x = R.unpack(raw, "int16", 12)
    r = R.random_replica(K, 32)
    e = R.tolerance(x, r)
    d = torch.from_numpy(raw).cuda()
    with MatchedFilterBank(r, "int16", 12, first_bin=-512, num_hypotheses=H, output="surface", fft_length=nfft) as bank:
        p = bank.process(raw)
        assert isinstance(p, np.ndarray) and p.shape == (H, F) and p.dtype == np.float32
        bank.reset()
        cut = np.concatenate([bank.process(d[: 2 * step_samples]).cpu().numpy(),
                              bank.process(d[2 * step_samples:]).cpu().numpy()], axis=1)
        assert p.tobytes() == cut.tobytes()
        rows = [0, 1, 511, 512, 513, 1023]
        yref = np.stack([R.compress(x, B.modulated(r, q, nfft)) for q in B.bins(-512, H, 1)[rows]])
        B.check_surface(np.ascontiguousarray(p[rows]), yref, e, "host surface")
        bank.reset()
        mine = np.full((H, F + 7), -3.0, np.float32)   # the caller's rows, a pitch of their own
        q = bank.process(raw.reshape(-1, 2), out=mine)
        assert q.ctypes.data == mine.ctypes.data and np.all(mine[:, F:] == -3.0) and q.tobytes() == p.tobytes()
    H = 6
    yref = B.surface(x, r, -2, H, 5, nfft)
    with MatchedFilterBank(r, "int16", 12, first_bin=-2, num_hypotheses=H, bin_step=5, fft_length=nfft) as bank:
        pin = pinned_empty((n, 2), np.int16)
        pin[:] = raw.reshape(-1, 2)
        power, hyp = bank.process(pin)
        assert isinstance(power, np.ndarray) and power.dtype == np.float32 and hyp.dtype == np.int32
        B.check_best(power, hyp, yref, e, "host best")


def test_async_on_a_caller_stream_and_a_stream_switch(torch):
    K, n, nfft, H = 700, 30000, 2048, 5
    raw = R.random_raw("int8", 8, n, 41)
    x = R.unpack(raw, "int8", 8)
    r = R.random_replica(K, 42)
    yref = B.surface(x, r, -1, H, 2, nfft, True)
    d = torch.from_numpy(raw).cuda()
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    for output in ("best", "surface"):
        with MatchedFilterBank(r, "int8", 8, first_bin=-1, num_hypotheses=H, bin_step=2, output=output, normalize=True,
                               fft_length=nfft) as bank:
            bank.set_stream(s.cuda_stream)
            with torch.cuda.stream(s):
                first = bank.process(d[: 2 * 10001], sync=False)
                second = bank.process(d[2 * 10001: 2 * 20000], sync=False)
            bank.set_stream(0)   # what the old stream still has queued comes first
            third = bank.process(d[2 * 20000:], sync=False)
            bank.sync()
            s.synchronize()
            parts = [host(first), host(second), host(third)]
        if output == "best":
            got = (np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts]))
        else:
            got = np.concatenate(parts, axis=1)
        check(got, output, yref, R.tolerance(x, r, True), ("async", output))


def test_capacity_and_pitch_leave_the_state_untouched(torch):
    K, n = 100, 5000
    raw = R.random_raw("int16", 12, n, 51)
    r = R.random_replica(K, 52)
    d = torch.from_numpy(raw).cuda()
    lib = L.load()
    need = C.c_uint64()
    for output, elem in (("best", 8), ("surface", 4)):
        with MatchedFilterBank(r, "int16", 12, first_bin=0, num_hypotheses=3, output=output, fft_length=1024) as bank:
            bank.process(d[: 2 * 1000])
            out = torch.full((3 * 4000 * 2,), -5.0, dtype=torch.float32, device="cuda")
            src, dst = C.c_void_p(d.data_ptr() + 4000), C.c_void_p(out.data_ptr())
            calls = [lambda: lib.pfb_mfbank_process(bank._h, src, 4000, dst, 3999, 4000, C.byref(need), L.PFB_MEM_DEVICE),
                     lambda: lib.pfb_mfbank_process_async(bank._h, src, 4000, dst, 0, 4000, C.byref(need))]
            for call in calls:
                assert call() == L.PFB_ERR_CAPACITY and need.value == 4000
            bad = [lambda: lib.pfb_mfbank_process(bank._h, C.c_void_p(d.data_ptr() + 4002), 10, dst, 4000, 4000, C.byref(need),
                                                  L.PFB_MEM_DEVICE),
                   lambda: lib.pfb_mfbank_process_async(bank._h, src, 10, C.c_void_p(out.data_ptr() + elem // 2), 4000, 4000,
                                                        C.byref(need)),
                   lambda: lib.pfb_mfbank_process(bank._h, src, 10, dst, 4000, 4000, C.byref(need), 2)]
            if output == "surface":   # a pitch shorter than the row
                bad.append(lambda: lib.pfb_mfbank_process(bank._h, src, 4000, dst, 4000, 3999, C.byref(need), L.PFB_MEM_DEVICE))
            for call in bad:
                assert call() == L.PFB_ERR_BAD_ARG
            assert bank.next_index == 1000 - K + 1 and bank.outputs_for(4000) == 4000
            torch.cuda.synchronize()
            assert bool((out == -5.0).all())


@pytest.mark.parametrize("file_format", [1, 3])
def test_iq_file_route(torch, tmp_path, file_format):
    K, n, nfft, H = 400, 30000, 1024, 4
    bw = 16 if file_format == 1 else 12
    raw = R.random_raw("int16", bw, n, 61)
    r = R.random_replica(K, 62)
    path = str(tmp_path / "dwell.iq")
    if file_format == 1:
        iqfile.write_iq_fmt1(path, raw.reshape(-1, 2), 56e6, start_time=3.5)
    else:
        iqfile.write_iq(path, raw.reshape(-1, 2), 56e6, 1e9, bw, start_time=3.5)
    x = R.unpack(raw, "int16", bw)
    yref = B.surface(x, r, -6, H, 4, nfft, True)
    for output in ("best", "surface"):
        with MatchedFilterBank(r, "int16", bw, first_bin=-6, num_hypotheses=H, bin_step=4, output=output, normalize=True,
                               fft_length=nfft) as bank:
            got, info = bank.process_iq_file(path)
            assert info.file_format == file_format and info.packet.numSamples == n and info.packet.sampleStartTime == 3.5
            check(got, output, yref, R.tolerance(x, r, True), ("file", file_format, output))
    with MatchedFilterBank(r, "int16", 12 if bw == 16 else 16, first_bin=0, num_hypotheses=2) as bank:
        with pytest.raises(L.PfbError) as err:   # the record's bit width against the handle's
            bank.process_iq_file(path)
        assert err.value.status == L.PFB_ERR_BAD_FORMAT


@pytest.mark.parametrize("bad", [np.nan, np.inf])
def test_samples_that_are_not_finite_spoil_their_blocks_only(torch, bad):
    K, nfft, H = 200, 1024, 3
    V = nfft - K + 1
    n = 4 * V + K - 1 + 17
    outputs = n - K + 1
    base = R.random_raw("cf32", 1, n, 71)
    r = R.random_replica(K, 72)
    for s in (0, K - 1, V, 2 * V + 300, n - 1):
        raw = base.copy()
        raw[2 * s] = bad
        clean = base.copy()
        clean[2 * s: 2 * s + 2] = 0.0   # the outputs that do not see sample s do not depend on it
        x = R.unpack(clean, "cf32", 1)
        yref = B.surface(x, r, -1, H, 1, nfft)
        lo, hi = R.outputs_seeing("fused", nfft, K, s, outputs)
        keep = np.ones(outputs, bool)
        keep[lo:hi] = False
        assert lo <= max(0, s - K + 1) and min(s, outputs - 1) < hi and keep.any()
        d = torch.from_numpy(raw).cuda()
        for output in ("best", "surface"):
            got = host(compress_bank(d, r, first_bin=-1, num_hypotheses=H, output=output, fft_length=nfft))
            check(got, output, yref, R.tolerance(x, r), ("not finite", s, output), keep)
            if output == "best":
                assert got[1].min() >= 0 and got[1].max() < H


def test_pulse_delay_and_offset_from_iq_files(torch, tmp_path):
    """the pair tx_rx_pulses_usrp.cpp writes, off two oscillators: the dwell holds the burst delayed and 9 bins of a
    4096-point FFT higher"""
    code = np.array([1, 1, 1, 1, 1, -1, -1, 1, 1, -1, 1, -1, 1])
    burst = np.repeat(code, 8)
    tx = np.stack([16000 * burst, 4000 * burst], axis=1).astype(np.int16)
    lag, n, fs, q = 3777, 20000, 25e6, 9
    rng = np.random.default_rng(71)
    rx = rng.normal(0.0, 200.0, size=(n, 2))
    turned = 0.05 * (tx[:, 0] + 1j * tx[:, 1]) * np.exp(2j * np.pi * q * np.arange(burst.size) / 4096)
    rx[lag: lag + burst.size] += np.stack([turned.real, turned.imag], axis=1)
    rx = np.rint(rx).astype(np.int16)
    tx_path, rx_path = str(tmp_path / "tx.iq"), str(tmp_path / "rx.iq")
    iqfile.write_iq_fmt1(tx_path, tx, fs, start_time=100.0)
    iqfile.write_iq_fmt1(rx_path, rx, fs, start_time=100.25)
    d = pulse_delay_and_offset_from_iq_files(tx_path, rx_path, 12.5 * fs / 4096)
    assert d["lag_samples"] == lag and d["lag_seconds"] == lag / fs and d["start_time_offset"] == 0.25
    assert d["hypothesis"] == 13 + q and d["offset_hz"] == q * fs / 4096
    x, r = R.unpack(rx.reshape(-1), "int16", 16), R.unpack(tx.reshape(-1), "int16", 16)
    ref = np.abs(R.compress(x, B.modulated(r, q, 4096))) ** 2
    assert int(np.argmax(ref)) == lag and abs(d["peak_power"] - ref[lag]) <= 1e-4 * ref[lag]
    long_tx = str(tmp_path / "long.iq")
    iqfile.write_iq_fmt1(long_tx, np.zeros((2049, 2), np.int16), fs)
    with pytest.raises(ValueError, match="2048"):
        pulse_delay_and_offset_from_iq_files(long_tx, rx_path, 1e3)
    with pytest.raises(ValueError, match="sample rate"):
        pulse_delay_and_offset_from_iq_files(tx_path, rx_path, fs)
