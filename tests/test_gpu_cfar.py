"""The CFAR detector on the MI355X (pfb_cfar_*): records, counts and stats byte for byte against the numpy restatement
(tests/cfar_ref.py) -- every sum tier and method over call lengths around the block and deciding boundaries, pointer
offsets and guard bytes, the capacity contract, cuttings, designed runs, bank cells, non-finite cells, the host, async and
reset routes, and the chain from a noisy pulse train to the event fit."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import cfar_ref as R  # noqa: E402
import mf_ref as M  # noqa: E402
import mfbank_ref as B  # noqa: E402
from gpu_support import cuda_torch  # noqa: E402
from sdr_channelizer_amd import (Cfar, PulseTrain, cfar_alpha, detect, detect_pulses, detections_to_pdws, fit_event,  # noqa: E402
                                 iqfile, pulse_detections_from_iq_file, replica_from_pulse_train)
from sdr_channelizer_amd import _lib as L  # noqa: E402
from sdr_channelizer_amd.cfar import DET_DTYPE, records  # noqa: E402
from sdr_channelizer_amd.pdw import extract_pdws_raw  # noqa: E402

METHODS = {"ca": R.CA, "go": R.GO, "so": R.SO}


@pytest.fixture(scope="module")
def torch():
    return cuda_torch()


def noisy(n, seed, spikes=12, level=300.0):
    """exponential noise whose level moves along the stream, with spikes well over any threshold"""
    rng = np.random.default_rng(seed)
    p = rng.exponential(1.0, n) * (1.0 + 0.8 * np.sin(np.arange(n) / 97.0))
    if n:
        p[rng.integers(0, n, spikes)] *= level
    return p.astype(np.float32)


def as_cells(p, hyp):
    if hyp is None:
        return np.ascontiguousarray(p, np.float32)
    c = np.zeros(len(p), R.CELL)
    c["power"], c["hypothesis"] = p, hyp
    return c.view(np.float32).reshape(-1, 2)


def stream(torch, det, p, cuts, kw, hyp=None, host=False, every=True, flush=True):
    """One stream through `det` (reset first), cut into calls of the lengths `cuts`: what has come out after each call,
    and after the flush, is what the restatement says has closed by then, and so are the stats."""
    det.reset()
    x = as_cells(p, hyp)
    got, pos = [np.zeros(0, DET_DTYPE)], 0
    ref = dict(kw, hyp=hyp)
    for m in cuts:
        part = x[pos:pos + m]
        got.append(records(det.process(part if host else torch.from_numpy(part).cuda())))
        pos += m
        assert det.next_index == pos
        if every:
            want, _ = R.detect(p, pos, False, **ref)
            assert np.concatenate(got).tobytes() == want.tobytes(), (pos, cuts)
    want, wstats = R.detect(p, pos, False, **ref)
    assert np.concatenate(got).tobytes() == want.tobytes() and det.stats == wstats, (cuts, det.stats, wstats)
    if flush:
        got.append(records(det.flush()))
        want, wstats = R.detect(p, pos, True, **ref)
        assert np.concatenate(got).tobytes() == want.tobytes() and det.stats == wstats, (cuts, det.stats, wstats)
    return np.concatenate(got)


def make(C_, G, T, method="ca", alpha=6.0, min_power=0.0, g=0, element="power"):
    det = Cfar(C_, G, T, alpha, method=method, element=element, merge_gap=g, min_power=min_power)
    return det, dict(C=C_, G=G, T=T, method=METHODS[method], alpha=alpha, min_power=min_power, merge_gap=g)


@pytest.mark.parametrize("method", list(METHODS))
@pytest.mark.parametrize("G,T", [(0, 1), (1, 2), (3, 32)])
@pytest.mark.parametrize("C_", [4, 16, 64, 256, 1024])
def test_sum_tiers_over_call_lengths(torch, C_, G, T, method):
    top = (G + T + 2) * C_
    if C_ == 4:
        lengths = list(range(top + 4))
    else:
        lengths = sorted({max(0, k * C_ + d) for k in range(G + T + 3) for d in (-1, 0, 1)})
    p = noisy(sum(lengths), C_ * 1000 + G)
    det, kw = make(C_, G, T, method, g=C_ // 2)
    with det:
        for n in lengths:   # each alone
            stream(torch, det, p[7:], [n], kw)
        stream(torch, det, p, lengths, kw, every=len(p) <= 1 << 14)   # one after the other
        assert det.last_kernel == det.plan.sum_kernel.decode()


@pytest.mark.parametrize("element", ["power", "cell"])
def test_every_tier_and_both_elements(torch, element):
    """Every block length, so every shape of the sum pass (1 to 64 lanes to a block, two and four sub-sums), with both
    element kinds: calls that put the carry / call seam inside a block, a lane's four cells and a 256-cell sub-sum, from
    pointers on and off a 16-byte boundary.  pfb_cfar_last_kernel names each of the six tiers."""
    named = set()
    for C_ in (4, 8, 16, 32, 64, 128, 256, 512, 1024):
        G, T = 1, 2
        n = 9 * C_ + 5
        p = noisy(n, 100 + C_, spikes=6)
        hyp = (np.arange(n, dtype=np.int32) * 11 - 7) if element == "cell" else None
        det, kw = make(C_, G, T, g=C_ // 4, element=element)
        with det:
            for cuts in ([n], [1, n - 1], [C_ // 2 + 1, 2 * C_ + 2, n - 2 * C_ - C_ // 2 - 3], [2 * C_ + 3] + [C_ + 1] * 3 + [n - 5 * C_ - 6]):
                assert sum(cuts) == n
                stream(torch, det, p, cuts, kw, hyp=hyp)
            assert det.last_kernel == det.plan.sum_kernel.decode()
            named.add(det.last_kernel)
    assert named == {f"pfb_cfar_sum<{tier},{element}>" for tier in ("lanes", "wave", "subsums")}, named


def raw_call(torch, det, x, n, cap, lead=5):
    """pfb_cfar_process on device pointers with guard bytes around the record buffer and the count"""
    buf = torch.full((lead * 48 + max(cap, 0) * 48 + 48,), 0xAB, dtype=torch.uint8, device="cuda")
    cnt = np.full(3, 0xABABABABABABABAB, np.uint64)
    rc = det._lib.pfb_cfar_process(det._h, C.c_void_p(x.data_ptr()), n, C.c_void_p(buf.data_ptr() + lead * 48), cap,
                                   C.cast(cnt[1:].ctypes.data, C.POINTER(C.c_uint64)), L.PFB_MEM_DEVICE)
    host = buf.cpu().numpy()
    got = int(cnt[1])
    assert cnt[0] == cnt[2] == 0xABABABABABABABAB
    wrote = min(got, cap)
    assert (host[: lead * 48] == 0xAB).all() and (host[lead * 48 + wrote * 48:] == 0xAB).all()
    return rc, got, host[lead * 48: lead * 48 + wrote * 48].view(DET_DTYPE)


@pytest.mark.parametrize("element", ["power", "cell"])
def test_pointer_offsets_guards_and_capacity(torch, element):
    C_, G, T, n = 16, 1, 2, 3000
    p = noisy(n, 5, spikes=40)
    p[942] = 1e5     # decided by the first call of 1001 cells (944 are), not yet closed: an open run is carried
    p[n - 5] = 1e5   # closes only at the flush
    hyp = (np.arange(n, dtype=np.int32) * 37 - 50000) if element == "cell" else None
    det, kw = make(C_, G, T, g=3, element=element)
    want, _ = R.detect(p, n, False, hyp=hyp, **kw)
    assert len(want) > 10
    per = 2 if element == "cell" else 1
    with det:
        for off in (0, 1, 2, 3):
            base = torch.zeros((n + 64) * per, dtype=torch.float32, device="cuda")
            assert base.data_ptr() % 256 == 0
            x = base[off * per: (off + n) * per]
            x.copy_(torch.from_numpy(as_cells(p, hyp).reshape(-1)))
            det.reset()
            state = det.stats
            rc, cnt, _ = raw_call(torch, det, x, n, len(want) - 1)    # one short: the count, and nothing has changed
            assert (rc, cnt) == (L.PFB_ERR_CAPACITY, len(want)) and det.stats == state and det.next_index == 0
            rc, cnt, got = raw_call(torch, det, x, n, len(want))      # the retry, with exactly enough room
            assert (rc, cnt) == (L.PFB_OK, len(want)) and got.tobytes() == want.tobytes(), off
            # the same after a first call that left cells and an open run behind
            det.reset()
            first = records(det.process(x[: 1001 * per]))
            state = det.stats
            assert state["open_run"] == 1 and state["cells_decided"] == 944
            rest, _ = R.detect(p, n, False, hyp=hyp, **kw)
            rest = rest[len(first):]
            rc, cnt, _ = raw_call(torch, det, x[1001 * per:], n - 1001, len(rest) - 1)
            assert (rc, cnt) == (L.PFB_ERR_CAPACITY, len(rest)) and det.stats == state and det.next_index == 1001
            rc, cnt, got = raw_call(torch, det, x[1001 * per:], n - 1001, len(rest))
            assert (rc, cnt) == (L.PFB_OK, len(rest)) and got.tobytes() == rest.tobytes(), off
            # the flush obeys the same contract
            tail, _ = R.detect(p, n, True, hyp=hyp, **kw)
            tail = tail[len(first) + len(rest):]
            assert len(tail) >= 1
            u = C.c_uint64()
            out = np.zeros(len(tail), DET_DTYPE)
            state = det.stats
            assert det._lib.pfb_cfar_flush(det._h, C.c_void_p(out.ctypes.data), len(tail) - 1, C.byref(u),
                                           L.PFB_MEM_HOST) == L.PFB_ERR_CAPACITY
            assert u.value == len(tail) and det.stats == state
            assert det._lib.pfb_cfar_flush(det._h, C.c_void_p(out.ctypes.data), len(tail), C.byref(u), L.PFB_MEM_HOST) == L.PFB_OK
            assert out.tobytes() == tail.tobytes()
            # after a flush: cells only after a reset; a second flush has nothing left
            assert det._lib.pfb_cfar_process(det._h, C.c_void_p(x.data_ptr()), 4, C.c_void_p(out.ctypes.data), 0, C.byref(u),
                                             L.PFB_MEM_DEVICE) == L.PFB_ERR_BAD_ARG
            assert len(det.flush()) == 0


def test_cuttings(torch):
    C_, G, T, n = 64, 1, 3, 20000
    p = noisy(n, 11, spikes=60)
    det, kw = make(C_, G, T, g=20)
    rng = np.random.default_rng(3)
    with det:
        whole = stream(torch, det, p, [n], kw)
        assert len(whole) > 20
        for _ in range(4):
            edges = np.sort(rng.integers(0, n + 1, 9))
            cuts = np.diff(np.concatenate([[0], edges, [n]])).tolist()
            a = stream(torch, det, p, cuts, kw)
            b = stream(torch, det, p, cuts, kw)   # the same cutting twice
            assert a.tobytes() == b.tobytes() == whole.tobytes()
        # one cell at a time across a block boundary (cell 640) and across the deciding boundary of block 5 (cell 640
        # completes block 9 = 5 + G + T)
        cuts = [630] + [1] * 20 + [n - 650]
        assert stream(torch, det, p, cuts, kw).tobytes() == whole.tobytes()
        # flushes: after nothing, after less than a block, with a partial last block, without any complete training block
        for m in (0, 5, C_ - 1, C_, C_ + 1, (G + 1) * C_, (G + 1) * C_ + C_ - 1, (G + 2) * C_, (G + 2) * C_ + 9, 1000):
            q = p.copy()
            q[m // 2] = 1e6
            out = stream(torch, det, q, [m], kw)
            if m <= (G + 1) * C_:   # blocks 0 .. G have no lead set, and no block past their guard is complete
                assert len(out) == 0 and det.stats["cells_without_noise"] == m and det.stats["cells_decided"] == m
            else:
                assert det.stats["cells_without_noise"] < m == det.stats["cells_decided"]


def designed(n, at, level=1000.0):
    p = np.ones(n, np.float32)
    p[np.asarray(at, np.int64)] = level
    return p


@pytest.mark.parametrize("g", [0, 1, 63, 64, 65, 5000])
def test_gaps_of_g_and_g_plus_one(torch, g):
    C_, G, T = 16, 0, 2
    a, b = 1000, 1000 + 3 * (g + 2) + 40
    at = [a, a + g + 1,             # g cells of not-over between them: one run
          b, b + g + 2]             # g + 1: two runs
    n = at[-1] + g + 200
    p = designed(n, at)
    det, kw = make(C_, G, T, alpha=4.0, g=g)
    with det:
        for cuts in ([n], [a + 1, n - a - 1], [a + 1, g + 1, n - a - g - 2], [b + 1, 1, n - b - 2]):
            out = stream(torch, det, p, cuts, kw)
            assert [(int(d["first_index"]), int(d["last_index"])) for d in out] == [(a, a + g + 1), (b, b), (b + g + 2, b + g + 2)]


def test_designed_runs(torch):
    C_, G, T, g = 64, 1, 2, 70
    n = 80000
    long_run = list(range(20000, 20000 + 40000, 60))                 # crosses words, tiles (16384 cells), blocks; 40000 cells long
    at = [100, 127, 128, 190] + long_run + [70000, 70050, 70100, 75000]
    p = designed(n, at)
    # ties of the peak: inside a word, across words, across calls -- the lowest index wins
    p[[100, 127]] = 5000.0
    p[[20000 + 60 * 5, 20000 + 60 * 300, 20000 + 60 * 600]] = 7000.0
    p[[70000, 70100]] = 9000.0
    det, kw = make(C_, G, T, alpha=4.0, g=g)
    with det:
        for cuts in ([n],
                     [110, n - 110],                                  # the first tie across a call
                     [25000, 10000, 10000, n - 45000],                # the long run over four calls, three whole calls inside it
                     [20100] + [2000] * 15 + [n - 50100],             # a run longer than a call, many times
                     [70010, 60, n - 70070],                          # the last tie across two cuts
                     [30000, 41000, n - 71000]):                      # two runs close in one call, one opened in the call before
            out = stream(torch, det, p, cuts, kw)
            assert [int(d["first_index"]) for d in out] == [100, 20000, 70000, 75000]
            assert [int(d["peak_index"]) for d in out] == [100, 20000 + 60 * 5, 70000, 75000]
            assert [int(d["cells_over"]) for d in out] == [4, len(long_run), 3, 1]
    # ONE_SIDED at the stream start (short lead set) and at flush (short lag set), not in between
    p = designed(3000, [10, 1500, 2990])
    det, kw = make(C_, G, T, alpha=4.0, g=5)
    with det:
        out = stream(torch, det, p, [3000], kw)
        assert [int(d["flags"]) for d in out] == [R.ONE_SIDED, 0, R.ONE_SIDED]


def test_bank_cells_and_min_power(torch):
    C_, G, T, n = 64, 1, 2, 6000
    at = [300, 301, 2000, 4000, 4003]
    p = designed(n, at)
    p[301], p[4003] = 2000.0, 3000.0
    hyp = np.zeros(n, np.int32)
    hyp[[300, 301, 2000, 4000, 4003]] = [7, -2147483648, 2147483647, -5, 123456789]
    for min_power, count in ((0.0, 3), (1500.0, 2), (1e4, 0)):     # under the spikes, between them, over them
        det, kw = make(C_, G, T, alpha=4.0, g=8, min_power=min_power, element="cell")
        with det:
            out = stream(torch, det, p, [1000, 3500, 1500], kw, hyp=hyp)
            assert len(out) == count
            if count == 3:
                assert out["hypothesis"].tolist() == [-2147483648, 2147483647, 123456789]
                assert out["peak_index"].tolist() == [301, 2000, 4003]


@pytest.mark.parametrize("method", list(METHODS))
def test_non_finite_cells(torch, method):
    C_, G, T, n = 16, 1, 2, 4000
    p = noisy(n, 17, spikes=30)
    p[[500, 1200]] = np.nan            # a NaN test cell (never over) that is also a training cell of its neighbours
    p[[1800, 1801]] = np.inf           # over, equal: the lower index is the peak; blinds the blocks that train on it
    p[2500] = -np.inf
    p[3000] = np.inf
    p[3001] = np.nan
    det, kw = make(C_, G, T, method, g=2)
    with det:
        out = stream(torch, det, p, [n], kw)
        stream(torch, det, p, [1801, 1, n - 1802], kw)
        peaks = out["peak_index"].tolist()
        assert 1800 in peaks and 3000 in peaks and not {500, 1200, 1801, 2500, 3001} & set(peaks)


def test_host_route_in_three_staging_steps(torch):
    C_, G, T = 1024, 1, 2
    n = 2 * (1 << 24) + 5
    rng = np.random.default_rng(23)
    p = rng.exponential(1.0, n).astype(np.float32)
    at = np.sort(rng.choice(n, 200, replace=False))
    at[:4] = [(1 << 24) - 1, 1 << 24, (1 << 25) - 700, (1 << 25) + 2]    # around both seams
    p[at] *= 400.0
    det, kw = make(C_, G, T, alpha=12.0, g=1000)
    with det:
        out = stream(torch, det, p, [n], kw, host=True, every=False)
        assert len(out) >= 150


def test_async_calls_truncation_and_reset(torch):
    C_, G, T, n = 64, 1, 2, 50000
    p = noisy(n, 29, spikes=80)
    det, kw = make(C_, G, T, g=10)
    cuts = [7000, 13000, 1, 20000, n - 40001]
    edges = np.cumsum([0] + cuts)
    want = [R.detect(p, int(e), False, **kw)[0] for e in edges]
    per_call = [len(want[k + 1]) - len(want[k]) for k in range(len(cuts))]
    assert min(per_call[0], per_call[1], per_call[3]) > 4
    cap = 3                                                            # smaller than most calls close
    x = torch.from_numpy(p).cuda()
    with det:
        side = torch.cuda.Stream()
        outs = [torch.full((cap + 1, 6), -1, dtype=torch.int64, device="cuda") for _ in cuts]
        counts = torch.full((len(cuts), 2), -1, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        for k, m in enumerate(cuts):
            if k == 2:
                det.set_stream(side.cuda_stream)                       # what is queued on the old stream comes first
            lo = int(edges[k])
            if k == 0:   # the C entry point itself, then the Python method over it
                rc = det._lib.pfb_cfar_process_async(det._h, C.c_void_p(x[lo:].data_ptr()), m, C.c_void_p(outs[k].data_ptr()),
                                                     cap, C.c_void_p(counts[k].data_ptr()))
                assert rc == L.PFB_OK
            else:
                det.process_async(x[lo:lo + m], outs[k][:cap], counts[k][:1])
        det.sync()
        torch.cuda.synchronize()
        got_counts = counts.cpu().numpy()
        assert got_counts[:, 0].tolist() == per_call and (got_counts[:, 1] == -1).all()
        for k in range(len(cuts)):
            rec = outs[k].cpu().numpy()
            wrote = min(cap, per_call[k])
            assert records(rec[:wrote]).tobytes() == want[k + 1][len(want[k]):][:wrote].tobytes(), k
            assert (rec[wrote:] == -1).all()
        stats = det.stats
        assert stats["detections"] == sum(per_call) and stats["dropped"] == sum(max(0, c - cap) for c in per_call)
        assert stats["cells_in"] == n
        det.set_stream(0)
        with pytest.raises(ValueError):
            det.process_async(x[:64], outs[0].view(torch.float32), counts[0][:1])
        with pytest.raises(ValueError):
            det.process_async(x[:64], outs[0][:, :5], counts[0][:1])
        # a reset between streams: the next stream knows nothing of this one
        q = noisy(9000, 31)
        stream(torch, det, q, [4000, 5000], kw)
    # the one-shot form
    assert detect(p, C_, G, T, 6.0, merge_gap=10).tobytes() == R.detect(p, n, True, **kw)[0].tobytes()


def train(first_pulse, pulses, q=0, pw=512, extent=40e6, sigma=0.1, nfft=4096, fs=56e6, pri=8192):
    """a noisy LFM pulse train, its replica, and where its pulses start; the carrier q bins of an nfft-point FFT up"""
    kw = dict(pw=pw, lfm_extent_hz=extent, sample_format="int16", bit_width=12, fs=fs, pri=pri, amplitude=0.1)
    r = replica_from_pulse_train(f0=-extent / 2, **kw)
    with PulseTrain(first_pulse=first_pulse, f0=-extent / 2 + q * fs / nfft, noise_sigma=sigma, seed=11, **kw) as pt:
        iq = pt.generate(pulses * pri)
    return iq, r, [first_pulse + k * pri for k in range(pulses)]


def test_the_chain_from_a_pulse_train_to_the_event_fit(torch, tmp_path):
    """LFM pulses of 512 samples 3 dB under the noise per sample: nothing for the envelope extractor at 15 dB, one
    detection per pulse on its first sample after compression."""
    fs, pulses = 56e6, 8
    iq, r, starts = train(3000, pulses)
    host = iq.cpu().numpy()
    assert len(extract_pdws_raw(iq, fs, 0.0, 0.0, bit_width=12, snr_threshold_db=15.0)) == 0   # under the envelope threshold
    # the reference first: the float64 matched filter into the restatement finds exactly the pulses
    K, C_, T = r.size, 64, 8
    alpha = float(np.float32(cfar_alpha(1e-7, 2 * T * C_)))
    y = M.compress(M.unpack(host, "int16", 12), r, True)
    pw = (y.real ** 2 + y.imag ** 2).astype(np.float32)
    ref, _ = R.detect(pw, len(pw), True, C=C_, G=-(-K // C_), T=T, alpha=alpha, merge_gap=K)
    assert ref["peak_index"].tolist() == starts
    found = detect_pulses(iq, r, normalize=True, chunk_samples=20000)
    dets = found.records
    assert (found.first_bin, found.bin_hz) == (0, 0.0)
    assert dets["peak_index"].tolist() == starts and (dets["hypothesis"] == -1).all()
    assert (dets["first_index"] <= dets["peak_index"]).all() and (dets["peak_power"] > alpha * dets["noise"]).all()
    # in one chunk: the matched filter's blocks start where a call starts, so the powers agree to its tolerance only
    found = detect_pulses(iq, r, normalize=True)
    assert found.records["peak_index"].tolist() == starts
    dets = found.records
    assert detect_pulses(host, r, normalize=True).records.tobytes() == dets.tobytes()   # the same from host memory
    pd = detections_to_pdws(dets, fs, 915e6, 10.0)
    assert np.array_equal(pd["toa"], (np.array(starts) + 1) / fs + 10.0)
    assert found.to_pdws(fs, 915e6, 10.0).tobytes() == pd.tobytes()
    # the same from a record on disk: format, bit width and fs from its header
    path = str(tmp_path / "train.iq")
    iqfile.write_iq(path, host, fs, 915e6, 12, start_time=10.0)
    from_file, rec = pulse_detections_from_iq_file(path, r, normalize=True)
    assert from_file.records.tobytes() == dets.tobytes() and (from_file.first_bin, from_file.bin_hz) == (0, 0.0)
    assert (rec.fs, rec.bitWidth, rec.iq.shape) == (fs, 12, host.shape)
    assert from_file.to_pdws(rec.fs, rec.fc, rec.sampleStartTime).tobytes() == pd.tobytes()
    fit_event(pd)    # a parabola over eight equal pulses may have no top: that it runs is the point


@pytest.mark.parametrize("q", [1, -1])
def test_the_chain_through_the_bank(torch, q, tmp_path):
    """The carrier moved by a whole bin.  An LFM trades delay for carrier along its ridge, 1.5 bins a sample for 42 MHz
    over 2048 samples: with three hypotheses the nearest cells on the ridge (one sample off, half a bin from a
    hypothesis) keep sinc(1/4)^2 = 0.81 of the peak, and 3 dB over the noise per sample -- still far under the
    extractor's 15 dB -- puts that 19 % at six standard deviations of the noise after compression (36 dB)."""
    fs, pulses, nfft = 56e6, 8, 4096
    iq, r, starts = train(3000, pulses, q=q, pw=2048, extent=42e6, sigma=0.05)
    host = iq.cpu().numpy()
    assert len(extract_pdws_raw(iq, fs, 0.0, 0.0, bit_width=12, snr_threshold_db=15.0)) == 0
    K, C_, T = r.size, 64, 8
    alpha = float(np.float32(cfar_alpha(1e-7, 2 * T * C_)))
    surf = B.surface(M.unpack(host, "int16", 12), r, -1, 3, 1, nfft, True)
    power, hyp = B.best((surf.real ** 2 + surf.imag ** 2).astype(np.float32))
    ref, _ = R.detect(power, len(power), True, C=C_, G=-(-K // C_), T=T, alpha=alpha, merge_gap=K, hyp=hyp)
    assert ref["peak_index"].tolist() == starts and (ref["hypothesis"] - 1 == q).all()
    dets, first_bin, bin_hz = found = detect_pulses(iq, r, normalize=True, max_offset_hz=0.9 * fs / nfft, fs=fs)
    assert (first_bin, bin_hz) == (-1, fs / nfft)
    assert dets["peak_index"].tolist() == starts and (first_bin + dets["hypothesis"] == q).all(), (q, dets)
    pd = detections_to_pdws(dets, fs, 915e6, 10.0, bin_hz=fs / nfft, first_bin=first_bin)
    assert np.allclose(pd["freq"], 915e6 + q * fs / nfft, rtol=0, atol=1e-3) and np.array_equal(pd["bin"], dets["hypothesis"])
    fit_event(pd)
    assert found.to_pdws(fs, 915e6, 10.0).tobytes() == pd.tobytes()
    path = str(tmp_path / "train.iq")
    iqfile.write_iq(path, host, fs, 915e6, 12)
    from_file, rec = pulse_detections_from_iq_file(path, r, normalize=True, max_offset_hz=0.9 * fs / nfft)   # fs: the header's
    assert from_file.records.tobytes() == dets.tobytes() and from_file[1:] == (first_bin, bin_hz)
