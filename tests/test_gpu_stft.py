"""STFT on the MI355X (pfb_stft_*): fused and generic kernels against the float64 reference (tests/stft_ref.py),
against each other and against the channelizer; streaming bit-exactness, the .iq front end, wide indices,
non-finite samples and unaligned device pointers."""
import ctypes as C
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import stft_ref  # noqa: E402
from gpu_support import cuda_torch  # noqa: E402
from sdr_channelizer_amd import Channelizer, Stft, iqfile, spectrogram_from_iq_file, stft, synth  # noqa: E402
from sdr_channelizer_amd import _lib as L  # noqa: E402

FUSED = (256, 512, 768, 1024, 2048)
FORMATS = (("int8", 8), ("int16", 12), ("int16", 16), ("cf32", 1))


@pytest.fixture(scope="module")
def torch():
    return cuda_torch()


def raw_input(fmt, bw, n, seed):
    rng = np.random.default_rng(seed)
    if fmt == "cf32":
        return rng.standard_normal(2 * n).astype(np.float32)
    lim = 2 ** (bw - 1)
    dt = np.int8 if fmt == "int8" else np.int16
    return rng.integers(-lim, lim, size=2 * n).astype(dt)


def reference(raw, fmt, bw, w, H, nfft, order):
    return stft_ref.stft(stft_ref.unpack(raw, fmt, bw), w, H, nfft, order)


def check(y, s, output, scale=1.0, floor=0.0):
    y = np.asarray(y)
    assert y.shape == s.shape, (y.shape, s.shape)
    if y.size == 0:
        return
    if output == "complex":
        assert np.abs(y - s).max() <= 1e-5 * np.abs(s).max()
        return
    p = stft_ref.power(s, scale)
    if output == "power":
        assert np.abs(y - p).max() <= 1e-5 * p.max()
        return
    big = p >= 1e-4 * p.max()
    ref_db = stft_ref.db(s, scale, floor)
    assert np.abs(y[big] - ref_db[big]).max() <= 1e-3
    lin = 10.0 ** (y[~big].astype(np.float64) / 10.0) - floor
    assert np.all(np.abs(lin - p[~big]) <= 1e-5 * p.max())


def run_device(torch, st, raw, cuts=()):
    x = torch.from_numpy(raw).cuda()
    n = raw.size // 2
    edges = [0] + sorted(cuts) + [n]
    outs = [st(x[2 * a: 2 * b]) for a, b in zip(edges[:-1], edges[1:])]
    return torch.cat(outs).cpu().numpy()


def run_host(st, raw, cuts=()):
    n = raw.size // 2
    edges = [0] + sorted(cuts) + [n]
    return np.concatenate([st(raw[2 * a: 2 * b]) for a, b in zip(edges[:-1], edges[1:])])


@pytest.mark.parametrize("nfft", FUSED)
@pytest.mark.parametrize("fmt,bw", FORMATS)
def test_fused_sizes_against_the_reference(torch, nfft, fmt, bw):
    w = np.hamming(nfft)
    raw = raw_input(fmt, bw, 7 * nfft + 5, nfft + bw)
    s = {o: reference(raw, fmt, bw, w, nfft, nfft, o) for o in ("centered", "twosided")}
    for output in ("complex", "power", "db"):
        for order in ("centered", "twosided"):
            with Stft(w, sample_format=fmt, bit_width=bw, output=output, frequency_range=order) as st:
                y = run_device(torch, st, raw)
                assert st.last_kernel.startswith(f"pfb_stft_fused<N{nfft},"), st.last_kernel
            check(y, s[order], output)


@pytest.mark.parametrize("nfft,Lw", [(700, 700), (1000, 1000), (97, 97), (4096, 4096), (600, 500)])
def test_generic_sizes_against_the_reference(torch, nfft, Lw):
    w = np.hanning(Lw)
    for fmt, bw in (("int16", 12), ("cf32", 1)):
        raw = raw_input(fmt, bw, 5 * Lw + 3, nfft)
        for output in ("complex", "power", "db"):
            with Stft(w, fft_length=nfft, sample_format=fmt, bit_width=bw, output=output) as st:
                y = run_device(torch, st, raw)
                assert st.last_kernel == "pfb_stft_generic", st.last_kernel
            check(y, reference(raw, fmt, bw, w, Lw, nfft, "centered"), output)


@pytest.mark.parametrize("H", [768, 384, 192, 500, 1])
@pytest.mark.parametrize("kernel", ["fused", "generic"])
def test_hops(torch, H, kernel):
    w = np.hamming(768)
    raw = raw_input("int16", 12, 768 * 6 + 11 if H > 1 else 2000, H)
    with Stft(w, hop=H, sample_format="int16", bit_width=12, output="complex", kernel=kernel) as st:
        y = run_device(torch, st, raw)
    check(y, reference(raw, "int16", 12, w, H, 768, "centered"), "complex")


@pytest.mark.parametrize("kernel", ["auto", "generic"])
def test_zero_padding(torch, kernel):
    w = np.hamming(768)
    raw = raw_input("int16", 16, 768 * 9 + 100, 5)
    for order in ("centered", "twosided"):
        with Stft(w, fft_length=1024, sample_format="int16", bit_width=16, output="power", frequency_range=order,
                  kernel=kernel) as st:
            y = run_device(torch, st, raw)
            assert ("fused" in st.last_kernel) == (kernel == "auto")
        check(y, reference(raw, "int16", 16, w, 768, 1024, order), "power")


def test_db_of_a_zero_frame_is_minus_infinity(torch):
    raw = raw_input("int16", 12, 4 * 1024, 9)
    raw[: 2 * 1024] = 0
    for kernel in ("fused", "generic"):
        with Stft(np.hamming(1024), sample_format="int16", output="db", kernel=kernel) as st:
            y = run_device(torch, st, raw)
        assert np.all(np.isneginf(y[0])) and np.all(np.isfinite(y[1:]))


def test_kernel_choice():
    w = np.ones(700, np.float32)
    with pytest.raises(L.PfbError) as e:
        Stft(w, kernel="fused")
    assert e.value.status == L.PFB_ERR_UNSUPPORTED
    with Stft(np.ones(768), fft_length=2048, kernel="fused") as st:
        st(np.zeros(4096, np.complex64))
        assert st.last_kernel == "pfb_stft_fused<N2048,cf32>"
    with Stft(np.ones(768), kernel="generic") as st:
        st(np.zeros(4096, np.complex64))
        assert st.last_kernel == "pfb_stft_generic"


def test_loadstore_study_is_opt_in_and_reversible(torch):
    """pfb_stft_set_experiment: the loads-and-stores-only timing variant of a fused kernel runs only when asked for, is
    refused on the generic kernel, and switching back gives the real transform."""
    lib = L.load()
    w = np.hamming(768)
    raw = raw_input("int16", 12, 768 * 4, 21)
    ref = reference(raw, "int16", 12, w, 768, 768, "centered")
    with Stft(w, sample_format="int16", kernel="generic") as st:
        assert lib.pfb_stft_set_experiment(st._h, 1) == L.PFB_ERR_UNSUPPORTED
    with Stft(w, sample_format="int16") as st:
        assert lib.pfb_stft_set_experiment(st._h, 2) == L.PFB_ERR_BAD_ARG
        assert lib.pfb_stft_set_experiment(st._h, 1) == L.PFB_OK
        run_device(torch, st, raw)
        assert st.last_kernel == "pfb_stft_loadstore<N768,int16>"
        assert lib.pfb_stft_set_experiment(st._h, 0) == L.PFB_OK
        st.reset()
        y = run_device(torch, st, raw)
        assert st.last_kernel == "pfb_stft_fused<N768,int16>"
    check(y, ref, "complex")


@pytest.mark.parametrize("nfft", FUSED)
@pytest.mark.parametrize("fmt,bw", [("int8", 8), ("int16", 12), ("cf32", 1)])
def test_fused_agrees_with_generic(torch, nfft, fmt, bw):
    Lw, H = nfft - nfft // 8, nfft // 3
    w = np.blackman(Lw)
    raw = raw_input(fmt, bw, 9 * nfft + 17, nfft * 3 + bw)
    ys = []
    for kernel in ("fused", "generic"):
        with Stft(w, hop=H, fft_length=nfft, sample_format=fmt, bit_width=bw, kernel=kernel) as st:
            ys.append(run_device(torch, st, raw))
    assert np.abs(ys[0] - ys[1]).max() <= 1e-5 * np.abs(ys[1]).max()


def _cuts(rng, n, Lw, H):
    cuts = {0, 1, min(n, Lw // 3), min(n, Lw), min(n, Lw + 2 * H), n}  # short cuts, frame boundaries
    cuts |= set(rng.integers(0, n + 1, size=6).tolist())
    return sorted(cuts)


@pytest.mark.parametrize("nfft,Lw,H", [(768, 768, 768), (768, 768, 192), (1024, 768, 500), (700, 700, 350), (97, 90, 1)])
def test_streaming_is_bit_exact(torch, nfft, Lw, H):
    rng = np.random.default_rng(nfft + H)
    w = np.hamming(Lw)
    n = 12 * Lw + 37 if H > 1 else 600
    raw = raw_input("int16", 12, n, H)
    with Stft(w, hop=H, fft_length=nfft, sample_format="int16", output="complex") as st:
        one = run_device(torch, st, raw)
        for trial in range(3):
            st.reset()
            cuts = _cuts(rng, n, Lw, H)
            assert np.array_equal(run_device(torch, st, raw, cuts), one), (trial, cuts)
            st.reset()
            assert np.array_equal(run_host(st, raw, cuts), one), (trial, cuts)
        st.reset()
        assert np.array_equal(run_host(st, raw), one)
    check(one, reference(raw, "int16", 12, w, H, nfft, "centered"), "complex")


def test_reset_and_capacity_error_leave_a_clean_state(torch):
    w = np.hamming(768)
    raw = raw_input("int16", 12, 768 * 5 + 100, 3)
    lib = L.load()
    with Stft(w, hop=384, sample_format="int16", output="power") as st:
        fresh = run_host(st, raw)
        st.reset()
        st(raw[: 2 * 1000])            # a partial frame carried
        st.reset()
        assert np.array_equal(run_host(st, raw), fresh)
        st.reset()
        first = st(raw[: 2 * 1000])
        rest = raw[2 * 1000:]
        need = st.frames_for(rest.size // 2)
        out = np.empty((need, 768), np.float32)
        f = C.c_uint64()
        rc = lib.pfb_stft_process(st._h, C.c_void_p(rest.ctypes.data), rest.size // 2, C.c_void_p(out.ctypes.data),
                                  need - 1, C.byref(f), L.PFB_MEM_HOST)
        assert rc == L.PFB_ERR_CAPACITY and f.value == need
        assert st.frames_for(rest.size // 2) == need  # nothing moved
        assert np.array_equal(np.concatenate([first, st(rest)]), fresh)


def test_spectrogram_my_iq_record(tmp_path):
    """spectrogram_my_iq.m:105-112 on a format-1 record: (I + jQ)/2^15, stft(iq, fs, 'Window', hamming(768),
    'OverlapLength', 0), abs(s).^2 -- through pfb_stft_process_iq_file and the Python helper."""
    fs = 56e6
    iq = synth.pulsed_iq_numpy(768 * 300 + 123, 16, np.int16).reshape(-1, 2)
    path = str(tmp_path / "rec.iq")
    iqfile.write_iq_fmt1(path, iq, fs)
    p, f, t, info = spectrogram_from_iq_file(path)
    s = stft_ref.stft(stft_ref.unpack(iq, "int16", 16), np.hamming(768), 768, 768, "centered")
    assert p.shape == (768, 300)
    check(p.T, s, "power")
    fr, tr = stft_ref.axes(768, 768, 768, fs, "centered", 0, 300)
    assert np.array_equal(f, fr) and np.allclose(t, tr, rtol=1e-15, atol=0)
    assert int(info.packet.sampleRateSps) == int(fs)
    # the same through [s, f, t] = stft(...) on the samples in memory
    s2, f2, t2 = stft(iq, fs, np.hamming(768), bit_width=16)
    check(s2.T, s, "complex")
    assert np.array_equal(f2, fr) and np.allclose(t2, tr, rtol=1e-15, atol=0)
    # a handle of another bit width refuses the record
    with Stft(np.hamming(768), sample_format="int16", bit_width=12) as st:
        with pytest.raises(L.PfbError) as e:
            st.process_iq_file(path)
        assert e.value.status == L.PFB_ERR_BAD_FORMAT


def test_record_longer_than_two_reader_chunks(tmp_path):
    """A record of more than two of the record reader's 2^24-sample chunks (both page-locked buffers reused, the
    prefetch running across chunk ends) gives the bits of one in-memory host call; a truncated copy is refused."""
    n = (1 << 25) + 12345
    iq = np.random.default_rng(29).integers(-128, 128, size=(n, 2), dtype=np.int8)
    path = str(tmp_path / "long.iq")
    iqfile.write_iq(path, iq, 56e6, 1e9, 8)
    with Stft(np.hamming(256), sample_format="int8", bit_width=8, output="power") as st:
        y, info = st.process_iq_file(path)
        st.reset()
        ref = st(iq)
        assert int(info.packet.numSamples) == n and y.shape == (n // 256, 256)
        assert np.array_equal(y, ref)
        short = str(tmp_path / "short.iq")
        with open(path, "rb") as src, open(short, "wb") as dst:
            dst.write(src.read(os.path.getsize(path) - 4096))
        with pytest.raises(L.PfbError) as e:
            st.process_iq_file(short)
        assert e.value.status == L.PFB_ERR_BAD_FORMAT


def test_page_locked_host_buffers_and_pipelined_staging(torch):
    """L = 256 at hop 1 fills a 64 MiB output staging buffer every 65536 samples: four staging chunks in flight over
    three streams give the bits of one device-resident call, from pageable and from page-locked buffers."""
    from sdr_channelizer_amd import pinned_empty
    n = 3 * 65536 + 4321
    raw = raw_input("int16", 12, n, 31)
    raw_p = pinned_empty(raw.shape, raw.dtype)
    raw_p[:] = raw
    with Stft(np.hamming(256), hop=1, sample_format="int16", output="power") as st:
        ref = run_device(torch, st, raw)
        assert ref.shape == (n - 255, 256)
        st.reset()
        out_p = pinned_empty(ref.shape, ref.dtype)
        assert np.array_equal(st(raw_p, out=out_p), ref)
        st.reset()
        assert np.array_equal(st(raw), ref)


def test_handle_reports_its_device(torch):
    lib = L.load()
    for device in (0, -1):
        with Stft(np.hamming(256), device=device) as st:
            dev = C.c_int(-1)
            assert lib.pfb_stft_get_device(st._h, C.byref(dev)) == L.PFB_OK
            assert dev.value == st.device_index == torch.cuda.current_device() == 0
    assert lib.pfb_stft_get_device(None, C.byref(dev)) == L.PFB_ERR_BAD_ARG


def test_device_input_is_checked_before_the_library_sees_it(torch):
    """The channelizer's rules: a numpy out for a CUDA input, or an interleaved tensor whose last dimension is not 2,
    is a ValueError"""
    raw = raw_input("int16", 12, 256 * 4, 5)
    x = torch.from_numpy(raw).cuda()
    with Stft(np.hamming(256), sample_format="int16", output="power") as st:
        with pytest.raises(ValueError):
            st(x, out=np.empty((4, 256), np.float32))
        with pytest.raises(ValueError):
            st(x.reshape(-1, 4))
        y = st(x.reshape(-1, 2)).cpu().numpy()
        st.reset()
        assert np.array_equal(y, st(raw))


def test_generate_pulsed_iq_psd_db():
    """generate_pulsed_iq.m:105, spectrogram(iq,1024,0,1024,Fs,'centered','yaxis'): a 1024-point Hamming STFT, PSD
    scale 1/(fs sum w^2), plotted in dB (eps added)."""
    fs = 56e6
    iq = synth.pulsed_iq_numpy(1024 * 64, 12, np.int16)
    w = np.hamming(1024)
    scale, eps = 1.0 / (fs * np.sum(w ** 2)), np.finfo(np.float64).eps
    with Stft(w, sample_format="int16", bit_width=12, output="db", scale=scale, db_floor=eps) as st:
        y = st(iq)
    check(y, reference(iq, "int16", 12, w, 1024, 1024, "centered"), "db", scale, eps)


@pytest.mark.parametrize("M", [768, 1024, 700])
def test_power_equals_the_channelizer_generic_kernel(torch, M):
    """H = L = nfft = M: |STFT|^2 in twosided order is the channelizer's |y|^2 with P = 1, D = M and the time-reversed
    window (two independent GPU paths)."""
    w = np.hamming(M).astype(np.float32)
    iq = synth.pulsed_iq_numpy(M * 50, 12, np.int16)
    x = torch.from_numpy(iq).cuda()
    with Channelizer(M, taps=w[::-1].copy(), bit_width=12, power=True) as ch:
        ch.set_option(L.PFB_OPT_KERNEL, 1)
        yc = ch(x).cpu().numpy()
    with Stft(w, sample_format="int16", bit_width=12, output="power", frequency_range="twosided") as st:
        ys = st(x).cpu().numpy()
    assert ys.shape == yc.shape
    assert np.abs(ys - yc).max() <= 1e-5 * yc.max()


def test_wide_indices(torch):
    """2^31 int16 samples (8 GiB in, 8 GiB of power out): the frames at the start, where sample and output byte offsets
    cross 2^31 and 2^32, and at the end match the reference computed on just those windows."""
    n, nfft = 1 << 31, 1024
    w = np.hamming(nfft)
    g = torch.Generator(device="cuda").manual_seed(7)
    x = torch.randint(-2048, 2048, (2 * n,), dtype=torch.int16, device="cuda", generator=g)
    with Stft(w, sample_format="int16", bit_width=12, output="power") as st:
        y = st(x)
        assert st.last_kernel == "pfb_stft_fused<N1024,int16>"
    F = y.shape[0]
    assert F == n // nfft
    picks = [0, 1, (1 << 19) - 1, 1 << 19, (1 << 20) - 1, 1 << 20, (1 << 21) - 2, F - 1]
    for m in picks:
        raw = x[2 * m * nfft: 2 * (m + 1) * nfft].cpu().numpy()
        s = reference(raw, "int16", 12, w, nfft, nfft, "centered")
        check(y[m: m + 1].cpu().numpy(), s, "power")
    del x, y
    torch.cuda.empty_cache()


@pytest.mark.parametrize("kernel,nfft", [("fused", 768), ("generic", 700)])
def test_non_finite_samples_stay_in_their_frames(torch, kernel, nfft):
    Lw, H = nfft, nfft // 4
    w = np.hamming(Lw)
    n = 12 * Lw
    raw = raw_input("cf32", 1, n, 11)
    clean = raw.copy()
    bad = {3 * Lw + 17: np.nan, 7 * Lw + 5: np.inf}
    for i, v in bad.items():
        raw[2 * i] = v
        clean[2 * i] = 0.0
    cuts = [3 * Lw + 17, 3 * Lw + 18, 7 * Lw + 4]  # a call cut next to each sample
    with Stft(w, hop=H, sample_format="cf32", kernel=kernel) as st:
        y = run_device(torch, st, raw, cuts)
        st.reset()
        yc = run_device(torch, st, clean, cuts)
    F = y.shape[0]
    hit = np.zeros(F, bool)
    for i in bad:
        m = np.arange(F)
        hit |= (m * H <= i) & (i < m * H + Lw)
    assert np.all(~np.isfinite(y[hit]).all(axis=1))
    assert np.array_equal(y[~hit], yc[~hit])


def test_unaligned_device_pointers(torch):
    w = np.hamming(768)
    for fmt, bw, output in (("int16", 12, "power"), ("int8", 8, "complex"), ("cf32", 1, "db")):
        raw = raw_input(fmt, bw, 768 * 6 + 1, 17)
        ref = reference(raw[2:], fmt, bw, w, 384, 768, "centered")
        x = torch.from_numpy(raw).cuda()[2:]           # one sample in
        odt = torch.complex64 if output == "complex" else torch.float32
        F = ref.shape[0]
        buf = torch.empty(F * 768 + 1, dtype=odt, device="cuda")
        with Stft(w, hop=384, sample_format=fmt, bit_width=bw, output=output) as st:
            y = st(x, out=buf[1:])                     # one output element in
            assert "fused" in st.last_kernel
        check(y.cpu().numpy(), ref, output)


def test_fuzz_against_the_reference(torch):
    cases = int(os.environ.get("PFB_STFT_FUZZ_CASES", "200"))
    rng = np.random.default_rng(20261016)
    sizes = list(FUSED) + [60, 97, 100, 300, 600, 700, 1000, 1536, 4096]
    for case in range(cases):
        nfft = int(rng.choice(sizes))
        Lw = int(rng.integers(max(1, nfft // 2), nfft + 1)) if rng.random() < 0.5 else nfft
        H = int(rng.choice([Lw, max(1, Lw // 2), max(1, Lw // 4), int(rng.integers(1, Lw + 1))]))
        fmt, bw = FORMATS[int(rng.integers(len(FORMATS)))]
        output = ("complex", "power", "db")[int(rng.integers(3))]
        order = ("centered", "twosided")[int(rng.integers(2))]
        n = int(rng.integers(0, 6 * Lw)) if H > 4 else int(rng.integers(0, Lw + 300))
        raw = raw_input(fmt, bw, n, case)
        cuts = sorted(set(rng.integers(0, n + 1, size=int(rng.integers(0, 5))).tolist()))
        w = rng.random(Lw)
        with Stft(w, hop=H, fft_length=nfft, sample_format=fmt, bit_width=bw, output=output,
                  frequency_range=order) as st:
            y = run_device(torch, st, raw, cuts) if case % 2 else run_host(st, raw, cuts)
        try:
            check(y, reference(raw, fmt, bw, w, H, nfft, order), output)
        except AssertionError as e:
            raise AssertionError(f"case {case}: nfft={nfft} L={Lw} H={H} {fmt}/{bw} {output} {order} n={n} "
                                 f"cuts={cuts}") from e
