"""The STFT entry points without a GPU: the host-only axes, argument validation before any device call, and the
float64 reference the GPU tests compare against (checked against a direct sum and the C oracle's channelizer)."""
import ctypes as C

import numpy as np
import pytest

from sdr_channelizer_amd import _lib as L
from sdr_channelizer_amd import stft_axes

import stft_ref


def _axes(nfft, Lw, H, fs, order, first, frames):
    f = np.empty(nfft)
    t = np.empty(frames)
    rc = L.load().pfb_stft_axes(nfft, Lw, H, fs, order, first, frames, f.ctypes.data_as(C.POINTER(C.c_double)),
                                t.ctypes.data_as(C.POINTER(C.c_double)))
    return rc, f, t


def test_axes_centered_even_and_odd():
    fs = 56e6
    rc, f, _ = _axes(768, 768, 768, fs, L.PFB_STFT_CENTERED, 0, 0)
    assert rc == L.PFB_OK
    assert f[0] == -383 * fs / 768 and f[-1] == 384 * fs / 768   # (-pi, pi]: Nyquist is the last row
    assert np.array_equal(f, np.arange(-383, 385) * fs / 768)
    rc, f, _ = _axes(97, 60, 60, 1e3, L.PFB_STFT_CENTERED, 0, 0)
    assert rc == L.PFB_OK and f[0] == -48 * 1e3 / 97 and f[48] == 0 and f[-1] == 48 * 1e3 / 97
    # not fftshift: at even nfft fftshift's rows start at -nfft/2, one row lower than stft's 'centered'
    f = _axes(768, 768, 768, fs, L.PFB_STFT_CENTERED, 0, 0)[1]
    shifted = np.fft.fftshift(np.fft.fftfreq(768, 1 / fs))
    assert shifted[0] == -384 * fs / 768 and np.allclose(f[:-1], shifted[1:], rtol=1e-15, atol=0)


def test_axes_twosided_and_time():
    rc, f, t = _axes(8, 6, 3, 8e3, L.PFB_STFT_TWOSIDED, 5, 3)
    assert rc == L.PFB_OK
    assert np.array_equal(f, np.arange(8) * 1e3)
    assert np.allclose(t, ((5 + np.arange(3)) * 3 + 3.0) / 8e3, rtol=0, atol=1e-15)
    rc, _, t = _axes(16, 15, 4, 2.0, L.PFB_STFT_CENTERED, 7, 2)
    assert rc == L.PFB_OK and t[0] == (7 * 4 + 7.5) / 2.0 and t[1] == (8 * 4 + 7.5) / 2.0
    f2, t2 = stft_axes(768, 768, 768, 56e6, "centered", 3, 4)
    fr, tr = stft_ref.axes(768, 768, 768, 56e6, "centered", 3, 4)
    assert np.array_equal(f2, fr) and np.allclose(t2, tr, rtol=1e-15, atol=0)
    assert _axes(8, 9, 3, 1.0, 0, 0, 0)[0] == L.PFB_ERR_BAD_ARG      # L > nfft
    assert _axes(8, 6, 7, 1.0, 0, 0, 0)[0] == L.PFB_ERR_BAD_ARG      # H > L
    assert _axes(8, 6, 3, 1.0, 2, 0, 0)[0] == L.PFB_ERR_BAD_ARG      # unknown order
    assert _axes(8, 6, 3, 0.0, 0, 0, 0)[0] == L.PFB_ERR_BAD_ARG      # fs


def _cfg(win, **kw):
    d = dict(struct_size=C.sizeof(L.PfbStftConfig), window_length=768, hop=0, fft_length=0,
             window=win.ctypes.data_as(C.POINTER(C.c_float)), sample_format=L.PFB_FMT_INT16_IQ, bit_width=12,
             output=L.PFB_STFT_POWER, freq_order=L.PFB_STFT_CENTERED, scale=0.0, db_floor=0.0, kernel=0, device_id=-1)
    d.update(kw)
    return L.PfbStftConfig(**d)


def test_create_validates_before_the_device():
    lib = L.load()
    win = np.hamming(8192).astype(np.float32)
    h = C.c_void_p()
    create = lambda **kw: lib.pfb_stft_create(C.byref(_cfg(win, **kw)), C.byref(h))  # noqa: E731
    assert lib.pfb_stft_create(None, C.byref(h)) == L.PFB_ERR_BAD_ARG
    assert create(window_length=0) == L.PFB_ERR_BAD_ARG
    assert create(window_length=769, fft_length=768) == L.PFB_ERR_BAD_ARG     # L > nfft
    assert create(hop=769) == L.PFB_ERR_BAD_ARG                                # H > L
    assert create(window=C.POINTER(C.c_float)()) == L.PFB_ERR_BAD_ARG          # NULL window
    assert create(struct_size=8) == L.PFB_ERR_BAD_ARG
    assert create(output=3) == L.PFB_ERR_BAD_ARG
    assert create(freq_order=2) == L.PFB_ERR_BAD_ARG
    assert create(kernel=3) == L.PFB_ERR_BAD_ARG
    assert create(scale=-1.0) == L.PFB_ERR_BAD_ARG
    assert create(db_floor=float("nan")) == L.PFB_ERR_BAD_ARG
    assert create(scale=1e39) == L.PFB_ERR_BAD_ARG          # applied in float32: would be +inf
    assert create(db_floor=1e-46) == L.PFB_ERR_BAD_ARG      # would round to 0 (-inf for zero bins again)
    assert create(scale=1e-39) == L.PFB_ERR_BAD_ARG         # below FLT_MIN
    assert lib.pfb_stft_set_experiment(None, 1) == L.PFB_ERR_BAD_ARG
    assert create(window_length=1000, fft_length=4097) == L.PFB_ERR_UNSUPPORTED
    assert create(window_length=4097) == L.PFB_ERR_UNSUPPORTED                # nfft = L > 4096
    assert create(sample_format=7) == L.PFB_ERR_BAD_FORMAT
    assert create(sample_format=L.PFB_FMT_INT8_IQ, bit_width=12) == L.PFB_ERR_BAD_FORMAT
    assert create(bit_width=17) == L.PFB_ERR_BAD_FORMAT
    assert create(window_length=700, kernel=L.PFB_STFT_KERNEL_FUSED) == L.PFB_ERR_UNSUPPORTED  # no fused 700
    assert lib.pfb_stft_process(None, None, 0, None, 0, None, 0) == L.PFB_ERR_BAD_ARG
    assert lib.pfb_stft_frames_for(None, 0, None) == L.PFB_ERR_BAD_ARG
    assert lib.pfb_stft_last_kernel(None) == b""


def test_valid_config_has_no_cpu_fallback():
    lib = L.load()
    if lib.pfb_device_count() > 0:
        pytest.skip("a GPU is present")
    win = np.hamming(768).astype(np.float32)
    h = C.c_void_p()
    for kw in ({}, dict(kernel=L.PFB_STFT_KERNEL_GENERIC, fft_length=1000), dict(window_length=97, hop=1)):
        assert lib.pfb_stft_create(C.byref(_cfg(win, **kw)), C.byref(h)) == L.PFB_ERR_NO_DEVICE
        assert not h


@pytest.mark.parametrize("nfft,Lw,H,order", [(16, 16, 16, "centered"), (16, 11, 4, "centered"), (15, 15, 5, "centered"),
                                            (12, 7, 1, "twosided"), (9, 9, 3, "twosided")])
def test_reference_against_the_direct_sum(nfft, Lw, H, order):
    rng = np.random.default_rng(nfft * 100 + Lw + H)
    x = rng.standard_normal(200) + 1j * rng.standard_normal(200)
    w = rng.random(Lw)
    a = stft_ref.stft(x, w, H, nfft, order)
    b = stft_ref.stft_direct(x, w, H, nfft, order)
    assert a.shape == (stft_ref.num_frames(200, Lw, H), nfft)
    assert np.abs(a - b).max() <= 1e-12 * np.abs(b).max()


@pytest.mark.parametrize("M", [8, 56, 64])
def test_reference_power_equals_the_oracle_channelizer(oracle, M):
    """H = L = nfft = M, P = 1, D = M, default input_offset, h = reversed window: the oracle's e^{+j} channelizer gives
    Y_k = e^{j 2 pi k (M-1)/M} S_k (u_p[f] = h[p] x[f M + M-1-p]), so |Y_k|^2 = |S_k|^2 bin for bin in twosided order;
    this pins the sign of the exponent and the framing."""
    from oracle.pfb_oracle import OracleConfig
    from sdr_channelizer_amd import synth
    iq = synth.pulsed_iq_numpy(M * 40, 12, np.int16)
    x = oracle.unpack(iq, 12)
    w = np.hamming(M)
    y = oracle.channelize(x, w[::-1].copy(), OracleConfig(M, 1, M), "direct")
    s = stft_ref.stft(stft_ref.unpack(iq, "int16", 12), w, M, M, "twosided")
    assert s.shape == y.shape
    assert np.abs(stft_ref.power(s) - np.abs(y) ** 2).max() <= 1e-12 * (np.abs(y) ** 2).max()
    k = np.arange(M)
    assert np.abs(y - s * np.exp(2j * np.pi * k * (M - 1) / M)).max() <= 1e-12 * np.abs(y).max()
