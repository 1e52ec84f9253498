"""Short-time Fourier transform of I/Q streams on the GPU, over the C ABI (pfb_stft_* in include/pfb_channelizer.h).

The reference computes its spectrograms with MathWorks' functions:

    [s,f,t] = stft(iq,fs,'Window',hamming(768),'OverlapLength',0)     spectrogram_my_iq.m:111
    mesh(t*1e3,(f+fc)*1e-6,abs(s).^2)                                   spectrogram_my_iq.m:112
    spectrogram(iq,1024,0,1024,Fs,'centered','yaxis')                   generate_pulsed_iq.m:105

``stft`` keeps stft's argument names and return order; ``Stft`` is the stateful, callable object behind it (a stream
cut into calls gives the same bits as one call); ``spectrogram_from_iq_file`` is spectrogram_my_iq.m's load +
normalise + stft + abs().^2 in one call.  The raw integer I/Q goes to the GPU as it is: the normalise step
(I + jQ)/2^(bitWidth-1) is folded into the window.  Nothing here computes on the CPU.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib as L
from ._handle import Handle, is_torch

_FMT = {"int8": L.PFB_FMT_INT8_IQ, "int16": L.PFB_FMT_INT16_IQ, "cf32": L.PFB_FMT_CF32}
_OUTPUT = {"complex": L.PFB_STFT_COMPLEX, "power": L.PFB_STFT_POWER, "db": L.PFB_STFT_DB}
_ORDER = {"centered": L.PFB_STFT_CENTERED, "twosided": L.PFB_STFT_TWOSIDED}
_KERNEL = {"auto": L.PFB_STFT_KERNEL_AUTO, "generic": L.PFB_STFT_KERNEL_GENERIC, "fused": L.PFB_STFT_KERNEL_FUSED}


def stft_axes(fft_length: int, window_length: int, hop: int, fs: float, frequency_range: str = "centered",
              first_frame: int = 0, frames: int = 0) -> tuple[np.ndarray, np.ndarray]:
    """(f, t): f[r] = k_r fs / nfft for every row, t[m] = ((first_frame + m) H + L/2) / fs, the segment centre
    (the time convention is unpinned)."""
    f = np.empty(int(fft_length), np.float64)
    t = np.empty(int(frames), np.float64)
    L.check(L.load().pfb_stft_axes(int(fft_length), int(window_length), int(hop), float(fs), _ORDER[frequency_range],
                                   int(first_frame), int(frames), f.ctypes.data_as(C.POINTER(C.c_double)),
                                   t.ctypes.data_as(C.POINTER(C.c_double))), "pfb_stft_axes")
    return f, t


def _format_of(x) -> str:
    if is_torch(x):
        import torch
        return {torch.int8: "int8", torch.int16: "int16"}.get(x.dtype, "cf32")
    dt = np.asarray(x).dtype
    return {np.dtype(np.int8): "int8", np.dtype(np.int16): "int16"}.get(dt, "cf32")


class Stft(Handle):
    """Stateful STFT of an I/Q stream: frame m covers samples [m H, m H + L) of everything fed since creation or
    ``reset()``; each call returns the frames it completes, frame-major, shape (frames, nfft) -- row r of a frame is
    bin k_r ('centered' or 'twosided' order).  numpy in -> numpy out, CUDA tensor in -> CUDA tensor out."""

    _kind, _destroy, _get_device = "STFT", "pfb_stft_destroy", "pfb_stft_get_device"

    def __init__(self, window, *, hop: int | None = None, overlap_length: int | None = None,
                 fft_length: int | None = None, sample_format: str = "cf32", bit_width: int = 12,
                 output: str = "complex", frequency_range: str = "centered", scale: float = 1.0, db_floor: float = 0.0,
                 kernel: str = "auto", device: int = -1):
        self._h = C.c_void_p()
        lib = L.load()
        self.window = np.ascontiguousarray(window, dtype=np.float32).reshape(-1)
        self.window_length = Lw = self.window.size
        if hop is not None and overlap_length is not None:
            raise ValueError("give hop or overlap_length, not both")
        self.hop = int(hop) if hop is not None else Lw - int(overlap_length or 0)
        if self.hop < 1:  # hop 0 would mean "L" to the library
            raise ValueError(f"hop must be at least 1 (overlap_length < window length), got {self.hop}")
        self.fft_length = int(fft_length) if fft_length is not None else Lw
        self.fmt = _FMT[sample_format]
        self.bit_width = int(bit_width)
        self.output = output
        self.frequency_range = frequency_range
        cfg = L.PfbStftConfig(C.sizeof(L.PfbStftConfig), Lw, self.hop, self.fft_length,
                              self.window.ctypes.data_as(C.POINTER(C.c_float)), self.fmt,
                              self.bit_width, _OUTPUT[output], _ORDER[frequency_range], float(scale), float(db_floor),
                              _KERNEL[kernel], int(device))
        L.check(lib.pfb_stft_create(C.byref(cfg), C.byref(self._h)), "pfb_stft_create")
        self._created(lib)
        self.frames_done = 0  # global index of the next frame (the time axis of later calls)

    def reset(self) -> None:
        L.check(self._lib.pfb_stft_reset(self._h), "pfb_stft_reset")
        self.frames_done = 0

    @property
    def last_kernel(self) -> str:
        return self._lib.pfb_stft_last_kernel(self._h).decode()

    def frames_for(self, num_samples: int) -> int:
        f = C.c_uint64()
        L.check(self._lib.pfb_stft_frames_for(self._h, int(num_samples), C.byref(f)), "pfb_stft_frames_for")
        return int(f.value)

    def set_stream(self, hip_stream: int) -> None:
        L.check(self._lib.pfb_stft_set_stream(self._h, C.c_void_p(hip_stream)), "pfb_stft_set_stream")

    def sync(self) -> None:
        L.check(self._lib.pfb_stft_sync(self._h), "pfb_stft_sync")

    def axes(self, fs: float, first_frame: int = 0, frames: int = 0) -> tuple[np.ndarray, np.ndarray]:
        return stft_axes(self.fft_length, self.window_length, self.hop, fs, self.frequency_range, first_frame, frames)

    # -- samples -----------------------------------------------------------------
    def __call__(self, iq, out=None, sync: bool = True):
        """Transform one buffer; returns the (frames, nfft) frames it completes."""
        complex_out = self.output == "complex"
        if is_torch(iq) and iq.is_cuda:
            n = self._device_samples(iq)
            F = self.frames_for(n)
            out = self._output(out, (F, self.fft_length), complex_out, iq.device)
            f = C.c_uint64()
            if sync:
                L.check(self._lib.pfb_stft_process(self._h, C.c_void_p(iq.data_ptr()), n, C.c_void_p(out.data_ptr()),
                                                   F, C.byref(f), L.PFB_MEM_DEVICE), "pfb_stft_process")
            else:
                L.check(self._lib.pfb_stft_process_async(self._h, C.c_void_p(iq.data_ptr()), n,
                                                         C.c_void_p(out.data_ptr()), F, C.byref(f)),
                        "pfb_stft_process_async")
            self.frames_done += F
            return out
        a, n = self._host_samples(iq)
        F = self.frames_for(n)
        res = self._output(out, (F, self.fft_length), complex_out)
        f = C.c_uint64()
        L.check(self._lib.pfb_stft_process(self._h, C.c_void_p(a.ctypes.data), n, C.c_void_p(res.ctypes.data), F,
                                           C.byref(f), L.PFB_MEM_HOST), "pfb_stft_process")
        self.frames_done += F
        return res

    def process_iq_file(self, path: str, reset: bool = True):
        """One .iq record from disk (header parsed and checked by the library, payload streamed in chunks).
        Returns (frames x nfft array, PfbIqInfo)."""
        from . import iqfile
        with open(path, "rb") as fh:
            info = iqfile.parse_header(fh.read(128))
        if reset:
            self.reset()
        F = self.frames_for(int(info.packet.numSamples))
        res = self._output(None, (F, self.fft_length), self.output == "complex")
        f = C.c_uint64()
        got = L.PfbIqInfo()
        L.check(self._lib.pfb_stft_process_iq_file(self._h, path.encode(), C.c_void_p(res.ctypes.data), F, C.byref(f),
                                                   C.byref(got)), "pfb_stft_process_iq_file")
        self.frames_done += int(f.value)
        return res[: f.value], got


def stft(x, fs: float, window, overlap_length: int = 0, fft_length: int | None = None,
         frequency_range: str = "centered", *, sample_format: str | None = None, bit_width: int = 12,
         output: str = "complex", scale: float = 1.0, db_floor: float = 0.0, kernel: str = "auto", device: int = -1):
    """MATLAB's ``[s, f, t] = stft(x, fs, 'Window', window, 'OverlapLength', overlap_length, 'FFTLength', fft_length,
    'FrequencyRange', frequency_range)`` for 'centered' and 'twosided'.  ``s`` is (nfft, frames): a transposed view of
    the frame-major result, so s[r, m] is MATLAB's s(r+1, m+1).  ``x``: complex or interleaved float32 samples, or the
    recorders' raw int8 / int16 I/Q (scaled by 2^-(bit_width-1)); numpy or a CUDA tensor.  fft_length=None means
    nfft = len(window) (stft's default FFTLength when only 'Window' is given is unpinned)."""
    fmt = sample_format or _format_of(x)
    with Stft(window, overlap_length=overlap_length, fft_length=fft_length, sample_format=fmt, bit_width=bit_width,
              output=output, frequency_range=frequency_range, scale=scale, db_floor=db_floor, kernel=kernel,
              device=device) as st:
        y = st(x)
        f, t = st.axes(fs, 0, y.shape[0])
    return y.T, f, t


def spectrogram_from_iq_file(path: str, window=None, overlap_length: int = 0, fft_length: int | None = None,
                             frequency_range: str = "centered", output: str = "power", scale: float = 1.0,
                             db_floor: float = 0.0, kernel: str = "auto", device: int = -1):
    """spectrogram_my_iq.m:105-112 for one record: iq = (I + jQ)/2^(bitWidth-1),
    [s,f,t] = stft(iq, fs, 'Window', hamming(768), 'OverlapLength', 0), abs(s).^2.  Returns (p, f, t, info): p is
    (nfft, frames) (a transposed view, p[r, m] = MATLAB's abs(s(r+1, m+1)).^2 with output="power"), f the baseband
    frequencies (the script plots f + fc, fc = info.packet.frequencyHz), t the segment centres in seconds.
    np.hamming is MATLAB's symmetric hamming()."""
    from . import iqfile
    if window is None:
        window = np.hamming(768)
    with open(path, "rb") as fh:
        info = iqfile.parse_header(fh.read(128))
    fmt = {L.PFB_FMT_INT8_IQ: "int8", L.PFB_FMT_INT16_IQ: "int16", L.PFB_FMT_CF32: "cf32"}[int(info.sample_format)]
    with Stft(window, overlap_length=overlap_length, fft_length=fft_length, sample_format=fmt,
              bit_width=int(info.packet.bitWidth), output=output, frequency_range=frequency_range, scale=scale,
              db_floor=db_floor, kernel=kernel, device=device) as st:
        y, info = st.process_iq_file(path)
        f, t = st.axes(float(info.packet.sampleRateSps), 0, y.shape[0])
    return y.T, f, t, info
