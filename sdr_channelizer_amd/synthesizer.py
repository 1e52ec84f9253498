"""Channel synthesis on the GPU, over the C ABI (pfb_chsyn_* in include/pfb_channelizer.h, where the arithmetic is
defined): the twin of ``Channelizer``.

``ChannelSynthesizer`` takes what a frame-major ``Channelizer`` writes -- F frames of M channel values -- and returns
the F * D samples of the full-rate stream they stand for, all channels or the ones a weight mask keeps;
``synthesize`` is the one-shot form.  ``design_synthesis_taps`` makes the taps that pair with the channelizer's own
prototype, ``synthesis_delay`` is the delay of such a pair, and ``isolate_band`` runs the whole chain -- a 2x
oversampled channelizer, a 0/1 mask, the synthesizer -- and returns the kept band aligned with its input.

For the 2x oversampled bank (D = M/2) with ``design_prototype(M, 12)`` on the analysis side and
``design_synthesis_taps(M, M // 2)`` here the chain returns its input to 3.6e-5 (-89 dB).  A critically sampled bank
(D = M) with the same Kaiser-windowed sinc on both sides reconstructs only to about 20 %: that prototype is a Nyquist
filter, not a root-Nyquist one, and what comes out at D = M is the business of the caller's taps.  Nothing here
computes on the CPU.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib as L
from ._handle import Handle, is_torch
from .channelizer import Channelizer, design_prototype

_ROUTE = {"auto": L.PFB_CHSYN_ROUTE_AUTO, "fused": L.PFB_CHSYN_ROUTE_FUSED, "generic": L.PFB_CHSYN_ROUTE_GENERIC}
_ROUTE_NAME = {v: k for k, v in _ROUTE.items()}
_OUTPUT = {"cf32": L.PFB_FMT_CF32, "int16": L.PFB_FMT_INT16_IQ}


def design_synthesis_taps(num_bands: int, decimation: int | None = None, taps_per_channel: int = 12) -> np.ndarray:
    """The synthesis taps that pair with ``design_prototype(num_bands, ...)`` at decimation D:
    ``design_prototype(D, taps_per_channel * M / D)``, M * taps_per_channel values with cutoff fs / (2 D)."""
    M = int(num_bands)
    D = M if decimation is None else int(decimation)
    if D < 1 or (M * taps_per_channel) % D:
        raise ValueError("decimation must divide num_bands * taps_per_channel")
    return design_prototype(D, taps_per_channel * M // D)


def synthesis_delay(analysis_taps_len: int, synthesis_taps_len: int, input_offset: int) -> int:
    """Samples by which synthesize(channelize(x)) lags x: L_h/2 + L_g/2 - input_offset."""
    return int(analysis_taps_len) // 2 + int(synthesis_taps_len) // 2 - int(input_offset)


def _config(taps: np.ndarray, M: int, D: int, scale, output, bit_width, fftshift, derotate, route, device,
            layout=L.PFB_LAYOUT_FRAME_MAJOR) -> L.PfbChsynConfig:
    flags = (L.PFB_CHSYN_FFTSHIFT if fftshift else 0) | (L.PFB_CHSYN_DEROTATE if derotate else 0)
    return L.PfbChsynConfig(C.sizeof(L.PfbChsynConfig), M, taps.size // M, D, taps.ctypes.data_as(C.POINTER(C.c_float)),
                            float(scale), _OUTPUT[output], int(bit_width), layout, flags, _ROUTE[route], int(device))


def _taps(taps, M: int) -> np.ndarray:
    t = np.ascontiguousarray(taps, dtype=np.float32).reshape(-1)
    if t.size == 0 or t.size % M:
        raise ValueError("taps must hold num_bands * taps_per_channel coefficients")
    return t


def describe(num_bands: int, taps, decimation: int | None = None, *, scale: float = 0.0, output: str = "cf32",
             bit_width: int = 12, fftshift: bool = False, derotate: bool = False, route: str = "auto") -> L.PfbChsynPlan:
    """The plan the library makes for these settings (pfb_chsyn_describe; host only, needs no device)."""
    M = int(num_bands)
    t = _taps(taps, M)
    cfg = _config(t, M, M if decimation is None else int(decimation), scale, output, bit_width, fftshift, derotate,
                  route, -1)
    plan = L.PfbChsynPlan()
    L.check(L.load().pfb_chsyn_describe(C.byref(cfg), C.byref(plan)), "pfb_chsyn_describe")
    return plan


class ChannelSynthesizer(Handle):
    """Stateful synthesizer of a frame stream: each call takes F frames (F x M complex64, the columns a ``Channelizer``
    with the same ``fftshift`` / ``derotate`` wrote) and returns F * D samples; a stream may be cut into calls of any
    length, and within one route every cutting gives the same bits.  numpy in -> numpy out, CUDA tensor in -> CUDA
    tensor out.  ``output="int16"`` returns (N, 2) int16 I,Q at ``bit_width`` instead of complex64."""

    _kind, _destroy, _get_device = "channel synthesizer", "pfb_chsyn_destroy", "pfb_chsyn_get_device"

    def __init__(self, num_bands: int, taps=None, decimation: int | None = None, *, taps_per_channel: int = 12,
                 scale: float = 0.0, output: str = "cf32", bit_width: int = 12, fftshift: bool = False,
                 derotate: bool = False, weights=None, route: str = "auto", device: int = -1):
        self._h = C.c_void_p()
        lib = L.load()
        M = int(num_bands)
        self.num_bands = M
        self.decimation = M if decimation is None else int(decimation)
        if taps is None:
            taps = design_synthesis_taps(M, self.decimation, taps_per_channel)
        self.taps = _taps(taps, M)
        self.output = output
        self.bit_width = int(bit_width)
        self.fmt = L.PFB_FMT_CF32  # of the input values: complex64
        cfg = _config(self.taps, M, self.decimation, scale, output, bit_width, fftshift, derotate, route, device)
        L.check(lib.pfb_chsyn_create(C.byref(cfg), C.byref(self._h)), "pfb_chsyn_create")
        self._created(lib)
        self.plan = L.PfbChsynPlan()
        L.check(lib.pfb_chsyn_describe(C.byref(cfg), C.byref(self.plan)), "pfb_chsyn_describe")
        if weights is not None:
            self.set_weights(weights)

    @property
    def route(self) -> str:
        return _ROUTE_NAME[int(self.plan.route)]

    def reset(self) -> None:
        L.check(self._lib.pfb_chsyn_reset(self._h), "pfb_chsyn_reset")

    def set_stream(self, hip_stream: int) -> None:
        L.check(self._lib.pfb_chsyn_set_stream(self._h, C.c_void_p(hip_stream)), "pfb_chsyn_set_stream")

    def sync(self) -> None:
        L.check(self._lib.pfb_chsyn_sync(self._h), "pfb_chsyn_sync")

    def set_weights(self, weights) -> None:
        """One real weight per COLUMN (None: all ones), in effect from the next frame on."""
        if weights is None:
            L.check(self._lib.pfb_chsyn_set_weights(self._h, None), "pfb_chsyn_set_weights")
            return
        w = np.ascontiguousarray(weights, dtype=np.float32).reshape(-1)
        if w.size != self.num_bands:
            raise ValueError(f"expected {self.num_bands} weights, got {w.size}")
        L.check(self._lib.pfb_chsyn_set_weights(self._h, C.c_void_p(w.ctypes.data)), "pfb_chsyn_set_weights")

    def set_frame_index(self, next_frame: int) -> None:
        L.check(self._lib.pfb_chsyn_set_frame_index(self._h, int(next_frame)), "pfb_chsyn_set_frame_index")

    @property
    def frame_index(self) -> int:
        m = C.c_uint64()
        L.check(self._lib.pfb_chsyn_get_frame_index(self._h, C.byref(m)), "pfb_chsyn_get_frame_index")
        return int(m.value)

    def samples_for(self, num_frames: int) -> int:
        s = C.c_uint64()
        L.check(self._lib.pfb_chsyn_samples_for(self._h, int(num_frames), C.byref(s)), "pfb_chsyn_samples_for")
        return int(s.value)

    @property
    def last_kernel(self) -> str:
        return self._lib.pfb_chsyn_last_kernel(self._h).decode()

    def _frames(self, shape, strides, itemsize: int) -> tuple[int, int]:
        """(frames, ld) of an (F, M) matrix whose rows may be further apart than M values."""
        M = self.num_bands
        if len(shape) != 2 or shape[1] != M:
            raise ValueError(f"expected frames of shape (F, {M}), got {tuple(shape)}")
        if shape[0] <= 1:
            return int(shape[0]), M
        if strides[1] != itemsize or strides[0] % itemsize or strides[0] < M * itemsize:
            raise ValueError("frames must be rows of contiguous values, at a stride of whole values")
        return int(shape[0]), strides[0] // itemsize

    def process(self, y, sync: bool = True):
        """Synthesize one buffer of frames; returns the F * D samples they complete."""
        n_out = C.c_uint64()
        if is_torch(y) and y.is_cuda:
            import torch
            if y.dtype != torch.complex64:
                raise TypeError(f"expected complex64 frames for this {self._kind}, got {y.dtype}")
            if y.device.index != self.device_index:
                raise ValueError(f"frames are on cuda:{y.device.index}, the {self._kind} on cuda:{self.device_index}")
            F, ld = self._frames(tuple(y.shape), tuple(s * 8 for s in y.stride()), 8)
            N = self.samples_for(F)
            out = (torch.empty(N, dtype=torch.complex64, device=y.device) if self.output == "cf32"
                   else torch.empty((N, 2), dtype=torch.int16, device=y.device))
            if sync:
                L.check(self._lib.pfb_chsyn_process(self._h, C.c_void_p(y.data_ptr()), F, ld, C.c_void_p(out.data_ptr()),
                                                    N, C.byref(n_out), L.PFB_MEM_DEVICE), "pfb_chsyn_process")
            else:
                L.check(self._lib.pfb_chsyn_process_async(self._h, C.c_void_p(y.data_ptr()), F, ld,
                                                          C.c_void_p(out.data_ptr()), N, C.byref(n_out)),
                        "pfb_chsyn_process_async")
            return out
        a = np.asarray(y)
        if a.dtype != np.complex64:
            raise TypeError(f"expected complex64 frames for this {self._kind}, got {a.dtype}")
        F, ld = self._frames(a.shape, a.strides, 8)
        N = self.samples_for(F)
        out = np.empty(N, dtype=np.complex64) if self.output == "cf32" else np.empty((N, 2), dtype=np.int16)
        L.check(self._lib.pfb_chsyn_process(self._h, C.c_void_p(a.ctypes.data), F, ld, C.c_void_p(out.ctypes.data), N,
                                            C.byref(n_out), L.PFB_MEM_HOST), "pfb_chsyn_process")
        return out

    __call__ = process


def synthesize(y, taps=None, *, decimation: int | None = None, taps_per_channel: int = 12, scale: float = 0.0,
               output: str = "cf32", bit_width: int = 12, fftshift: bool = False, derotate: bool = False, weights=None,
               route: str = "auto", device: int = -1):
    """``ChannelSynthesizer(M, taps, ...).process(y)`` in one call; M is the width of ``y``."""
    with ChannelSynthesizer(int(y.shape[1]), taps, decimation, taps_per_channel=taps_per_channel, scale=scale,
                            output=output, bit_width=bit_width, fftshift=fftshift, derotate=derotate, weights=weights,
                            route=route, device=device) as sy:
        return sy.process(y)


def isolate_band(iq, num_bands: int, columns, *, sample_format: str | None = None, bit_width: int = 12,
                 taps_per_channel: int = 12, fftshift: bool = False, route: str = "auto", device: int = -1):
    """The part of ``iq`` that falls into the given channelizer ``columns``, as a complex64 stream at the full rate:
    a 2x oversampled channelizer (M = num_bands, D = M/2, ``design_prototype(M, taps_per_channel)``), a 0/1 mask over
    its columns (in the fftshift-ed order with ``fftshift=True``), the synthesizer with
    ``design_synthesis_taps(M, M/2, taps_per_channel)``.  The delay of the pair is removed: index i of the result
    lines up with index i of the input, and the result is as long as the input.  Raw I/Q as ``Channelizer`` takes it
    (int8 / int16 at ``bit_width``, or complex64 / float32 pairs); numpy in -> numpy out, CUDA tensor in -> CUDA
    tensor out."""
    from .matched_filter import _format_of
    M = int(num_bands)
    if M % 2:
        raise ValueError("isolate_band needs an even band count: the bank is 2x oversampled")
    D = M // 2
    h = design_prototype(M, taps_per_channel)
    g = design_synthesis_taps(M, D, taps_per_channel)
    delay = synthesis_delay(h.size, g.size, D - 1)
    mask = np.zeros(M, dtype=np.float32)
    mask[np.asarray(list(columns), dtype=np.int64)] = 1.0
    on_device = is_torch(iq) and iq.is_cuda
    fmt = sample_format or _format_of(iq)
    if on_device:
        import torch
        x = torch.view_as_real(iq) if iq.is_complex() else iq
        x = x.reshape(-1, 2)
        n = x.shape[0]
        pad = -(-(n + delay) // D) * D - n  # the frames that hold the last delayed sample, whole
        x = torch.cat([x, torch.zeros((pad, 2), dtype=x.dtype, device=x.device)]).contiguous()
    else:
        x = np.asarray(iq)
        if np.iscomplexobj(x):
            x = np.ascontiguousarray(x, dtype=np.complex64).view(np.float32)
        x = x.reshape(-1, 2)
        n = x.shape[0]
        pad = -(-(n + delay) // D) * D - n
        x = np.concatenate([x, np.zeros((pad, 2), dtype=x.dtype)])
    with Channelizer(M, taps=h, decimation=D, sample_format=fmt, bit_width=bit_width, fftshift=fftshift,
                     device=device) as ch, \
            ChannelSynthesizer(M, g, D, fftshift=fftshift, weights=mask, route=route, device=device) as sy:
        out = sy.process(ch(x))
    return out[delay:delay + n]
