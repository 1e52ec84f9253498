"""Matched filtering (pulse compression) of I/Q streams on the GPU, over the C ABI (pfb_mf_* in
include/pfb_channelizer.h, where the arithmetic is defined).

The reference makes coded pulses -- LFM sweeps and Barker-13 chips (generate_pulsed_iq.m:17-19,43-59), the 13-chip
burst tx_rx_pulses_usrp.cpp transmits and records next to the dwell it receives -- and has nothing that finds one
other than by its envelope.  ``MatchedFilter`` correlates a stream with a replica r,

    y[m] = g * sum_n conj(r[n]) * x[m+n],

so that output m is the sample at which a pulse equal to the replica starts; ``compress`` is the one-shot form,
``replica_from_pulse_train`` makes the replica of a ``PulseTrain`` configuration, ``pulse_delay_from_iq_files`` turns
the TX / RX record pair into a delay.  Nothing here computes on the CPU.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib as L
from ._handle import Handle, is_torch

_FMT = {"int8": L.PFB_FMT_INT8_IQ, "int16": L.PFB_FMT_INT16_IQ, "cf32": L.PFB_FMT_CF32}
_FMT_NAME = {v: k for k, v in _FMT.items()}
_OUTPUT = {"complex": L.PFB_MF_COMPLEX, "power": L.PFB_MF_POWER}
_ROUTE = {"auto": L.PFB_MF_ROUTE_AUTO, "fused": L.PFB_MF_ROUTE_FUSED, "partitioned": L.PFB_MF_ROUTE_PARTITIONED}
MAX_REPLICA = 65536


def _replica(replica) -> np.ndarray:
    r = np.asarray(replica)
    if not np.iscomplexobj(r) and r.ndim == 2 and r.shape[1] == 2:  # (K, 2) re, im columns
        r = r[:, 0].astype(np.float32) + 1j * r[:, 1].astype(np.float32)
    return np.ascontiguousarray(r, dtype=np.complex64).reshape(-1)


def _config(r: np.ndarray, sample_format, bit_width, output, normalize, fft_length, route, device) -> L.PfbMfConfig:
    return L.PfbMfConfig(C.sizeof(L.PfbMfConfig), r.size, r.view(np.float32).ctypes.data_as(C.POINTER(C.c_float)),
                         _FMT[sample_format], int(bit_width), _OUTPUT[output], L.PFB_MF_NORMALIZE if normalize else 0,
                         int(fft_length), _ROUTE[route], int(device))


def describe(replica, sample_format: str = "int16", bit_width: int = 12, output: str = "complex",
             normalize: bool = False, fft_length: int = 0, route: str = "auto") -> L.PfbMfPlan:
    """The plan the library makes for these settings (pfb_mf_describe; host only, needs no device)."""
    r = _replica(replica)
    cfg = _config(r, sample_format, bit_width, output, normalize, fft_length, route, -1)
    plan = L.PfbMfPlan()
    L.check(L.load().pfb_mf_describe(C.byref(cfg), C.byref(plan)), "pfb_mf_describe")
    return plan


class MatchedFilter(Handle):
    """Stateful matched filter of an I/Q stream against ``replica`` (complex, 1 <= K <= 65536 samples): each call
    returns the outputs its samples complete, N samples so far giving max(0, N - K + 1); a stream may be cut into calls
    of any length.  numpy in -> numpy out, CUDA tensor in -> CUDA tensor out."""

    _kind, _destroy, _get_device = "matched filter", "pfb_mf_destroy", "pfb_mf_get_device"

    def __init__(self, replica, sample_format: str = "int16", bit_width: int = 12, output: str = "complex",
                 normalize: bool = False, fft_length: int = 0, route: str = "auto", device: int = -1):
        self._h = C.c_void_p()
        lib = L.load()
        self.replica = _replica(replica)
        self.fmt = _FMT[sample_format]
        self.bit_width = int(bit_width)
        self.output = output
        cfg = _config(self.replica, sample_format, bit_width, output, normalize, fft_length, route, device)
        L.check(lib.pfb_mf_create(C.byref(cfg), C.byref(self._h)), "pfb_mf_create")
        self._created(lib)
        self.plan = L.PfbMfPlan()
        L.check(lib.pfb_mf_describe(C.byref(cfg), C.byref(self.plan)), "pfb_mf_describe")

    def reset(self) -> None:
        L.check(self._lib.pfb_mf_reset(self._h), "pfb_mf_reset")

    def set_stream(self, hip_stream: int) -> None:
        L.check(self._lib.pfb_mf_set_stream(self._h, C.c_void_p(hip_stream)), "pfb_mf_set_stream")

    def sync(self) -> None:
        L.check(self._lib.pfb_mf_sync(self._h), "pfb_mf_sync")

    @property
    def last_kernel(self) -> str:
        return self._lib.pfb_mf_last_kernel(self._h).decode()

    @property
    def next_index(self) -> int:
        """Stream index of the next output to be produced."""
        m = C.c_uint64()
        L.check(self._lib.pfb_mf_next_index(self._h, C.byref(m)), "pfb_mf_next_index")
        return int(m.value)

    def outputs_for(self, num_samples: int) -> int:
        f = C.c_uint64()
        L.check(self._lib.pfb_mf_outputs_for(self._h, int(num_samples), C.byref(f)), "pfb_mf_outputs_for")
        return int(f.value)

    def process(self, iq, out=None, sync: bool = True):
        """Filter one buffer; returns the outputs it completes: complex64, or float32 |y|^2 with output="power"."""
        complex_out = self.output == "complex"
        f = C.c_uint64()
        if is_torch(iq) and iq.is_cuda:
            n = self._device_samples(iq)
            F = self.outputs_for(n)
            out = self._output(out, (1, F), complex_out, iq.device).reshape(-1)
            if sync:
                L.check(self._lib.pfb_mf_process(self._h, C.c_void_p(iq.data_ptr()), n, C.c_void_p(out.data_ptr()), F,
                                                 C.byref(f), L.PFB_MEM_DEVICE), "pfb_mf_process")
            else:
                L.check(self._lib.pfb_mf_process_async(self._h, C.c_void_p(iq.data_ptr()), n,
                                                       C.c_void_p(out.data_ptr()), F, C.byref(f)),
                        "pfb_mf_process_async")
            return out
        a, n = self._host_samples(iq)
        F = self.outputs_for(n)
        res = self._output(out, (1, F), complex_out).reshape(-1)
        L.check(self._lib.pfb_mf_process(self._h, C.c_void_p(a.ctypes.data), n, C.c_void_p(res.ctypes.data), F,
                                         C.byref(f), L.PFB_MEM_HOST), "pfb_mf_process")
        return res

    __call__ = process

    def process_iq_file(self, path: str, reset: bool = True):
        """One .iq record from disk (header checked by the library, payload streamed in chunks).
        Returns (outputs, PfbIqInfo)."""
        from . import iqfile
        with open(path, "rb") as fh:
            info = iqfile.parse_header(fh.read(128))
        if reset:
            self.reset()
        F = self.outputs_for(int(info.packet.numSamples))
        res = self._output(None, (1, F), self.output == "complex").reshape(-1)
        f = C.c_uint64()
        got = L.PfbIqInfo()
        L.check(self._lib.pfb_mf_process_iq_file(self._h, str(path).encode(), C.c_void_p(res.ctypes.data), F, C.byref(f),
                                                 C.byref(got)), "pfb_mf_process_iq_file")
        return res[: f.value], got


def _format_of(x) -> str:
    if is_torch(x):
        import torch
        return {torch.int8: "int8", torch.int16: "int16"}.get(x.dtype, "cf32")
    return {np.dtype(np.int8): "int8", np.dtype(np.int16): "int16"}.get(np.asarray(x).dtype, "cf32")


def compress(iq, replica, *, sample_format: str | None = None, bit_width: int = 12, output: str = "complex",
             normalize: bool = False, fft_length: int = 0, route: str = "auto", device: int = -1):
    """``MatchedFilter(replica, ...).process(iq)`` in one call; the sample format follows iq's dtype."""
    with MatchedFilter(replica, sample_format or _format_of(iq), bit_width, output, normalize, fft_length, route,
                       device) as mf:
        return mf.process(iq)


def compress_iq_file(path: str, replica, *, output: str = "complex", normalize: bool = False, fft_length: int = 0,
                     route: str = "auto", device: int = -1):
    """One whole .iq record against ``replica``: format and bit width from its header.  Returns (y, info)."""
    from . import iqfile
    with open(path, "rb") as fh:
        info = iqfile.parse_header(fh.read(128))
    with MatchedFilter(replica, _FMT_NAME[int(info.sample_format)], int(info.packet.bitWidth), output, normalize,
                       fft_length, route, device) as mf:
        return mf.process_iq_file(path)


def replica_from_pulse_train(**kw) -> np.ndarray:
    """One pulse of a ``PulseTrain`` configuration (keywords: pulse_source._config) as complex64 in full scales,
    (I + jQ) / 2^(bit_width-1): the train with its noise off, generated on the GPU from the first pulse's first sample
    over the pulse's length (after the Barker adjustment) and read back once."""
    from .pulse_source import PulseTrain
    kw = dict(kw, noise_sigma=0.0)
    with PulseTrain(**kw) as pt:
        n = int(pt.params.pulse_samples)
        iq = pt.generate(n, start=int(pt.config.first_pulse)).cpu().numpy()
        full = 1.0 if pt.fmt == L.PFB_FMT_CF32 else float(1 << (int(pt.config.bit_width) - 1))
    return (iq[:, 0].astype(np.float32) / np.float32(full) + 1j * (iq[:, 1].astype(np.float32) / np.float32(full))) \
        .astype(np.complex64)


def pulse_delay_from_iq_files(tx_path: str, rx_path: str, device: int = -1) -> dict:
    """The record pair tx_rx_pulses_usrp.cpp writes: the transmitted burst is the replica, the received dwell is
    compressed with it (power output, argmax on the device).  Returns lag_samples (the sample of the RX record at which
    the burst starts), lag_seconds = lag / fs, peak_power and start_time_offset = rx.sampleStartTime -
    tx.sampleStartTime, the difference of the two records' clocks."""
    import torch

    from . import iqfile
    tx, rx = iqfile.read_iq(tx_path), iqfile.read_iq(rx_path)
    K = tx.iq.shape[0]
    if K > MAX_REPLICA:
        raise ValueError(f"{tx_path}: the TX record has {K} samples, a replica takes at most {MAX_REPLICA}")
    if K < 1 or rx.iq.shape[0] < K:
        raise ValueError(f"the RX record ({rx.iq.shape[0]} samples) is shorter than the TX record ({K})")
    full = np.float32(1 << (tx.bitWidth - 1))
    r = (tx.iq[:, 0].astype(np.float32) / full + 1j * (tx.iq[:, 1].astype(np.float32) / full)).astype(np.complex64)
    fmt = "int8" if rx.iq.dtype == np.int8 else "int16"
    with MatchedFilter(r, fmt, rx.bitWidth, "power", device=device) as mf:
        d_rx = torch.from_numpy(np.array(rx.iq)).to(torch.device("cuda", mf.device_index))  # a writable copy for torch
        p = mf.process(d_rx)
        peak, lag = torch.max(p, dim=0)
        lag, peak = int(lag.item()), float(peak.item())
    return {"lag_samples": lag, "lag_seconds": lag / rx.fs, "peak_power": peak,
            "start_time_offset": rx.sampleStartTime - tx.sampleStartTime}
