"""A bank of frequency-offset hypotheses on the matched filter, over the C ABI (pfb_mfbank_* in
include/pfb_channelizer.h, where the arithmetic is defined): delay and carrier of a coded pulse in one pass.

``MatchedFilter`` finds a pulse only at the carrier its replica was made for; the reference draws its carriers at random
(generate_pulsed_iq.m:13) and records TX and RX off two oscillators (tx_rx_pulses_usrp.cpp).  ``MatchedFilterBank``
correlates with H copies of the replica, copy h modulated to q_h = (first_bin + h) * bin_step bins of the FFT,

    y_h[m] = g * sum_n conj(r[n]) * exp(-2j pi q_h n / fft_length) * x[m+n],        p_h[m] = |y_h[m]|^2,

and returns per output the largest power and its h (``output="best"``) or all of them (``output="surface"``).
``compress_bank`` is the one-shot form, ``bank_frequencies`` the offsets in Hz, ``pulse_delay_and_offset_from_iq_files``
turns the TX / RX record pair into a delay and a carrier offset.  Nothing here computes on the CPU.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib as L
from ._handle import Handle, is_torch
from .matched_filter import _FMT, _format_of, _replica

_OUTPUT = {"best": L.PFB_MFBANK_BEST, "surface": L.PFB_MFBANK_SURFACE}
_NO_REPLICA = C.POINTER(C.c_float)()


def _config(r, sample_format, bit_width, first_bin, num_hypotheses, bin_step, output, normalize, fft_length,
            device) -> L.PfbMfbankConfig:
    ptr = _NO_REPLICA if r is None else r.view(np.float32).ctypes.data_as(C.POINTER(C.c_float))
    return L.PfbMfbankConfig(C.sizeof(L.PfbMfbankConfig), 0 if r is None else r.size, ptr, _FMT[sample_format],
                             int(bit_width), _OUTPUT[output], L.PFB_MF_NORMALIZE if normalize else 0, int(fft_length),
                             int(first_bin), int(num_hypotheses), int(bin_step), int(device))


def describe_bank(replica, sample_format: str = "int16", bit_width: int = 12, *, first_bin: int, num_hypotheses: int,
                  bin_step: int = 1, output: str = "best", normalize: bool = False,
                  fft_length: int = 0) -> L.PfbMfbankPlan:
    """The plan the library makes for these settings (pfb_mfbank_describe; host only, needs no device)."""
    r = _replica(replica)
    cfg = _config(r, sample_format, bit_width, first_bin, num_hypotheses, bin_step, output, normalize, fft_length, -1)
    plan = L.PfbMfbankPlan()
    L.check(L.load().pfb_mfbank_describe(C.byref(cfg), C.byref(plan)), "pfb_mfbank_describe")
    return plan


def bank_frequencies(fs: float, *, first_bin: int, num_hypotheses: int, bin_step: int = 1,
                     fft_length: int = 0) -> np.ndarray:
    """f_h = (first_bin + h) * bin_step * fs / fft_length in Hz, h = 0 .. H-1 (pfb_mfbank_frequencies; host only)."""
    cfg = _config(None, "int16", 12, first_bin, num_hypotheses, bin_step, "best", False, fft_length, -1)
    out = np.zeros(max(int(num_hypotheses), 0), np.float64)
    L.check(L.load().pfb_mfbank_frequencies(C.byref(cfg), float(fs), out.ctypes.data_as(C.POINTER(C.c_double))),
            "pfb_mfbank_frequencies")
    return out


class MatchedFilterBank(Handle):
    """Stateful bank of H matched filters of an I/Q stream against ``replica`` (complex, 1 <= K <= fft_length/2) at the
    offsets (first_bin + h) * bin_step bins: each call returns the outputs its samples complete, N samples so far giving
    max(0, N - K + 1); a stream may be cut into calls of any length.  numpy in -> numpy out, CUDA tensor in -> CUDA
    tensors out."""

    _kind, _destroy, _get_device = "matched-filter bank", "pfb_mfbank_destroy", "pfb_mfbank_get_device"

    def __init__(self, replica, sample_format: str = "int16", bit_width: int = 12, *, first_bin: int,
                 num_hypotheses: int, bin_step: int = 1, output: str = "best", normalize: bool = False,
                 fft_length: int = 0, device: int = -1):
        self._h = C.c_void_p()
        lib = L.load()
        self.replica = _replica(replica)
        self.fmt = _FMT[sample_format]
        self.bit_width = int(bit_width)
        self.output = output
        self.num_hypotheses = int(num_hypotheses)
        self._cfg = _config(self.replica, sample_format, bit_width, first_bin, num_hypotheses, bin_step, output,
                            normalize, fft_length, device)
        L.check(lib.pfb_mfbank_create(C.byref(self._cfg), C.byref(self._h)), "pfb_mfbank_create")
        self._created(lib)
        self._plan = L.PfbMfbankPlan()
        L.check(lib.pfb_mfbank_describe(C.byref(self._cfg), C.byref(self._plan)), "pfb_mfbank_describe")

    @property
    def plan(self) -> L.PfbMfbankPlan:
        return self._plan

    def frequencies(self, fs: float) -> np.ndarray:
        """The offset in Hz each hypothesis assumes at sample rate fs."""
        out = np.zeros(self.num_hypotheses, np.float64)
        L.check(self._lib.pfb_mfbank_frequencies(C.byref(self._cfg), float(fs), out.ctypes.data_as(C.POINTER(C.c_double))),
                "pfb_mfbank_frequencies")
        return out

    def reset(self) -> None:
        L.check(self._lib.pfb_mfbank_reset(self._h), "pfb_mfbank_reset")

    def set_stream(self, hip_stream: int) -> None:
        L.check(self._lib.pfb_mfbank_set_stream(self._h, C.c_void_p(hip_stream)), "pfb_mfbank_set_stream")

    def sync(self) -> None:
        L.check(self._lib.pfb_mfbank_sync(self._h), "pfb_mfbank_sync")

    @property
    def last_kernel(self) -> str:
        return self._lib.pfb_mfbank_last_kernel(self._h).decode()

    @property
    def next_index(self) -> int:
        """Stream index of the next output to be produced."""
        m = C.c_uint64()
        L.check(self._lib.pfb_mfbank_next_index(self._h, C.byref(m)), "pfb_mfbank_next_index")
        return int(m.value)

    def outputs_for(self, num_samples: int) -> int:
        f = C.c_uint64()
        L.check(self._lib.pfb_mfbank_outputs_for(self._h, int(num_samples), C.byref(f)), "pfb_mfbank_outputs_for")
        return int(f.value)

    # -- the caller's view of the two outputs -------------------------------------
    def _buffer(self, out, F: int, device=None):
        """(the array the library writes, row pitch in elements).  best: (F, 2) float32, a cell per row; surface:
        (H, F) float32, or the caller's 2-D ``out`` with at least F columns, whose row stride is the pitch."""
        H = self.num_hypotheses
        if self.output == "best":
            return self._output(out, (F, 2), False, device), 0
        if out is None:
            return self._output(None, (H, F), False, device), F
        torch_out = device is not None
        ok = (is_torch(out) and out.is_cuda and out.device == device) if torch_out else isinstance(out, np.ndarray)
        if ok:
            ok = str(out.dtype).endswith("float32") and out.ndim == 2 and out.shape[0] == H and out.shape[1] >= F
        if ok:
            pitch, inner = (out.stride(0), out.stride(1)) if torch_out else (out.strides[0] // 4, out.strides[1] // 4)
            ok = (inner == 1 or out.shape[1] <= 1) and (pitch >= F or H == 1)
        if not ok:
            raise ValueError(f"out must be a float32 ({H}, >= {F}) array with contiguous rows, on the input's device")
        return out, max(int(pitch), F)

    def _result(self, buf, F: int):
        if self.output == "surface":
            return buf[:, :F]
        cells = buf[:F]
        if is_torch(cells):
            import torch
            return cells[:, 0], cells[:, 1].view(torch.int32)
        return cells[:, 0], cells[:, 1].view(np.int32)

    def process(self, iq, out=None, sync: bool = True):
        """Process one buffer; returns what its samples complete: ``(power, hypothesis)``, float32 and int32 views of
        the cells, or the float32 ``(H, outputs)`` surface."""
        f = C.c_uint64()
        if is_torch(iq) and iq.is_cuda:
            n = self._device_samples(iq)
            F = self.outputs_for(n)
            buf, pitch = self._buffer(out, F, iq.device)
            if sync:
                L.check(self._lib.pfb_mfbank_process(self._h, C.c_void_p(iq.data_ptr()), n, C.c_void_p(buf.data_ptr()), F,
                                                     pitch, C.byref(f), L.PFB_MEM_DEVICE), "pfb_mfbank_process")
            else:
                L.check(self._lib.pfb_mfbank_process_async(self._h, C.c_void_p(iq.data_ptr()), n,
                                                           C.c_void_p(buf.data_ptr()), F, pitch, C.byref(f)),
                        "pfb_mfbank_process_async")
            return self._result(buf, F)
        a, n = self._host_samples(iq)
        F = self.outputs_for(n)
        buf, pitch = self._buffer(out, F)
        L.check(self._lib.pfb_mfbank_process(self._h, C.c_void_p(a.ctypes.data), n, C.c_void_p(buf.ctypes.data), F, pitch,
                                             C.byref(f), L.PFB_MEM_HOST), "pfb_mfbank_process")
        return self._result(buf, F)

    __call__ = process

    def process_iq_file(self, path: str, reset: bool = True):
        """One .iq record from disk (header checked by the library, payload streamed in chunks).
        Returns (what ``process`` returns, PfbIqInfo)."""
        from . import iqfile
        with open(path, "rb") as fh:
            info = iqfile.parse_header(fh.read(128))
        if reset:
            self.reset()
        F = self.outputs_for(int(info.packet.numSamples))
        buf, pitch = self._buffer(None, F)
        f = C.c_uint64()
        got = L.PfbIqInfo()
        L.check(self._lib.pfb_mfbank_process_iq_file(self._h, str(path).encode(), C.c_void_p(buf.ctypes.data), F, pitch,
                                                     C.byref(f), C.byref(got)), "pfb_mfbank_process_iq_file")
        return self._result(buf, int(f.value)), got


def compress_bank(iq, replica, *, first_bin: int, num_hypotheses: int, bin_step: int = 1,
                  sample_format: str | None = None, bit_width: int = 12, output: str = "best", normalize: bool = False,
                  fft_length: int = 0, device: int = -1):
    """``MatchedFilterBank(replica, ...).process(iq)`` in one call; the sample format follows iq's dtype."""
    with MatchedFilterBank(replica, sample_format or _format_of(iq), bit_width, first_bin=first_bin,
                           num_hypotheses=num_hypotheses, bin_step=bin_step, output=output, normalize=normalize,
                           fft_length=fft_length, device=device) as bank:
        return bank.process(iq)


def pulse_delay_and_offset_from_iq_files(tx_path: str, rx_path: str, max_offset_hz: float, device: int = -1) -> dict:
    """``pulse_delay_from_iq_files`` for a TX / RX pair whose oscillators differ by up to ``max_offset_hz``: the burst is
    the replica, the dwell goes through a bank of the 4096-point bins within +-max_offset_hz (best output; the peak over
    time and hypothesis is found on the device).  Returns that function's lag_samples, lag_seconds, peak_power and
    start_time_offset, plus hypothesis (the h of the peak) and offset_hz (its f_h: RX carrier minus TX carrier, to half
    a bin of rx.fs / 4096)."""
    import torch

    from . import iqfile
    nfft = 4096
    tx, rx = iqfile.read_iq(tx_path), iqfile.read_iq(rx_path)
    K = tx.iq.shape[0]
    if K > nfft // 2:
        raise ValueError(f"{tx_path}: the TX record has {K} samples, a bank replica takes at most {nfft // 2}")
    if K < 1 or rx.iq.shape[0] < K:
        raise ValueError(f"the RX record ({rx.iq.shape[0]} samples) is shorter than the TX record ({K})")
    bins = int(np.ceil(abs(float(max_offset_hz)) * nfft / rx.fs))
    if 2 * bins + 1 > nfft:
        raise ValueError(f"max_offset_hz = {max_offset_hz} is beyond the sample rate's +-{rx.fs / 2} Hz")
    full = np.float32(1 << (tx.bitWidth - 1))
    r = (tx.iq[:, 0].astype(np.float32) / full + 1j * (tx.iq[:, 1].astype(np.float32) / full)).astype(np.complex64)
    fmt = "int8" if rx.iq.dtype == np.int8 else "int16"
    with MatchedFilterBank(r, fmt, rx.bitWidth, first_bin=-bins, num_hypotheses=2 * bins + 1, fft_length=nfft,
                           device=device) as bank:
        d_rx = torch.from_numpy(np.array(rx.iq)).to(torch.device("cuda", bank.device_index))  # a writable copy for torch
        p, hyp = bank.process(d_rx)
        peak, lag = torch.max(p, dim=0)
        h = int(hyp[lag].item())
        lag, peak = int(lag.item()), float(peak.item())
        offset = float(bank.frequencies(rx.fs)[h])
    return {"lag_samples": lag, "lag_seconds": lag / rx.fs, "peak_power": peak,
            "start_time_offset": rx.sampleStartTime - tx.sampleStartTime, "offset_hz": offset, "hypothesis": h}
