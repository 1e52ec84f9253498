"""Magnitude / phase traces and plot envelopes of I/Q streams on the GPU, over the C ABI (pfb_trace_* in
include/pfb_channelizer.h).

The first thing the reference does with a record is to look at it:

    iq = double(iq)/2^(bitWidth-1);  iq = iq(1,:) + 1j*iq(2,:);      plot_my_iq.m:105-108
    mag = abs(iq);  phase = rad2deg(angle(iq));                       plot_my_iq.m:110-111
    plot(t,mag,'.') ... plot(t,phase,'.')                             plot_my_iq.m:122,129

Nobody draws 2^30 dots.  ``Trace`` cuts the stream into bins of ``bin_samples`` samples -- one pixel column each -- and
gives every bin's power extent (min, max, mean) and where its peak sits; ``mag_phase`` gives the full-rate float32
traces of a stretch, for the zoomed view.  ``envelope`` and ``envelope_from_iq_file`` are the one-shots: they return the
per-column magnitudes in float64, taken on the host from the records (one square root per bin).  Drawing stays with the
caller; nothing here computes over samples on the CPU.
"""
from __future__ import annotations

import ctypes as C
from typing import NamedTuple

import numpy as np

from . import _lib as L
from ._handle import Handle, is_torch

_FMT = {"int8": L.PFB_FMT_INT8_IQ, "int16": L.PFB_FMT_INT16_IQ, "cf32": L.PFB_FMT_CF32}
TILE = 4096  # samples per segment of the envelope kernels (kTile, csrc/pfb_trace.hip): longer bins are folded from partials

# pfb_trace_bin
BIN_DTYPE = np.dtype([("peak_sample", "<u8"), ("power_min", "<f8"), ("power_max", "<f8"), ("power_mean", "<f8"),
                      ("peak_i", "<f4"), ("peak_q", "<f4"), ("count", "<u4"), ("reserved", "<u4")])


class Envelope(NamedTuple):
    """What a plot of one column per bin needs, float64 from the records."""
    t: np.ndarray               # bin start / fs when fs is known, else the bin's first sample index
    mag_min: np.ndarray         # sqrt(power_min)
    mag_max: np.ndarray         # sqrt(power_max)
    rms: np.ndarray             # sqrt(power_mean)
    peak_sample: np.ndarray     # global index of the first sample holding mag_max
    peak_phase_deg: np.ndarray  # rad2deg(angle()) of that sample
    count: np.ndarray           # samples in the bin: bin_samples, fewer only in a final partial bin
    bin_samples: int
    info: L.PfbIqInfo | None = None


def choose_bin(num_samples: int, max_bins: int) -> int:
    """max(1, ceil(num_samples / max_bins)) (pfb_trace_choose_bin; host only)."""
    b = C.c_uint32()
    L.check(L.load().pfb_trace_choose_bin(int(num_samples), int(max_bins), C.byref(b)), "pfb_trace_choose_bin")
    return int(b.value)


def as_records(bins) -> np.ndarray:
    """A structured numpy array (BIN_DTYPE) of what ``Trace.envelope`` returned: a view for a numpy result, a copy to
    the host for the (bins, 48) uint8 tensor of a CUDA call."""
    if is_torch(bins):
        bins = bins.cpu().numpy()
    return bins if bins.dtype == BIN_DTYPE else np.ascontiguousarray(bins).view(BIN_DTYPE).reshape(-1)


def to_envelope(records: np.ndarray, bin_samples: int, first_sample: int = 0, fs: float | None = None,
                info: L.PfbIqInfo | None = None) -> Envelope:
    """The host's share: one sqrt and one atan2 per bin, in float64.  Bin k starts at first_sample + k bin_samples."""
    r = as_records(records)
    start = first_sample + np.arange(r.size, dtype=np.float64) * bin_samples
    return Envelope(start / fs if fs else start, np.sqrt(r["power_min"]), np.sqrt(r["power_max"]),
                    np.sqrt(r["power_mean"]), r["peak_sample"].copy(),
                    np.degrees(np.arctan2(r["peak_q"].astype(np.float64), r["peak_i"].astype(np.float64))),
                    r["count"].copy(), int(bin_samples), info)


class Trace(Handle):
    """Stateful envelope of an I/Q stream: bin k covers samples [k B, (k+1) B) of everything fed since creation,
    ``reset()`` or ``flush()``; each call returns the records of the bins it completes, and any cutting of the stream
    into calls gives the same records (cf32: but for the last bits of power_mean)."""

    _kind, _destroy, _get_device = "trace", "pfb_trace_destroy", "pfb_trace_get_device"

    def __init__(self, bin_samples: int, sample_format: str = "int16", bit_width: int = 12, device: int = -1):
        self._h = C.c_void_p()
        lib = L.load()
        self.bin_samples = int(bin_samples)
        self.fmt = _FMT[sample_format]
        self.bit_width = int(bit_width)
        if not 0 <= self.bin_samples < 2 ** 32:
            raise ValueError(f"bin_samples must be 1 .. 2^31, got {bin_samples}")
        cfg = L.PfbTraceConfig(C.sizeof(L.PfbTraceConfig), self.fmt, self.bit_width, self.bin_samples, 0, int(device))
        L.check(lib.pfb_trace_create(C.byref(cfg), C.byref(self._h)), "pfb_trace_create")
        self._created(lib)

    def reset(self) -> None:
        L.check(self._lib.pfb_trace_reset(self._h), "pfb_trace_reset")

    def set_stream(self, hip_stream: int) -> None:
        L.check(self._lib.pfb_trace_set_stream(self._h, C.c_void_p(hip_stream)), "pfb_trace_set_stream")

    def sync(self) -> None:
        L.check(self._lib.pfb_trace_sync(self._h), "pfb_trace_sync")

    def bins_for(self, num_samples: int) -> int:
        f = C.c_uint64()
        L.check(self._lib.pfb_trace_bins_for(self._h, int(num_samples), C.byref(f)), "pfb_trace_bins_for")
        return int(f.value)

    def envelope(self, iq, out=None, sync: bool = True):
        """The records of the bins this buffer completes.  numpy in -> a structured array (BIN_DTYPE); CUDA tensor in
        -> a (bins, 48) uint8 tensor on the same device (``as_records`` views it).  ``out``: the same kind, with room
        for ``bins_for(samples)`` records.  sync=False only enqueues on the handle's stream (CUDA input)."""
        f = C.c_uint64()
        if is_torch(iq) and iq.is_cuda:
            import torch
            n = self._device_samples(iq)
            F = self.bins_for(n)
            if out is None:
                out = torch.empty((F, BIN_DTYPE.itemsize), dtype=torch.uint8, device=iq.device)
            elif (not is_torch(out) or out.device != iq.device or out.dtype != torch.uint8 or not out.is_contiguous()
                  or out.numel() < F * BIN_DTYPE.itemsize):
                raise ValueError(f"out must be a contiguous uint8 tensor on {iq.device} with room for {F} records")
            if sync:
                L.check(self._lib.pfb_trace_envelope(self._h, C.c_void_p(iq.data_ptr()), n, C.c_void_p(out.data_ptr()),
                                                     F, C.byref(f), L.PFB_MEM_DEVICE), "pfb_trace_envelope")
            else:
                L.check(self._lib.pfb_trace_envelope_async(self._h, C.c_void_p(iq.data_ptr()), n,
                                                           C.c_void_p(out.data_ptr()), F, C.byref(f)),
                        "pfb_trace_envelope_async")
            return out.reshape(-1)[:F * BIN_DTYPE.itemsize].reshape(F, BIN_DTYPE.itemsize)
        a, n = self._host_samples(iq)
        F = self.bins_for(n)
        if out is None:
            out = np.zeros(F, dtype=BIN_DTYPE)
        elif (not isinstance(out, np.ndarray) or out.dtype != BIN_DTYPE or out.size < F or not out.flags.c_contiguous):
            raise ValueError(f"out must be a C-contiguous BIN_DTYPE numpy array with room for {F} records")
        L.check(self._lib.pfb_trace_envelope(self._h, C.c_void_p(a.ctypes.data), n, C.c_void_p(out.ctypes.data), F,
                                             C.byref(f), L.PFB_MEM_HOST), "pfb_trace_envelope")
        return out.reshape(-1)[:F]

    def flush(self) -> np.ndarray:
        """The open bin as a structured array of one record (count < bin_samples), or of none; the next sample starts
        a new bin."""
        rec, have = L.PfbTraceBin(), C.c_int32()
        L.check(self._lib.pfb_trace_flush(self._h, C.byref(rec), C.byref(have)), "pfb_trace_flush")
        return np.frombuffer(bytes(rec), dtype=BIN_DTYPE).copy()[:have.value]

    def mag_phase(self, iq, phase: bool = True):
        """(mag, phase_deg) of every sample, float32: abs(iq/2^(bit_width-1)) and rad2deg(angle(iq)); phase=False
        computes the magnitude alone and returns (mag, None).  numpy in -> numpy out, CUDA tensor in -> CUDA tensors.
        Stateless: the envelope's bins are not touched."""
        if is_torch(iq) and iq.is_cuda:
            import torch
            n = self._device_samples(iq)
            mag = torch.empty(n, dtype=torch.float32, device=iq.device)
            ph = torch.empty(n, dtype=torch.float32, device=iq.device) if phase else None
            L.check(self._lib.pfb_trace_samples(self._h, C.c_void_p(iq.data_ptr()), n, C.c_void_p(mag.data_ptr()),
                                                C.c_void_p(ph.data_ptr()) if phase else None, L.PFB_MEM_DEVICE),
                    "pfb_trace_samples")
            return mag, ph
        a, n = self._host_samples(iq)
        mag = np.empty(n, np.float32)
        ph = np.empty(n, np.float32) if phase else None
        L.check(self._lib.pfb_trace_samples(self._h, C.c_void_p(a.ctypes.data), n, C.c_void_p(mag.ctypes.data),
                                            C.c_void_p(ph.ctypes.data) if phase else None, L.PFB_MEM_HOST),
                "pfb_trace_samples")
        return mag, ph


def _format_of(x) -> str:
    if is_torch(x):
        import torch
        return {torch.int8: "int8", torch.int16: "int16"}.get(x.dtype, "cf32")
    return {np.dtype(np.int8): "int8", np.dtype(np.int16): "int16"}.get(np.asarray(x).dtype, "cf32")


def envelope(iq, bin_samples: int | None = None, max_bins: int | None = None, *, bit_width: int = 12,
             sample_format: str | None = None, fs: float | None = None, device: int = -1) -> Envelope:
    """One buffer as at most ``max_bins`` columns (or in bins of ``bin_samples``), the final partial bin included.
    ``iq``: the recorders' raw int8 / int16 I/Q, or complex / interleaved float32; numpy or a CUDA tensor."""
    if (bin_samples is None) == (max_bins is None):
        raise ValueError("give bin_samples or max_bins, not both")
    fmt = sample_format or _format_of(iq)
    n = iq.numel() if is_torch(iq) else np.asarray(iq).size
    n = n if (is_torch(iq) and iq.is_complex()) or (not is_torch(iq) and np.iscomplexobj(iq)) else n // 2
    B = int(bin_samples) if bin_samples is not None else choose_bin(n, max_bins)
    with Trace(B, fmt, bit_width, device) as tr:
        recs = np.concatenate([as_records(tr.envelope(iq)), tr.flush()])
    return to_envelope(recs, B, 0, fs)


def envelope_from_iq_file(path: str, max_bins: int = 4096, device: int = -1) -> Envelope:
    """plot_my_iq.m for one record, as columns: the library reads the header, takes format, bit width and length from
    it, chooses the bin and streams the payload; ``t`` is in seconds of the record's sample rate."""
    from . import iqfile
    with open(path, "rb") as fh:
        head = iqfile.parse_header(fh.read(128))
    B = choose_bin(int(head.packet.numSamples), max_bins)
    cap = -(-int(head.packet.numSamples) // B)
    recs = np.zeros(cap, dtype=BIN_DTYPE)
    f, b, info = C.c_uint64(), C.c_uint32(), L.PfbIqInfo()
    L.check(L.load().pfb_trace_envelope_from_iq_file(str(path).encode(), int(max_bins), C.c_void_p(recs.ctypes.data), cap,
                                                     C.byref(f), C.byref(b), C.byref(info), int(device)),
            "pfb_trace_envelope_from_iq_file")
    return to_envelope(recs[:f.value], int(b.value), 0, float(info.packet.sampleRateSps) or None, info)
