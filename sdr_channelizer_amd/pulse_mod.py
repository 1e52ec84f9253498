"""Modulation on pulse over the C ABI (pfb_mop_* in include/pfb_channelizer.h, where every figure is defined): what is
inside each pulse of a list -- its mid frequency, its sweep and the phase flips of a code.

``PulseModulation`` takes a series (int8 / int16 I,Q rows, a complex64 stream, or a complex64 matrix whose columns
are measured where they lie) and a list of pulses, and returns one ``MOP_DTYPE`` record per pulse and the positions
of its first negative second-order terms.  ``modulation_figures`` turns records into Hz; ``phase_code`` and
``replica_from_measurement`` compute on the CPU, on the records: the chips of a binary code, and the replica the
matched filter and everything behind it want.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib as L
from ._handle import Handle, is_torch

PULSE_DTYPE = np.dtype([("start", "u8"), ("length", "u4"), ("column", "u4")])
MOP_DTYPE = np.dtype([("start", "u8"), ("length", "u4"), ("column", "u4"), ("n", "u4"), ("flags", "u4"),
                      ("neg_count", "u4"), ("first_neg", "u4"), ("last_neg", "u4"), ("peak_index", "u4"),
                      ("negs_listed", "u4"), ("reserved", "u4"), ("energy", "f8"), ("peak_power", "f8"),
                      ("s1_re", "f8"), ("s1_im", "f8"), ("s2_re", "f8"), ("s2_im", "f8")])
FIGURE_DTYPE = np.dtype([("freq_hz", "f8"), ("rate_hz_per_s", "f8"), ("extent_hz", "f8"), ("mean_power", "f8"),
                         ("flips", "f8"), ("kind", "u4"), ("reserved", "u4")])
KINDS = ("unmodulated", "lfm", "phase coded", "both", "not measurable")
NONE = 0xFFFFFFFF
_FMT = {"int8": L.PFB_FMT_INT8_IQ, "int16": L.PFB_FMT_INT16_IQ, "cf32": L.PFB_FMT_CF32}


def _config(sample_format, bit_width, trim, max_negatives, device=-1) -> L.PfbMopConfig:
    if any(not 0 <= int(v) <= 0xffffffff for v in (bit_width, trim, max_negatives)):
        raise ValueError("the settings are unsigned 32-bit numbers")
    fmt = _FMT[sample_format] if isinstance(sample_format, str) else int(sample_format)
    return L.PfbMopConfig(C.sizeof(L.PfbMopConfig), fmt, int(bit_width), int(trim), int(max_negatives), int(device))


def describe_modulation(sample_format="int16", bit_width: int = 12, trim: int = 0, max_negatives: int = 32) -> L.PfbMopPlan:
    """The plan of the library for these settings: tier thresholds, grid cap, scratch (pfb_mop_describe; host only)."""
    cfg = _config(sample_format, bit_width, trim, max_negatives)
    plan = L.PfbMopPlan()
    L.check(L.load().pfb_mop_describe(C.byref(cfg), C.byref(plan)), "pfb_mop_describe")
    return plan


def pack_pulses(starts, lengths, columns=None) -> np.ndarray:
    """The 16-byte pulse list (PULSE_DTYPE) of these starts (global indices), lengths and columns (0 when None)."""
    s = np.asarray(starts)
    if s.dtype.kind not in "ui" or np.asarray(lengths).dtype.kind not in "ui":
        raise TypeError("starts and lengths are integers")
    out = np.zeros(s.size, PULSE_DTYPE)
    if s.size and (s.min() < 0 or np.min(lengths) < 0 or np.max(lengths) > NONE):
        raise ValueError("a start is not negative, a length is an unsigned 32-bit number")
    out["start"], out["length"] = s.reshape(-1), np.asarray(lengths).reshape(-1)
    if columns is not None:
        out["column"] = np.asarray(columns).reshape(-1)
    return out


def _format_of(x) -> str:
    if is_torch(x):
        import torch
        return {torch.int8: "int8", torch.int16: "int16"}.get(x.dtype, "cf32")
    return {np.dtype(np.int8): "int8", np.dtype(np.int16): "int16"}.get(np.asarray(x).dtype, "cf32")


class PulseModulation(Handle):
    """Measures pulses of ``sample_format`` series: ``trim`` samples are left out at each end of a pulse, the first
    ``max_negatives`` (0 .. 128) negative second-order terms of each are listed."""

    _kind, _destroy, _get_device = "pulse modulation handle", "pfb_mop_destroy", "pfb_mop_get_device"

    def __init__(self, sample_format: str = "int16", bit_width: int = 12, trim: int = 0, max_negatives: int = 32,
                 device: int = -1):
        self._h = C.c_void_p()
        lib = L.load()
        cfg = _config(sample_format, bit_width, trim, max_negatives, device)
        L.check(lib.pfb_mop_create(C.byref(cfg), C.byref(self._h)), "pfb_mop_create")
        self._created(lib)
        self.fmt = int(cfg.sample_format)
        self.trim, self.max_negatives = int(trim), int(max_negatives)
        self.plan = L.PfbMopPlan()
        L.check(lib.pfb_mop_describe(C.byref(cfg), C.byref(self.plan)), "pfb_mop_describe")

    def set_stream(self, hip_stream: int) -> None:
        L.check(self._lib.pfb_mop_set_stream(self._h, C.c_void_p(hip_stream)), "pfb_mop_set_stream")

    def sync(self) -> None:
        L.check(self._lib.pfb_mop_sync(self._h), "pfb_mop_sync")

    @property
    def last_kernel(self) -> str:
        """The kernels the last call launched, joined with '+'."""
        return self._lib.pfb_mop_last_kernel(self._h).decode()

    def _series(self, x):
        """(pointer, rows, ld, mem, what keeps the pointer alive)"""
        if is_torch(x) and x.is_cuda:
            self._device_samples(x)
            if self.fmt == L.PFB_FMT_CF32:
                if x.is_complex():
                    rows, ld = (int(x.shape[0]), int(x.shape[1])) if x.dim() == 2 else (x.numel(), 1)
                else:
                    rows, ld = x.numel() // 2, 1
            else:
                rows, ld = x.numel() // 2, 1
            return x.data_ptr(), rows, ld, L.PFB_MEM_DEVICE, x
        a = np.asarray(x.numpy() if is_torch(x) else x)
        if self.fmt == L.PFB_FMT_CF32 and np.iscomplexobj(a) and a.ndim == 2:
            a = np.ascontiguousarray(a, np.complex64)
            return a.ctypes.data, a.shape[0], a.shape[1], L.PFB_MEM_HOST, a
        flat, rows = self._host_samples(a)
        return flat.ctypes.data, rows, 1, L.PFB_MEM_HOST, flat

    def _pulses(self, starts, lengths, columns):
        """(pointer, count, mem, keep, torch device or None)"""
        if is_torch(starts) and starts.is_cuda:
            import torch
            if lengths is not None or starts.dtype != torch.uint8 or starts.numel() % 16 or not starts.is_contiguous():
                raise TypeError("a device list is one contiguous uint8 tensor of 16-byte pulses (pack_pulses)")
            if starts.device.index != self.device_index:
                raise ValueError(f"the list is on cuda:{starts.device.index}, the {self._kind} on cuda:{self.device_index}")
            return starts.data_ptr(), starts.numel() // 16, L.PFB_MEM_DEVICE, starts, starts.device
        p = np.ascontiguousarray(starts) if lengths is None else pack_pulses(starts, lengths, columns)
        if p.dtype != PULSE_DTYPE:
            raise TypeError("a host list is a PULSE_DTYPE array, or starts and lengths")
        return p.ctypes.data, p.size, L.PFB_MEM_HOST, p, None

    def measure(self, x, starts, lengths=None, columns=None, base_index: int = 0):
        """(records, negs) of the pulses [starts, starts + lengths) of x, whose row 0 has the global index
        ``base_index`` (pfb_mop_measure).  x and the list are each taken where they lie.  A host list -- ``starts`` and
        ``lengths`` (and ``columns`` of a complex64 matrix), or one PULSE_DTYPE array -- gives numpy: MOP_DTYPE records
        and a (pulses, max_negatives) uint32 array.  A device list -- ``pack_pulses`` as a CUDA uint8 tensor -- gives
        CUDA tensors: (pulses, 96) uint8 (``records_to_numpy`` reads it) and (pulses, max_negatives) int32."""
        xp, rows, ld, mem, _kx = self._series(x)
        pp, count, pmem, _kp, dev = self._pulses(starts, lengths, columns)
        rec, negs, rp, qp = self._outputs(count, dev)
        L.check(self._lib.pfb_mop_measure(self._h, C.c_void_p(xp), rows, ld, int(base_index), mem, C.c_void_p(pp), count,
                                          pmem, C.c_void_p(rp), C.c_void_p(qp)), "pfb_mop_measure")
        return rec, negs

    __call__ = measure

    def _outputs(self, count, dev):
        if dev is None:
            rec = np.zeros(count, MOP_DTYPE)
            negs = np.full((count, self.max_negatives), NONE, np.uint32)
            return rec, negs, rec.ctypes.data, negs.ctypes.data if negs.size else None
        import torch
        # not filled: the library writes every record and every entry, and a fill on torch's stream could land late
        rec = torch.empty((count, MOP_DTYPE.itemsize), dtype=torch.uint8, device=dev)
        negs = torch.empty((count, self.max_negatives), dtype=torch.int32, device=dev)
        return rec, negs, rec.data_ptr(), negs.data_ptr() if negs.numel() else None

    def measure_async(self, x, pulses, base_index: int = 0, out=None):
        """Queue the measurement on the handle's stream without waiting for it (pfb_mop_measure_async): x and the
        packed list are CUDA tensors; returns the CUDA (records, negs), or fills ``out`` = (records, negs)."""
        xp, rows, ld, mem, _kx = self._series(x)
        pp, count, pmem, _kp, dev = self._pulses(pulses, None, None)
        if mem != L.PFB_MEM_DEVICE or pmem != L.PFB_MEM_DEVICE:
            raise TypeError("measure_async takes CUDA tensors")
        if out is None:
            rec, negs, rp, qp = self._outputs(count, dev)
        else:
            rec, negs = out
            rp, qp = rec.data_ptr(), negs.data_ptr() if negs is not None and negs.numel() else None
        L.check(self._lib.pfb_mop_measure_async(self._h, C.c_void_p(xp), rows, ld, int(base_index), C.c_void_p(pp), count,
                                                C.c_void_p(rp), C.c_void_p(qp)), "pfb_mop_measure_async")
        return rec, negs


def records_to_numpy(records) -> np.ndarray:
    """MOP_DTYPE records from what ``PulseModulation.measure`` returned (a numpy array, or the CUDA byte tensor)."""
    if is_torch(records):
        return records.cpu().numpy().reshape(-1).view(MOP_DTYPE).copy()
    return np.asarray(records)


def measure_pulses(x, starts, lengths=None, columns=None, *, base_index: int = 0, bit_width: int = 12, trim: int = 0,
                   max_negatives: int = 32):
    """One ``PulseModulation.measure`` over x; the sample format follows x's dtype."""
    dev = x.device.index if is_torch(x) and x.is_cuda else -1
    with PulseModulation(_format_of(x), bit_width, trim, max_negatives, dev) as m:
        return m.measure(x, starts, lengths, columns, base_index)


def pulses_from_pdws(pdws, series_rate: float, t0: float) -> np.ndarray:
    """PULSE_DTYPE pulses of a PDW table whose toa / pw are seconds of a series at ``series_rate`` rows a second that
    began at ``t0`` (pfb_mop_pulses_from_pdw; host only).  A toa is a double that holds the record's start time too: with
    an epoch start of 1.7e9 s it resolves 2.4e-7 s, 13 samples at 56 MHz -- trim accordingly, or take the pulses from
    sample indices (CFAR detections)."""
    from .pdw import PDW_DTYPE
    p = np.ascontiguousarray(pdws)
    if p.dtype != PDW_DTYPE:
        raise TypeError("expected PDW_DTYPE records")
    out = np.zeros(p.size, PULSE_DTYPE)
    L.check(L.load().pfb_mop_pulses_from_pdw(C.c_void_p(p.ctypes.data), p.size, float(series_rate), float(t0),
                                             C.c_void_p(out.ctypes.data)), "pfb_mop_pulses_from_pdw")
    return out


def measure_pdws(x, pdws, fs: float, sample_start_time: float, *, decimation: int = 1, bit_width: int = 12, trim: int = 0,
                 max_negatives: int = 32):
    """Measure the pulses a PDW extraction found in x: raw-stream PDWs (``extract_pdws_raw``) against the stream, or,
    with ``decimation`` = the channelizer's, channelized PDWs (``extract_pdws``) against the frame-major matrix, each
    in the column it was found in.  Returns (records, negs), numpy."""
    pulses = pulses_from_pdws(pdws, float(fs) / int(decimation), sample_start_time)
    return measure_pulses(x, pulses, bit_width=bit_width, trim=trim, max_negatives=max_negatives)


def modulation_figures(records, fs: float) -> np.ndarray:
    """FIGURE_DTYPE per record at sample rate ``fs`` (of the measured series): freq_hz, rate_hz_per_s, extent_hz,
    mean_power, flips and kind, an index into KINDS (pfb_mop_figures; host only)."""
    rec = np.ascontiguousarray(records_to_numpy(records))
    out = np.zeros(rec.size, FIGURE_DTYPE)
    L.check(L.load().pfb_mop_figures(C.c_void_p(rec.ctypes.data), rec.size, float(fs), C.c_void_p(out.ctypes.data)),
            "pfb_mop_figures")
    return out


def phase_code(negs, n: int) -> tuple[float, np.ndarray]:
    """(chip_samples, signs) of a binary phase code from the negatives of one pulse of ``n`` measured samples (host
    only).  A flip in front of sample b makes the two adjacent negatives b - 2 and b - 1: the chip boundaries are the
    pairs, single negatives are noise.  chip_samples is the largest spacing d = (smallest gap between boundaries) / k
    that every gap is a whole multiple of within one sample, refined over all the gaps; signs holds one +-1 per
    chip, fixed up to a global sign.  Without a boundary the pulse is one chip."""
    v = np.asarray(negs, np.int64).reshape(-1)
    v = np.sort(v[(v >= 0) & (v != NONE)])
    bounds, k = [], 0
    while k + 1 < v.size:
        if v[k + 1] == v[k] + 1:
            bounds.append(int(v[k]) + 2)
            k += 2
        else:
            k += 1
    if not bounds:
        return float(n), np.ones(1, np.int8)
    edges = np.array([0] + bounds + [int(n)], np.float64)
    gaps = np.diff(edges)
    inner = gaps[1:-1] if len(bounds) > 1 else gaps
    chip = float(inner.min())
    for k in range(1, 65):
        d = inner.min() / k
        if d < 2:
            break
        if np.all(np.abs(inner - np.round(inner / d) * d) <= 1.0):
            chip = float(inner.sum() / np.round(inner / d).sum())
            break
    counts = np.maximum(np.round(gaps / chip).astype(np.int64), 0)
    signs = np.concatenate([np.full(c, 1 if j % 2 == 0 else -1, np.int8) for j, c in enumerate(counts)])
    return chip, signs


def replica_from_measurement(records, negs, fs: float, bit_width: int = 12) -> np.ndarray:
    """A complex64 replica from measured pulses of one emitter, in ``replica_from_pulse_train``'s scaling (full scales,
    (I + jQ) / 2^(bit_width-1); ``bit_width`` = 0 for cf32 records): the median mid frequency, sweep, length and mean
    power of the measurable records, and the code ``phase_code`` recovers from the pulse with the median flip count
    (``negs`` None or empty, as with max_negatives = 0: no code).  Host only."""
    rec = records_to_numpy(records)
    fig = modulation_figures(rec, fs)
    ok = fig["kind"] != L.PFB_MOP_KIND_NOT_MEASURABLE
    if not ok.any():
        raise ValueError("no measurable pulse")
    rec, fig = rec[ok], fig[ok]
    q = None if negs is None else np.asarray(negs.cpu().numpy() if is_torch(negs) else negs)
    n = int(np.median(rec["n"]))
    f, extent = float(np.median(fig["freq_hz"])), float(np.median(fig["extent_hz"]))
    if abs(extent) < fs / n:
        extent = 0.0                                        # under one Rayleigh bin: no sweep
    amp = np.sqrt(float(np.median(fig["mean_power"]))) / (float(1 << (bit_width - 1)) if bit_width else 1.0)
    t = np.arange(n, dtype=np.float64) / fs
    rate = extent * fs / (n - 1) if n > 1 else 0.0
    phase = 2 * np.pi * ((f - extent / 2) * t + 0.5 * rate * t * t)
    flips = np.sort(rec["neg_count"])[len(rec) // 2]
    pick = int(np.flatnonzero(rec["neg_count"] == flips)[0])
    if q is None or q.size == 0:                            # no list was kept (max_negatives = 0): one chip, no code
        chip, signs = float(n), np.ones(1, np.int8)
    else:
        chip, signs = phase_code(q.reshape(len(ok), -1)[ok][pick], int(rec["n"][pick]))
    code = signs[np.minimum((np.arange(n) / chip).astype(np.int64), len(signs) - 1)]
    return (amp * code * np.exp(1j * phase)).astype(np.complex64)


def modulation_from_iq_file(path: str, *, snr_threshold_db: float = 18.0, trailing_threshold_db: float = 3.0, trim: int = 0,
                            max_negatives: int = 32, device: int = -1):
    """One .iq record, read once: the raw-stream PDW extraction (``extract_pdws_raw``) with fs, fc, bit width and start
    time from its header, then the measurement of every pulse it found by the host route, which uploads the pulses'
    windows only.  Returns (pdws, records, negs, figures, record), the last an ``iqfile.IqRecord``."""
    from . import iqfile
    from .pdw import extract_pdws_raw
    r = iqfile.read_iq(path)
    pdws = extract_pdws_raw(r.iq, r.fs, r.fc, r.sampleStartTime, bit_width=r.bitWidth, snr_threshold_db=snr_threshold_db,
                            trailing_threshold_db=trailing_threshold_db, device=device)
    pulses = pulses_from_pdws(pdws, r.fs, r.sampleStartTime)
    with PulseModulation(_format_of(r.iq), r.bitWidth, trim, max_negatives, device) as m:
        rec, negs = m.measure(r.iq, pulses)
    return pdws, rec, negs, modulation_figures(rec, r.fs), r
