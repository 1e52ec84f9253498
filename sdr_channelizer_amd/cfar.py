"""A CFAR detector over the C ABI (pfb_cfar_* in include/pfb_channelizer.h, where the arithmetic is defined): pulse
lists from the compressed stream the matched filter and its bank leave on the device.

``Cfar`` takes float32 powers (``element="power"``, what ``MatchedFilter(output="power")`` returns) or the bank's
(power, hypothesis) cells (``element="cell"``), cut into calls of any length, and returns one record per pulse: the run
of cells over ``alpha`` times the local noise, its peak, the noise there and the hypothesis of the peak.  ``detect`` is
the one-shot form, ``detect_pulses`` runs matched filter and detector chunk by chunk on the device,
``detections_to_pdws`` turns records into what ``fit_event`` takes.  Nothing here computes on the CPU.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import NamedTuple

import numpy as np

from . import _lib as L
from ._handle import Handle, is_torch
from .pdw import PDW_DTYPE

DET_DTYPE = np.dtype([("first_index", "u8"), ("last_index", "u8"), ("peak_index", "u8"), ("peak_power", "f4"),
                      ("noise", "f4"), ("hypothesis", "i4"), ("cells_over", "u4"), ("flags", "u4"), ("reserved", "u4")])
_ELEMENT = {"power": L.PFB_CFAR_POWER, "cell": L.PFB_CFAR_BANK_CELL}
_METHOD = {"ca": L.PFB_CFAR_CA, "go": L.PFB_CFAR_GO, "so": L.PFB_CFAR_SO}
_WORDS = DET_DTYPE.itemsize // 8  # a record as int64 words: how a tensor holds it


class PulseDetections(NamedTuple):
    """What ``detect_pulses`` returns, with or without the bank: the records, and the grid their ``hypothesis`` counts
    on -- hypothesis h is the bin first_bin + h, bin_hz wide.  Without the bank hypothesis is -1 and bin_hz is 0."""
    records: np.ndarray
    first_bin: int
    bin_hz: float

    def to_pdws(self, fs: float, fc: float, start: float) -> np.ndarray:
        return detections_to_pdws(self.records, fs, fc, start, bin_hz=self.bin_hz, first_bin=self.first_bin)


def cfar_alpha(pfa: float, training_cells: int) -> float:
    """N (pfa^(-1/N) - 1): the factor of CA-CFAR over N training cells of square-law noise (pfb_cfar_alpha; host only).
    GO and SO have other factors."""
    a = C.c_double()
    L.check(L.load().pfb_cfar_alpha(float(pfa), int(training_cells), C.byref(a)), "pfb_cfar_alpha")
    return float(a.value)


def _config(block_cells, guard_blocks, train_blocks, alpha, method, element, merge_gap, min_power, device) -> L.PfbCfarConfig:
    return L.PfbCfarConfig(C.sizeof(L.PfbCfarConfig), _ELEMENT[element], _METHOD[method], int(block_cells),
                           int(guard_blocks), int(train_blocks), int(merge_gap), float(alpha), float(min_power), 0,
                           int(device))


def describe_cfar(block_cells: int, guard_blocks: int, train_blocks: int, alpha: float = 1.0, method: str = "ca",
                  element: str = "power", merge_gap: int = 0, min_power: float = 0.0) -> L.PfbCfarPlan:
    """The plan the library makes for these settings (pfb_cfar_describe; host only, needs no device)."""
    cfg = _config(block_cells, guard_blocks, train_blocks, alpha, method, element, merge_gap, min_power, -1)
    plan = L.PfbCfarPlan()
    L.check(L.load().pfb_cfar_describe(C.byref(cfg), C.byref(plan)), "pfb_cfar_describe")
    return plan


def records(t) -> np.ndarray:
    """The records a ``Cfar`` returned as a tensor, as a structured numpy array."""
    if is_torch(t):
        t = t.cpu().numpy()
    return np.ascontiguousarray(t).view(DET_DTYPE).reshape(-1)


class Cfar(Handle):
    """Stateful CFAR detector of a stream of cells: blocks of ``block_cells`` cells, ``guard_blocks`` guard and
    ``train_blocks`` training blocks on each side, the factor given as ``alpha`` or derived from ``pfa`` (the CA
    factor for 2 * train_blocks * block_cells training cells).  Each call returns the detections that close in it;
    ``flush`` ends the stream.  numpy in -> structured numpy array out (DET_DTYPE); CUDA tensor in -> an (n, 6) int64
    tensor of the same records (``records`` views it)."""

    _kind, _destroy, _get_device = "CFAR detector", "pfb_cfar_destroy", "pfb_cfar_get_device"

    def __init__(self, block_cells: int, guard_blocks: int, train_blocks: int, alpha: float | None = None, *,
                 pfa: float | None = None, method: str = "ca", element: str = "power", merge_gap: int = 0,
                 min_power: float = 0.0, device: int = -1):
        if (alpha is None) == (pfa is None):
            raise ValueError("give one of alpha and pfa")
        if alpha is None:
            alpha = cfar_alpha(pfa, 2 * int(train_blocks) * int(block_cells))
        self._h = C.c_void_p()
        lib = L.load()
        self.element = element
        self.alpha = float(np.float32(alpha))
        self._cfg = _config(block_cells, guard_blocks, train_blocks, alpha, method, element, merge_gap, min_power, device)
        L.check(lib.pfb_cfar_create(C.byref(self._cfg), C.byref(self._h)), "pfb_cfar_create")
        self._created(lib)
        self.plan = L.PfbCfarPlan()
        L.check(lib.pfb_cfar_describe(C.byref(self._cfg), C.byref(self.plan)), "pfb_cfar_describe")
        self._capacity = 1024

    def reset(self) -> None:
        L.check(self._lib.pfb_cfar_reset(self._h), "pfb_cfar_reset")

    def set_stream(self, hip_stream: int) -> None:
        L.check(self._lib.pfb_cfar_set_stream(self._h, C.c_void_p(hip_stream)), "pfb_cfar_set_stream")

    def sync(self) -> None:
        L.check(self._lib.pfb_cfar_sync(self._h), "pfb_cfar_sync")

    @property
    def last_kernel(self) -> str:
        return self._lib.pfb_cfar_last_kernel(self._h).decode()

    @property
    def next_index(self) -> int:
        """Global index of the next cell to be taken."""
        m = C.c_uint64()
        L.check(self._lib.pfb_cfar_next_index(self._h, C.byref(m)), "pfb_cfar_next_index")
        return int(m.value)

    @property
    def stats(self) -> dict:
        s = L.PfbCfarStats()
        L.check(self._lib.pfb_cfar_get_stats(self._h, C.byref(s)), "pfb_cfar_get_stats")
        return {name: int(getattr(s, name)) for name, _ in L.PfbCfarStats._fields_}

    # -- cells ---------------------------------------------------------------------
    def _host_cells(self, x) -> tuple[np.ndarray, int]:
        a = np.asarray(x)
        if a.dtype == np.dtype([("power", "f4"), ("hypothesis", "i4")]):
            a = a.view(np.float32)
        if a.dtype != np.float32:
            raise TypeError(f"expected float32 cells for this {self._kind}, got {a.dtype}")
        a = np.ascontiguousarray(a).reshape(-1)
        per = 2 if self.element == "cell" else 1
        if a.size % per:
            raise ValueError("bank cells are (power, hypothesis) pairs")
        return a, a.size // per

    def _device_cells(self, x) -> int:
        import torch
        if x.dtype != torch.float32:
            raise TypeError(f"expected torch.float32 cells for this {self._kind}, got {x.dtype}")
        if x.device.index != self.device_index:
            raise ValueError(f"cells are on cuda:{x.device.index}, the {self._kind} on cuda:{self.device_index}")
        if not x.is_contiguous():
            raise ValueError("device cells must be contiguous")
        per = 2 if self.element == "cell" else 1
        if x.numel() % per or (per == 2 and x.dim() >= 2 and x.shape[-1] != 2):
            raise ValueError("bank cells are (power, hypothesis) pairs: the last dimension must be 2")
        return x.numel() // per

    def _call(self, fn, device):
        """Run fn(pointer, capacity, count) with a record buffer, grown and run again on PFB_ERR_CAPACITY."""
        count = C.c_uint64()
        while True:
            cap = self._capacity
            if device is None:
                buf = np.zeros(cap, DET_DTYPE)
                ptr = buf.ctypes.data
            else:
                import torch
                buf = torch.zeros((cap, _WORDS), dtype=torch.int64, device=device)
                ptr = buf.data_ptr()
            rc = fn(C.c_void_p(ptr), cap, C.byref(count))
            if rc != L.PFB_ERR_CAPACITY:
                break
            self._capacity = max(int(count.value), 2 * cap)  # the state is as before the call
        return rc, buf[: int(count.value)]

    def process(self, x):
        """Take one buffer of cells; returns the detections that close in it."""
        if is_torch(x) and x.is_cuda:
            n = self._device_cells(x)
            rc, out = self._call(lambda p, cap, cnt: self._lib.pfb_cfar_process(
                self._h, C.c_void_p(x.data_ptr()), n, p, cap, cnt, L.PFB_MEM_DEVICE), x.device)
        else:
            a, n = self._host_cells(x)
            rc, out = self._call(lambda p, cap, cnt: self._lib.pfb_cfar_process(
                self._h, C.c_void_p(a.ctypes.data), n, p, cap, cnt, L.PFB_MEM_HOST), None)
        L.check(rc, "pfb_cfar_process")
        return out

    __call__ = process

    def process_async(self, x, out, count) -> None:
        """Queue one buffer of device cells on the handle's stream without a host sync (pfb_cfar_process_async): the
        records that close go to ``out``, an (capacity, 6) int64 CUDA tensor, their number to ``count``, an int64 CUDA
        tensor of one element.  What does not fit is dropped and counted in ``stats["dropped"]``."""
        import torch
        n = self._device_cells(x)
        for t, what in ((out, "out"), (count, "count")):
            if not (is_torch(t) and t.is_cuda and t.dtype == torch.int64 and t.is_contiguous()
                    and t.device.index == self.device_index):
                raise ValueError(f"{what} must be a contiguous int64 tensor on cuda:{self.device_index}")
        if out.numel() % _WORDS or count.numel() < 1:
            raise ValueError(f"out holds records of {_WORDS} int64 words, count one element")
        L.check(self._lib.pfb_cfar_process_async(self._h, C.c_void_p(x.data_ptr()), n, C.c_void_p(out.data_ptr()),
                                                 out.numel() // _WORDS, C.c_void_p(count.data_ptr())),
                "pfb_cfar_process_async")

    def flush(self, device=None):
        """End the stream: decide what is left, close the open run.  ``device``: a torch device for a tensor result."""
        if device is None:
            rc, out = self._call(lambda p, cap, cnt: self._lib.pfb_cfar_flush(self._h, p, cap, cnt, L.PFB_MEM_HOST), None)
        else:
            rc, out = self._call(lambda p, cap, cnt: self._lib.pfb_cfar_flush(self._h, p, cap, cnt, L.PFB_MEM_DEVICE), device)
        L.check(rc, "pfb_cfar_flush")
        return out


def detect(x, block_cells: int, guard_blocks: int, train_blocks: int, alpha: float | None = None, *,
           pfa: float | None = None, method: str = "ca", element: str = "power", merge_gap: int = 0,
           min_power: float = 0.0, device: int = -1) -> np.ndarray:
    """``Cfar(...).process(x)`` and ``flush()`` in one call: every detection of x as one stream, a structured array."""
    with Cfar(block_cells, guard_blocks, train_blocks, alpha, pfa=pfa, method=method, element=element,
              merge_gap=merge_gap, min_power=min_power, device=device) as det:
        return np.concatenate([records(det.process(x)), records(det.flush())])


def detect_pulses(iq, replica, *, block_cells: int = 64, guard_blocks: int | None = None, train_blocks: int = 8,
                  alpha: float | None = None, pfa: float | None = None, method: str = "ca", merge_gap: int | None = None,
                  min_power: float = 0.0, max_offset_hz: float | None = None, fs: float | None = None,
                  sample_format: str | None = None, bit_width: int = 12, normalize: bool = False,
                  chunk_samples: int = 1 << 22, device: int = -1):
    """The pulses of an I/Q stream that match ``replica`` (K samples): a ``MatchedFilter`` with power output -- or, with
    ``max_offset_hz`` and ``fs``, a ``MatchedFilterBank`` over the 4096-point bins within +-max_offset_hz -- feeds a
    ``Cfar`` chunk by chunk on the device; the compressed stream never leaves the GPU.  Defaults: guard_blocks =
    ceil(K / block_cells), merge_gap = K, pfa = 1e-7.  ``peak_index`` of a detection is the stream sample at which the
    pulse starts.  Returns a ``PulseDetections`` (records, first_bin, bin_hz) either way: with the bank, hypothesis h of a
    record is the bin first_bin + h, bin_hz = fs / 4096 each."""
    import torch

    from .matched_filter import MatchedFilter, _format_of, _replica
    from .mf_bank import MatchedFilterBank
    r = _replica(replica)
    K = r.size
    if alpha is None and pfa is None:
        pfa = 1e-7
    G = -(-K // block_cells) if guard_blocks is None else guard_blocks
    g = K if merge_gap is None else merge_gap
    fmt = sample_format or _format_of(iq)
    banked = max_offset_hz is not None
    if banked:
        if fs is None:
            raise ValueError("max_offset_hz needs fs")
        nfft = 4096
        bins = int(math.ceil(abs(float(max_offset_hz)) * nfft / float(fs)))
        if 2 * bins + 1 > nfft:
            raise ValueError(f"max_offset_hz = {max_offset_hz} is beyond the sample rate's +-{fs / 2} Hz")
        mf = MatchedFilterBank(r, fmt, bit_width, first_bin=-bins, num_hypotheses=2 * bins + 1, normalize=normalize,
                               fft_length=nfft, device=device)
    else:
        mf = MatchedFilter(r, fmt, bit_width, "power", normalize, device=device)
    found = []
    with mf, Cfar(block_cells, G, train_blocks, alpha, pfa=pfa, method=method, element="cell" if banked else "power",
                  merge_gap=g, min_power=min_power, device=mf.device_index) as det:
        dev = torch.device("cuda", mf.device_index)
        on_device = is_torch(iq) and iq.is_cuda
        x = iq if on_device else np.asarray(iq)
        if not on_device and np.iscomplexobj(x):
            x = np.ascontiguousarray(x, np.complex64).view(np.float32).reshape(-1, 2)
        x = x.reshape(-1, 2) if not (on_device and x.is_complex()) else x
        n = x.shape[0]
        for s in range(0, n, chunk_samples):
            part = x[s:s + chunk_samples]
            d = part if on_device else torch.from_numpy(np.array(part)).to(dev)
            if banked:
                F = mf.outputs_for(d.shape[0])
                cells = torch.empty((F, 2), dtype=torch.float32, device=dev)
                mf.process(d, out=cells)
            else:
                cells = mf.process(d)
            found.append(records(det.process(cells)))
        found.append(records(det.flush()))
    dets = np.concatenate(found) if found else np.zeros(0, DET_DTYPE)
    return PulseDetections(dets, -bins, float(fs) / nfft) if banked else PulseDetections(dets, 0, 0.0)


def pulse_detections_from_iq_file(path: str, replica, **kw):
    """``detect_pulses`` on one .iq record: format, bit width and fs from its header.  Returns (the
    ``PulseDetections``, the record as iqfile.read_iq gives it)."""
    from . import iqfile
    rec = iqfile.read_iq(path)
    fmt = "int8" if rec.iq.dtype == np.int8 else "int16"
    kw.setdefault("fs", rec.fs)
    return detect_pulses(rec.iq, replica, sample_format=fmt, bit_width=rec.bitWidth, **kw), rec


def detections_to_pdws(dets, fs: float, fc: float, start: float, *, bin_hz: float = 0.0, first_bin: int = 0,
                       bin_step: int = 1) -> np.ndarray:
    """Detections as pulse descriptor words (pfb_cfar_to_pdw; host only), what ``fit_event`` accepts: toa of the peak
    (1-based, as the extractors), pw of the run, snr = 10 log10(peak_power / noise), freq = fc + (first_bin +
    hypothesis) * bin_step * bin_hz for bank detections."""
    d = np.ascontiguousarray(dets, dtype=DET_DTYPE).reshape(-1)
    out = np.zeros(d.size, PDW_DTYPE)
    L.check(L.load().pfb_cfar_to_pdw(C.c_void_p(d.ctypes.data), d.size, float(fs), float(fc), float(start), float(bin_hz),
                                     int(first_bin), int(bin_step), out.ctypes.data_as(C.POINTER(L.PfbPdw))),
            "pfb_cfar_to_pdw")
    return out
