"""PDW deinterleaver over the C ABI (pfb_deint_* in include/pfb_channelizer.h, where every figure is defined): which
pulses of a time-ordered list belong together, and each train's repetition interval.

``Deinterleaver`` takes uint64 arrival ticks in non-decreasing order -- the ``peak_index`` of CFAR detections, PDW
``toa`` turned into ticks -- builds a difference histogram of them to propose periods, pulls the train of the best
candidate out by a sequence search and goes round again until nothing is left.  ``run`` returns one ``EMITTER_DTYPE``
record per train in extraction order and one int32 label per pulse, -1 for unassigned.  Only ``merge_emitters``
computes on the CPU, on the records.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib as L
from ._handle import Handle, is_torch

EMITTER_DTYPE = np.dtype([("first_tick", "u8"), ("last_tick", "u8"), ("period", "f8"), ("pulses", "u4"),
                          ("periods", "u4"), ("bin", "u4"), ("candidate_period", "u4"), ("first_pulse", "u4"),
                          ("hist_count", "u4")])
STATS_FIELDS = ("rounds", "candidates_tried", "candidates_refused", "pulses_assigned")
MAX_PULSES = 1 << 20


def _config(min_period, max_period, bin_ticks, max_level, detect_percent, min_pulses, max_missing, tolerance,
            fill_percent, max_emitters, device=-1) -> L.PfbDeintConfig:
    vals = (min_period, max_period, bin_ticks, max_level, detect_percent, min_pulses, max_missing, tolerance,
            fill_percent, max_emitters)
    if any(not 0 <= int(v) <= 0xffffffff for v in vals):
        raise ValueError("the deinterleaver's settings are unsigned 32-bit numbers")
    return L.PfbDeintConfig(C.sizeof(L.PfbDeintConfig), *(int(v) for v in vals), 0, int(device))


def describe_deinterleaver(min_period: int, max_period: int, bin_ticks: int = 1, *, num_pulses: int = 0,
                           max_level: int = 16, detect_percent: int = 30, min_pulses: int = 8, max_missing: int = 4,
                           tolerance: int = 0, fill_percent: int = 50, max_emitters: int = 64) -> L.PfbDeintPlan:
    """The plan the library makes for these settings and a list of num_pulses (pfb_deint_describe; host only)."""
    cfg = _config(min_period, max_period, bin_ticks, max_level, detect_percent, min_pulses, max_missing, tolerance,
                  fill_percent, max_emitters)
    plan = L.PfbDeintPlan()
    L.check(L.load().pfb_deint_describe(C.byref(cfg), int(num_pulses), C.byref(plan)), "pfb_deint_describe")
    return plan


def ticks_from_toa(toa, tick_rate: float, t0: float = 0.0) -> tuple[np.ndarray, np.ndarray]:
    """(ticks, order): tick = round((toa - t0) * tick_rate) to nearest even, sorted ascending and stably; ticks[i] is
    the tick of element order[i] (pfb_deint_ticks_from_toa; host only).  ``toa`` is a float64 array, or a structured
    array with a ``toa`` field (PDW_DTYPE), which is walked in place."""
    a = np.asarray(toa)
    if a.dtype.names and "toa" in a.dtype.names:
        a = np.ascontiguousarray(a).reshape(-1)
        ptr = a.ctypes.data + a.dtype.fields["toa"][1]
        stride, n = a.dtype.itemsize, a.size
        if a.dtype.fields["toa"][0] != np.float64:
            raise TypeError("the toa field must be float64")
    else:
        a = np.ascontiguousarray(a, np.float64).reshape(-1)
        ptr, stride, n = a.ctypes.data, 8, a.size
    ticks, order = np.zeros(n, np.uint64), np.zeros(n, np.uint32)
    L.check(L.load().pfb_deint_ticks_from_toa(C.c_void_p(ptr), stride, n, float(t0), float(tick_rate),
                                              C.c_void_p(ticks.ctypes.data), C.c_void_p(order.ctypes.data)),
            "pfb_deint_ticks_from_toa")
    return ticks, order


class Deinterleaver(Handle):
    """Deinterleaver of arrival ticks with periods from ``min_period`` to ``max_period`` ticks, ``bin_ticks`` to a
    histogram bin.  ``run`` takes a CUDA tensor (int64, every tick >= 0: torch has no uint64 arithmetic) where it lies
    and returns CUDA tensors, or a numpy array of non-negative integers and returns numpy."""

    _kind, _destroy, _get_device = "deinterleaver", "pfb_deint_destroy", "pfb_deint_get_device"

    def __init__(self, min_period: int, max_period: int, bin_ticks: int = 1, *, max_level: int = 16,
                 detect_percent: int = 30, min_pulses: int = 8, max_missing: int = 4, tolerance: int = 0,
                 fill_percent: int = 50, max_emitters: int = 64, device: int = -1):
        self._h = C.c_void_p()
        lib = L.load()
        cfg = _config(min_period, max_period, bin_ticks, max_level, detect_percent, min_pulses, max_missing, tolerance,
                      fill_percent, max_emitters, device)
        L.check(lib.pfb_deint_create(C.byref(cfg), C.byref(self._h)), "pfb_deint_create")
        self._created(lib)
        self.max_emitters = int(max_emitters)
        self.plan = L.PfbDeintPlan()
        L.check(lib.pfb_deint_describe(C.byref(cfg), 0, C.byref(self.plan)), "pfb_deint_describe")
        self.num_bins = int(self.plan.num_bins)

    def set_stream(self, hip_stream: int) -> None:
        L.check(self._lib.pfb_deint_set_stream(self._h, C.c_void_p(hip_stream)), "pfb_deint_set_stream")

    def sync(self) -> None:
        L.check(self._lib.pfb_deint_sync(self._h), "pfb_deint_sync")

    @property
    def last_kernel(self) -> str:
        """The kernels the last call launched, joined with '+'."""
        return self._lib.pfb_deint_last_kernel(self._h).decode()

    @property
    def stats(self) -> dict:
        """rounds, candidates_tried, candidates_refused and pulses_assigned of the last run."""
        st = L.PfbDeintStats()
        L.check(self._lib.pfb_deint_get_stats(self._h, C.byref(st)), "pfb_deint_get_stats")
        return {k: int(getattr(st, k)) for k in STATS_FIELDS}

    def _ticks(self, ticks):
        """(pointer, count, mem, what keeps the pointer alive, the torch device or None)"""
        if is_torch(ticks) and ticks.is_cuda:
            import torch
            if ticks.dtype != torch.int64:
                raise TypeError(f"expected torch.int64 ticks for this {self._kind}, got {ticks.dtype}")
            if ticks.device.index != self.device_index:
                raise ValueError(f"ticks are on cuda:{ticks.device.index}, the {self._kind} on cuda:{self.device_index}")
            if not ticks.is_contiguous():
                raise ValueError("device ticks must be contiguous")
            return ticks.data_ptr(), ticks.numel(), L.PFB_MEM_DEVICE, ticks, ticks.device
        a = np.asarray(ticks.numpy() if is_torch(ticks) else ticks)
        if a.dtype.kind not in "ui":
            raise TypeError(f"expected integer ticks for this {self._kind}, got {a.dtype}")
        if a.dtype.kind == "i" and a.size and a.min() < 0:
            raise ValueError("ticks are not negative")
        a = np.ascontiguousarray(a, np.uint64).reshape(-1)
        return a.ctypes.data, a.size, L.PFB_MEM_HOST, a, None

    def run(self, ticks, capacity: int | None = None):
        """(records, labels) of the whole search (pfb_deint_run).  For device ticks both are CUDA tensors: the records
        a uint8 tensor of count x 48 bytes (``records_to_numpy`` reads it), the labels int32."""
        ptr, n, mem, _keep, dev = self._ticks(ticks)
        cap = self.max_emitters if capacity is None else int(capacity)
        count = C.c_uint64()
        if dev is None:
            rec, labels = np.zeros(cap, EMITTER_DTYPE), np.full(n, -1, np.int32)
            rp, lp = rec.ctypes.data, labels.ctypes.data
        else:
            import torch
            rec = torch.zeros((cap, EMITTER_DTYPE.itemsize), dtype=torch.uint8, device=dev)
            labels = torch.full((n,), -1, dtype=torch.int32, device=dev)
            rp, lp = rec.data_ptr(), labels.data_ptr()
        L.check(self._lib.pfb_deint_run(self._h, C.c_void_p(ptr), n, mem, C.c_void_p(rp), cap, C.byref(count),
                                        C.c_void_p(lp)), "pfb_deint_run")
        return rec[:int(count.value)], labels

    __call__ = run

    def histogram(self, ticks) -> np.ndarray:
        """Step 1 alone on the whole list: num_bins uint32 counts (pfb_deint_histogram), numpy."""
        ptr, n, mem, _keep, _dev = self._ticks(ticks)
        out = np.zeros(self.num_bins, np.uint32)
        if mem == L.PFB_MEM_DEVICE:
            import torch
            d = torch.zeros(self.num_bins, dtype=torch.int32, device=_dev)
            L.check(self._lib.pfb_deint_histogram(self._h, C.c_void_p(ptr), n, mem, C.c_void_p(d.data_ptr()), d.numel()),
                    "pfb_deint_histogram")
            return d.cpu().numpy().view(np.uint32)
        L.check(self._lib.pfb_deint_histogram(self._h, C.c_void_p(ptr), n, mem, C.c_void_p(out.ctypes.data), out.size),
                "pfb_deint_histogram")
        return out

    def successors(self, ticks, period: int):
        """Steps 3 and 4 alone on the whole list at one period: (succ, step, len), int32 numpy arrays
        (pfb_deint_successors); succ is -1 and step 0 where there is no successor."""
        ptr, n, mem, _keep, dev = self._ticks(ticks)
        if mem == L.PFB_MEM_DEVICE:
            import torch
            d = torch.zeros((3, n), dtype=torch.int32, device=dev)
            p = [C.c_void_p(d[k].data_ptr()) for k in range(3)]
            L.check(self._lib.pfb_deint_successors(self._h, C.c_void_p(ptr), n, mem, int(period), *p),
                    "pfb_deint_successors")
            out = d.cpu().numpy()
            return out[0], out[1], out[2]
        out = np.zeros((3, n), np.int32)
        p = [C.c_void_p(out[k].ctypes.data) for k in range(3)]
        L.check(self._lib.pfb_deint_successors(self._h, C.c_void_p(ptr), n, mem, int(period), *p), "pfb_deint_successors")
        return out[0], out[1], out[2]


def records_to_numpy(records) -> np.ndarray:
    """EMITTER_DTYPE records from what ``Deinterleaver.run`` returned (a numpy array, or the CUDA byte tensor)."""
    if is_torch(records):
        return records.cpu().numpy().reshape(-1).view(EMITTER_DTYPE).copy()
    return np.asarray(records)


def deinterleave(ticks, min_period: int, max_period: int, bin_ticks: int = 1, **settings):
    """One ``Deinterleaver.run`` over ``ticks``: (records as numpy EMITTER_DTYPE, labels where the ticks lie)."""
    dev = ticks.device.index if is_torch(ticks) and ticks.is_cuda else -1
    with Deinterleaver(min_period, max_period, bin_ticks, device=dev, **settings) as d:
        rec, labels = d.run(ticks)
    return records_to_numpy(rec), labels


def deinterleave_pdws(pdws, tick_rate: float, min_period: int, max_period: int, bin_ticks: int = 1, *,
                      t0: float | None = None, **settings):
    """Deinterleave a PDW table (any order) by its ``toa``: ticks = round((toa - t0) * tick_rate), t0 the earliest toa
    unless given.  Returns (records, labels), the labels in the caller's order."""
    p = np.asarray(pdws)
    if t0 is None:
        t0 = float(p["toa"].min()) if p.size else 0.0
    ticks, order = ticks_from_toa(p, tick_rate, t0)
    rec, sorted_labels = deinterleave(ticks, min_period, max_period, bin_ticks, **settings)
    labels = np.full(p.size, -1, np.int32)
    labels[order] = sorted_labels
    return rec, labels


def deinterleave_detections(found, min_period: int, max_period: int, bin_ticks: int = 1, **settings):
    """Deinterleave CFAR detections -- what ``detect_pulses`` returned, or DET_DTYPE records -- by their ``peak_index``,
    in samples.  The detectors' records come in stream order, so the labels are in the caller's order."""
    ticks = np.ascontiguousarray(np.asarray(getattr(found, "records", found))["peak_index"], np.uint64)
    return deinterleave(ticks, min_period, max_period, bin_ticks, **settings)


def merge_emitters(records, labels, rel_tol: float = 1e-3, tolerance: float = 1.0):
    """Join what one run split (host only).  Two records are one train that a long gap broke when their ``period``
    agrees within ``rel_tol`` and the later one's first tick continues the earlier one's last: the gap is a whole
    number k >= 1 of mean periods to within ``tolerance`` * k ticks.  The later record is folded into the earlier one
    (ticks, pulses, periods + k, period recomputed) and its label replaced.

    Returns (merged records, new labels, remainder): ``remainder[i]`` is the index of an earlier merged record whose
    period this one's is an integer multiple (2 or more) of within ``rel_tol`` -- what is left of a train whose other
    pulses went elsewhere -- or -1."""
    rec = records_to_numpy(records).copy()
    lab = np.array(labels.cpu().numpy() if is_torch(labels) else labels, np.int32)
    target = list(range(rec.size))          # where each record ended up
    keep: list[int] = []
    for i in range(rec.size):
        for j in keep:
            a, b = rec[j], rec[i]
            if abs(a["period"] - b["period"]) > rel_tol * max(a["period"], b["period"]):
                continue
            first, second = (a, b) if a["last_tick"] < b["first_tick"] else (b, a)
            if first["last_tick"] >= second["first_tick"]:
                continue                     # they overlap in time: two emitters
            gap = float(second["first_tick"] - first["last_tick"])
            mean = 0.5 * (a["period"] + b["period"])
            k = int(round(gap / mean))
            if k < 1 or abs(gap - k * mean) > tolerance * k:
                continue
            m = rec[j].copy()
            m["first_tick"], m["last_tick"] = first["first_tick"], second["last_tick"]
            m["first_pulse"] = first["first_pulse"]
            m["pulses"] = a["pulses"] + b["pulses"]
            m["periods"] = a["periods"] + b["periods"] + k
            m["period"] = float(m["last_tick"] - m["first_tick"]) / float(m["periods"])
            rec[j] = m
            target[i] = j
            break
        else:
            keep.append(i)
    new_index = {old: new for new, old in enumerate(keep)}
    out = rec[keep]
    new_lab = lab.copy()
    for old in range(rec.size):
        new_lab[lab == old] = new_index[target[old]]
    remainder = np.full(out.size, -1, np.int32)
    for i in range(out.size):
        for j in range(i):
            ratio = out[i]["period"] / out[j]["period"]
            m = int(round(ratio))
            if m >= 2 and abs(ratio - m) <= rel_tol * m:
                remainder[i] = j
                break
    return out, new_lab, remainder
