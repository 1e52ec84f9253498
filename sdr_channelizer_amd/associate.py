"""PDW association over the C ABI (pfb_assoc_* in include/pfb_channelizer.h, where every figure is defined): which rows
of a channelized PDW table are one pulse.

``PulseAssociator`` takes ``ASSOC_ITEM_DTYPE`` items (start, length, cell, weight) in non-decreasing order of start,
links the items that touch in time and lie within ``cell_reach`` cells of each other, and returns one ``GROUP_DTYPE``
record per connected set and one int32 group number per item.  ``associate_pdws`` and ``fuse_pdws`` take a PDW table
in any order; only ``fuse_pdws`` computes on the CPU, on the records.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib as L
from ._handle import Handle, is_torch
from .pdw import PDW_DTYPE

ASSOC_ITEM_DTYPE = np.dtype([("start", "u8"), ("length", "u4"), ("cell", "i4"), ("weight", "f4"), ("reserved", "u4")])
GROUP_DTYPE = np.dtype([("first_tick", "u8"), ("end_tick", "u8"), ("length_sum", "u8"), ("members", "u4"),
                        ("first_item", "u4"), ("best_item", "u4"), ("best_cell", "i4"), ("cell_lo", "i4"),
                        ("cell_hi", "i4")])
STATS_FIELDS = ("groups", "edges", "clipped", "largest_group", "linked_items", "rounds")
MAX_ITEMS = 1 << 20


def _config(cell_reach, slack_ticks, window_items, device=-1) -> L.PfbAssocConfig:
    vals = (cell_reach, slack_ticks, window_items)
    if any(not 0 <= int(v) <= 0xffffffff for v in vals):
        raise ValueError("the associator's settings are unsigned 32-bit numbers")
    return L.PfbAssocConfig(C.sizeof(L.PfbAssocConfig), *(int(v) for v in vals), 0, int(device))


def describe_associator(cell_reach: int = 1, slack_ticks: int = 0, window_items: int = 64, *,
                        num_items: int = 0) -> L.PfbAssocPlan:
    """The plan the library makes for these settings and a list of num_items (pfb_assoc_describe; host only)."""
    cfg = _config(cell_reach, slack_ticks, window_items)
    plan = L.PfbAssocPlan()
    L.check(L.load().pfb_assoc_describe(C.byref(cfg), int(num_items), C.byref(plan)), "pfb_assoc_describe")
    return plan


def items_from_pdws(pdws, tick_rate: float, t0: float = 0.0) -> tuple[np.ndarray, np.ndarray]:
    """(items, order): start = round((toa - t0) * tick_rate), length = round(pw * tick_rate), cell = bin, weight = mag,
    sorted by start ascending and stably; items[i] comes from pdws[order[i]] (pfb_assoc_items_from_pdws; host only)."""
    p = np.ascontiguousarray(np.asarray(pdws), PDW_DTYPE).reshape(-1)
    items, order = np.zeros(p.size, ASSOC_ITEM_DTYPE), np.zeros(p.size, np.uint32)
    L.check(L.load().pfb_assoc_items_from_pdws(C.c_void_p(p.ctypes.data), p.size, float(t0), float(tick_rate),
                                               C.c_void_p(items.ctypes.data), C.c_void_p(order.ctypes.data)),
            "pfb_assoc_items_from_pdws")
    return items, order


class PulseAssociator(Handle):
    """Associator of items within ``cell_reach`` cells and ``slack_ticks`` ticks of each other, looked for among the
    ``window_items`` items behind each.  ``run`` takes a CUDA tensor of the items' bytes (uint8, n x 24) where it lies
    and returns CUDA tensors, or a numpy ``ASSOC_ITEM_DTYPE`` array and returns numpy."""

    _kind, _destroy, _get_device = "associator", "pfb_assoc_destroy", "pfb_assoc_get_device"

    def __init__(self, cell_reach: int = 1, slack_ticks: int = 0, window_items: int = 64, *, device: int = -1):
        self._h = C.c_void_p()
        lib = L.load()
        cfg = _config(cell_reach, slack_ticks, window_items, device)
        L.check(lib.pfb_assoc_create(C.byref(cfg), C.byref(self._h)), "pfb_assoc_create")
        self._created(lib)
        self.plan = L.PfbAssocPlan()
        L.check(lib.pfb_assoc_describe(C.byref(cfg), 0, C.byref(self.plan)), "pfb_assoc_describe")

    def set_stream(self, hip_stream: int) -> None:
        L.check(self._lib.pfb_assoc_set_stream(self._h, C.c_void_p(hip_stream)), "pfb_assoc_set_stream")

    def sync(self) -> None:
        L.check(self._lib.pfb_assoc_sync(self._h), "pfb_assoc_sync")

    @property
    def last_kernel(self) -> str:
        """The kernels the last call launched, joined with '+'."""
        return self._lib.pfb_assoc_last_kernel(self._h).decode()

    @property
    def stats(self) -> dict:
        """groups, edges, clipped, largest_group, linked_items and rounds of the last run."""
        st = L.PfbAssocStats()
        L.check(self._lib.pfb_assoc_get_stats(self._h, C.byref(st)), "pfb_assoc_get_stats")
        return {k: int(getattr(st, k)) for k in STATS_FIELDS}

    def _items(self, items):
        """(pointer, count, mem, what keeps the pointer alive, the torch device or None)"""
        if is_torch(items) and items.is_cuda:
            import torch
            if items.dtype != torch.uint8 or items.numel() % ASSOC_ITEM_DTYPE.itemsize:
                raise TypeError(f"expected the items' bytes (torch.uint8, n x 24) for this {self._kind}, got "
                                f"{items.dtype} of {items.numel()} elements")
            if items.device.index != self.device_index:
                raise ValueError(f"items are on cuda:{items.device.index}, the {self._kind} on cuda:{self.device_index}")
            if not items.is_contiguous():
                raise ValueError("device items must be contiguous")
            return items.data_ptr(), items.numel() // ASSOC_ITEM_DTYPE.itemsize, L.PFB_MEM_DEVICE, items, items.device
        a = np.asarray(items.numpy() if is_torch(items) else items)
        if a.dtype != ASSOC_ITEM_DTYPE:
            raise TypeError(f"expected ASSOC_ITEM_DTYPE items for this {self._kind}, got {a.dtype}")
        a = np.ascontiguousarray(a).reshape(-1)
        return a.ctypes.data, a.size, L.PFB_MEM_HOST, a, None

    def run(self, items, capacity: int | None = None):
        """(records, labels) of the whole association (pfb_assoc_run).  For device items both are CUDA tensors: the
        records a uint8 tensor of count x 48 bytes (``groups_to_numpy`` reads it), the labels int32."""
        ptr, n, mem, _keep, dev = self._items(items)
        cap = n if capacity is None else int(capacity)
        count = C.c_uint64()
        if dev is None:
            rec, labels = np.zeros(cap, GROUP_DTYPE), np.full(n, -1, np.int32)
            rp, lp = rec.ctypes.data, labels.ctypes.data
        else:
            import torch
            rec = torch.zeros((cap, GROUP_DTYPE.itemsize), dtype=torch.uint8, device=dev)
            labels = torch.full((n,), -1, dtype=torch.int32, device=dev)
            rp, lp = rec.data_ptr(), labels.data_ptr()
        L.check(self._lib.pfb_assoc_run(self._h, C.c_void_p(ptr), n, mem, C.c_void_p(rp), cap, C.byref(count),
                                        C.c_void_p(lp)), "pfb_assoc_run")
        return rec[:int(count.value)], labels

    __call__ = run

    def links(self, items):
        """The edge search alone: (first_link, link_count), int32 numpy arrays (pfb_assoc_links); first_link is -1
        where an item has no link behind it."""
        ptr, n, mem, _keep, dev = self._items(items)
        if mem == L.PFB_MEM_DEVICE:
            import torch
            d = torch.zeros((2, n), dtype=torch.int32, device=dev)
            L.check(self._lib.pfb_assoc_links(self._h, C.c_void_p(ptr), n, mem, C.c_void_p(d[0].data_ptr()),
                                              C.c_void_p(d[1].data_ptr())), "pfb_assoc_links")
            out = d.cpu().numpy()
            return out[0], out[1]
        out = np.zeros((2, n), np.int32)
        L.check(self._lib.pfb_assoc_links(self._h, C.c_void_p(ptr), n, mem, C.c_void_p(out[0].ctypes.data),
                                          C.c_void_p(out[1].ctypes.data)), "pfb_assoc_links")
        return out[0], out[1]


def groups_to_numpy(records) -> np.ndarray:
    """GROUP_DTYPE records from what ``PulseAssociator.run`` returned (a numpy array, or the CUDA byte tensor)."""
    if is_torch(records):
        return records.cpu().numpy().reshape(-1).view(GROUP_DTYPE).copy()
    return np.asarray(records)


def associate(items, cell_reach: int = 1, slack_ticks: int = 0, window_items: int = 64):
    """One ``PulseAssociator.run`` over ``items``: (records as numpy GROUP_DTYPE, labels where the items lie)."""
    dev = items.device.index if is_torch(items) and items.is_cuda else -1
    with PulseAssociator(cell_reach, slack_ticks, window_items, device=dev) as a:
        rec, labels = a.run(items)
    return groups_to_numpy(rec), labels


def _associate_table(p, tick_rate, cell_reach, slack_ticks, window_items, t0):
    if t0 is None:
        t0 = float(p["toa"].min()) if p.size else 0.0
    items, order = items_from_pdws(p, tick_rate, t0)
    rec, sorted_labels = associate(items, cell_reach, slack_ticks, window_items)
    labels = np.full(p.size, -1, np.int32)
    labels[order] = sorted_labels
    return rec, labels, order


def associate_pdws(pdws, tick_rate: float, cell_reach: int = 1, slack_ticks: int = 0, window_items: int = 64,
                   t0: float | None = None):
    """Associate a PDW table (any order): start = round((toa - t0) * tick_rate), t0 the earliest toa unless given,
    length = round(pw * tick_rate), cell = bin, weight = mag.  Returns (groups, labels), the labels in the caller's
    order; the records' first_item and best_item index the table sorted by start (``items_from_pdws``)."""
    rec, labels, _ = _associate_table(np.asarray(pdws), tick_rate, cell_reach, slack_ticks, window_items, t0)
    return rec, labels


def fuse_pdws(pdws, tick_rate: float, cell_reach: int = 1, slack_ticks: int = 0, window_items: int = 64,
              t0: float | None = None) -> np.ndarray:
    """One PDW per group, in the groups' order (host only, from the records): ``toa`` is the root member's own, ``pw``
    = (end_tick - first_tick) / tick_rate, ``freq``, ``snr``, ``mag`` and ``bin`` are the best member's, ``sat`` is
    the OR of the members'."""
    p = np.asarray(pdws)
    rec, labels, order = _associate_table(p, tick_rate, cell_reach, slack_ticks, window_items, t0)
    out = np.zeros(rec.size, PDW_DTYPE)
    if rec.size == 0:
        return out
    root, best = p[order[rec["first_item"]]], p[order[rec["best_item"]]]
    out["toa"] = root["toa"]
    out["pw"] = (rec["end_tick"] - rec["first_tick"]).astype(np.float64) / float(tick_rate)
    for name in ("freq", "snr", "mag", "bin"):
        out[name] = best[name]
    sat = np.zeros(rec.size, np.int32)
    np.maximum.at(sat, labels, (p["sat"] != 0).astype(np.int32))
    out["sat"] = sat
    return out
