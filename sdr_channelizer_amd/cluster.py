"""PDW clustering over the C ABI (pfb_cluster_* in include/pfb_channelizer.h, where every figure is defined): which
pulses of a list share a cell of frequency and pulse width, before anybody looks at their times.

``PulseClusterer`` takes ``CLUSTER_ITEM_DTYPE`` items (u, v: two integer features) in the caller's order, counts them
in a grid of ``cells_u`` x ``cells_v`` cells, joins the dense cells within ``reach_u`` and ``reach_v`` of each other and
returns one ``CLUSTER_GROUP_DTYPE`` record per cluster, one int32 cluster number per item (-1 for none) and the items'
indices partitioned by cluster in their own order.  ``deinterleave_clustered`` is the chain the unit is for: cluster a
PDW table, cut its tick list by cluster on the device and search every cluster for periods on its own.  Only the
bookkeeping of that chain computes on the CPU.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib as L
from ._handle import Handle, is_torch
from .deinterleave import EMITTER_DTYPE, Deinterleaver, records_to_numpy, ticks_from_toa
from .pdw import PDW_DTYPE

CLUSTER_ITEM_DTYPE = np.dtype([("u", "i4"), ("v", "i4")])
CLUSTER_GROUP_DTYPE = np.dtype([("root_u", "i4"), ("root_v", "i4"), ("pulses", "u4"), ("cells", "u4"), ("u_min", "i4"),
                                ("u_max", "i4"), ("v_min", "i4"), ("v_max", "i4"), ("sum_u", "i8"), ("sum_v", "i8"),
                                ("peak_u", "i4"), ("peak_v", "i4"), ("peak_count", "u4"), ("first_item", "u4")])
STATS_FIELDS = ("outside", "unassigned", "dense_cells", "border_cells", "components", "hook_rounds")
MAX_ITEMS = 1 << 20
MAX_CELLS = 1 << 20
MAX_CLUSTERS = 65535
BORDER = 1
# what deinterleave_clustered adds: per emitter its cluster, per cluster what its search cost
CLUSTERED_EMITTER_DTYPE = np.dtype(EMITTER_DTYPE.descr + [("cluster", "i4")])
SEARCHED_GROUP_DTYPE = np.dtype(CLUSTER_GROUP_DTYPE.descr + [("emitters", "u4"), ("rounds", "u4"), ("candidates_tried", "u4"),
                                                             ("candidates_refused", "u4"), ("pulses_assigned", "u4")])


def _config(cells_u, cells_v, reach_u, reach_v, min_cell_count, min_pulses, border, device=-1) -> L.PfbClusterConfig:
    vals = (cells_u, cells_v, reach_u, reach_v, min_cell_count, min_pulses)
    if any(not 0 <= int(v) <= 0xffffffff for v in vals):
        raise ValueError("the clusterer's settings are unsigned 32-bit numbers")
    return L.PfbClusterConfig(C.sizeof(L.PfbClusterConfig), *(int(v) for v in vals), BORDER if border else 0, int(device))


def describe_clusterer(cells_u: int, cells_v: int = 1, reach_u: int = 1, reach_v: int = 0, min_cell_count: int = 1,
                       min_pulses: int = 1, border: bool = False, *, num_items: int = 0) -> L.PfbClusterPlan:
    """The plan the library makes for these settings and a list of num_items (pfb_cluster_describe; host only)."""
    cfg = _config(cells_u, cells_v, reach_u, reach_v, min_cell_count, min_pulses, border)
    plan = L.PfbClusterPlan()
    L.check(L.load().pfb_cluster_describe(C.byref(cfg), int(num_items), C.byref(plan)), "pfb_cluster_describe")
    return plan


def items_from_pdws(pdws, freq_step_hz: float, pw_step_s: float = 0.0, freq0: float = 0.0) -> np.ndarray:
    """Items of a PDW table, in the table's order: u = floor((freq - freq0) / freq_step_hz), v = floor(pw / pw_step_s),
    or 0 with pw_step_s = 0; a figure that is not finite or does not fit an int32 gives u = INT32_MIN, outside every
    grid (pfb_cluster_items_from_pdws; host only)."""
    p = np.ascontiguousarray(np.asarray(pdws), PDW_DTYPE).reshape(-1)
    items = np.zeros(p.size, CLUSTER_ITEM_DTYPE)
    L.check(L.load().pfb_cluster_items_from_pdws(C.c_void_p(p.ctypes.data), p.size, PDW_DTYPE.itemsize, float(freq0),
                                                 float(freq_step_hz), float(pw_step_s), C.c_void_p(items.ctypes.data)),
            "pfb_cluster_items_from_pdws")
    return items


class PulseClusterer(Handle):
    """Clusterer of (u, v) items on a grid of ``cells_u`` x ``cells_v`` cells.  ``run`` takes a CUDA tensor (int32,
    n x 2) where it lies and returns CUDA tensors, or a numpy ``CLUSTER_ITEM_DTYPE`` array and returns numpy."""

    _kind, _destroy, _get_device = "clusterer", "pfb_cluster_destroy", "pfb_cluster_get_device"

    def __init__(self, cells_u: int, cells_v: int = 1, reach_u: int = 1, reach_v: int = 0, min_cell_count: int = 1,
                 min_pulses: int = 1, border: bool = False, *, device: int = -1):
        self._h = C.c_void_p()
        lib = L.load()
        cfg = _config(cells_u, cells_v, reach_u, reach_v, min_cell_count, min_pulses, border, device)
        L.check(lib.pfb_cluster_create(C.byref(cfg), C.byref(self._h)), "pfb_cluster_create")
        self._created(lib)
        self.plan = L.PfbClusterPlan()
        L.check(lib.pfb_cluster_describe(C.byref(cfg), 0, C.byref(self.plan)), "pfb_cluster_describe")
        self.cells_u, self.cells_v = int(cells_u), int(cells_v)
        self.capacity = 64      # records a run has room for; grows when the library asks for more

    def set_stream(self, hip_stream: int) -> None:
        L.check(self._lib.pfb_cluster_set_stream(self._h, C.c_void_p(hip_stream)), "pfb_cluster_set_stream")

    def sync(self) -> None:
        L.check(self._lib.pfb_cluster_sync(self._h), "pfb_cluster_sync")

    @property
    def last_kernel(self) -> str:
        """The kernels the last call launched, joined with '+'."""
        return self._lib.pfb_cluster_last_kernel(self._h).decode()

    @property
    def stats(self) -> dict:
        """outside, unassigned, dense_cells, border_cells, components and hook_rounds of the last run."""
        st = L.PfbClusterStats()
        L.check(self._lib.pfb_cluster_get_stats(self._h, C.byref(st)), "pfb_cluster_get_stats")
        return {k: int(getattr(st, k)) for k in STATS_FIELDS}

    def _items(self, items):
        """(pointer, count, mem, what keeps the pointer alive, the torch device or None)"""
        if is_torch(items) and items.is_cuda:
            import torch
            if items.dtype != torch.int32 or items.numel() % 2 or (items.dim() >= 2 and items.shape[-1] != 2):
                raise TypeError(f"expected (u, v) pairs (torch.int32, n x 2) for this {self._kind}, got {items.dtype} "
                                f"of shape {tuple(items.shape)}")
            if items.device.index != self.device_index:
                raise ValueError(f"items are on cuda:{items.device.index}, the {self._kind} on cuda:{self.device_index}")
            if not items.is_contiguous():
                raise ValueError("device items must be contiguous")
            return items.data_ptr(), items.numel() // 2, L.PFB_MEM_DEVICE, items, items.device
        a = np.asarray(items.numpy() if is_torch(items) else items)
        if a.dtype != CLUSTER_ITEM_DTYPE:
            raise TypeError(f"expected CLUSTER_ITEM_DTYPE items for this {self._kind}, got {a.dtype}")
        a = np.ascontiguousarray(a).reshape(-1)
        return a.ctypes.data, a.size, L.PFB_MEM_HOST, a, None

    def run(self, items, want_order: bool = True, capacity: int | None = None):
        """(records, labels, order, offsets) of the whole clustering (pfb_cluster_run); order and offsets are None
        without ``want_order``.  For device items all are CUDA tensors: the records a uint8 tensor of count x 64 bytes
        (``groups_to_numpy`` reads it), the rest int32.  With ``capacity`` None the room for records grows until the
        clusters fit; a given capacity that is too small raises PFB_ERR_CAPACITY."""
        ptr, n, mem, _keep, dev = self._items(items)
        cap = self.capacity if capacity is None else int(capacity)
        count = C.c_uint64()
        while True:
            if dev is None:
                rec, labels = np.zeros(cap, CLUSTER_GROUP_DTYPE), np.full(n, -1, np.int32)
                order = np.zeros(max(n, 1), np.uint32) if want_order else None
                offsets = np.zeros(cap + 2, np.uint32) if want_order else None
                ptrs = [x.ctypes.data if x is not None else None for x in (rec, labels, order, offsets)]
            else:
                import torch
                rec = torch.zeros((cap, CLUSTER_GROUP_DTYPE.itemsize), dtype=torch.uint8, device=dev)
                labels = torch.full((n,), -1, dtype=torch.int32, device=dev)
                # an empty tensor has no pointer, and a null order asks for no order at all: room for one item at least
                order = torch.zeros((max(n, 1),), dtype=torch.int32, device=dev) if want_order else None
                offsets = torch.zeros((cap + 2,), dtype=torch.int32, device=dev) if want_order else None
                ptrs = [x.data_ptr() if x is not None else None for x in (rec, labels, order, offsets)]
            rp, lp, op, fp = (C.c_void_p(p) for p in ptrs)
            rc = self._lib.pfb_cluster_run(self._h, C.c_void_p(ptr), n, mem, rp, cap, C.byref(count), lp, op, fp)
            if rc == L.PFB_ERR_CAPACITY and capacity is None and cap < int(count.value) <= MAX_CLUSTERS:
                cap = self.capacity = int(count.value)
                continue
            L.check(rc, "pfb_cluster_run")
            g = int(count.value)
            return rec[:g], labels, (order[:n] if want_order else None), (offsets[:g + 2] if want_order else None)

    __call__ = run

    def _cells(self, entry, items, dtype):
        ptr, n, mem, _keep, dev = self._items(items)
        cells = self.cells_u * self.cells_v
        if mem == L.PFB_MEM_DEVICE:
            import torch
            d = torch.zeros(cells, dtype=torch.int32, device=dev)
            L.check(getattr(self._lib, entry)(self._h, C.c_void_p(ptr), n, mem, C.c_void_p(d.data_ptr()), cells), entry)
            return d.cpu().numpy().view(dtype).reshape(self.cells_u, self.cells_v)
        out = np.zeros(cells, dtype)
        L.check(getattr(self._lib, entry)(self._h, C.c_void_p(ptr), n, mem, C.c_void_p(out.ctypes.data), cells), entry)
        return out.reshape(self.cells_u, self.cells_v)

    def histogram(self, items) -> np.ndarray:
        """Step 1 alone: the counts of the cells, uint32, cells_u x cells_v (pfb_cluster_histogram), numpy."""
        return self._cells("pfb_cluster_histogram", items, np.uint32)

    def cell_roots(self, items) -> np.ndarray:
        """Per cell the root g of its component, -1 for none, int32, cells_u x cells_v (pfb_cluster_cell_roots), numpy."""
        return self._cells("pfb_cluster_cell_roots", items, np.int32)

    def gather(self, src, order):
        """dst[k] = src[order[k]] on the device (pfb_cluster_gather): ``src`` a CUDA tensor of 4- or 8-byte elements,
        ``order`` an int32 CUDA tensor of indices into it, what ``run`` returned.  Waits for the copy."""
        import torch
        if not (is_torch(src) and src.is_cuda and is_torch(order) and order.is_cuda):
            raise TypeError("gather takes CUDA tensors")
        if src.element_size() not in (4, 8) or order.dtype != torch.int32:
            raise TypeError("gather takes 4- or 8-byte elements and int32 indices")
        if not (src.is_contiguous() and order.is_contiguous()) or src.dim() != 1:
            raise ValueError("gather takes flat contiguous tensors")
        if src.device.index != self.device_index or order.device.index != self.device_index:
            raise ValueError(f"the tensors are not on cuda:{self.device_index}, where the {self._kind} is")
        dst = torch.empty(order.numel(), dtype=src.dtype, device=src.device)
        L.check(self._lib.pfb_cluster_gather(self._h, C.c_void_p(src.data_ptr()), src.element_size(),
                                             C.c_void_p(order.data_ptr()), order.numel(), C.c_void_p(dst.data_ptr())),
                "pfb_cluster_gather")
        self.sync()
        return dst


def groups_to_numpy(records) -> np.ndarray:
    """CLUSTER_GROUP_DTYPE records from what ``PulseClusterer.run`` returned (a numpy array, or the CUDA byte tensor)."""
    if is_torch(records):
        return records.cpu().numpy().reshape(-1).view(CLUSTER_GROUP_DTYPE).copy()
    return np.asarray(records)


def pack_items(u, v=None):
    """CLUSTER_ITEM_DTYPE items from integer arrays (v = 0 when None), or the n x 2 int32 CUDA tensor from CUDA tensors."""
    if is_torch(u) and u.is_cuda:
        import torch
        v = torch.zeros_like(u) if v is None else v
        return torch.stack((u.to(torch.int32), v.to(torch.int32)), dim=1).contiguous()
    items = np.zeros(np.asarray(u).size, CLUSTER_ITEM_DTYPE)
    items["u"] = np.asarray(u).reshape(-1)
    if v is not None:
        items["v"] = np.asarray(v).reshape(-1)
    return items


def cluster_pulses(u, v=None, *, cells_u: int | None = None, cells_v: int | None = None, want_order: bool = True, **cfg):
    """One ``PulseClusterer.run`` over the items (u, v): (records as numpy, labels, order, offsets where the items lie).
    A grid that is not given is the smallest that holds every non-negative feature."""
    items = pack_items(u, v)
    on_device = is_torch(items)
    if cells_u is None or cells_v is None:
        host = items.cpu().numpy() if on_device else items.view(np.int32).reshape(-1, 2)
        top = host.max(axis=0) if len(host) else np.zeros(2, np.int64)
        cells_u = max(int(top[0]) + 1, 1) if cells_u is None else cells_u
        cells_v = max(int(top[1]) + 1, 1) if cells_v is None else cells_v
    dev = items.device.index if on_device else -1
    with PulseClusterer(cells_u, cells_v, device=dev, **cfg) as c:
        rec, labels, order, offsets = c.run(items, want_order)
    return groups_to_numpy(rec), labels, order, offsets


def _table_items(p, freq_step_hz, pw_step_s, freq0, freq):
    """(items, freq0) of a PDW table, with ``freq`` in place of its own where given"""
    if freq is not None:
        p = p.copy()
        p["freq"] = np.asarray(freq, np.float64).reshape(-1)
    if freq0 is None:
        ok = p["freq"][np.isfinite(p["freq"])]
        freq0 = float(ok.min()) if ok.size else 0.0
    return items_from_pdws(p, freq_step_hz, pw_step_s, freq0), freq0


def _grid_of(items, cells_u, cells_v):
    u, v = items["u"], items["v"]
    inside = u >= 0
    if cells_u is None:
        cells_u = int(u[inside].max()) + 1 if inside.any() else 1
    if cells_v is None:
        cells_v = max(int(v[inside].max()) + 1, 1) if inside.any() else 1
    if cells_u * cells_v > MAX_CELLS:
        raise ValueError(f"a grid of {cells_u} x {cells_v} cells is more than {MAX_CELLS}: take wider steps")
    return cells_u, cells_v


def cluster_pdws(pdws, freq_step_hz: float, pw_step_s: float = 0.0, freq0: float | None = None,
                 cells_u: int | None = None, cells_v: int | None = None, *, freq=None, **cfg):
    """Cluster a PDW table in the caller's order by ``freq`` (cells of freq_step_hz from freq0, the lowest finite freq
    unless given) and, with pw_step_s > 0, by ``pw``.  The grid is sized from the table when not given.  ``freq``
    replaces the table's own frequencies, e.g. with ``modulation_figures(...)["freq_hz"]``.  Returns (records, labels,
    order, offsets), numpy."""
    p = np.ascontiguousarray(np.asarray(pdws), PDW_DTYPE).reshape(-1)
    items, _ = _table_items(p, freq_step_hz, pw_step_s, freq0, freq)
    cells_u, cells_v = _grid_of(items, cells_u, cells_v)
    with PulseClusterer(cells_u, cells_v, **cfg) as c:
        rec, labels, order, offsets = c.run(items)
    return rec, labels, order, offsets


def deinterleave_clustered(pdws, tick_rate: float, min_period: int, max_period: int, bin_ticks: int = 1, *,
                           freq_step_hz: float, pw_step_s: float = 0.0, freq0: float | None = None, freq=None,
                           cells_u: int | None = None, cells_v: int | None = None, reach_u: int = 1, reach_v: int = 0,
                           min_cell_count: int = 1, cluster_min_pulses: int = 1, border: bool = False,
                           t0: float | None = None, **settings):
    """Deinterleave a PDW table (any order) one cluster at a time.  The table is put in time order (``ticks_from_toa``),
    clustered by frequency and pulse width on the device, its ticks are cut into per-cluster lists by one
    ``gather`` there, and one ``Deinterleaver`` (``settings`` are its keywords) searches each cluster's slice where it
    lies.  ``freq`` replaces the table's own frequencies (measured ones: ``modulation_figures(...)["freq_hz"]``).

    Returns (emitters, labels, clusters): ``emitters`` are CLUSTERED_EMITTER_DTYPE records numbered by cluster, then by
    extraction order, their ``first_pulse`` an index into the caller's table; ``labels`` holds per PDW of the caller's
    table its emitter or -1; ``clusters`` are SEARCHED_GROUP_DTYPE records: the cluster and what its search cost."""
    import torch
    p = np.ascontiguousarray(np.asarray(pdws), PDW_DTYPE).reshape(-1)
    if t0 is None:
        t0 = float(p["toa"].min()) if p.size else 0.0
    ticks, by_time = ticks_from_toa(p, tick_rate, t0)
    items, _ = _table_items(p[by_time], freq_step_hz, pw_step_s, freq0,
                            None if freq is None else np.asarray(freq, np.float64).reshape(-1)[by_time])
    cells_u, cells_v = _grid_of(items, cells_u, cells_v)
    with PulseClusterer(cells_u, cells_v, reach_u, reach_v, min_cell_count, cluster_min_pulses, border) as c:
        device_index = c.device_index
        dev = torch.device("cuda", device_index)
        d_items = torch.from_numpy(items.view(np.int32).reshape(-1, 2)).to(dev)
        d_ticks = torch.from_numpy(ticks.view(np.int64)).to(dev)
        rec, _, d_order, d_offsets = c.run(d_items)
        cut = c.gather(d_ticks, d_order)
    groups = groups_to_numpy(rec)
    order, offsets = d_order.cpu().numpy().astype(np.int64), d_offsets.cpu().numpy().astype(np.int64)
    clusters = np.zeros(groups.size, SEARCHED_GROUP_DTYPE)
    for name in CLUSTER_GROUP_DTYPE.names:
        clusters[name] = groups[name]
    caller = by_time.astype(np.int64)[order]            # position in the cut list -> index in the caller's table
    labels = np.full(p.size, -1, np.int32)
    found = []
    with Deinterleaver(min_period, max_period, bin_ticks, device=device_index, **settings) as d:
        for k in range(groups.size):
            lo, hi = int(offsets[k]), int(offsets[k + 1])
            r, lab = d.run(cut[lo:hi])
            r, lab = records_to_numpy(r), lab.cpu().numpy()
            base = sum(len(f) for f in found)
            hit = lab >= 0
            labels[caller[lo:hi][hit]] = base + lab[hit]
            e = np.zeros(r.size, CLUSTERED_EMITTER_DTYPE)
            for name in EMITTER_DTYPE.names:
                e[name] = r[name]
            e["first_pulse"] = caller[lo + r["first_pulse"].astype(np.int64)]
            e["cluster"] = k
            found.append(e)
            st = d.stats
            clusters[k]["emitters"] = r.size
            for name in ("rounds", "candidates_tried", "candidates_refused", "pulses_assigned"):
                clusters[k][name] = st[name]
    emitters = np.concatenate(found) if found else np.zeros(0, CLUSTERED_EMITTER_DTYPE)
    return emitters, labels, clusters


def deinterleave_clustered_figures(pdws, figures, tick_rate: float, min_period: int, max_period: int, bin_ticks: int = 1,
                                   *, freq_step_hz: float, center_hz: float = 0.0, **kw):
    """``deinterleave_clustered`` on measured frequencies: ``figures`` is what ``modulation_figures`` returned for the
    table's pulses, one per PDW in the table's order; the cells are of ``center_hz + figures["freq_hz"]``."""
    f = np.asarray(figures)["freq_hz"].astype(np.float64) + float(center_hz)
    return deinterleave_clustered(pdws, tick_rate, min_period, max_period, bin_ticks, freq_step_hz=freq_step_hz, freq=f, **kw)
