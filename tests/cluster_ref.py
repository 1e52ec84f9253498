"""The PDW clustering restated in numpy from the definition in include/pfb_channelizer.h (pfb_cluster_*), step by step:
the histogram, the dense cells, the components and their rounds, the border rule, the clusters, the records, the stable
partition.  Every figure is an integer or a comparison, so the device is held to these bytes.  The literal_* forms are
the plain loops over cells with a union-find that the vectorised ones are tested against (test_cluster_cpu.py)."""
from dataclasses import dataclass

import numpy as np

ITEM = np.dtype([("u", "i4"), ("v", "i4")])
GROUP = np.dtype([("root_u", "i4"), ("root_v", "i4"), ("pulses", "u4"), ("cells", "u4"), ("u_min", "i4"), ("u_max", "i4"),
                  ("v_min", "i4"), ("v_max", "i4"), ("sum_u", "i8"), ("sum_v", "i8"), ("peak_u", "i4"), ("peak_v", "i4"),
                  ("peak_count", "u4"), ("first_item", "u4")])
STATS = ("outside", "unassigned", "dense_cells", "border_cells", "components", "hook_rounds")
MAX_CLUSTERS = 65535


@dataclass(frozen=True)
class Cfg:
    U: int
    V: int = 1
    ru: int = 1
    rv: int = 0
    minc: int = 1
    minp: int = 1
    border: bool = False

    @property
    def cells(self) -> int:
        return self.U * self.V

    def settings(self) -> dict:
        """the keyword arguments of sdr_channelizer_amd.PulseClusterer"""
        return dict(cells_u=self.U, cells_v=self.V, reach_u=self.ru, reach_v=self.rv, min_cell_count=self.minc,
                    min_pulses=self.minp, border=self.border)


def items_of(u, v=None) -> np.ndarray:
    it = np.zeros(np.asarray(u).size, ITEM)
    it["u"] = u
    if v is not None:
        it["v"] = v
    return it


def cell_of(items, c: Cfg) -> np.ndarray:
    """g of every item, -1 outside the grid"""
    u, v = items["u"].astype(np.int64), items["v"].astype(np.int64)
    inside = (u >= 0) & (u < c.U) & (v >= 0) & (v < c.V)
    return np.where(inside, u * c.V + v, -1)


# -- step 1 ------------------------------------------------------------------------------------------------------------
def histogram(items, c: Cfg) -> np.ndarray:
    g = cell_of(items, c)
    return np.bincount(g[g >= 0], minlength=c.cells).astype(np.uint32)


# -- steps 2 and 3 -----------------------------------------------------------------------------------------------------
def components(H, c: Cfg):
    """(label, rounds): per cell the root of its component, -1 for a cell that is not dense, and hook_rounds"""
    dense = (H >= c.minc).reshape(c.U, c.V)
    L = np.where(dense, np.arange(c.cells).reshape(c.U, c.V), -1)
    rounds = 0
    if not dense.any():
        return L.reshape(-1).astype(np.int32), 0
    # one of each pair: (du, dv) after (0, 0) in reading order
    offsets = [(du, dv) for du in range(0, c.ru + 1) for dv in range(-c.rv, c.rv + 1) if (du, dv) > (0, 0)]
    while True:
        new = L.reshape(-1).copy()
        lowered = False
        for du, dv in offsets:
            if du >= c.U or abs(dv) >= c.V:
                continue
            a = L[:c.U - du, max(0, -dv):c.V - max(0, dv)]
            b = L[du:, max(0, dv):c.V - max(0, -dv)]
            m = (a >= 0) & (b >= 0) & (a != b)
            if m.any():
                lowered = True
                np.minimum.at(new, np.maximum(a[m], b[m]), np.minimum(a[m], b[m]))
        rounds += 1
        if not lowered:
            break
        ok = new >= 0
        while True:                                   # every label to the end of its chain
            nxt = new.copy()
            nxt[ok] = new[new[ok]]
            if (nxt == new).all():
                break
            new = nxt
        L = new.reshape(c.U, c.V)
    return L.reshape(-1).astype(np.int32), rounds


# -- step 4 ------------------------------------------------------------------------------------------------------------
def cell_roots(H, c: Cfg):
    """(root of every cell after the border step, border cells, rounds)"""
    label, rounds = components(H, c)
    root = label.copy()
    joined = 0
    if c.border:
        L = label.reshape(c.U, c.V)
        for g in np.nonzero((H > 0) & (H < c.minc))[0]:
            u, v = divmod(int(g), c.V)
            box = L[max(u - c.ru, 0):u + c.ru + 1, max(v - c.rv, 0):v + c.rv + 1]
            if (box >= 0).any():
                root[g] = box[box >= 0].min()
                joined += 1
    return root, joined, rounds


# -- steps 5 and 6 -----------------------------------------------------------------------------------------------------
def run(items, c: Cfg, capacity=None):
    """(records, labels, order, offsets, stats, G); records .. stats are None when the call is refused for capacity"""
    items = np.ascontiguousarray(items, ITEM).reshape(-1)
    n = items.size
    H = histogram(items, c)
    root, joined, rounds = cell_roots(H, c)
    member = np.nonzero(root >= 0)[0]
    pulses = np.zeros(c.cells, np.int64)
    np.add.at(pulses, root[member], H[member].astype(np.int64))
    is_root = root == np.arange(c.cells)
    roots = np.nonzero(is_root & (pulses >= c.minp))[0]             # ascending: the numbering
    G = len(roots)
    if G > MAX_CLUSTERS or (capacity is not None and G > capacity):
        return None, None, None, None, None, G
    number = np.full(c.cells, -1, np.int64)
    number[roots] = np.arange(G)
    g = cell_of(items, c)
    labels = np.full(n, -1, np.int32)
    inside = g >= 0
    r = root[g[inside]]
    labels[inside] = np.where(r >= 0, number[np.maximum(r, 0)], -1)
    rec = np.zeros(G, GROUP)
    if G:
        cells = member[number[root[member]] >= 0]                   # the cells of clusters, and each one's cluster
        k = number[root[cells]]
        big = np.iinfo(np.int64).max
        lo_u, hi_u, lo_v, hi_v = (np.full(G, s * big) for s in (1, -1, 1, -1))
        np.minimum.at(lo_u, k, cells // c.V)
        np.maximum.at(hi_u, k, cells // c.V)
        np.minimum.at(lo_v, k, cells % c.V)
        np.maximum.at(hi_v, k, cells % c.V)
        by_peak = np.lexsort((cells, -H[cells].astype(np.int64), k))  # by cluster, then largest H, then lowest g
        peak = cells[by_peak][np.searchsorted(k[by_peak], np.arange(G))]
        mine = np.nonzero(labels >= 0)[0]
        sum_u, sum_v, first = np.zeros(G, np.int64), np.zeros(G, np.int64), np.full(G, big)
        np.add.at(sum_u, labels[mine], items["u"][mine].astype(np.int64))
        np.add.at(sum_v, labels[mine], items["v"][mine].astype(np.int64))
        np.minimum.at(first, labels[mine], mine)
        rec["root_u"], rec["root_v"], rec["pulses"] = roots // c.V, roots % c.V, pulses[roots]
        rec["cells"] = np.bincount(k, minlength=G)
        rec["u_min"], rec["u_max"], rec["v_min"], rec["v_max"] = lo_u, hi_u, lo_v, hi_v
        rec["sum_u"], rec["sum_v"], rec["first_item"] = sum_u, sum_v, first
        rec["peak_u"], rec["peak_v"], rec["peak_count"] = peak // c.V, peak % c.V, H[peak]
    key = np.where(labels < 0, G, labels)
    order = np.argsort(key, kind="stable").astype(np.uint32)
    offsets = np.zeros(G + 2, np.uint32)
    offsets[1:G + 1] = np.cumsum(np.bincount(key, minlength=G + 1)[:G])
    offsets[G + 1] = n
    stats = dict(outside=int((~inside).sum()), unassigned=int((inside & (labels < 0)).sum()),
                 dense_cells=int((H >= c.minc).sum()), border_cells=joined, components=int(is_root.sum()),
                 hook_rounds=rounds)
    return rec, labels, order, offsets, stats, G


# -- the literal form: loops over cells, a union-find ------------------------------------------------------------------
def literal_run(items, c: Cfg):
    """(records as dicts, labels, stats without hook_rounds) by the definition's sentences, one at a time"""
    H = [0] * c.cells
    outside = 0
    for it in items:
        u, v = int(it["u"]), int(it["v"])
        if 0 <= u < c.U and 0 <= v < c.V:
            H[u * c.V + v] += 1
        else:
            outside += 1
    dense = [h >= c.minc for h in H]
    parent = list(range(c.cells))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    for g in range(c.cells):
        for k in range(g + 1, c.cells):
            if dense[g] and dense[k] and abs(g // c.V - k // c.V) <= c.ru and abs(g % c.V - k % c.V) <= c.rv:
                a, b = find(g), find(k)
                parent[max(a, b)] = min(a, b)                        # the root stays the lowest g
    root = [find(g) if dense[g] else -1 for g in range(c.cells)]
    joined = 0
    if c.border:
        dense_root = list(root)
        for g in range(c.cells):
            if 0 < H[g] < c.minc:
                near = [dense_root[k] for k in range(c.cells) if dense[k] and abs(g // c.V - k // c.V) <= c.ru
                        and abs(g % c.V - k % c.V) <= c.rv]
                if near:
                    root[g] = min(near)
                    joined += 1
    comps = sorted({r for r in root if r >= 0})
    pulses = {r: sum(H[g] for g in range(c.cells) if root[g] == r) for r in comps}
    clusters = [r for r in comps if pulses[r] >= c.minp]
    labels = []
    for it in items:
        u, v = int(it["u"]), int(it["v"])
        lab = -1
        if 0 <= u < c.U and 0 <= v < c.V and root[u * c.V + v] in clusters:
            lab = clusters.index(root[u * c.V + v])
        labels.append(lab)
    records = []
    for k, r in enumerate(clusters):
        cells = [g for g in range(c.cells) if root[g] == r]
        mine = [i for i, lab in enumerate(labels) if lab == k]
        peak = max(cells, key=lambda g: (H[g], -g))
        records.append(dict(root_u=r // c.V, root_v=r % c.V, pulses=pulses[r], cells=len(cells),
                            u_min=min(g // c.V for g in cells), u_max=max(g // c.V for g in cells),
                            v_min=min(g % c.V for g in cells), v_max=max(g % c.V for g in cells),
                            sum_u=sum(int(items["u"][i]) for i in mine), sum_v=sum(int(items["v"][i]) for i in mine),
                            peak_u=peak // c.V, peak_v=peak % c.V, peak_count=H[peak], first_item=mine[0]))
    inside = len(items) - outside
    stats = dict(outside=outside, unassigned=inside - sum(lab >= 0 for lab in labels), dense_cells=sum(dense),
                 border_cells=joined, components=len(comps))
    return records, np.array(labels, np.int32), stats, np.array(root, np.int32)


def literal_rounds(H, c: Cfg) -> int:
    """hook_rounds by the header's sentences: every linked pair reads the labels as the round found them"""
    dense = [g for g in range(c.cells) if H[g] >= c.minc]
    if not dense:
        return 0
    pairs = [(g, k) for g in dense for k in dense if g < k and abs(g // c.V - k // c.V) <= c.ru
             and abs(g % c.V - k % c.V) <= c.rv]
    L = {g: g for g in dense}
    rounds = 0
    while True:
        new = dict(L)
        lowered = False
        for g, k in pairs:
            a, b = min(L[g], L[k]), max(L[g], L[k])
            if a != b:
                new[b] = min(new[b], a)
                lowered = True
        rounds += 1
        if not lowered:
            return rounds
        for g in dense:
            x = g
            while new[x] != x:
                x = new[x]
            L[g] = x


def items_from_pdws(pdws, freq0: float, freq_step: float, pw_step: float = 0.0) -> np.ndarray:
    """pfb_cluster_items_from_pdws: one IEEE subtraction, one division and a floor per figure"""
    with np.errstate(all="ignore"):
        u = np.floor((np.asarray(pdws["freq"], np.float64) - np.float64(freq0)) / np.float64(freq_step))
        v = np.floor(np.asarray(pdws["pw"], np.float64) / np.float64(pw_step)) if pw_step > 0 else np.zeros(len(pdws))
    lo, hi = -2147483648.0, 2147483647.0
    ok = np.isfinite(u) & np.isfinite(v) & (u >= lo) & (u <= hi) & (v >= lo) & (v <= hi)
    it = np.zeros(len(pdws), ITEM)
    it["u"] = np.where(ok, u, lo).astype(np.int64)
    it["v"] = np.where(ok, v, 0).astype(np.int64)
    return it
