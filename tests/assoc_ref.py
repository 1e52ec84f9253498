"""The numpy restatement of the PDW association, written from the header's definition (pfb_assoc_* in
include/pfb_channelizer.h) and from nothing else: the edges of every item's window, the connected components by
synchronous rounds of hooking and pointer doubling, the groups' numbers, records and stats.  ``literal_*`` are the
definition as loops over pairs with a union-find, for small lists: what the restatement itself is held to."""
from dataclasses import dataclass

import numpy as np

ITEM = np.dtype([("start", "u8"), ("length", "u4"), ("cell", "i4"), ("weight", "f4"), ("reserved", "u4")])
GROUP = np.dtype([("first_tick", "u8"), ("end_tick", "u8"), ("length_sum", "u8"), ("members", "u4"),
                  ("first_item", "u4"), ("best_item", "u4"), ("best_cell", "i4"), ("cell_lo", "i4"), ("cell_hi", "i4")])
STATS = ("groups", "edges", "clipped", "largest_group", "linked_items")     # without rounds: not a function of the input
MAX_TICK = 1 << 62


@dataclass(frozen=True)
class Cfg:
    Rc: int = 1          # cell_reach
    g: int = 0           # slack_ticks
    K: int = 64          # window_items

    def settings(self):
        return dict(cell_reach=self.Rc, slack_ticks=self.g, window_items=self.K)


def items(start, length, cell, weight=None):
    """an ITEM array from columns"""
    out = np.zeros(len(start), ITEM)
    out["start"], out["length"], out["cell"] = start, length, cell
    out["weight"] = 1.0 if weight is None else weight
    return out


def acceptable(it, c):
    """what the device checks in its first pass: the order of the starts and the bound"""
    s = it["start"].astype(object)
    return all(int(s[k]) <= int(s[k + 1]) for k in range(len(s) - 1)) and \
        all(int(v["start"]) < MAX_TICK and int(v["start"]) + int(v["length"]) + c.g < MAX_TICK for v in it)


def weight_key(w):
    """the order-preserving uint32 key of the float's bits"""
    b = np.ascontiguousarray(w, np.float32).view(np.uint32)
    return np.where(b & np.uint32(0x80000000), ~b, b ^ np.uint32(0x80000000)).astype(np.uint32)


def edges(it, c):
    """(a, b, clipped): the pairs a < b that satisfy the rule, sorted by (a, b), and the clipped flag of every item"""
    n = len(it)
    start = it["start"].astype(np.uint64)
    lim = start + it["length"].astype(np.uint64) + np.uint64(c.g)
    cell = it["cell"].astype(np.int64)
    A, B = [], []
    for d in range(1, min(c.K, n - 1) + 1 if n else 0):
        near = start[d:] <= lim[:n - d]
        if not near.any():
            break            # sorted: start[i + d + 1] >= start[i + d] for every i
        ok = near & (np.abs(cell[d:] - cell[:n - d]) <= c.Rc)
        a = np.flatnonzero(ok)
        A.append(a)
        B.append(a + d)
    clipped = np.zeros(n, bool)
    if n > c.K + 1:
        clipped[:n - c.K - 1] = start[c.K + 1:] <= lim[:n - c.K - 1]
    if not A:
        return np.zeros(0, np.int64), np.zeros(0, np.int64), clipped
    a, b = np.concatenate(A), np.concatenate(B)
    order = np.lexsort((b, a))
    return a[order], b[order], clipped


def links(it, c):
    """(first_link, link_count) per item, int32: what pfb_assoc_links writes"""
    n = len(it)
    a, b, _ = edges(it, c)
    count = np.bincount(a, minlength=n).astype(np.int32)
    first = np.full(n, -1, np.int32)
    if len(a):
        lead = np.flatnonzero(np.r_[True, a[1:] != a[:-1]])       # sorted by (a, b): the first of every a is its lowest b
        first[a[lead]] = b[lead]
    return first, count


def components(n, a, b):
    """(label, rounds): label[i] = the smallest index of i's component, by synchronous rounds of hooking (a minimum on
    the larger root's entry) and pointer doubling until flat; rounds counts the rounds that hooked and the last one"""
    lab = np.arange(n, dtype=np.int64)
    rounds = 0
    while len(a):
        rounds += 1
        ra, rb = lab[a], lab[b]
        diff = ra != rb
        if not diff.any():
            break
        np.minimum.at(lab, np.maximum(ra, rb)[diff], np.minimum(ra, rb)[diff])
        while True:
            nxt = lab[lab]
            if (nxt == lab).all():
                break
            lab = nxt
    return lab, rounds


def run(it, c):
    """(records, labels, stats): what pfb_assoc_run writes and pfb_assoc_get_stats reports, rounds left out"""
    n = len(it)
    a, b, clipped = edges(it, c)
    lab, _ = components(n, a, b)
    roots = np.flatnonzero(lab == np.arange(n))
    number = np.full(n, -1, np.int64)
    number[roots] = np.arange(len(roots))
    labels = number[lab].astype(np.int32)
    G = len(roots)
    rec = np.zeros(G, GROUP)
    if n:
        start = it["start"].astype(np.uint64)
        end = start + it["length"].astype(np.uint64)
        cell = it["cell"].astype(np.int32)
        rec["first_tick"] = start[roots]
        rec["first_item"] = roots
        e = np.zeros(G, np.uint64)
        np.maximum.at(e, labels, end)
        rec["end_tick"] = e
        s = np.zeros(G, np.uint64)
        np.add.at(s, labels, it["length"].astype(np.uint64))
        rec["length_sum"] = s
        rec["members"] = np.bincount(labels, minlength=G)
        best = np.zeros(G, np.uint64)
        np.maximum.at(best, labels, (weight_key(it["weight"]).astype(np.uint64) << np.uint64(32))
                      | (np.uint64(0xffffffff) - np.arange(n, dtype=np.uint64)))
        rec["best_item"] = (np.uint64(0xffffffff) - (best & np.uint64(0xffffffff))).astype(np.uint32)
        rec["best_cell"] = cell[rec["best_item"]]
        lo, hi = np.full(G, np.iinfo(np.int32).max, np.int32), np.full(G, np.iinfo(np.int32).min, np.int32)
        np.minimum.at(lo, labels, cell)
        np.maximum.at(hi, labels, cell)
        rec["cell_lo"], rec["cell_hi"] = lo, hi
    members = rec["members"].astype(np.int64)
    stats = dict(groups=G, edges=len(a), clipped=int(clipped.sum()), largest_group=int(members.max()) if G else 0,
                 linked_items=int(members[members >= 2].sum()))
    return rec, labels, stats


# -- the definition as loops -------------------------------------------------------------------------------------------
def literal_edges(it, c):
    n = len(it)
    out, clipped = [], []
    for i in range(n):
        lim = int(it["start"][i]) + int(it["length"][i]) + c.g
        for j in range(i + 1, n):
            if j - i > c.K or int(it["start"][j]) > lim:
                break
            if abs(int(it["cell"][i]) - int(it["cell"][j])) <= c.Rc:
                out.append((i, j))
        clipped.append(i + c.K + 1 < n and int(it["start"][i + c.K + 1]) <= lim)
    return out, clipped


def literal_run(it, c):
    """(records as a list of dicts, labels, stats) from a union-find over literal_edges and plain Python"""
    n = len(it)
    pairs, clipped = literal_edges(it, c)
    parent = list(range(n))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    for i, j in pairs:
        ri, rj = find(i), find(j)
        if ri != rj:
            parent[max(ri, rj)] = min(ri, rj)
    root = [find(i) for i in range(n)]
    order = sorted(set(root))
    labels = np.array([order.index(r) for r in root], np.int32)
    keys = weight_key(it["weight"]) if n else []
    recs = []
    for r in order:
        mem = [i for i in range(n) if root[i] == r]
        best = max(mem, key=lambda i: (int(keys[i]), -i))
        cells = [int(it["cell"][i]) for i in mem]
        recs.append(dict(first_tick=int(it["start"][r]), end_tick=max(int(it["start"][i]) + int(it["length"][i]) for i in mem),
                         length_sum=sum(int(it["length"][i]) for i in mem), members=len(mem), first_item=r, best_item=best,
                         best_cell=int(it["cell"][best]), cell_lo=min(cells), cell_hi=max(cells)))
    sizes = [r["members"] for r in recs]
    stats = dict(groups=len(recs), edges=len(pairs), clipped=sum(clipped), largest_group=max(sizes, default=0),
                 linked_items=sum(s for s in sizes if s >= 2))
    return recs, labels, stats


def items_from_pdws(pdws, t0, tick_rate):
    """(items, order) as pfb_assoc_items_from_pdws: to nearest, ties to even, a stable sort by start"""
    start = np.rint((pdws["toa"] - t0) * tick_rate)
    length = np.rint(pdws["pw"] * tick_rate)
    it = items(start.astype(np.uint64), length.astype(np.uint32), pdws["bin"], pdws["mag"].astype(np.float32))
    order = np.argsort(it["start"], kind="stable").astype(np.uint32)
    return it[order], order
