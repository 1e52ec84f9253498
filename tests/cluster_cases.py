"""Designed inputs of the PDW clustering (pfb_cluster_*), shared by test_cluster_cpu.py -- which proves on the numpy
restatement that each list does what it is there for -- and test_gpu_cluster.py, which holds the device to the
restatement's bytes on them.  A case is (items, Cfg); the tile sizes and the tier bound are the plan's
(test_cluster_cpu.py checks them against pfb_cluster_describe)."""
import functools

import numpy as np

import cluster_ref as R
import deint_ref as DR

HIST_TILE, LABEL_TILE, PART_TILE, LDS_CELLS = 4096, 256, 1024, 8192
I32_MIN, I32_MAX = -(1 << 31), (1 << 31) - 1


def from_cells(cells, seed=0, extra=()):
    """items of (u, v, count) cells in a shuffled order, then `extra` (u, v) items"""
    u = np.repeat([c[0] for c in cells], [c[2] for c in cells]).astype(np.int64)
    v = np.repeat([c[1] for c in cells], [c[2] for c in cells]).astype(np.int64)
    p = np.random.default_rng(seed).permutation(u.size)
    ex = np.array(list(extra), np.int64).reshape(-1, 2)
    return R.items_of(np.concatenate([u[p], ex[:, 0]]), np.concatenate([v[p], ex[:, 1]]))


def random_list(seed, n, c: R.Cfg, blobs=6, stray=0.2):
    """n items: `blobs` blobs a few cells wide, a share of strays that also fall outside the grid"""
    rng = np.random.default_rng(seed)
    cu, cv = rng.integers(0, c.U, blobs), rng.integers(0, c.V, blobs)
    who = rng.integers(0, blobs, n)
    u = cu[who] + np.rint(rng.normal(0, 1.2, n)).astype(np.int64)
    v = cv[who] + np.rint(rng.normal(0, 0.8, n)).astype(np.int64)
    s = rng.random(n) < stray
    u[s] = rng.integers(-2, c.U + 2, int(s.sum()))
    v[s] = rng.integers(-1, c.V + 1, int(s.sum()))
    return R.items_of(u, v)


def _bit_reversed(k, bits):
    return int(format(k, "0%db" % bits)[::-1], 2)


def _column_tops(side):
    """the top row of the column at v = 2 k: k's bits reversed.  A column's lowest g is its top, so along the columns
    the roots of a first round alternate high, low at every scale and each later round joins only half of what is left"""
    bits = (side // 2).bit_length() - 1
    return [_bit_reversed(k, bits) for k in range(side // 2)]


def serpentine(side=64):
    """columns of dense cells at even v from their tops down, each joined to the next by one cell, in turn in the last
    row and three rows above it: one winding component"""
    cells = []
    for k, top in enumerate(_column_tops(side)):
        cells += [(u, 2 * k, 1) for u in range(top, side)]
        if 2 * k + 1 < side - 1:
            cells.append((side - 1 if k % 2 == 0 else side - 4, 2 * k + 1, 1))
    return from_cells(cells, 3), R.Cfg(side, side, 1, 1)


def comb(side=64):
    """teeth along u at every second v, from their tops down to a spine along the last row"""
    cells = [(side - 1, v, 1) for v in range(side)]
    for k, top in enumerate(_column_tops(side)):
        cells += [(u, 2 * k, 1) for u in range(top, side - 1)]
    return from_cells(cells, 4), R.Cfg(side, side, 1, 1)


def isolated(G, side, extra=((-1, 0), (0, -1))):
    """G cells of one item each, no two within reach 0 of each other: G clusters; the extras are unassigned"""
    g = np.random.default_rng(G).permutation(side * side)[:G]
    return from_cells([(int(k) // side, int(k) % side, 1) for k in g], G, extra), R.Cfg(side, side, 0, 0)


def alternating(n=2 * PART_TILE + 300):
    """labels 0, 1, 2, -1, 0, 1, ... down the list: every lane's rank depends on all lanes below it, in every wave and
    across the partition's tiles; the clusters' cells are (0, 0), (4, 0), (8, 0), the fourth item lies outside"""
    i = np.arange(n)
    return R.items_of(np.where(i % 4 == 3, -5, 4 * (i % 4)), np.zeros(n, np.int64)), R.Cfg(12, 1, 1, 0)


REACH = R.Cfg(40, 40, 3, 2)
BORDER = R.Cfg(8, 8, 1, 1, minc=3, border=True)
# X = (0,5) (1,5) (2,5), root g = 5; Y = (2,3), root g = 19; the border cell (2,4) touches both, and Y's cell first
BORDER_CELLS = [(0, 5, 3), (1, 5, 3), (2, 5, 4), (2, 3, 5), (2, 4, 2), (6, 1, 1)]
MINP = R.Cfg(30, 2, 1, 0, minc=2, minp=10)

CASES = {
    "n_0": lambda: (R.items_of([]), R.Cfg(5, 5)),
    "n_1": lambda: (R.items_of([2], [3]), R.Cfg(5, 5)),
    "n_2": lambda: (R.items_of([2, 4], [3, 3]), R.Cfg(5, 5)),
    "grid_1x1": lambda: (R.items_of([0, 0, 1, -1, 0], [0, 0, 0, 0, 1]), R.Cfg(1, 1, 8, 8)),
    "grid_1xV": lambda: (random_list(11, 700, R.Cfg(1, 37, 0, 1, minc=2), 3), R.Cfg(1, 37, 0, 1, minc=2)),
    "grid_Ux1": lambda: (random_list(12, 900, R.Cfg(300, 1, 2, 0, minc=2, border=True), 5), R.Cfg(300, 1, 2, 0, minc=2, border=True)),
    "grid_lds_bound": lambda: (random_list(13, 3000, R.Cfg(128, 64, 1, 1, minc=2), 8), R.Cfg(128, 64, 1, 1, minc=2)),
    "grid_lds_bound_1d": lambda: (random_list(14, 3000, R.Cfg(LDS_CELLS, 1, 2, 0), 8), R.Cfg(LDS_CELLS, 1, 2, 0)),
    "grid_over_lds_bound": lambda: (random_list(14, 3000, R.Cfg(LDS_CELLS + 1, 1, 2, 0), 8), R.Cfg(LDS_CELLS + 1, 1, 2, 0)),
    "grid_17_wide": lambda: (random_list(15, 2000, R.Cfg(50, 17, 1, 1, minc=2, border=True), 7), R.Cfg(50, 17, 1, 1, minc=2, border=True)),
    "reach_u_at": lambda: (from_cells([(10, 10, 2), (13, 10, 2)]), REACH),
    "reach_u_over": lambda: (from_cells([(10, 10, 2), (14, 10, 2)]), REACH),
    "reach_v_at": lambda: (from_cells([(10, 10, 2), (10, 12, 2)]), REACH),
    "reach_v_over": lambda: (from_cells([(10, 10, 2), (10, 13, 2)]), REACH),
    "reach_diag_at": lambda: (from_cells([(10, 10, 2), (13, 12, 2), (16, 10, 1)]), REACH),
    "reach_diag_over": lambda: (from_cells([(10, 10, 2), (14, 12, 2), (20, 20, 1), (23, 23, 1)]), REACH),
    "reach_0": lambda: (from_cells([(5, 5, 2), (5, 6, 2), (6, 5, 1), (6, 6, 3)]), R.Cfg(9, 9, 0, 0)),
    "reach_8": lambda: (from_cells([(0, 0, 1), (8, 8, 1), (16, 0, 2), (25, 0, 1), (16, 17, 1), (39, 39, 1), (31, 31, 1)]),
                        R.Cfg(40, 40, 8, 8)),
    "min_cell_count": lambda: (from_cells([(2, 2, 4), (6, 6, 5)]), R.Cfg(9, 9, 1, 1, minc=5)),
    "min_pulses": lambda: (from_cells([(1, 0, 6), (2, 0, 4), (8, 1, 5), (9, 1, 4), (15, 0, 10), (20, 0, 2), (20, 1, 2)]), MINP),
    "border_lowest_root": lambda: (from_cells(BORDER_CELLS), BORDER),
    "border_off": lambda: (from_cells(BORDER_CELLS), R.Cfg(8, 8, 1, 1, minc=3)),
    "outside": lambda: (from_cells([(0, 0, 2), (6, 4, 2)], 1, [(-1, 0), (7, 0), (0, -1), (0, 5), (I32_MIN, 0), (I32_MAX, 0),
                                                              (0, I32_MIN), (0, I32_MAX), (I32_MIN, I32_MIN),
                                                              (I32_MAX, I32_MAX), (7, 5), (-1, -1)]), R.Cfg(7, 5, 1, 1)),
    "one_cell": lambda: (R.items_of(np.full(5000, 3), np.full(5000, 1)), R.Cfg(6, 2, 1, 1, minc=5000, minp=5000)),
    "sum_past_2_32": lambda: (R.items_of(np.full(5000, (1 << 20) - 1)), R.Cfg(1 << 20, 1, 1, 0)),
    "serpentine": serpentine,
    "comb": comb,
    "isolated_254": lambda: isolated(254, 20),
    "isolated_255": lambda: isolated(255, 20),
    "isolated_256": lambda: isolated(256, 20),
    "isolated_257": lambda: isolated(257, 20),
    "isolated_65535": lambda: isolated(65535, 256),
    "isolated_65536": lambda: isolated(65536, 256),
    "alternating": alternating,
    "duplicates": lambda: (R.items_of(np.tile([3, 3, 9, 3, 9, 9, 20, 3], 40), np.tile([1, 1, 0, 1, 0, 0, 1, 1], 40)),
                           R.Cfg(12, 2, 1, 0)),
}
for _name, _tile in (("hist", HIST_TILE), ("label", LABEL_TILE), ("part", PART_TILE)):
    for _tag, _n in (("less_1", _tile - 1), ("at", _tile), ("plus_1", _tile + 1), ("two_plus_1", 2 * _tile + 1)):
        CASES["%s_tile_%s" % (_name, _tag)] = functools.partial(
            lambda n: (random_list(n, n, R.Cfg(40, 3, 1, 1, minc=2, border=True)), R.Cfg(40, 3, 1, 1, minc=2, border=True)), _n)


@functools.lru_cache(maxsize=None)
def inputs(name):
    return CASES[name]()


@functools.lru_cache(maxsize=None)
def expected(name, capacity=None):
    """R.run of the case, computed once and shared; the arrays are not to be written"""
    it, c = inputs(name)
    return R.run(it, c, capacity)


@functools.lru_cache(maxsize=None)
def big():
    """2^20 items on a 1024 x 1024 grid: 1024 blobs and a tenth strays"""
    c = R.Cfg(1024, 1024, 1, 1, minc=2, minp=50, border=True)
    return random_list(99, 1 << 20, c, blobs=1024, stray=0.1), c


# -- the scene the unit is for -----------------------------------------------------------------------------------------
def scene_with_trains(n: int, trains: int, seed: int):
    """tools/deint_rate.py's scene(n, trains, seed), tick for tick, with each pulse's train beside it (-1: a stray)"""
    rng = np.random.default_rng(seed)
    periods = np.unique(np.linspace(2000, 4000, trains).astype(np.int64) | 1)
    rate = float(np.sum(0.9 / periods)) / 0.98
    span = int(n / rate * 1.05)
    parts, who = [], []
    for k, p in enumerate(periods):
        j = np.arange((span - 1) // p)
        x = int(rng.integers(0, p)) + j * p + rng.integers(-1, 2, j.size)
        keep = rng.random(j.size) >= 0.1
        parts.append(x[keep])
        who.append(np.full(int(keep.sum()), k))
    parts.append(rng.integers(0, span, n // 50))
    who.append(np.full(n // 50, -1))
    t, w = np.maximum(np.concatenate(parts), 0), np.concatenate(who)
    by_time = np.argsort(t, kind="stable")
    return t[by_time][:n].astype(np.uint64), w[by_time][:n], periods


SCENE_DEINT = DR.Cfg(pmin=1000, pmax=9000, W=4, Lv=16, detect=30, min_pulses=8, X=4, tol=5, fill=50, max_emitters=64)
SCENE_CELLS, SCENE_FIRST, SCENE_PITCH = 424, 20, 12
SCENE_CLUSTER = R.Cfg(SCENE_CELLS, 1, 1, 0, minc=3, minp=8, border=True)


def scene_features(who, seed=1):
    """the frequency cell of every pulse: train k around cell 20 + 12 k with a measurement spread of a few cells (normal,
    sigma one cell), the strays anywhere"""
    rng = np.random.default_rng(seed)
    u = SCENE_FIRST + SCENE_PITCH * who + np.rint(rng.normal(0, 1.0, who.size)).astype(np.int64)
    stray = who < 0
    u[stray] = rng.integers(0, SCENE_CELLS, int(stray.sum()))
    return R.items_of(u)


# -- the chain at a size for the device --------------------------------------------------------------------------------
CHAIN_RATE = 1e6
CHAIN_DEINT = DR.Cfg(pmin=1000, pmax=6000, W=2, Lv=8, detect=30, min_pulses=8, X=4, tol=3, fill=50, max_emitters=8)
CHAIN_STEP_HZ, CHAIN_FREQ0 = 1e6, 1e9
CHAIN_CLUSTER = dict(reach_u=1, reach_v=0, min_cell_count=2, cluster_min_pulses=8, border=True)


def chain_table(seed=5):
    """(pdws in a shuffled order, each one's train, the periods): eight trains of about 64 pulses, 5 MHz apart, a few
    strays"""
    from sdr_channelizer_amd.pdw import PDW_DTYPE
    rng = np.random.default_rng(seed)
    periods = np.array([2001, 2311, 2617, 2903, 3203, 3511, 3803, 4111])
    ticks, who, freq = [], [], []
    for k, p in enumerate(periods):
        n = 64 + int(rng.integers(-4, 5))
        x = int(rng.integers(0, p)) + np.arange(n) * p + rng.integers(-1, 2, n)
        keep = rng.random(n) >= 0.05
        ticks.append(x[keep])
        who.append(np.full(int(keep.sum()), k))
        freq.append(CHAIN_FREQ0 + 3.5e6 + 5e6 * k + rng.normal(0, 0.3e6, int(keep.sum())))
    ticks.append(rng.integers(0, 64 * 3000, 12))
    who.append(np.full(12, -1))
    freq.append(CHAIN_FREQ0 + rng.random(12) * 45e6)
    t, w, f = np.maximum(np.concatenate(ticks), 0), np.concatenate(who), np.concatenate(freq)
    p = rng.permutation(t.size)
    pdws = np.zeros(t.size, PDW_DTYPE)
    pdws["toa"], pdws["freq"], pdws["pw"], pdws["snr"], pdws["mag"] = t[p] / CHAIN_RATE, f[p], 1e-6, 20.0, 1.0
    return pdws, w[p], periods


def reference_chain(pdws, deint: DR.Cfg, rate, step_hz, freq0, cells_u, cluster: R.Cfg):
    """The chain on the restatements alone: (emitters as (cluster, record) pairs, labels in the table's order, the
    clusters' records, the summed stats)"""
    ticks, by_time = DR.ticks_from_toa(pdws["toa"], float(pdws["toa"].min()), rate)
    items = R.items_from_pdws(pdws[by_time], freq0, step_hz)
    rec, labels, order, offsets, _, G = R.run(items, cluster)
    out, lab = [], np.full(len(pdws), -1, np.int32)
    total = dict(rounds=0, candidates_tried=0, candidates_refused=0, pulses_assigned=0)
    for k in range(G):
        mine = order[offsets[k]:offsets[k + 1]].astype(np.int64)
        r, sub, st = DR.run(ticks[mine], deint)
        hit = sub >= 0
        lab[by_time[mine[hit]]] = len(out) + sub[hit]
        out += [(k, x) for x in r]
        for key in total:
            total[key] += st[key]
    return out, lab, rec, total
