"""Designed inputs of the PDW association: small lists that sit on one sentence of the definition each, the lists at the
tile and tier boundaries, and the measured scene of a channelized chirp and edge tone (15 and 10 rows a pulse) tiled to
any length.  CASES maps a name to a function that returns (items, Cfg); expected(name) is the restatement's result,
computed once."""
import functools

import numpy as np

import assoc_ref as R

TILE = 256            # pfb_assoc_plan.tile_items
LDS_WINDOW = 1024     # pfb_assoc_plan.lds_window
INT_MIN, INT_MAX = -(1 << 31), (1 << 31) - 1


def rows(*r):
    """items from (start, length, cell[, weight]) tuples, in the order given"""
    return R.items([x[0] for x in r], [x[1] for x in r], [x[2] for x in r], [x[3] if len(x) > 3 else 1.0 for x in r])


# -- the measured scene ------------------------------------------------------------------------------------------------
PRI, PULSE = 400, 40                      # frames: 22 400 and 2240 samples of a 56-channel bank at decimation 56
CHIRP_ROWS, TONE_ROWS = 15, 10


def chirp_rows(p):
    """a chirp through cells 30 .. 36: seven dwells that follow one another, four one-frame rows at each edge"""
    out = [(p + s, n, 30 + k, 0.2 + 0.1 * (3 - abs(k - 3))) for k, (s, n) in
           enumerate(((0, 7), (6, 7), (12, 7), (18, 7), (24, 6), (29, 6), (34, 6)))]
    out += [(p, 1, c, 0.01) for c in (29, 28, 27, 26)] + [(p + PULSE - 1, 1, c, 0.01) for c in (37, 38, 39, 40)]
    return out


def tone_rows(p, upper):
    """a tone on the edge of cells 20 and 21: two full rows, two one-frame rows on each side at each edge"""
    out = [(p, PULSE, 20, 0.30 if not upper else 0.29), (p, PULSE, 21, 0.29 if not upper else 0.30)]
    for at in (p, p + PULSE - 1):
        out += [(at, 1, c, 0.01) for c in (19, 18, 22, 23)]
    return out


def scene(n_items):
    """the first n_items rows of the alternating train, sorted stably by start; also the pulse of every row"""
    out, who = [], []
    pulse = 0
    while len(out) < n_items:
        r = chirp_rows(pulse * PRI) if pulse % 2 == 0 else tone_rows(pulse * PRI, (pulse // 2) % 2 == 1)
        out += r
        who += [pulse] * len(r)
        pulse += 1
    it = rows(*out)
    order = np.argsort(it["start"], kind="stable")
    return it[order][:n_items], np.array(who)[order][:n_items]


SCENE = R.Cfg(Rc=1, g=0, K=8)


# -- one sentence each -------------------------------------------------------------------------------------------------
def at_distance(K, d, Rc=1):
    """item 0 lies over everything; d - 1 items in cells of their own follow, then one in item 0's cell: a link at
    distance d exactly, and nothing else"""
    r = [(0, 100, 0)] + [(1, 0, 1000 + 10 * k) for k in range(d - 1)] + [(1, 0, 0)]
    return rows(*r), R.Cfg(Rc=Rc, g=0, K=K)


def slack(g, over):
    return rows((5, 10, 3), (15 + g + over, 4, 3)), R.Cfg(Rc=0, g=g, K=4)


def staircase(n):
    return rows(*[(10 * k, 10, k) for k in range(n)]), R.Cfg(Rc=1, g=0, K=4)


def star(K):
    """one long item over K followers that do not touch one another"""
    return rows((0, 10 * K + 100, 0, 2.0), *[(10 * k + 1, 5, 64 if k % 2 else -64, 1.0) for k in range(K)]), R.Cfg(Rc=64, g=0, K=K)


def backward(m=40):
    """m items in odd cells, not linked to one another, then m - 1 in the even cells between them, each over two: the
    smallest label reaches the later odd cells only through items that come after them"""
    r = [(k, 1000, 5 + 2 * k) for k in range(m)] + [(m + k, 1000, 6 + 2 * k) for k in range(m - 1)]
    return rows(*r), R.Cfg(Rc=1, g=0, K=2 * m)


def weights():
    nan, inf = float("nan"), float("inf")
    neg_nan = np.array([0xffc00000], np.uint32).view(np.float32)[0]
    groups = [(1.0, 1.0, 1.0), (-0.0, 0.0), (0.0, -0.0), (-inf, -1e30), (inf, nan), (nan, inf), (neg_nan, -inf),
              (-1.0, -2.0, -1.0), (0.5, 3e38, 3e38), (1e-45, 0.0)]
    r = []
    for k, ws in enumerate(groups):
        r += [(100 * k, 10, 7, w) for w in ws]
    it = rows(*r)
    return it, R.Cfg(Rc=0, g=0, K=4)


def full_range():
    top = (1 << 62) - (1 << 33)
    big = (1 << 32) - 1
    g = (1 << 31) - 1
    r = [(0, big, 1), (5, big, 1), (1 << 61, big, -2), ((1 << 61) + 7, big, -3), ((1 << 61) + 9, big, -2),
         (top - 3, big, 0), (top - 3, big, 1), (top - 1, big, 0), (top - 1, 0, 1), (top - 1, big, 1)]
    return rows(*r), R.Cfg(Rc=1, g=g, K=16)


def random_list(seed, n, K=6, Rc=1, g=2, cells=6, span=4):
    rng = np.random.default_rng(seed)
    start = np.sort(rng.integers(0, max(1, span * n), n)).astype(np.uint64)
    it = R.items(start, rng.integers(0, 12, n), rng.integers(-cells, cells, n), rng.integers(0, 4, n).astype(np.float32))
    return it, R.Cfg(Rc=Rc, g=g, K=K)


CASES = {
    "n_0": lambda: (rows(), R.Cfg()),
    "n_1": lambda: (rows((7, 3, 2)), R.Cfg()),
    "n_2": lambda: (rows((7, 3, 2), (9, 3, 3)), R.Cfg()),
    "n_2_apart": lambda: (rows((7, 3, 2), (11, 3, 3)), R.Cfg()),
    "tile_less_1": lambda: (scene(TILE - 1)[0], SCENE),
    "tile": lambda: (scene(TILE)[0], SCENE),
    "tile_plus_1": lambda: (scene(TILE + 1)[0], SCENE),
    "tiles_3_plus_1": lambda: (scene(3 * TILE + 1)[0], SCENE),
    "k1_at_1": lambda: at_distance(1, 1),
    "k1_at_2": lambda: at_distance(1, 2),
    "k7_at_7": lambda: at_distance(7, 7),
    "k7_at_8": lambda: at_distance(7, 8),
    "lds_window_at_k": lambda: at_distance(LDS_WINDOW, LDS_WINDOW),
    "lds_window_at_k_plus_1": lambda: at_distance(LDS_WINDOW, LDS_WINDOW + 1),
    "global_window_at_k": lambda: at_distance(LDS_WINDOW + 1, LDS_WINDOW + 1),
    "global_window_at_k_plus_1": lambda: at_distance(LDS_WINDOW + 1, LDS_WINDOW + 2),
    "window_4096": lambda: at_distance(4096, 4096),
    "slack_0_at": lambda: slack(0, 0),
    "slack_0_over": lambda: slack(0, 1),
    "slack_large_at": lambda: slack((1 << 31) - 1, 0),
    "slack_large_over": lambda: slack((1 << 31) - 1, 1),
    "cells_at_reach": lambda: (rows((0, 9, 5), (1, 9, 8), (100, 9, -7), (101, 9, -4), (200, 9, -1), (201, 9, 2)), R.Cfg(Rc=3, K=4)),
    "cells_over_reach": lambda: (rows((0, 9, 5), (1, 9, 9), (100, 9, -7), (101, 9, -3), (200, 9, -2), (201, 9, 2)), R.Cfg(Rc=3, K=4)),
    "cells_extreme": lambda: (rows((0, 9, INT_MIN), (1, 9, INT_MAX), (2, 9, INT_MIN + 64), (3, 9, INT_MAX - 65)), R.Cfg(Rc=64, K=4)),
    "reach_0_split_pulse": lambda: (rows((0, 10, 4), (10, 10, 4), (20, 10, 5), (31, 10, 5)), R.Cfg(Rc=0, K=4)),
    "staircase": lambda: staircase(3 * TILE + 1),
    "star": lambda: star(300),
    "backward": lambda: backward(),
    "duplicates": lambda: (rows(*([(5, 4, 1, 2.0)] * 5 + [(6, 4, 9, 1.0)] * 3 + [(50, 0, 1, 0.0)] * 4)), R.Cfg(Rc=0, K=8)),
    "weights": weights,
    "full_range": full_range,
    "random_dense": lambda: random_list(11, 2 * TILE + 37, K=12, span=1),
    "random_sparse": lambda: random_list(12, 2 * TILE + 37, K=3, span=6),
}
BIG = 1 << 20


@functools.lru_cache(maxsize=None)
def inputs(name):
    if name == "big":
        return scene(BIG)[0], SCENE
    return CASES[name]()


@functools.lru_cache(maxsize=None)
def expected(name):
    """(records, labels, stats, (first_link, link_count)) of the restatement; computed once, never changed"""
    it, c = inputs(name)
    assert R.acceptable(it[:4096], c)
    return R.run(it, c) + (R.links(it, c),)
