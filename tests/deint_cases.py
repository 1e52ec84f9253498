"""Designed inputs of the deinterleaver's tests (test_deint_cpu.py, test_gpu_deint.py): the four-train scene and its
companions, and the small lists that sit on one sentence of the definition each.  Every case is (ticks, Cfg); the
expected figures come from deint_ref, computed once per case and shared."""
import functools

import numpy as np

import deint_ref as R

TILE = 1024          # pfb_deint_plan.tile_pulses
GROUP = 256          # pfb_deint_plan.successor_threads
LDS_BINS = 8192      # pfb_deint_plan.lds_bins

# -- the designed scene ------------------------------------------------------------------------------------------------
# Four trains in 2^21 ticks: PRI 2048, 3000, 3517 and a second 2048 that starts 1200 ticks after the first; every pulse
# jittered by -1 .. 1 ticks, one in ten dropped, 100 stray pulses.  tolerance = 5: two jittered neighbours differ by up
# to 2 ticks from the period, and a chain that has stepped onto a foreign pulse 3 ticks off must still find the next
# pulse of its train, 5 ticks off the target.
SCENE_TRAINS = ((2048, 300), (3000, 77), (3517, 1501), (2048, 1500))
SCENE_SPAN = 1 << 21
SCENE_STRAYS = 100
SCENE = R.Cfg(pmin=400, pmax=8000, W=4, Lv=16, detect=30, min_pulses=8, X=4, tol=5, fill=50, max_emitters=64)
SCENE_NO_FILL = R.Cfg(pmin=400, pmax=8000, W=4, Lv=16, detect=30, min_pulses=8, X=4, tol=5, fill=1, max_emitters=64)


def interleave(trains, span, strays, seed, drop=0.10, jitter=1, base=0):
    """(ticks, who): the trains' pulses and the strays in time order; who is the train of each pulse, -1 for a stray"""
    rng = np.random.default_rng(seed)
    t, who = [], []
    for e, (pri, off) in enumerate(trains):
        k = np.arange((span - off) // pri + 1)
        x = off + k * pri + (rng.integers(-jitter, jitter + 1, k.size) if jitter else 0)
        keep = rng.random(k.size) >= drop
        t.append(x[keep])
        who.append(np.full(int(keep.sum()), e))
    t.append(rng.integers(0, span, strays))
    who.append(np.full(strays, -1))
    t, who = np.maximum(np.concatenate(t), 0), np.concatenate(who)
    order = np.argsort(t, kind="stable")
    return (t[order].astype(np.uint64) + np.uint64(base)), who[order]


@functools.lru_cache(maxsize=None)
def scene():
    return interleave(SCENE_TRAINS, SCENE_SPAN, SCENE_STRAYS, 5)


@functools.lru_cache(maxsize=None)
def expected(name):
    """deint_ref.run of a named case: (records, labels, stats)"""
    t, c = CASES[name]() if name in CASES else NAMED[name]()
    return R.run(t, c)


def quality(who, records, labels):
    """per record (the train it is mostly made of, purity, the share of that train it holds), and the strays assigned"""
    rows = []
    for e in range(len(records)):
        mine = who[labels == e]
        vals, cnt = np.unique(mine, return_counts=True)
        top = int(vals[np.argmax(cnt)])
        rows.append((top, cnt.max() / mine.size, cnt.max() / max(int((who == top).sum()), 1)))
    return rows, int(((who == -1) & (labels >= 0)).sum())


# -- small lists -------------------------------------------------------------------------------------------------------
def train(period, n, start=0):
    return (start + period * np.arange(n)).astype(np.uint64)


def mix(n, seed, periods=(1210, 1777, 2391), span_per=100, dup=True, jitter=1, base=0, exact=True):
    """n pulses of a few trains with strays, drops and (dup) some duplicated ticks"""
    span = max(n * span_per * 10, 1 << 14)
    t = interleave([(p, 13 * (i + 1)) for i, p in enumerate(periods)], span, max(n // 20, 1), seed, jitter=jitter)[0]
    t = t[:n].copy()
    assert len(t) == n or not exact
    if dup and n > 8:
        t[n // 2] = t[n // 2 - 1]
        t[n // 3 + 1] = t[n // 3]
        t.sort()
    return t + np.uint64(base)


SMALL = R.Cfg(pmin=50, pmax=400, W=1, Lv=4, detect=30, min_pulses=5, X=1, tol=2, fill=50, max_emitters=8)
MIX = R.Cfg(pmin=1000, pmax=5000, W=2, Lv=12, detect=30, min_pulses=6, X=3, tol=5, fill=50, max_emitters=8)


def bins_case(nb):
    """a list for exactly nb bins of one tick: pmin = 1000"""
    c = R.Cfg(pmin=1000, pmax=1000 + nb - 1, W=1, Lv=12, detect=30, min_pulses=6, X=3, tol=5, fill=50, max_emitters=8)
    assert c.NB == nb

    def make():
        t = mix(1500, nb, periods=(1003, 1000 + min(nb, 2500) - 1, 1000 + min(nb, 1700) // 2))
        tail = t[-1] + np.cumsum([c.pmax - 1] * 8 + [c.pmax] * 8 + [c.pmax + 1] * 2).astype(np.uint64)   # the top bins
        return np.concatenate([t, tail]), c
    return make


BIG = 1 << 30        # periods over 2^30: ten of them span more than 2^32 ticks
WIDE = R.Cfg(pmin=BIG, pmax=BIG + (1 << 18) - 4, W=4, Lv=4, detect=30, min_pulses=5, X=1, tol=4, fill=50, max_emitters=4)
WIDE_PERIODS = (BIG + 2, BIG + (1 << 17) + 2)       # the middle ticks of bins 0 and 32768


def wide_list(base=0):
    a, b = train(WIDE_PERIODS[0], 12, 1000), train(WIDE_PERIODS[1], 9, 77)
    return np.sort(np.concatenate([a, b])).astype(np.uint64) + np.uint64(base)


FILL_STEPS = np.array([0, 100, 200, 300, 400, 600, 800], np.uint64)        # tau = 100: 6 hits in 8 periods = 75 %
FILL_BETTER = np.array([0, 100, 200, 300, 400, 500, 600, 800], np.uint64)  # one hit more: 7 in 8


def fill_cfg(percent):
    return R.Cfg(pmin=90, pmax=300, W=1, Lv=3, detect=30, min_pulses=5, X=1, tol=2, fill=percent, max_emitters=4)


CASES = {
    **{f"train_{n}": (lambda n=n: (train(100, n, 7), SMALL)) for n in (0, 1, 2, 4, 5)},
    **{f"tile_{n}": (lambda n=n: (mix(n, n), MIX)) for n in (TILE - 1, TILE, TILE + 1, TILE + MIX.Lv, 2 * TILE + 3)},
    **{f"group_{n}": (lambda n=n: (mix(n, n), MIX)) for n in (GROUP - 1, GROUP, GROUP + 1)},
    "one_bin": lambda: (np.sort(np.concatenate([train(100, 40, 5), train(100, 30, 61)])),
                        R.Cfg(pmin=100, pmax=100, W=1, Lv=4, detect=30, min_pulses=5, X=2, tol=0, fill=50, max_emitters=4)),
    **{f"bins_{nb}": bins_case(nb) for nb in (LDS_BINS - 1, LDS_BINS, LDS_BINS + 1, 65536)},
    "level_1": lambda: (mix(700, 3, periods=(1210,), span_per=200), R.Cfg(1000, 5000, 2, 1, 30, 6, 3, 5, 50, 8)),
    # 6 ticks between neighbours: every one of the 256 levels lies under pmax
    "level_256": lambda: (np.sort(np.concatenate([train(6, 1500, 0), mix(300, 9, span_per=3, dup=False, exact=False)])),
                          R.Cfg(1000, 5000, 2, 256, 30, 6, 3, 5, 50, 2)),
    "missing_0": lambda: (mix(900, 4), R.Cfg(1000, 5000, 2, 12, 30, 6, 0, 5, 50, 8)),
    "missing_8": lambda: (mix(900, 4), R.Cfg(1000, 5000, 2, 12, 30, 6, 8, 5, 50, 8)),
    "equal_chains": lambda: (np.sort(np.concatenate([train(100, 10, 0), train(100, 10, 37)])), SMALL),
    "duplicates": lambda: (np.repeat(train(100, 12, 3), 2), SMALL),
    "fill_at_boundary": lambda: (FILL_STEPS, fill_cfg(75)),
    "fill_refused": lambda: (FILL_STEPS, fill_cfg(76)),
    "fill_one_hit_better": lambda: (FILL_BETTER, fill_cfg(76)),
    "wide": lambda: (wide_list(), WIDE),
    "under_2_62": lambda: (wide_list((1 << 62) - 1 - int(wide_list()[-1])), WIDE),
    "max_emitters": lambda: (scene()[0], R.Cfg(**{**SCENE.__dict__, "max_emitters": 2})),
}
NAMED = {"scene": lambda: (scene()[0], SCENE), "scene_no_fill": lambda: (scene()[0], SCENE_NO_FILL)}


def chain_lists():
    """perfect trains of 2^k - 1 .. 2^k + 2 pulses: the doubling rounds change where the hops pass a power of two"""
    return [train(100, n, 11) for k in (1, 2, 3, 5, 10) for n in range((1 << k) - 1, (1 << k) + 3) if n >= 1]


def window_lists(c: R.Cfg, tau: int):
    """for every step m + 1: a pulse at each edge of the window and one tick outside it, and the ties"""
    out = []
    for m in range(c.X + 1):
        w = (m + 1) * c.e
        for off in (-w - 1, -w, w, w + 1):
            out.append(np.array([5, 5 + (m + 1) * tau + off, 5 + 40 * tau], np.uint64))
    out.append(np.array([0, tau - 2, tau + 2], np.uint64))                       # a tie: the lower index
    out.append(np.array([0, tau - 2, tau - 2, tau + 2, tau + 2], np.uint64))     # among duplicates the lowest
    out.append(np.array([0, 0, tau, tau, 2 * tau, 2 * tau, 2 * tau], np.uint64))  # a duplicate as the successor
    out.append(np.array([0, tau - 1, tau + 2, 2 * tau - 2, 2 * tau + 1], np.uint64))
    return out


def edge_list(c: R.Cfg):
    """neighbour differences of exactly pmin and pmax and one outside each, apart and summed over two levels"""
    gaps = [c.pmin - 1, c.pmin, c.pmax, c.pmax + 1, c.pmin, c.pmax - c.pmin, c.pmax - c.pmin + 1, 3 * c.pmax, c.pmin]
    return np.concatenate([[3], 3 + np.cumsum(gaps)]).astype(np.uint64)
