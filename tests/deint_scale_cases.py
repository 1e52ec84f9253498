"""Designed inputs of the deinterleaver's tests at the list sizes it accepts (test_deint_scale_cpu.py,
test_gpu_deint_scale.py): lists of 2^18 to 2^20 pulses, each the smallest that reaches one path of pfb_deint.hip that
only a long list takes, and the small lists that walk the second search among duplicates.  Every case is (ticks, Cfg);
the expected figures come from deint_ref, computed once per case and shared, and are not written to."""
import functools

import numpy as np

import deint_cases as DC
import deint_ref as R

TILE = DC.TILE
# The boundaries the lists sit on.  pfb_deint_plan does not report them, so they are pinned here, each with the place in
# csrc/pfb_deint.hip it restates; test_deint_scale_cpu.py holds them to one another.
SCAN_WAVE = 256               # deint_scan: a lane takes counts[threadIdx.x * 4 + k], k < 4, and a wave of block_scan has 64
ARGMAX_STRIDE = 1024 * 256    # run(): deint_argmax is launched with min(.., 1024u) workgroups of kThreads = 256 lanes
MAX_PULSES = 1 << 20          # kMaxPulses, check_list()'s n > kMaxPulses
MAX_ROUNDS = 20               # kMaxRounds: the jump tables level_bytes() allocates


def frozen(a):
    a.setflags(write=False)
    return a


# -- 1. one chain of the longest list ----------------------------------------------------------------------------------
CHAIN_TAU = 100


def chain_edge_lengths():
    """chains around 2^18 pulses: the doubling rounds go from 18 to 19, and hops == 2^rounds is deint_mark_tables' and
    the doubling's special case"""
    return [(1 << 18) + d for d in (-1, 0, 1, 2)]


# -- 2. four trains, 2^20 pulses ---------------------------------------------------------------------------------------
FOUR_PERIODS = (2001, 2667, 3333, 4001)
FOUR = R.Cfg(pmin=1000, pmax=9000, W=4, Lv=16, detect=30, min_pulses=8, X=4, tol=5, fill=50, max_emitters=64)
FOUR_W1 = R.Cfg(pmin=1000, pmax=9000, W=1, Lv=16, detect=30, min_pulses=8, X=4, tol=5, fill=50, max_emitters=64)
FOUR_WIDE = R.Cfg(pmin=1000, pmax=1000 + 65535, W=1, Lv=16, detect=30, min_pulses=8, X=4, tol=5, fill=50, max_emitters=64)
FOUR_SEED = 20


@functools.lru_cache(maxsize=None)
def four_trains():
    """2^20 ticks: the four periods at a random phase each, jitter -1 .. 1, nothing dropped, 2 % strays"""
    n = MAX_PULSES
    rng = np.random.default_rng(FOUR_SEED)
    rate = sum(1.0 / p for p in FOUR_PERIODS) / 0.98
    span = int(n / rate * 1.05)
    parts = []
    for p in FOUR_PERIODS:
        k = np.arange((span - 1) // p)
        parts.append(int(rng.integers(0, p)) + k * p + rng.integers(-1, 2, k.size))
    parts.append(rng.integers(0, span, n // 50))
    t = np.sort(np.maximum(np.concatenate(parts), 0))
    assert len(t) >= n
    return frozen(t[:n].astype(np.uint64))


# -- 3. the scan's edges: 5 tiles (the scan's second lane), then the last and first tile of each of its waves ----------
SCAN_EDGES = (4 * TILE + 1, SCAN_WAVE * TILE, SCAN_WAVE * TILE + 1, 2 * SCAN_WAVE * TILE + 1, 3 * SCAN_WAVE * TILE + 1)


# -- 4. a winner past the argmax's first stride ------------------------------------------------------------------------
LATE = R.Cfg(pmin=900, pmax=2000, W=1, Lv=4, detect=1, min_pulses=8, X=1, tol=2, fill=50, max_emitters=4)
LATE_LONG, LATE_PAIR = 300000, 150000


def winner_list(late: bool):
    """a train at period 1777 and, apart from it in time, two interleaved trains at period 1003, 400 ticks from one
    another: the two equally long chains of the first candidate lie after (late) or before the long train"""
    def pair(start):
        return np.sort(np.concatenate([DC.train(1003, LATE_PAIR, start), DC.train(1003, LATE_PAIR, start + 400)]))
    gap = 50000
    if late:
        long_ = DC.train(1777, LATE_LONG, 0)
        return frozen(np.concatenate([long_, pair(int(long_[-1]) + gap)]))
    two = pair(0)
    return frozen(np.concatenate([two, DC.train(1777, LATE_LONG, int(two[-1]) + gap)]))


# -- 5. successors far on, in dense lists ------------------------------------------------------------------------------
DENSE = R.Cfg(pmin=1000, pmax=9000, W=4, Lv=16, min_pulses=8, X=8, tol=0)
DENSE_N = 300000
DENSE_A_TAUS = (1001, 9000, 60000)
DENSE_B_TAU = 9000
SLICE = 3000                  # the first and last pulses of a dense list that the literal loops can afford


@functools.lru_cache(maxsize=None)
def dense(which):
    """'a': neighbours 0 .. 3 ticks apart, every window full; 'b': 0 .. 59 apart, windows sometimes empty, but never
    the eighth (65 ticks wide); 'c': 0 .. 99 apart, so that the ninth and last window is reached too"""
    rng = np.random.default_rng({"a": 31, "b": 32, "c": 33}[which])
    return frozen(np.cumsum(rng.integers(0, {"a": 4, "b": 60, "c": 100}[which], DENSE_N)).astype(np.uint64))


RUN_FROM, RUN_AHEAD, RUN_LEN = 100000, 20000, 5000


@functools.lru_cache(maxsize=None)
def dense_run():
    """(ticks, tau, i, j): list 'a' with a run of 5000 equal ticks 20000 entries after pulse i, alone in i's first
    window at period tau and one tick under its target, so succ(i) is the lowest index of the run, j"""
    t = dense("a").copy()
    at = RUN_FROM + RUN_AHEAD
    v = t[at]
    t[at:at + RUN_LEN] = v
    t[at + RUN_LEN:] += np.uint64(2 * DENSE.e)          # nothing at or over the target inside the window
    j = int(np.searchsorted(t, v, "left"))
    return frozen(t), int(v) + 1 - int(t[RUN_FROM]), RUN_FROM, j


# -- 6. runs of duplicates under the target ----------------------------------------------------------------------------
DUP = R.Cfg(pmin=50, pmax=400, W=1, Lv=4, min_pulses=3, X=2, tol=2)
DUP_TAU = 100
DUP_FILLS, DUP_RUNS, DUP_OFFS = (0, 7, 8, 9, 23, 24, 25, 40), (2, 8, 9, 10, 24, 25, 100), (-2, -1, 0, 2)


def duplicate_list(fill, run, off, tau=DUP_TAU):
    """a pulse at 0, `fill` pulses that lie in none of its windows, `run` copies of tau + off, one pulse at tau + 2 and
    three at 2 tau + off: the lowest of the run is found `fill` entries after the pulse and `run` before the end of
    the search"""
    t = [0] + [3 + k % 40 for k in range(fill)] + [tau + off] * run + [tau + 2] + [2 * tau + off] * 3
    return np.sort(np.array(t, np.uint64))


@functools.lru_cache(maxsize=None)
def duplicate_lists():
    """((fill, run, off), ticks, deint_ref.lengths, deint_ref.literal_successors) of every combination"""
    out = []
    for fill in DUP_FILLS:
        for run in DUP_RUNS:
            for off in DUP_OFFS:
                t = frozen(duplicate_list(fill, run, off))
                out.append(((fill, run, off), t, R.lengths(t, DUP, DUP_TAU), R.literal_successors(t, DUP, DUP_TAU)))
    return out


# -- the cases and what the restatement makes of them ------------------------------------------------------------------
CASES = {
    "one_chain_max": lambda: (frozen(DC.train(CHAIN_TAU, MAX_PULSES, 11)), DC.SMALL),
    "four_trains_max": lambda: (four_trains(), FOUR),
    **{f"scan_edge_{n}": (lambda n=n: (four_trains()[:n], FOUR)) for n in SCAN_EDGES},
    "late_winner": lambda: (winner_list(True), LATE),
    "early_winner": lambda: (winner_list(False), LATE),
    "short_on_long_handle": lambda: (DC.CASES["group_257"]()[0], FOUR),     # its ticks alone, under the long list's settings
}


@functools.lru_cache(maxsize=None)
def case(name):
    return CASES[name]()


@functools.lru_cache(maxsize=None)
def expected(name):
    """deint_ref.run of a named case: (records, labels, stats)"""
    rec, labels, stats = R.run(*case(name))
    return frozen(rec), frozen(labels), stats


@functools.lru_cache(maxsize=None)
def expected_histogram(name, c=None):
    t, own = case(name)
    return frozen(R.histogram(t, own if c is None else c))


@functools.lru_cache(maxsize=None)
def expected_lengths(name, tau):
    """deint_ref.lengths of a named case or a dense list at one period: (succ, step, len)"""
    if name == "dense_run":
        t, c = dense_run()[0], DENSE
    elif name.startswith("dense_"):
        t, c = dense(name[-1]), DENSE
    else:
        t, c = case(name)
    return tuple(frozen(x) for x in R.lengths(t, c, tau))


def alive_before_round(labels, r):
    """the original indices alive when round r = 1, 2, .. begins, for a run that accepted one record in each round
    before r: record E leaves in round E + 1"""
    return np.nonzero((labels < 0) | (labels >= r - 1))[0]
