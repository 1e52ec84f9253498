"""The PDW deinterleaver restated in numpy from the definition in include/pfb_channelizer.h (pfb_deint_*), sentence by
sentence: the difference histogram, the candidate rule, the successor windows, the chains, the rounds.  Every figure
is an integer (the record's period is one IEEE division), so the device is held to these bytes.  The literal_* forms
are the plain loops the vectorised ones are tested against (test_deint_cpu.py)."""
from dataclasses import dataclass

import numpy as np

EMITTER = np.dtype([("first_tick", "u8"), ("last_tick", "u8"), ("period", "f8"), ("pulses", "u4"), ("periods", "u4"),
                    ("bin", "u4"), ("candidate_period", "u4"), ("first_pulse", "u4"), ("hist_count", "u4")])


@dataclass(frozen=True)
class Cfg:
    pmin: int
    pmax: int
    W: int = 1
    Lv: int = 16
    detect: int = 30
    min_pulses: int = 8
    X: int = 4
    tol: int = 0
    fill: int = 50
    max_emitters: int = 64

    @property
    def NB(self) -> int:
        return (self.pmax - self.pmin) // self.W + 1

    @property
    def e(self) -> int:
        return self.tol if self.tol else self.W

    def tau(self, k: int) -> int:
        return self.pmin + k * self.W + self.W // 2

    def settings(self) -> dict:
        """the keyword arguments of sdr_channelizer_amd.Deinterleaver after (min_period, max_period, bin_ticks)"""
        return dict(max_level=self.Lv, detect_percent=self.detect, min_pulses=self.min_pulses, max_missing=self.X,
                    tolerance=self.tol, fill_percent=self.fill, max_emitters=self.max_emitters)


def ticks(a) -> np.ndarray:
    return np.ascontiguousarray(a, np.uint64).reshape(-1)


# -- step 1 ------------------------------------------------------------------------------------------------------------
def histogram(a, c: Cfg) -> np.ndarray:
    a = ticks(a)
    C = np.zeros(c.NB, np.int64)
    for level in range(1, min(c.Lv, max(a.size - 1, 0)) + 1):
        d = (a[level:] - a[:-level]).astype(np.int64)      # a tick is under 2^62
        d = d[(d >= c.pmin) & (d <= c.pmax)]
        if d.size:
            C += np.bincount((d - c.pmin) // c.W, minlength=c.NB)
    return C.astype(np.uint32)


def literal_histogram(a, c: Cfg) -> np.ndarray:
    a = [int(v) for v in ticks(a)]
    C = [0] * c.NB
    for i in range(len(a)):
        for j in range(i + 1, len(a)):
            if 1 <= j - i <= c.Lv:
                d = a[j] - a[i]
                if c.pmin <= d <= c.pmax:
                    C[(d - c.pmin) // c.W] += 1
    return np.array(C, np.uint32)


# -- step 2 ------------------------------------------------------------------------------------------------------------
def needed(c: Cfg, span: int, k: int) -> int:
    """the three-bin sum bin k must reach"""
    return max(c.min_pulses - 1, -((-(span // c.tau(k)) * c.detect) // 100))


def is_candidate(C, c: Cfg, span: int, k: int) -> bool:
    left = int(C[k - 1]) if k > 0 else 0
    right = int(C[k + 1]) if k + 1 < len(C) else 0
    here = int(C[k])
    return here > left and here >= right and left + here + right >= needed(c, span, k)


def candidates(C, c: Cfg, span: int) -> list:
    """(k, tau_k, S_k) of every candidate bin, k ascending"""
    C = np.asarray(C).astype(np.int64)
    padded = np.concatenate([[0], C, [0]])
    left, right = padded[:-2], padded[2:]
    rough = np.nonzero((C > left) & (C >= right) & (left + C + right >= c.min_pulses - 1))[0]
    return [(int(k), c.tau(int(k)), int(left[k] + C[k] + right[k])) for k in rough if is_candidate(C, c, span, int(k))]


# -- step 3 ------------------------------------------------------------------------------------------------------------
def successors(a, c: Cfg, tau: int):
    """(succ, step): int32, -1 and 0 where a pulse has no successor"""
    a = ticks(a)
    n = a.size
    succ, step = np.full(n, -1, np.int32), np.zeros(n, np.int32)
    me = np.arange(n)
    for m in range(c.X + 1):
        todo = np.nonzero(succ < 0)[0]
        if not todo.size:
            break
        target = a[todo] + np.uint64((m + 1) * tau)
        w = np.uint64((m + 1) * c.e)
        lo = np.maximum(np.searchsorted(a, target - w, "left"), me[todo] + 1)   # the window: indices [lo, hi)
        hi = np.searchsorted(a, target + w, "right")
        at = np.clip(np.searchsorted(a, target, "left"), lo, hi)                  # the first of them at or over the target
        over_ok = at < hi
        over_d = np.where(over_ok, a[np.minimum(at, n - 1)] - target, np.uint64(0))
        under_ok = at > lo
        v = a[np.maximum(at - 1, 0)]                                              # the largest under the target ...
        under_j = np.maximum(np.searchsorted(a, v, "left"), lo)                   # ... at its lowest index in the window
        under_d = np.where(under_ok, target - v, np.uint64(0))
        take_under = under_ok & (~over_ok | (under_d <= over_d))                  # a tie goes to the lower index
        take_over = over_ok & ~take_under
        j = np.where(take_under, under_j, at)
        got = take_under | take_over
        succ[todo[got]] = j[got]
        step[todo[got]] = m + 1
    return succ, step


def literal_successors(a, c: Cfg, tau: int):
    a = [int(v) for v in ticks(a)]
    succ, step = [-1] * len(a), [0] * len(a)
    for i in range(len(a)):
        for m in range(c.X + 1):
            target, w = a[i] + (m + 1) * tau, (m + 1) * c.e
            best = None
            for j in range(i + 1, len(a)):
                if target - w <= a[j] <= target + w and (best is None or abs(a[j] - target) < abs(a[best] - target)):
                    best = j
            if best is not None:
                succ[i], step[i] = best, m + 1
                break
    return np.array(succ, np.int32), np.array(step, np.int32)


# -- step 4 ------------------------------------------------------------------------------------------------------------
def chains(succ, step):
    """(len, per, end) of every pulse: a successor lies further on, so one pass from the back"""
    n = len(succ)
    ln, per, end = np.ones(n, np.int32), np.zeros(n, np.int32), np.arange(n, dtype=np.int32)
    for i in range(n - 1, -1, -1):
        s = succ[i]
        if s >= 0:
            ln[i], per[i], end[i] = 1 + ln[s], step[i] + per[s], end[s]
    return ln, per, end


def literal_chain(succ, step, i: int):
    """(len, per, end, the pulses) of the chain that starts at i, by walking it"""
    walk, per = [i], 0
    while succ[walk[-1]] >= 0:
        per += int(step[walk[-1]])
        walk.append(int(succ[walk[-1]]))
    return len(walk), per, walk[-1], walk


def accepted(c: Cfg, ln: int, per: int) -> bool:
    return ln >= c.min_pulses and 100 * (ln - 1) >= c.fill * per


# -- the rounds --------------------------------------------------------------------------------------------------------
def run(t, c: Cfg):
    """(records, labels, stats) of the whole search"""
    t = ticks(t)
    labels = np.full(t.size, -1, np.int32)
    records = []
    stats = dict(rounds=0, candidates_tried=0, candidates_refused=0, pulses_assigned=0)
    while len(records) < c.max_emitters:
        idx = np.nonzero(labels < 0)[0]
        a = t[idx]
        if a.size < c.min_pulses:
            break
        C = histogram(a, c)
        stats["rounds"] += 1
        span = int(a[-1]) - int(a[0])
        for k, tau, S in candidates(C, c, span):
            stats["candidates_tried"] += 1
            succ, step = successors(a, c, tau)
            ln, per, end = chains(succ, step)
            b = int(np.argmax(ln))                         # the first of the largest
            if not accepted(c, int(ln[b]), int(per[b])):
                stats["candidates_refused"] += 1
                continue
            walk = literal_chain(succ, step, b)[3]
            labels[idx[walk]] = len(records)
            first, last = int(a[b]), int(a[end[b]])
            rec = np.zeros((), EMITTER)
            rec["first_tick"], rec["last_tick"] = first, last
            rec["period"] = np.float64(last - first) / np.float64(int(per[b]))
            rec["pulses"], rec["periods"], rec["bin"], rec["candidate_period"] = int(ln[b]), int(per[b]), k, tau
            rec["first_pulse"], rec["hist_count"] = int(idx[b]), S
            records.append(rec)
            stats["pulses_assigned"] += int(ln[b])
            break
        else:
            break
    return (np.array(records, EMITTER) if records else np.zeros(0, EMITTER)), labels, stats


def lengths(a, c: Cfg, tau: int):
    """what pfb_deint_successors returns: (succ, step, len)"""
    succ, step = successors(a, c, tau)
    return succ, step, chains(succ, step)[0]


def ticks_from_toa(toa, t0: float, rate: float):
    """(ticks, order) of pfb_deint_ticks_from_toa: to nearest, ties to even, then a stable sort"""
    tick = np.rint((np.asarray(toa, np.float64) - np.float64(t0)) * np.float64(rate))
    order = np.argsort(tick, kind="stable").astype(np.uint32)
    return tick[order].astype(np.uint64), order
