"""Fractional-period epoch folding and the regridder restated in numpy from the header comment of
include/pfb_channelizer.h (pfb_qfold_*, pfb_regrid_*), not from the device code.  Everything wider than 64 bits is a
Python int; the float32 profile is added one cell at a time in index order (np.add.at is sequential and unbuffered);
counts by the closed form; the score record over the used bins.  `literal_*` are the same sentences as per-cell Python
loops, which test_qfold_cpu.py holds the restatement to.  A support module, not a test."""
from fractions import Fraction

import numpy as np

import fold_ref

ONE = 1 << 32
SCORE = np.dtype([("period_q32", "u8"), ("num_bins", "u4"), ("bins_used", "u4"), ("peak_bin", "u4"), ("reserved", "u4"),
                  ("peak_cells", "u8"), ("peak_sum", "f4"), ("peak_mean", "f4"), ("sum_means", "f8"),
                  ("sum_sq_means", "f8"), ("cells", "u8")])
EXACT = [n for n in SCORE.names if n not in ("sum_means", "sum_sq_means")]   # compared byte for byte
SHARED = ["num_bins", "bins_used", "peak_bin", "reserved", "peak_cells", "peak_sum", "peak_mean", "cells"]  # with pfb_fold_score

same_floats, spread_stream, z = fold_ref.same_floats, fold_ref.spread_stream, fold_ref.z


def q32(x):
    """samples (int, Fraction, or a decimal string) as the Q32 integer, rounded to nearest"""
    return int(round(Fraction(x) * ONE))


def start(m, Pq):
    """ceil(m Pq / 2^32)"""
    return -((-int(m) * int(Pq)) >> 32)


def period_of(i, Pq):
    """floor(i 2^32 / Pq): the largest m with start(m) <= i"""
    return (int(i) << 32) // int(Pq)


def num_bins(Pq, C):
    return (int(Pq) >> 32) // C


def bins(i0, n, Pq, C):
    """bins of the cells with global indices i0 .. i0 + n - 1"""
    if n == 0:
        return np.zeros(0, np.int64)
    m0, m1 = period_of(i0, Pq), period_of(i0 + n - 1, Pq)
    starts = np.array([start(m, Pq) - i0 for m in range(m0, m1 + 2)], np.int64)    # relative to i0: small numbers
    first = np.clip(starts[:-1], 0, n)
    reps = np.clip(starts[1:], 0, n) - first
    off = np.arange(n, dtype=np.int64) - np.repeat(starts[:-1], reps)
    return np.minimum(off // C, num_bins(Pq, C) - 1)


def fold(p, Pq, C, first=0, profile=None):
    """the profile after cells p (global indices first ..) have been added to `profile` (None: all +0), float32"""
    F = np.zeros(num_bins(Pq, C), np.float32) if profile is None else np.array(profile, np.float32)
    p = np.asarray(p, np.float32)
    with np.errstate(all="ignore"):
        np.add.at(F, bins(first, len(p), Pq, C), p)
    return F


def cells_before(N, Pq, C):
    """n_j(N): (M - 1) C + clamp(N - start(M - 1) - j C, 0, C) for j < NB - 1, the rest in the last bin.  M and
    start(M - 1) are Python ints; every n_j is at most N <= 2^62 and fits int64"""
    NB = num_bins(Pq, C)
    out = np.zeros(NB, np.int64)
    if N == 0:
        return out
    M = period_of(N - 1, Pq) + 1
    rel = N - start(M - 1, Pq)
    out[:-1] = (M - 1) * C + np.clip(rel - np.arange(NB - 1, dtype=np.int64) * C, 0, C)
    out[-1] = N - int(out[:-1].sum())
    return out


def counts(N, Pq, C, N0=0):
    """the handle's counts after set_index(N0) and N - N0 cells: uint64"""
    return (cells_before(N, Pq, C) - cells_before(N0, Pq, C)).astype(np.uint64)


def _means(F, n):
    used = np.flatnonzero(n > 0)
    with np.errstate(all="ignore"):
        return used, F[used].astype(np.float64) / n[used].astype(np.float64)


def score(F, N, Pq, C, N0=0):
    """the record of one candidate after set_index(N0) and cells N0 .. N - 1"""
    rec = np.zeros((), SCORE)
    rec["period_q32"], rec["num_bins"], rec["cells"] = Pq, num_bins(Pq, C), N - N0
    n = counts(N, Pq, C, N0)
    used, m = _means(F, n)
    rec["bins_used"] = len(used)
    if len(used) == 0:
        return rec
    with np.errstate(all="ignore"):
        k = 0 if np.isnan(m[0]) else int(np.nanargmax(m))   # the walk of literal_peak over the used bins
        best = int(used[k])
        rec["peak_bin"], rec["peak_cells"] = best, n[best]
        rec["peak_sum"], rec["peak_mean"] = F[best], np.float32(m[k])
        rec["sum_means"], rec["sum_sq_means"] = m.sum(), (m * m).sum()
    return rec


def sums_bound(F, N, Pq, C, N0=0):
    """(bound on sum_means, bound on sum_sq_means): (bins_used + 1) 2^-53 sum |terms|; inf where a term is not finite"""
    used, m = _means(F, counts(N, Pq, C, N0))
    if len(used) == 0:
        return 0.0, 0.0
    with np.errstate(all="ignore"):
        if not np.isfinite(m).all() or not np.isfinite(m * m).all():
            return np.inf, np.inf
        return (len(used) + 1) * 2.0 ** -53 * np.abs(m).sum(), (len(used) + 1) * 2.0 ** -53 * (m * m).sum()


def same_record(got, want, bound):
    """got is want: byte for byte (NaNs as in same_floats) but for the two float64 sums, which lie within `bound` (or
    are both not finite)"""
    for name in EXACT:
        if SCORE[name].kind == "f":
            if not same_floats(got[name], want[name]):
                return False
        elif np.asarray(got[name]).tobytes() != np.asarray(want[name]).tobytes():
            return False
    for name, b in zip(("sum_means", "sum_sq_means"), bound):
        g, w = float(got[name]), float(want[name])
        if np.isfinite(b) and np.isfinite(w):
            if not abs(g - w) <= b:
                return False
        elif np.isfinite(g):
            return False
    return True


class Walk:
    """the restatement taken along a stream cut at any points: profiles held per candidate, records on demand"""

    def __init__(self, periods_q32, C, N0=0):
        self.periods, self.C = [int(q) for q in periods_q32], C
        self.seek(N0)

    def seek(self, N0):
        self.N0 = self.N = N0
        self.F = [np.zeros(num_bins(q, self.C), np.float32) for q in self.periods]

    def take(self, p):
        self.F = [fold(p, q, self.C, self.N, F) for q, F in zip(self.periods, self.F)]
        self.N += len(p)

    def records(self):
        return np.array([score(F, self.N, q, self.C, self.N0) for F, q in zip(self.F, self.periods)], SCORE)

    def bounds(self):
        return [sums_bound(F, self.N, q, self.C, self.N0) for F, q in zip(self.F, self.periods)]


# -- the regridder --------------------------------------------------------------------------------------------------
def regrid_source(t, Pq, R, origin):
    """the input index of output element t = k R + r: origin + start(k) + r"""
    k, r = divmod(int(t), R)
    return origin + start(k, Pq) + r


def regrid_before(X, Pq, R, origin):
    """the output elements whose source lies before input element X (bisection on the definition)"""
    lo, hi = 0, max(X, 1) * R + R            # source(t) >= t / R ... a generous bracket: source(hi) >= X
    while regrid_source(hi, Pq, R, origin) < X:
        hi *= 2
    while lo < hi:
        mid = (lo + hi) // 2
        if regrid_source(mid, Pq, R, origin) < X:
            lo = mid + 1
        else:
            hi = mid
    return lo


def regrid(x, s, Pq, R, origin):
    """what a call with input x = elements [s, s + len(x)) writes: (first output index t0, the elements)"""
    t0, t1 = regrid_before(s, Pq, R, origin), regrid_before(s + len(x), Pq, R, origin)
    idx = np.array([regrid_source(t, Pq, R, origin) - s for t in range(t0, t1)], np.int64)
    return t0, np.asarray(x)[idx] if len(idx) else np.asarray(x)[:0]


def regrid_doppler(Pq, ND, fs, centered=False):
    d = np.arange(ND) - (ND // 2 if centered else 0)
    return d * fs / (ND * (Pq / ONE))


# -- the literal loops ------------------------------------------------------------------------------------------
def literal_fold(p, Pq, C, first=0):
    NB = (Pq >> 32) // C
    F = [np.float32(0.0)] * NB
    cnt = [0] * NB
    js = []
    with np.errstate(all="ignore"):
        for k in range(len(p)):
            i = first + k
            m = (i * ONE) // Pq
            s = (m * Pq + ONE - 1) // ONE
            j = min((i - s) // C, NB - 1)
            F[j] = np.float32(F[j] + np.float32(p[k]))
            cnt[j] += 1
            js.append(j)
    return np.array(F, np.float32), np.array(cnt, np.uint64), np.array(js, np.int64)


def literal_peak(m, used):
    """walk the used bins ascending, replace only on a strictly greater mean"""
    best = used[0]
    for j in used[1:]:
        if m[j] > m[best]:
            best = j
    return best
