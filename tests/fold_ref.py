"""Epoch folding restated in numpy from the header comment of include/pfb_channelizer.h (pfb_fold_*), not from the
device code: bins by the formula, a float32 profile added one cell at a time in index order (np.add.at is sequential
and unbuffered), counts by the closed form, the score record.  `literal_*` are the same sentences as per-cell Python
loops, which test_fold_cpu.py holds the restatement to.  A support module, not a test."""
import numpy as np

SCORE = np.dtype([("period", "u4"), ("num_bins", "u4"), ("bins_used", "u4"), ("peak_bin", "u4"), ("peak_cells", "u4"),
                  ("reserved", "u4"), ("peak_sum", "f4"), ("peak_mean", "f4"), ("sum_means", "f8"),
                  ("sum_sq_means", "f8"), ("cells", "u8")])
EXACT = [n for n in SCORE.names if n not in ("sum_means", "sum_sq_means")]   # compared byte for byte


def num_bins(L, C):
    return L // C


def bins(i, L, C):
    """bin of the cells with global indices i under period L"""
    return np.minimum((np.asarray(i, np.int64) % L) // C, num_bins(L, C) - 1)


def fold(p, L, C, start=0, profile=None):
    """the profile after cells p (global indices start ..) have been added to `profile` (None: all +0), float32"""
    F = np.zeros(num_bins(L, C), np.float32) if profile is None else np.array(profile, np.float32)
    p = np.asarray(p, np.float32)
    with np.errstate(all="ignore"):
        np.add.at(F, bins(start + np.arange(len(p), dtype=np.int64), L, C), p)
    return F


def counts(N, L, C):
    """n_L[j](N) = floor(N / L) (b - a) + clamp((N mod L) - a, 0, b - a)"""
    NB = num_bins(L, C)
    a = np.arange(NB, dtype=np.int64) * C
    b = a + C
    b[-1] = L
    return ((N // L) * (b - a) + np.clip(N % L - a, 0, b - a)).astype(np.uint64)


def score(F, N, L, C):
    """the record of one candidate after N cells"""
    NB = num_bins(L, C)
    rec = np.zeros((), SCORE)
    rec["period"], rec["num_bins"], rec["cells"] = L, NB, N
    n = counts(N, L, C)
    used = int((n > 0).sum())
    assert (n[:used] > 0).all() and used == min(NB, -(-N // C))      # the leading ones
    rec["bins_used"] = used
    if used == 0:
        return rec
    with np.errstate(all="ignore"):
        m = F[:used].astype(np.float64) / n[:used].astype(np.float64)
        # the walk of literal_peak: a NaN in the first used bin stays, else the first of the largest values that are numbers
        best = 0 if np.isnan(m[0]) else int(np.nanargmax(m))
        rec["peak_bin"], rec["peak_cells"] = best, n[best]
        rec["peak_sum"], rec["peak_mean"] = F[best], np.float32(m[best])
        rec["sum_means"], rec["sum_sq_means"] = m.sum(), (m * m).sum()
    return rec


def sums_bound(F, N, L, C):
    """(bound on sum_means, bound on sum_sq_means): (bins_used + 1) 2^-53 sum |terms|; inf where a term is not finite
    (then only non-finite-ness is compared)"""
    n = counts(N, L, C)
    used = int((n > 0).sum())
    if used == 0:
        return 0.0, 0.0
    with np.errstate(all="ignore"):
        m = F[:used].astype(np.float64) / n[:used].astype(np.float64)
        if not np.isfinite(m).all() or not np.isfinite(m * m).all():
            return np.inf, np.inf
        return (used + 1) * 2.0 ** -53 * np.abs(m).sum(), (used + 1) * 2.0 ** -53 * (m * m).sum()


def scores(p, periods, C, N=None):
    """(records, profiles) of every candidate after the first N cells of p (None: all)"""
    N = len(p) if N is None else N
    prof = [fold(p[:N], int(L), C) for L in periods]
    return np.array([score(F, N, int(L), C) for F, L in zip(prof, periods)], SCORE), prof


def z(rec):
    """(peak_mean - mu) / sqrt(sum_sq_means / bins_used - mu^2); 0 where bins_used < 8 or the variance is not positive"""
    rec = np.atleast_1d(rec)
    out = np.zeros(len(rec))
    for k, r in enumerate(rec):
        if r["bins_used"] < 8:
            continue
        mu = r["sum_means"] / r["bins_used"]
        var = r["sum_sq_means"] / r["bins_used"] - mu * mu
        if var > 0:
            out[k] = (float(r["peak_mean"]) - mu) / np.sqrt(var)
    return out


def ranked(rec, C):
    """indices of the records by z descending, ties to the smaller period, then to list order"""
    zz = z(rec)
    return sorted(range(len(rec)), key=lambda k: (-zz[k], int(rec[k]["period"]), k))


def same_floats(got, want):
    """the same bytes, element by element -- or both NaN: IEEE 754 fixes when an addition gives a NaN, not the sign and
    payload of the NaN it gives (Inf - Inf is 0xffc00000 on x86 and 0x7fc00000 on the GPU)"""
    g, w = np.ascontiguousarray(got, np.float32).reshape(-1), np.ascontiguousarray(want, np.float32).reshape(-1)
    return g.shape == w.shape and bool(((g.view(np.uint32) == w.view(np.uint32)) | (np.isnan(g) & np.isnan(w))).all())


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


# -- the literal loops ------------------------------------------------------------------------------------------
def literal_fold(p, L, C, start=0):
    NB = L // C
    F = [np.float32(0.0)] * NB
    cnt = [0] * NB
    with np.errstate(all="ignore"):
        for k in range(len(p)):
            i = start + k
            j = min((i % L) // C, NB - 1)
            F[j] = np.float32(F[j] + np.float32(p[k]))
            cnt[j] += 1
    return np.array(F, np.float32), np.array(cnt, np.uint64)


def literal_peak(m):
    """walk j ascending, replace only on a strictly greater mean: ties to the lowest j, a NaN never displaces anything, a
    NaN in the first bin stays"""
    best = 0
    for j in range(1, len(m)):
        if m[j] > m[best]:
            best = j
    return best


# -- designed inputs --------------------------------------------------------------------------------------------
def spread_stream(n, seed):
    """positive cells with exponents spread over 2^-12 .. 2^12 and full mantissas: a sum of them depends on its order"""
    rng = np.random.default_rng(seed)
    return (rng.uniform(1.0, 2.0, n) * 2.0 ** rng.integers(-12, 13, n)).astype(np.float32)


def fold_pairwise(p, L, C):
    """the same cells per bin, added as a balanced tree: NOT the definition"""
    j = bins(np.arange(len(p), dtype=np.int64), L, C)
    out = np.zeros(num_bins(L, C), np.float32)
    for b in range(len(out)):
        v = list(np.asarray(p, np.float32)[j == b])
        while len(v) > 1:
            v = [np.float32(v[k] + v[k + 1]) if k + 1 < len(v) else v[k] for k in range(0, len(v), 2)]
        out[b] = v[0] if v else 0.0
    return out


def fold_reversed(p, L, C):
    """the same cells per bin, added in descending index: NOT the definition"""
    j = bins(np.arange(len(p), dtype=np.int64), L, C)
    out = np.zeros(num_bins(L, C), np.float32)
    np.add.at(out, j[::-1], np.asarray(p, np.float32)[::-1])
    return out
