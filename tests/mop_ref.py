"""The modulation-on-pulse unit restated in numpy from its definition in include/pfb_channelizer.h (the pfb_mop_*
section), independently of the C code: int64 limbs (and Python integers, in ``literal``) for the integer formats,
float64 terms for cf32.  For the integer formats ``measure`` gives the bytes the library must give; for cf32 it gives
the terms' exact sums (math.fsum) and, per sum, the bound the header states."""
import math

import numpy as np

MOP = np.dtype([("start", "u8"), ("length", "u4"), ("column", "u4"), ("n", "u4"), ("flags", "u4"), ("neg_count", "u4"),
                ("first_neg", "u4"), ("last_neg", "u4"), ("peak_index", "u4"), ("negs_listed", "u4"), ("reserved", "u4"),
                ("energy", "f8"), ("peak_power", "f8"), ("s1_re", "f8"), ("s1_im", "f8"), ("s2_re", "f8"), ("s2_im", "f8")])
PULSE = np.dtype([("start", "u8"), ("length", "u4"), ("column", "u4")])
OUTSIDE, SHORT, TRUNCATED, NEGS_CLIPPED = 1, 2, 4, 8
NONE = 0xFFFFFFFF
MAX_N = 1 << 20
SUMS = ("energy", "s1_re", "s1_im", "s2_re", "s2_im")
EXACT = ("start", "length", "column", "n", "flags", "neg_count", "first_neg", "last_neg", "peak_index", "negs_listed",
         "reserved")


def pulses(starts, lengths, columns=None):
    p = np.zeros(len(starts), PULSE)
    p["start"], p["length"] = starts, lengths
    if columns is not None:
        p["column"] = columns
    return p


def geometry(start, length, column, num_samples, ld, base, trim):
    """(n, flags, first row) of one pulse"""
    start, length, column = int(start), int(length), int(column)
    if column >= ld or start < base or start + length > base + num_samples:
        return 0, OUTSIDE | SHORT, 0
    m = length - 2 * trim if length > 2 * trim else 0
    n = min(m, MAX_N)
    flags = (TRUNCATED if m > MAX_N else 0) | (SHORT if n < 3 else 0)
    return n, flags, start - base + trim


def components(x, row0, n, column=0):
    """(I, Q) of u[0 .. n): int64 for (rows, 2) integers, float64 for complex64 (rows,) or (rows, ld)"""
    x = np.asarray(x)
    if np.iscomplexobj(x):
        col = x[row0:row0 + n] if x.ndim == 1 else x[row0:row0 + n, column]
        return col.real.astype(np.float64), col.imag.astype(np.float64)
    return x[row0:row0 + n, 0].astype(np.int64), x[row0:row0 + n, 1].astype(np.int64)


def terms(I, Q):
    """every term of the definition, one IEEE (or integer) operation at a time"""
    n = len(I)
    t = {"p": I * I + Q * Q}
    a = I[1:] * I[:-1] + Q[1:] * Q[:-1]
    b = Q[1:] * I[:-1] - I[1:] * Q[:-1]
    L = (n - 1) // 2 if n else 0
    t["a"], t["b"], t["L"] = a, b, L
    if n >= 2:
        k = n - 1 - L                         # i = 0 .. n-2-L
        t["s2re"] = a[L:L + k] * a[:k] + b[L:L + k] * b[:k]
        t["s2im"] = b[L:L + k] * a[:k] - a[L:L + k] * b[:k]
    else:
        t["s2re"] = t["s2im"] = a[:0]
    t["c"] = a[1:] * a[:-1] + b[1:] * b[:-1] if n >= 3 else a[:0]
    return t


def limb_sum(v):
    """the two-limb sum of int64 terms, reported as the header says; and the exact Python integer"""
    hi, lo = int((v >> 32).sum()), int((v & 0xFFFFFFFF).sum())
    return math.ldexp(float(hi), 32) + float(lo), (hi << 32) + lo


def one(I, Q, max_negatives):
    """(fields of the record but the echo and the geometry's flags, the negatives listed, bounds of the five sums)"""
    n = len(I)
    t = terms(I, Q)
    r, bound = {}, {}
    integer = I.dtype.kind == "i"
    if integer:
        r["energy"], r["s1_re"], r["s1_im"] = float(int(t["p"].sum())), float(int(t["a"].sum())), float(int(t["b"].sum()))
        r["s2_re"], r["s2_im"] = limb_sum(t["s2re"])[0], limb_sum(t["s2im"])[0]
        bound = dict.fromkeys(SUMS, 0.0)
    else:
        with np.errstate(all="ignore"):
            mags = {"energy": t["p"], "s1_re": np.abs(I[1:] * I[:-1]) + np.abs(Q[1:] * Q[:-1]),
                    "s1_im": np.abs(Q[1:] * I[:-1]) + np.abs(I[1:] * Q[:-1])}
            k = len(t["s2re"])
            a, b, L = t["a"], t["b"], t["L"]
            mags["s2_re"] = np.abs(a[L:L + k] * a[:k]) + np.abs(b[L:L + k] * b[:k])
            mags["s2_im"] = np.abs(b[L:L + k] * a[:k]) + np.abs(a[L:L + k] * b[:k])
            for name, v in (("energy", t["p"]), ("s1_re", t["a"]), ("s1_im", t["b"]), ("s2_re", t["s2re"]),
                            ("s2_im", t["s2im"])):
                r[name] = math.fsum(v) if np.isfinite(v).all() else float(np.sum(v))
                bound[name] = (n + 4) * 2.0 ** -53 * float(np.sum(mags[name]))
    with np.errstate(invalid="ignore"):
        neg = np.flatnonzero(t["c"] < 0)
        p = t["p"]
        ok = ~np.isnan(p) if not integer else np.ones(n, bool)
    r["neg_count"] = len(neg)
    r["first_neg"], r["last_neg"] = (int(neg[0]), int(neg[-1])) if len(neg) else (NONE, NONE)
    r["negs_listed"] = min(len(neg), max_negatives)
    if ok.any():
        best = p[ok].max()
        r["peak_index"] = int(np.flatnonzero(ok & (p == best))[0])
        r["peak_power"] = float(best)
    else:
        r["peak_index"], r["peak_power"] = NONE, 0.0
    return r, neg[:max_negatives], bound


def measure(x, plist, base=0, trim=0, max_negatives=32, ld=None):
    """(records, negs, bounds): MOP records and (pulses, max_negatives) uint32 negatives of the PULSE list over x, and
    per record the bounds of the five sums (zeros for the integer formats)"""
    x = np.asarray(x)
    rows = x.shape[0]
    if ld is None:
        ld = x.shape[1] if np.iscomplexobj(x) and x.ndim == 2 else 1
    rec = np.zeros(len(plist), MOP)
    negs = np.full((len(plist), max_negatives), NONE, np.uint32)
    bounds = np.zeros((len(plist), 5))
    for k, p in enumerate(plist):
        n, flags, row0 = geometry(p["start"], p["length"], p["column"], rows, ld, base, trim)
        I, Q = components(x, row0, n, int(p["column"]) if n else 0)
        r, listed, bound = one(I, Q, max_negatives)
        rec[k]["start"], rec[k]["length"], rec[k]["column"], rec[k]["n"] = p["start"], p["length"], p["column"], n
        rec[k]["flags"] = flags | (NEGS_CLIPPED if r["neg_count"] > max_negatives else 0)
        for name, v in r.items():
            rec[k][name] = v
        negs[k, :len(listed)] = listed
        bounds[k] = [bound[s] for s in SUMS]
    return rec, negs, bounds


def measure_many(x, plist, max_negatives=32):
    """`measure` for long lists of short pulses of an integer series, all inside it, base 0, no trim: the pulses of one
    length are taken together, one row each (test_mop_cpu.py holds it to `measure`)"""
    x = np.asarray(x)
    rec = np.zeros(len(plist), MOP)
    negs = np.full((len(plist), max_negatives), NONE, np.uint32)
    rec["start"], rec["length"], rec["column"], rec["n"] = plist["start"], plist["length"], plist["column"], plist["length"]
    for n in np.unique(plist["length"]):
        n = int(n)
        assert 3 <= n <= 64
        rows = np.flatnonzero(plist["length"] == n)
        at = plist["start"][rows].astype(np.int64)[:, None] + np.arange(n)[None, :]
        I, Q = x[at, 0].astype(np.int64), x[at, 1].astype(np.int64)
        p = I * I + Q * Q
        a = I[:, 1:] * I[:, :-1] + Q[:, 1:] * Q[:, :-1]
        b = Q[:, 1:] * I[:, :-1] - I[:, 1:] * Q[:, :-1]
        L = (n - 1) // 2
        k = n - 1 - L
        s2re = a[:, L:L + k] * a[:, :k] + b[:, L:L + k] * b[:, :k]
        s2im = b[:, L:L + k] * a[:, :k] - a[:, L:L + k] * b[:, :k]
        c = a[:, 1:] * a[:, :-1] + b[:, 1:] * b[:, :-1]
        rec["energy"][rows], rec["s1_re"][rows], rec["s1_im"][rows] = p.sum(1), a.sum(1), b.sum(1)
        for name, v in (("s2_re", s2re), ("s2_im", s2im)):      # k <= 63 terms under 2^62: the limbs as the header has them
            hi, lo = (v >> 32).sum(1), (v & 0xFFFFFFFF).sum(1)
            rec[name][rows] = np.ldexp(hi.astype(np.float64), 32) + lo.astype(np.float64)
        rec["peak_index"][rows], rec["peak_power"][rows] = p.argmax(1), p.max(1)
        neg = c < 0
        count = neg.sum(1)
        rec["neg_count"][rows], rec["negs_listed"][rows] = count, np.minimum(count, max_negatives)
        rec["first_neg"][rows] = np.where(count > 0, neg.argmax(1), NONE)
        rec["last_neg"][rows] = np.where(count > 0, n - 3 - neg[:, ::-1].argmax(1), NONE)
        rec["flags"][rows] = np.where(count > max_negatives, NEGS_CLIPPED, 0)
        order = np.argsort(~neg, axis=1, kind="stable")[:, :max_negatives]      # the negatives' positions first, ascending
        listed = np.where(np.arange(order.shape[1])[None, :] < count[:, None], order, NONE)
        negs[rows[:, None], np.arange(order.shape[1])[None, :]] = listed
    return rec, negs


def literal(I, Q):
    """the definition as per-sample loops over Python integers: every sum exact, whatever its size"""
    I, Q = [int(v) for v in I], [int(v) for v in Q]
    n = len(I)
    a = [I[i + 1] * I[i] + Q[i + 1] * Q[i] for i in range(n - 1)]
    b = [Q[i + 1] * I[i] - I[i + 1] * Q[i] for i in range(n - 1)]
    L = (n - 1) // 2 if n else 0
    out = {"energy": sum(I[i] * I[i] + Q[i] * Q[i] for i in range(n)), "s1_re": sum(a), "s1_im": sum(b),
           "s2_re": sum(a[i + L] * a[i] + b[i + L] * b[i] for i in range(max(n - 1 - L, 0) if n >= 2 else 0)),
           "s2_im": sum(b[i + L] * a[i] - a[i + L] * b[i] for i in range(max(n - 1 - L, 0) if n >= 2 else 0))}
    neg = [i for i in range(n - 2) if a[i + 1] * a[i] + b[i + 1] * b[i] < 0]
    out["negs"] = neg
    pw = [I[i] * I[i] + Q[i] * Q[i] for i in range(n)]
    out["peak_power"] = max(pw) if n else 0
    out["peak_index"] = pw.index(max(pw)) if n else NONE
    return out


def figures(rec, fs):
    """pfb_mop_figures by its formulas: rows of (freq, rate, extent, mean_power, flips, kind)"""
    out = []
    for r in rec:
        n = int(r["n"])
        L = (n - 1) // 2 if n else 0
        freq = math.atan2(r["s1_im"], r["s1_re"]) / (2 * math.pi) * fs
        rate = math.atan2(r["s2_im"], r["s2_re"]) / (2 * math.pi * L) * fs * fs if L else 0.0
        extent = rate * (n - 1) / fs if n else 0.0
        if n < 3 or int(r["flags"]) & OUTSIDE:
            kind = 4
        else:
            kind = (1 if abs(extent) >= fs / n else 0) | (2 if r["neg_count"] >= 2 else 0)
        out.append((freq, rate, extent, r["energy"] / n if n else 0.0, r["neg_count"] / 2.0, kind))
    return out


def same_sums(got, want, bounds):
    """cf32: every sum of `got` within its bound of `want`; what is not finite agrees in kind"""
    for k in range(len(want)):
        for j, name in enumerate(SUMS + ("peak_power",)):
            g, w = float(got[k][name]), float(want[k][name])
            if name == "peak_power":
                ok = g == w or (math.isnan(g) and math.isnan(w))
            elif math.isfinite(w) and math.isfinite(bounds[k][j]):
                ok = abs(g - w) <= bounds[k][j]
            else:
                ok = (math.isnan(g) and math.isnan(w)) or g == w or not math.isfinite(bounds[k][j])
            if not ok:
                return False, (k, name, g, w, bounds[k][j] if j < 5 else 0.0)
    return True, None
