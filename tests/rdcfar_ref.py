"""The range-Doppler CFAR detector restated in numpy from the header text (include/pfb_channelizer.h, the pfb_rdcfar
section), not from the device code.  A is a loop over j that adds rolled arrays; the lead and lag sums are loops over
gate offsets with masks: each loop step is one elementwise float64 addition, so the order is the definition's (a masked
step adds +0.0, which leaves a sum that began at +0.0 as it is).  The peak box is walked per over cell."""
import numpy as np

DET = np.dtype([("map", "u8"), ("row", "u4"), ("gate", "u4"), ("power", "f4"), ("noise", "f4"), ("training_cells", "u4"),
                ("flags", "u4")])
CA, GO, SO = 0, 1, 2
ONE_SIDED = 1


def column_sums(P, Wd, reverse=False):
    """A[d][r]: float64, j = -Wd .. Wd ascending, from +0.0; reverse=True walks descending (for the order-dependence
    proof only)"""
    P = np.asarray(P, np.float32)
    A = np.zeros(P.shape, np.float64)
    with np.errstate(all="ignore"):
        for j in (range(Wd, -Wd - 1, -1) if reverse else range(-Wd, Wd + 1)):
            A = A + np.roll(P, -j, axis=0).astype(np.float64)   # row d of the rolled array is row (d + j) mod ND
    return A


def counts(R, Gr, Tr):
    """(nL, nR) per gate"""
    r = np.arange(R)
    nl = np.clip(r - Gr, 0, Tr)
    nr = np.clip(R - 1 - r - Gr, 0, Tr)
    return nl, nr


def side_sums(A, Gr, Tr, reverse=False):
    """(sumL, sumR): ascending gate, from +0.0; reverse=True walks descending (for the order-dependence proof only)"""
    ND, R = A.shape
    r = np.arange(R)
    pad = np.concatenate([A, np.zeros((ND, 1))], axis=1)   # [R]: a slot for "not there"
    out = []
    with np.errstate(all="ignore"):
        for first in (r - Gr - Tr, r + Gr + 1):
            s = np.zeros((ND, R))
            for t in (range(Tr - 1, -1, -1) if reverse else range(Tr)):
                g = first + t
                ok = (g >= 0) & (g < R)
                s = s + np.where(ok[None, :], pad[:, np.where(ok, g, R)], 0.0)
            out.append(s)
    return out


def noise_of(P, Wd, Gr, Tr, method, A=None, sums=None):
    """(noise float32 (ND, R), NaN where a cell has none; nL + nR per gate)"""
    ND, R = np.shape(P)
    A = column_sums(P, Wd) if A is None else A
    sl, sr = side_sums(A, Gr, Tr) if sums is None else sums
    nl, nr = counts(R, Gr, Tr)
    col = float(2 * Wd + 1)
    nan = np.full((ND, R), np.nan)
    with np.errstate(all="ignore"):
        if method == CA:
            m = np.where(nl + nr > 0, (sl + sr) / ((nl + nr) * col), nan)
        else:
            a, c = sl / (nl * col), sr / (nr * col)
            both = np.maximum(a, c) if method == GO else np.minimum(a, c)   # NaN on either side gives NaN
            m = np.where((nl > 0) & (nr > 0), both, np.where(nl > 0, a, np.where(nr > 0, c, nan)))
        return m.astype(np.float32), nl + nr


def decide(P, Wd, Gr, Tr, method, alpha, min_power):
    """(over (ND, R) bool, noise float32, nL + nR per gate) of one map"""
    P = np.asarray(P, np.float32)
    noise, trained = noise_of(P, Wd, Gr, Tr, method)
    with np.errstate(all="ignore"):
        thr = np.float32(alpha) * noise   # one float32 multiply
        over = (P > thr) & (P > np.float32(min_power))
    return over, noise, trained


def is_peak(P, d, r, Gr, Pd):
    """no cell of the peak box of (d, r) beats it"""
    ND, R = P.shape
    rows = (d + np.arange(-Pd, Pd + 1)) % ND
    g = np.arange(max(r - Gr, 0), min(r + Gr, R - 1) + 1)
    box = P[rows][:, g]
    lower = (rows[:, None] < d) | ((rows[:, None] == d) & (g[None, :] < r))
    with np.errstate(all="ignore"):
        return not bool(((box > P[d, r]) | ((box == P[d, r]) & lower)).any())


def detect(maps, Wd, Gr, Tr, Pd, method=CA, alpha=1.0, min_power=0.0, first_map=0):
    """(records of maps (n, ND, R), stats of these maps alone)"""
    maps = np.asarray(maps, np.float32)
    n, ND, R = maps.shape
    out, n_over = [], 0
    for m in range(n):
        P = maps[m]
        over, noise, trained = decide(P, Wd, Gr, Tr, method, alpha, min_power)
        n_over += int(over.sum())
        for d, r in zip(*np.nonzero(over)):   # row-major: ascending (row, gate)
            if is_peak(P, int(d), int(r), Gr, Pd):
                out.append((first_map + m, d, r, P[d, r], noise[d, r], trained[r] * (2 * Wd + 1),
                            ONE_SIDED if trained[r] < 2 * Tr else 0))
    nl, nr = counts(R, Gr, Tr)
    stats = {"maps_in": n, "cells_over": n_over, "cells_without_noise": n * ND * int(((nl + nr) == 0).sum()),
             "detections": len(out), "dropped": 0}
    return (np.array(out, DET) if out else np.zeros(0, DET)), stats
