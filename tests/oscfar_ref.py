"""The ordered-statistic CFAR detector restated in numpy from the header text (include/pfb_channelizer.h, the
pfb_oscfar section), not from the device code: gather every cell's training values into an array with one slot per
(row offset, gate offset), sort the slots, take the k'-th.  A slot whose gate lies outside the map holds NaN: NaNs sort
last, and k' <= n, so an absent slot is chosen only where a real NaN would be.  The peak box, the training counts and
the record are rdcfar_ref's.  alpha_ref restates the product formula of pfb_oscfar_alpha."""
import math

import numpy as np

from rdcfar_ref import DET, ONE_SIDED, counts, is_peak

CHUNK = 1 << 24   # slots sorted at a time


def full_cells(Wd, Tr):
    """N: what a cell away from the gate edges trains on"""
    return 2 * Tr * (2 * Wd + 1)


def ranks(R, Wd, Gr, Tr, rank):
    """(k' per gate, n per gate): k' = ceil(k n / N) in integers; 0 where n = 0"""
    nl, nr = counts(R, Gr, Tr)
    n = (nl + nr) * (2 * Wd + 1)
    N = full_cells(Wd, Tr)
    return (rank * n + N - 1) // N, n


def training(P, Wd, Gr, Tr, rows=None):
    """V[d][r][slot], float32: the training values of the cells of `rows` (all by default), NaN where a gate is absent"""
    P = np.asarray(P, np.float32)
    ND, R = P.shape
    rows = np.arange(ND) if rows is None else np.asarray(rows)
    r = np.arange(R)
    pad = np.concatenate([P, np.full((ND, 1), np.nan, np.float32)], axis=1)   # column R: "not there"
    gates = np.concatenate([r[:, None] - Gr - Tr + np.arange(Tr)[None, :], r[:, None] + Gr + 1 + np.arange(Tr)[None, :]], axis=1)
    gates = np.where((gates >= 0) & (gates < R), gates, R)                     # (R, 2 Tr)
    V = np.empty((len(rows), R, 2 * Tr * (2 * Wd + 1)), np.float32)
    for s, j in enumerate(range(-Wd, Wd + 1)):
        V[:, :, s * 2 * Tr:(s + 1) * 2 * Tr] = pad[(rows + j) % ND][:, gates]
    return V


def sorted_training(P, Wd, Gr, Tr):
    """the training values of every cell in ascending order, NaNs and absent slots last: (ND, R, N).  Depends on the
    map and the geometry only, so one sort serves every rank."""
    P = np.asarray(P, np.float32)
    ND, R = P.shape
    N = full_cells(Wd, Tr)
    step = max(1, CHUNK // (R * N))
    S = np.empty((ND, R, N), np.float32)
    for d0 in range(0, ND, step):
        rows = np.arange(d0, min(d0 + step, ND))
        S[rows] = np.sort(training(P, Wd, Gr, Tr, rows), axis=2)
    return S


def noise_of(P, Wd, Gr, Tr, rank, S=None):
    """(noise float32 (ND, R): the k'-th smallest, NaN where a cell has none or too few numbers; n per gate)"""
    ND, R = np.shape(P)
    S = sorted_training(P, Wd, Gr, Tr) if S is None else S
    kk, n = ranks(R, Wd, Gr, Tr, rank)
    pick = np.take_along_axis(S, np.broadcast_to(np.maximum(kk - 1, 0)[None, :, None], (ND, R, 1)), axis=2)[:, :, 0]
    noise = np.where(n[None, :] > 0, pick, np.float32(np.nan)).astype(np.float32)
    return noise + np.float32(0.0), n      # -0.0 + 0.0 = +0.0: a zero is reported as +0.0


def decide(P, Wd, Gr, Tr, rank, alpha, min_power, S=None):
    """(over (ND, R) bool, noise float32, n per gate) of one map"""
    P = np.asarray(P, np.float32)
    noise, n = noise_of(P, Wd, Gr, Tr, rank, S)
    with np.errstate(all="ignore"):
        thr = np.float32(alpha) * noise   # one float32 multiply
        over = (P > thr) & (P > np.float32(min_power))
    return over, noise, n


def detect(maps, Wd, Gr, Tr, Pd, rank, alpha=1.0, min_power=0.0, first_map=0, sorts=None):
    """(records of maps (n, ND, R), stats of these maps alone); sorts: sorted_training of each map, to share"""
    maps = np.asarray(maps, np.float32)
    count, ND, R = maps.shape
    out, n_over = [], 0
    for m in range(count):
        P = maps[m]
        over, noise, n = decide(P, Wd, Gr, Tr, rank, alpha, min_power, None if sorts is None else sorts[m])
        n_over += int(over.sum())
        for d, r in zip(*np.nonzero(over)):   # row-major: ascending (row, gate)
            if is_peak(P, int(d), int(r), Gr, Pd):
                out.append((first_map + m, d, r, P[d, r], noise[d, r], n[r],
                            ONE_SIDED if n[r] < full_cells(Wd, Tr) else 0))
    _, n = ranks(R, Wd, Gr, Tr, rank)
    stats = {"maps_in": count, "cells_over": n_over, "cells_without_noise": count * ND * int((n == 0).sum()),
             "detections": len(out), "dropped": 0}
    return (np.array(out, DET) if out else np.zeros(0, DET)), stats


def log_pfa(alpha, N, k):
    """log of prod_{i=0}^{k-1} (N - i) / (N - i + alpha)"""
    return -sum(math.log1p(alpha / (N - i)) for i in range(k))


def alpha_ref(pfa, N, k):
    """the root of the product formula, by bisection in float64"""
    want = math.log(pfa)
    lo, hi = 0.0, 1.0
    while log_pfa(hi, N, k) > want:
        hi *= 2.0
    for _ in range(200):
        mid = 0.5 * (lo + hi)
        if log_pfa(mid, N, k) > want:
            lo = mid
        else:
            hi = mid
    return 0.5 * (lo + hi)
