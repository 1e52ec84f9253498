"""Pulse-Doppler integration restated in float64 numpy from the header text (include/pfb_channelizer.h, the pfb_pd
section), not from the device code: the gate matrix of an interval, the four outputs, the rule by which an interval
completes, and the allowances the GPU tests hold the library to.  A support module, not a test."""
import functools

import numpy as np

COMPLEX, POWER, BEST, NONCOHERENT = 0, 1, 2, 3
LENGTHS = (8, 16, 32, 64, 128, 256, 512, 1024)
CELL = np.dtype([("power", "f4"), ("hypothesis", "i4")])


def doppler_length(K, nd=0):
    """ND: the smallest of the set >= K for nd = 0; None where the library refuses"""
    if nd == 0:
        nd = next((v for v in LENGTHS if v >= K), None)
    return nd if nd in LENGTHS and 1 <= K <= nd else None


def cpi_samples(L, R, K):
    return (K - 1) * L + R


def first_cpi(start, o, L, K):
    """the first interval whose first sample o + c K L is not before the index the stream (re)started at"""
    return 0 if start <= o else -(-(start - o) // (K * L))


def completed(total, o, L, R, K, start=0):
    """how many intervals have completed once the samples start .. total-1 have been taken"""
    c0 = first_cpi(start, o, L, K)
    end = o + c0 * K * L + cpi_samples(L, R, K)   # one past the sample that completes interval c0
    return 0 if end > total else (total - end) // (K * L) + 1


def gates(x, c, o, L, R, K, base=0):
    """A_c[k][r] = x[o + (c K + k) L + r] as complex128, x[0] being stream index `base`; samples that x does not hold
    are zeros (what pfb_pd_flush takes them for)"""
    x = np.asarray(x)
    k, r = np.meshgrid(np.arange(K), np.arange(R), indexing="ij")
    at = o + (c * K + k) * L + r - base
    ok = (at >= 0) & (at < len(x))
    return np.where(ok, x[np.where(ok, at, 0)].astype(np.complex128), 0.0) if len(x) else np.zeros((K, R), np.complex128)


def window(K, w=None):
    return np.ones(K, np.float32) if w is None else np.asarray(w, np.float32)


def rows(ND, centered):
    """the d of each written row"""
    return np.arange(-ND // 2, ND // 2) if centered else np.arange(ND)


@functools.lru_cache(maxsize=4)
def kernel_matrix(K, ND, centered):
    """E[row][k] = e^{-j 2 pi d k / ND}, the phase reduced modulo one turn in integers first"""
    d = rows(ND, centered)
    return np.exp(-2j * np.pi * ((d[:, None] * np.arange(K)[None, :]) % ND) / ND)


def transform(A, w, ND, centered=False):
    """Z[row][r] = sum_k w[k] A[k][r] e^{-j 2 pi d k / ND} for the rows in written order"""
    K = A.shape[0]
    with np.errstate(all="ignore"):
        return kernel_matrix(K, ND, bool(centered)) @ (window(K, w).astype(np.float64)[:, None] * A)


def power(Z):
    with np.errstate(all="ignore"):
        return Z.real ** 2 + Z.imag ** 2


def best(P, ND, centered=False):
    """(power, hypothesis) per gate: the walk over the written rows, replacing only on a strictly greater power"""
    d = rows(ND, centered)
    bp, bh = P[0].copy(), np.full(P.shape[1], d[0])
    with np.errstate(all="ignore"):
        for i in range(1, ND):
            m = P[i] > bp   # false for a NaN on either side
            bp, bh = np.where(m, P[i], bp), np.where(m, d[i], bh)
    return bp, bh


def noncoherent(A, w=None):
    with np.errstate(all="ignore"):
        return ((window(A.shape[0], w).astype(np.float64) ** 2)[:, None] * (A.real ** 2 + A.imag ** 2)).sum(axis=0)


def frequencies(L, ND, fs, centered=False):
    return rows(ND, centered) * fs / (ND * L)


def bound(A, w=None):
    """per gate: 1e-5 ||w||_2 ||A[:, r]||_2, which by Cauchy-Schwarz is 1e-5 of a bound on |Z|"""
    with np.errstate(all="ignore"):
        return 1e-5 * np.linalg.norm(window(A.shape[0], w).astype(np.float64)) * np.linalg.norm(A, axis=0)


def power_bound(A, w=None):
    """| |Z|^2 - |Zref|^2 | <= |Z - Zref| (|Z| + |Zref|) <= b (2 B + b), B = ||w|| ||A[:, r]|| >= |Zref|, b = 1e-5 B"""
    b = bound(A, w)
    return b * (2e5 * b + b)


def intervals(x, total, flushed, o, L, R, K, start=0, base=0):
    """the gate matrices of the intervals that have come out once samples start .. total-1 of x were taken (x[0] is
    stream index `base`), plus the open one after a flush"""
    c0 = first_cpi(start, o, L, K)
    n = completed(total, o, L, R, K, start)
    seen = np.asarray(x)[: max(total - base, 0)]
    out = [gates(seen, c0 + i, o, L, R, K, base) for i in range(n)]
    if flushed and o + (c0 + n) * K * L < total:   # the next interval has opened
        out.append(gates(seen, c0 + n, o, L, R, K, base))
    return out
