"""numpy restatement of the channel synthesizer (pfb_chsyn_* in include/pfb_channelizer.h), for the tests only.

``synthesize`` is the definition in float64: per frame the weighted columns go through an M-point e^{+j} DFT, and each
output sample is the Q-term sum over the frames that reach it, taken in ascending q.  ``synthesize_f32`` takes the
same sums in the same order in float32 / complex64; ``synthesize_literal`` is the double sum over (m, k) written out,
for tiny sizes.  ``allowance`` is the magnitude A[s] the GPU tests scale their tolerance by.
"""
from __future__ import annotations

import numpy as np

FFTSHIFT, DEROTATE = 1, 2


def channel_of_column(M: int, flags: int) -> np.ndarray:
    """k(c): the channel column c holds."""
    c = np.arange(M)
    return (c + (M + 1) // 2) % M if flags & FFTSHIFT else c


def _weights(M: int, weights) -> np.ndarray:
    return np.ones(M) if weights is None else np.asarray(weights, dtype=np.float64).reshape(M)


def frame_rows(y, M: int, flags: int = 0, weights=None, frame0: int = 0, D: int | None = None, dtype=np.complex128):
    """v_m[p] of every frame as the FIR reads it: the DFT of the weighted columns in channel order, and with DEROTATE
    the row read at (p + m D) mod M."""
    y = np.asarray(y).reshape(-1, M)
    F = y.shape[0]
    real = np.float32 if dtype == np.complex64 else np.float64
    u = np.zeros((F, M), dtype=dtype)
    u[:, channel_of_column(M, flags)] = (y.astype(dtype) * _weights(M, weights).astype(real)[None, :]).astype(dtype)
    if dtype == np.complex64:
        # complex64 sums against float64 twiddles rounded once, k ascending
        tw = np.exp(2j * np.pi * (np.outer(np.arange(M), np.arange(M)) % M) / M).astype(np.complex64)
        v = np.zeros((F, M), dtype=np.complex64)
        for k in range(M):
            v = (v + u[:, k:k + 1] * tw[k][None, :]).astype(np.complex64)
    else:
        v = np.fft.ifft(u, axis=1) * M
    if flags & DEROTATE:
        D = M if D is None else D
        m = frame0 + np.arange(F)
        idx = (np.arange(M)[None, :] + ((m * D) % M)[:, None]) % M
        v = np.take_along_axis(v, idx, axis=1)
    return v


def _fir(v, g, M: int, D: int, scale, history, dtype):
    """x[bD + d] = scale * sum_q g[d + qD] v_{b-q}[(d + qD) mod M], q ascending; ``history``: the Q-1 rows before v[0]
    (None: zeros).  Returns (x, the last Q-1 rows)."""
    real = np.float32 if dtype == np.complex64 else np.float64
    g = np.asarray(g, dtype=real)
    Q = g.size // D
    F = v.shape[0]
    hist = np.zeros((Q - 1, M), dtype=dtype) if history is None else np.asarray(history, dtype=dtype)
    rows = np.concatenate([hist, v.astype(dtype)], axis=0)  # frame f at rows[f + Q - 1]
    acc = np.zeros((F, D), dtype=dtype)
    d = np.arange(D)
    for q in range(Q):
        idx = d + q * D
        acc = (acc + g[idx][None, :] * rows[Q - 1 - q: Q - 1 - q + F][:, idx % M]).astype(dtype)
    x = (acc * real(scale)).astype(dtype).reshape(-1)
    return x, rows[rows.shape[0] - (Q - 1):] if Q > 1 else rows[:0]


def synthesize(y, g, M: int, D: int | None = None, scale: float = 0.0, flags: int = 0, weights=None, frame0: int = 0,
               history=None, dtype=np.complex128, return_history: bool = False):
    """F*D samples from F frames (y: F x M, frame-major columns).  scale = 0 means D."""
    D = M if D is None else D
    g = np.asarray(g)
    assert g.size % M == 0 and (D == M or 2 * D == M)
    v = frame_rows(y, M, flags, weights, frame0, D, dtype)
    x, hist = _fir(v, g, M, D, scale if scale else float(D), history, dtype)
    return (x, hist) if return_history else x


def synthesize_f32(y, g, M: int, D: int | None = None, scale: float = 0.0, flags: int = 0, weights=None,
                   frame0: int = 0):
    """The float32 / complex64 twin: the same sums in the stated order."""
    return synthesize(np.asarray(y).astype(np.complex64), np.asarray(g, dtype=np.float32), M, D, scale, flags,
                      None if weights is None else np.asarray(weights, dtype=np.float32), frame0, dtype=np.complex64)


def synthesize_literal(y, g, M: int, D: int | None = None, scale: float = 0.0, flags: int = 0, weights=None,
                       frame0: int = 0) -> np.ndarray:
    """The definition as loops over (s, q, c), float64; tiny sizes only."""
    D = M if D is None else D
    y = np.asarray(y, dtype=np.complex128).reshape(-1, M)
    g = np.asarray(g, dtype=np.float64)
    w = _weights(M, weights)
    F, Q = y.shape[0], g.size // D
    sc = scale if scale else float(D)
    kc = channel_of_column(M, flags)
    x = np.zeros(F * D, dtype=np.complex128)
    for b in range(F):
        for d in range(D):
            acc = 0j
            for q in range(Q):
                m = b - q
                if m < 0:
                    continue
                p = (d + q * D) % M
                if flags & DEROTATE:
                    p = (p + (frame0 + m) * D) % M
                vm = 0j
                for c in range(M):
                    vm += w[c] * y[m, c] * np.exp(2j * np.pi * ((int(kc[c]) * p) % M) / M)
                acc += g[d + q * D] * vm
            x[b * D + d] = sc * acc
    return x


def allowance(y, g, M: int, D: int | None = None, scale: float = 0.0, weights=None) -> np.ndarray:
    """A[s] = |scale| sum_q |g[d + qD]| ||w o y[b-q, :]||_1 for every output sample s = bD + d."""
    D = M if D is None else D
    y = np.asarray(y, dtype=np.complex128).reshape(-1, M)
    g = np.abs(np.asarray(g, dtype=np.float64))
    Q, F = g.size // D, y.shape[0]
    n1 = np.concatenate([np.zeros(Q - 1), (np.abs(y) * np.abs(_weights(M, weights))[None, :]).sum(axis=1)])
    A = np.zeros((F, D))
    for q in range(Q):
        A += g[q * D:(q + 1) * D][None, :] * n1[Q - 1 - q: Q - 1 - q + F][:, None]
    return abs(scale if scale else float(D)) * A.reshape(-1)


def quantize_int16(x, bit_width: int) -> np.ndarray:
    """round(x 2^(bit_width-1)), halves away from zero, saturated to the bit width; (N, 2) int16 I,Q.  The product
    and the rounding are taken in float32 as the kernel takes them."""
    full = np.float32(1 << (bit_width - 1))
    x = np.asarray(x).astype(np.complex64)
    out = np.empty((x.size, 2), dtype=np.int16)
    for i, part in enumerate((x.real, x.imag)):
        t = (part.astype(np.float32) * full).astype(np.float64)  # the float32 product, rounded from here exactly
        r = np.sign(t) * np.floor(np.abs(t) + 0.5)
        out[:, i] = np.clip(np.nan_to_num(r, nan=0.0), -float(full), float(full) - 1).astype(np.int16)
    return out


def synthesis_delay(analysis_len: int, synthesis_len: int, input_offset: int) -> int:
    return analysis_len // 2 + synthesis_len // 2 - input_offset
