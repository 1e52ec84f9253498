"""float64 reference of the STFT contract (include/pfb_channelizer.h, pfb_stft_*), numpy only.

frame m covers x[m H .. m H + L - 1];  s[r, m] = sum_{n<L} w[n] x[m H + n] e^{-j 2 pi k_r n / nfft}
'centered': k_r = r - nfft/2 + 1 (even nfft) / r - (nfft-1)/2 (odd);  'twosided': k_r = r.
Results are frame-major, shape (frames, nfft): row m is MATLAB's column m+1 of s.
"""
from __future__ import annotations

import numpy as np


def unpack(iq, fmt: str, bit_width: int = 12) -> np.ndarray:
    """Raw interleaved I,Q (int8 / int16 / float32 or complex) -> complex128, (I + jQ) / 2^(bit_width-1)."""
    a = np.asarray(iq)
    if np.iscomplexobj(a):
        return a.astype(np.complex128).reshape(-1)
    a = a.reshape(-1, 2).astype(np.float64)
    x = a[:, 0] + 1j * a[:, 1]
    return x if fmt == "cf32" else x / 2.0 ** (bit_width - 1)


def num_frames(n: int, L: int, H: int) -> int:
    return (n - L) // H + 1 if n >= L else 0


def bins(nfft: int, order: str = "centered") -> np.ndarray:
    r = np.arange(nfft)
    if order == "twosided":
        return r
    return r - (nfft // 2 - 1 if nfft % 2 == 0 else (nfft - 1) // 2)


def stft(x: np.ndarray, window, H: int, nfft: int, order: str = "centered") -> np.ndarray:
    w = np.asarray(window, dtype=np.float64)
    L = w.size
    F = num_frames(x.size, L, H)
    if F == 0:
        return np.zeros((0, nfft), np.complex128)
    idx = np.arange(F)[:, None] * H + np.arange(L)[None, :]
    S = np.fft.fft(x[idx] * w[None, :], nfft, axis=1)
    return S[:, np.mod(bins(nfft, order), nfft)]


def stft_direct(x: np.ndarray, window, H: int, nfft: int, order: str = "centered") -> np.ndarray:
    """The definition summed term by term, O(nfft L) per frame: checks stft() itself."""
    w = np.asarray(window, dtype=np.float64)
    L = w.size
    F = num_frames(x.size, L, H)
    k = bins(nfft, order)
    E = np.exp(-2j * np.pi * np.outer(k, np.arange(L)) / nfft)
    return np.array([E @ (w * x[m * H: m * H + L]) for m in range(F)]).reshape(F, nfft)


def power(s: np.ndarray, scale: float = 1.0) -> np.ndarray:
    return scale * np.abs(s) ** 2


def db(s: np.ndarray, scale: float = 1.0, floor: float = 0.0) -> np.ndarray:
    with np.errstate(divide="ignore"):
        return 10.0 * np.log10(power(s, scale) + floor)


def axes(nfft: int, L: int, H: int, fs: float, order: str, first_frame: int, frames: int):
    f = bins(nfft, order) * fs / nfft
    t = ((first_frame + np.arange(frames)) * H + L / 2.0) / fs
    return f, t
