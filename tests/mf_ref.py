"""float64 numpy restatement of the matched filter (pfb_mf_* in include/pfb_channelizer.h) and the bound every
tolerance of its tests derives from.  Imported by basename like stft_ref.

    x[n] = (I[n] + jQ[n]) / 2^(bit_width-1)            (cf32: as given)
    y[m] = g * sum_{n=0}^{K-1} conj(r[n]) * x[m+n]        m = 0 .. N-K, nothing for N < K
    g = 1, or 1 / sum|r|^2 with normalize
"""
import numpy as np

FORMATS = (("int8", 8), ("int16", 12), ("cf32", 1))
TOL = 1e-5   # fp32 FFT results against the float64 restatement: the convention of tests/test_gpu_stft.py


def unpack(raw, fmt, bw):
    """interleaved raw samples (what goes to the library) -> complex128 in full scales"""
    a = np.asarray(raw).reshape(-1).astype(np.float64)
    full = 1.0 if fmt == "cf32" else 2.0 ** (bw - 1)
    return (a[0::2] + 1j * a[1::2]) / full


def gain(r, normalize):
    r = np.asarray(r, np.complex128)
    return 1.0 / float(np.sum(r.real ** 2 + r.imag ** 2)) if normalize else 1.0


def compress_loop(x, r, normalize=False):
    """the definition, literally"""
    x, r = np.asarray(x, np.complex128), np.asarray(r, np.complex128)
    K, N = r.size, x.size
    y = np.zeros(max(0, N - K + 1), np.complex128)
    for m in range(y.size):
        acc = 0j
        for n in range(K):
            acc += np.conj(r[n]) * x[m + n]
        y[m] = acc
    return gain(r, normalize) * y


def compress(x, r, normalize=False):
    """the same by one zero-padded FFT correlation in float64"""
    x, r = np.asarray(x, np.complex128), np.asarray(r, np.complex128)
    K, N = r.size, x.size
    if N < K:
        return np.zeros(0, np.complex128)
    L = 1 << int(np.ceil(np.log2(N + K)))
    y = np.fft.ifft(np.fft.fft(x, L) * np.conj(np.fft.fft(r, L)))[: N - K + 1]
    return gain(r, normalize) * y


def bound(x, r):
    """Bnd = ||r||_2 * max_m ||x[m .. m+K-1]||_2: the Cauchy-Schwarz limit of |y| / g, by a cumulative sum of |x|^2"""
    x, r = np.asarray(x, np.complex128), np.asarray(r, np.complex128)
    K = r.size
    if x.size < K:
        return 0.0
    c = np.concatenate([[0.0], np.cumsum(x.real ** 2 + x.imag ** 2)])
    return float(np.sqrt(np.sum(r.real ** 2 + r.imag ** 2)) * np.sqrt(np.max(c[K:] - c[:-K])))


def tolerance(x, r, normalize=False):
    """e = 1e-5 * g * Bnd: |y - ref| <= e for complex output"""
    return TOL * gain(r, normalize) * bound(x, r)


def span_tolerance(x, r, lo, hi, normalize=False):
    """The local allowance of samples [lo, hi): e of that slice alone.  The device computes a block from the block's own
    input span, so the outputs of blocks whose spans lie in [lo, hi) owe nothing to louder samples elsewhere."""
    return tolerance(np.asarray(x)[lo:hi], r, normalize)


def block_outputs(route, nfft, K):
    """outputs per block: the plan's block_outputs"""
    return nfft - K + 1 if route == "fused" else nfft // 2


def block_span(route, nfft, K, b):
    """The call-local samples [lo, hi) block b of a call is computed from (local sample 0 is the first carried one;
    what lies past the call's end reads as zero).  Fused: the block's nfft samples.  Partitioned: output block b combines
    the spectra of P half-overlapped nfft-point blocks, P + 1 half-blocks of B = nfft/2 samples."""
    if route == "fused":
        lo = b * (nfft - K + 1)
        return lo, lo + nfft
    B = nfft // 2
    P = -(-K // B)
    return b * B, (b + P + 1) * B


def outputs_seeing(route, nfft, K, s, outputs):
    """The call-local outputs [lo, hi) of the blocks whose input spans hold call-local sample s, of a call that completes
    `outputs` outputs: those a sample that is not finite may spoil.  Empty: lo == hi."""
    V = block_outputs(route, nfft, K)
    blocks = -(-outputs // V)
    if route == "fused":
        first, last = -(-(s - nfft + 1) // V), s // V
    else:
        B = nfft // 2
        first, last = s // B - -(-K // B), s // B
    first, last = max(first, 0), min(last, blocks - 1)
    if first > last:
        return 0, 0
    return first * V, min((last + 1) * V, outputs)


def worst_ratio(y, ref, e, output):
    """The largest error over its allowance (<= 1 passes), and over the 1e-5 allowance's own unit: returns
    (ratio, error / (g Bnd)).  Power output: |p - |ref|^2| <= e (2|ref| + e), the same bound carried through the square."""
    y = np.asarray(y)
    if y.size == 0:
        return 0.0, 0.0
    if output == "complex":
        err = np.abs(y.astype(np.complex128) - ref)
        allow = np.full(err.shape, e)
    else:
        err = np.abs(y.astype(np.float64) - np.abs(ref) ** 2)
        allow = e * (2 * np.abs(ref) + e)
    if e == 0.0:
        return (0.0 if not err.any() else np.inf), 0.0
    k = int(np.argmax(err / allow))
    return float(err[k] / allow[k]), float(err[k] / allow[k] * TOL)


def random_replica(K, seed):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal(K) + 1j * rng.standard_normal(K)).astype(np.complex64)


def random_raw(fmt, bw, n, seed):
    """n samples, interleaved, of the dtype the library takes"""
    rng = np.random.default_rng(seed)
    if fmt == "cf32":
        return rng.standard_normal(2 * n).astype(np.float32)
    lim = 2 ** (bw - 1)
    return rng.integers(-lim, lim, size=2 * n).astype(np.int8 if fmt == "int8" else np.int16)
