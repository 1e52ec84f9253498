"""The inputs the pulse-Doppler tests share: the shape grid, streams whose strongest Doppler row is clear of rounding,
exact ties, designed tones, and the pulse train under the single-pulse threshold.  test_pd_cpu.py asserts on the
float64 restatement alone that each design is what test_gpu_pd.py takes it for.  A support module, not a test."""
import numpy as np

import cfar_ref
import mf_ref
import pd_ref as R
import synth_ref


def tile_gates(nd):
    """plan.tile_gates of the transform kernels (test_pd_cpu.py holds it to pfb_pd_describe)"""
    return 256 if nd <= 16 else (4096 if nd <= 512 else 8192) // nd


def shapes(nd):
    """the grid of one Doppler length: (K, R, L), rows starting at odd element offsets for most L"""
    T = tile_gates(nd)
    out = []
    for K in sorted({1, nd // 2 + 1, nd - 1, nd}):
        for Rg in (1, T - 1, T, T + 1, 2 * T + 3):
            for L in sorted({Rg, Rg + 1, Rg + 5, 3 * Rg}):
                out.append((K, Rg, L))
    return out


def grid_window(K, index):
    """every third shape no window, else a positive taper with a ragged edge"""
    if index % 3 == 0:
        return None
    k = np.arange(K)
    return (0.6 - 0.4 * np.cos(2 * np.pi * (k + 0.5) / K) + 0.05 * (k % 3)).astype(np.float32)


def grid_flags(index):
    """(centered, input 8 bytes off a 16-byte boundary, output one element off one) of shape `index`: a hash, so that
    none of the three follows K, R or L"""
    h = (index * 2654435761 >> 7) & 7
    return bool(h & 1), bool(h & 2), bool(h & 4)


def tone_row(nd, c, r):
    """the Doppler row the grid's streams put a tone in, per interval and gate"""
    return (7 * r + 3 * c + 1) % nd


def grid_tail(K, L):
    """samples behind the last whole interval: up to three, and too few to complete another"""
    return min(3, K * L - 1)


def grid_stream(nd, K, Rg, L, seed, cpis=2, amplitude=2.0):
    """(x complex64, origin): unit noise everywhere, `cpis` whole intervals after `origin` ignored samples and
    grid_tail(K, L) samples behind them; gate r of interval c carries a tone of `amplitude` in row tone_row(nd, c, r)"""
    rng = np.random.default_rng(seed)
    o = seed % 7
    n = o + (cpis - 1) * K * L + R.cpi_samples(L, Rg, K) + grid_tail(K, L)
    x = (rng.standard_normal(n) + 1j * rng.standard_normal(n)) / np.sqrt(2.0)
    k, r = np.meshgrid(np.arange(K), np.arange(Rg), indexing="ij")
    for c in range(cpis):
        x[o + (c * K + k) * L + r] += amplitude * np.exp(2j * np.pi * ((tone_row(nd, c, r) * k) % nd) / nd)
    return x.astype(np.complex64), o


def clear_gates(P, A, w):
    """the gates whose largest power leads the runner-up by more than twice the allowance on a power"""
    top = np.sort(P, axis=0)[-2:]
    return (top[1] - top[0]) > 2.0 * R.power_bound(A, w)


def tie_stream(K, Rg, L, seed):
    """one interval whose only nonzero pulse is k = 0: every Doppler row of a gate holds the same value"""
    rng = np.random.default_rng(seed)
    x = np.zeros(R.cpi_samples(L, Rg, K), np.complex64)
    x[:Rg] = (rng.standard_normal(Rg) + 1j * rng.standard_normal(Rg)).astype(np.complex64)
    return x


def tone_stream(nd, Rg, L, d0_of_gate):
    """one interval of K = nd pulses: gate r is the unit tone e^{j 2 pi d0 k / nd} across the pulses, nothing else"""
    x = np.zeros(R.cpi_samples(L, Rg, nd), np.complex64)
    k, r = np.meshgrid(np.arange(nd), np.arange(Rg), indexing="ij")
    x[k * L + r] = np.exp(2j * np.pi * ((np.asarray(d0_of_gate)[r] * k) % nd) / nd).astype(np.complex64)
    return x


# -- the chain: a Barker-13 train whose pulses, compressed, sit at the noise level ------------------------------
CHAIN = dict(fs=2.0e6, pw=104, pri=2048, first_pulse=700, amplitude=0.0347, noise_sigma=0.25, seed=5, bit_width=16)
CHAIN_K, CHAIN_CPIS = 64, 3
CHAIN_SYNTH = dict(sample_format="cf32", barker13=True, barker_degrees=True, phase_from_zero=True, f0=31250.0)
CHAIN_CFAR = dict(block_cells=64, train_blocks=8)


def chain_stream(noise=True):
    """the train as the library's pulse source makes it (cf32, full scale 1), restated by synth_ref: (n, 2) float32"""
    c = CHAIN
    flags = synth_ref.BARKER13 | synth_ref.BARKER_DEGREES | synth_ref.PHASE_FROM_ZERO
    d = synth_ref.derive(c["pw"], c["pri"], c["fs"], CHAIN_SYNTH["f0"], c["bit_width"], flags, 0.0, c["amplitude"],
                         c["noise_sigma"] if noise else 0.0)
    n = CHAIN_CPIS * CHAIN_K * c["pri"] if noise else d["pw"]
    start = 0 if noise else c["first_pulse"]
    return synth_ref.stream(start, n, d, synth_ref.cos_table(c["bit_width"], c["amplitude"]), c["seed"], c["bit_width"],
                            "cf32", c["first_pulse"], 0, flags)


def chain_replica():
    iq = chain_stream(noise=False)
    return (iq[:, 0] + 1j * iq[:, 1]).astype(np.complex64)


def chain_shift(iq, bins):
    """the stream multiplied by e^{j 2 pi bins n / (K L)}, in float64 and rounded once: (n, 2) float32"""
    n = np.arange(len(iq))
    z = (iq[:, 0].astype(np.float64) + 1j * iq[:, 1]) * np.exp(2j * np.pi * ((bins * n) % (CHAIN_K * CHAIN["pri"]))
                                                               / (CHAIN_K * CHAIN["pri"]))
    return np.stack([z.real, z.imag], axis=1).astype(np.float32)


def chain_alphas(cfar_alpha):
    """(the single-pulse detector's factor, the train detector's): detect_pulses' and detect_pulse_train's defaults"""
    cells = 2 * CHAIN_CFAR["train_blocks"] * CHAIN_CFAR["block_cells"]
    harmonic = float(np.sum(1.0 / np.arange(1, CHAIN_K + 1)))
    return (float(np.float32(cfar_alpha(1e-7, cells))), float(np.float32(cfar_alpha(1e-6 / CHAIN_K, cells) / harmonic)))


def chain_reference(iq, alpha_single, alpha_train):
    """(single-pulse detections, train detections as (cpi, gate, bin) tuples) of the float64 chain"""
    r = chain_replica()
    Kr, C, T = r.size, CHAIN_CFAR["block_cells"], CHAIN_CFAR["train_blocks"]
    G = -(-Kr // C)
    y = mf_ref.compress(mf_ref.unpack(iq, "cf32", 16), r, True)
    p = (y.real ** 2 + y.imag ** 2).astype(np.float32)
    single, _ = cfar_ref.detect(p, len(p), True, C=C, G=G, T=T, alpha=alpha_single, merge_gap=Kr)
    L, K = CHAIN["pri"], CHAIN_K
    found = []
    for c, A in enumerate(R.intervals(y, len(y), True, 0, L, L, K)):
        bp, bh = R.best(R.power(R.transform(A, None, K, True)), K, True)
        det, _ = cfar_ref.detect(bp.astype(np.float32), L, True, C=C, G=G, T=T, alpha=alpha_train, merge_gap=Kr, hyp=bh)
        found += [(c, int(d["peak_index"]), int(d["hypothesis"])) for d in det]
    return single, found
