"""The inputs the fractional-PRI tests share: the period grid, the motivating scene (a train at 2048.37 samples that no
integer fold finds) and the chain scene (a Barker-13 train under the single-pulse threshold at a fractional PRI).
test_qfold_cpu.py asserts on the restatements alone that each design is what test_gpu_qfold.py takes it for.  A support
module, not a test."""
import functools
from fractions import Fraction

import numpy as np

import cfar_ref
import mf_ref
import pd_cases
import pd_ref
import qfold_ref as R

BIN_CELLS = (1, 2, 3, 4, 5, 8, 16, 64)
GRID_BINS = (1, 63, 64, 65, 513)             # one tile, a tile boundary, a tail tile of one bin
FRACTIONS = (0, 1, 1 << 31, (1 << 32) - 1)
TILE_DEFAULT = (8, 16, 32, 64)               # the widths qfold_tile runs by the library's choice


def direct_name(C):
    return f"pfb_qfold_direct<{C}>" if C <= 4 else "pfb_qfold_direct<n>"


def kernel_name(C):
    """plan.kernel: the tier the library chooses for bin_cells = C"""
    return f"pfb_qfold_tile<{C}>" if C in TILE_DEFAULT else direct_name(C)


def grid_periods(C, bins=GRID_BINS):
    """the candidates of one handle, Q32: NB bins with Pi = NB C (the last bin alternates C and C + 1 cells) and
    Pi = NB C + C - 1, each at every fraction; NB = 1 with Pi = C is the one-bin period.  One period twice."""
    out = []
    for NB in bins:
        for rem in sorted({0, C - 1}):
            for Pf in FRACTIONS:
                out.append(((NB * C + rem) << 32) | Pf)
    out.append(out[5])
    return out


def checkpoints(C, Pq):
    """N of {0, 1, C, Pi - 1, Pi, Pi + 1, start(2) - 1, start(2), start(2) + 1, 5 periods + 3} of one period"""
    Pi = Pq >> 32
    s2 = R.start(2, Pq)
    return sorted({0, 1, C, Pi - 1, Pi, Pi + 1, s2 - 1, s2, s2 + 1, R.start(5, Pq) + 3})


def grid_checkpoints(C, periods):
    """the checkpoints of every period of the grid, ascending, and the end of the grid's stream"""
    pts = {n for q in periods for n in checkpoints(C, q)}
    return sorted(pts | {grid_cells(C, periods)})


def grid_cells(C, periods):
    """5 periods + 3 of the longest candidate"""
    return R.start(5, max(periods)) + 3


# -- the motivating scene: exponential noise, 512 pulses of +1.5 at 700 + ceil(k 2048.37) --------------------------
SCENE_C, SCENE_CELLS, SCENE_PULSES, SCENE_FIRST = 4, 1 << 20, 512, 700
SCENE_PERIOD = Fraction(204837, 100)
SCENE_Q = R.q32(SCENE_PERIOD)
SCENE_INTEGERS = list(range(2040, 2057))
SCENE_OFFSETS = [Fraction(s * d, 1000) for d in (0, 2, 4, 10, 20) for s in ((1,) if d == 0 else (-1, 1))]


def scene(seed):
    """the power stream of one seed, float32"""
    rng = np.random.default_rng(seed)
    p = rng.exponential(1.0, SCENE_CELLS).astype(np.float32)
    at = np.array([SCENE_FIRST + R.start(k, SCENE_Q) for k in range(SCENE_PULSES)])
    p[at[at < SCENE_CELLS]] += np.float32(1.5)
    return p


def scene_z(p, periods_q32):
    """z of every candidate over the whole stream, by the restatement"""
    rec = np.array([R.score(R.fold(p, q, SCENE_C), len(p), q, SCENE_C) for q in periods_q32], R.SCORE)
    return R.z(rec), rec


# -- the chain scene: pd_cases' pulse, placed at first + ceil(k Pq / 2^32), with a Doppler step -------------------
CHAIN_PERIOD = Fraction(204837, 100)
CHAIN_Q = R.q32(CHAIN_PERIOD)
CHAIN_K, CHAIN_CPIS = pd_cases.CHAIN_K, pd_cases.CHAIN_CPIS
CHAIN_FIRST = pd_cases.CHAIN["first_pulse"]
CHAIN_ROW = 2048                             # row_samples: floor(period)
CHAIN_BIN = 5                                # the Doppler row of the train: a phase step of 2 pi 5 / 64 a pulse
CHAIN_SAMPLES = R.start(CHAIN_CPIS * CHAIN_K, CHAIN_Q) + pd_cases.CHAIN["pw"] - 1   # the compressed stream ends with the last row
CHAIN_FOLD_C = 4
# The search step the record can resolve: a candidate off by d walks the last of the K CPIS pulses d K CPIS cells, and
# the train stays in one phase bin while that is under bin_cells -- d < 4 / 192 = 0.021.  Candidates closer together
# than that differ by noise alone, so "the true period first" can only mean to within one such step.
CHAIN_STEP = 0.02


@functools.lru_cache(maxsize=4)
def chain_stream(period_q32=CHAIN_Q):
    """(n, 2) float32: complex noise of pd_cases' sigma and its pulse, pulse k at first + ceil(k Pq / 2^32) with phase
    2 pi CHAIN_BIN k / K; float64 sums rounded once"""
    c = pd_cases.CHAIN
    rng = np.random.default_rng(c["seed"])
    x = (rng.normal(0, c["noise_sigma"], CHAIN_SAMPLES) + 1j * rng.normal(0, c["noise_sigma"], CHAIN_SAMPLES))
    r = pd_cases.chain_replica().astype(np.complex128)
    for k in range(CHAIN_CPIS * CHAIN_K):
        at = CHAIN_FIRST + R.start(k, period_q32)
        if at + len(r) <= CHAIN_SAMPLES:
            x[at:at + len(r)] += r * np.exp(2j * np.pi * ((CHAIN_BIN * k) % CHAIN_K) / CHAIN_K)
    out = np.stack([x.real, x.imag], axis=1).astype(np.float32)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=4)
def chain_compressed(period_q32=CHAIN_Q):
    """the float64 matched filter's output of the chain's stream (valid part), complex128"""
    return mf_ref.compress(mf_ref.unpack(chain_stream(period_q32), "cf32", 16), pd_cases.chain_replica(), True)


def chain_powers(period_q32=CHAIN_Q):
    y = chain_compressed(period_q32)
    return (y.real ** 2 + y.imag ** 2).astype(np.float32)


def chain_alphas(cfar_alpha):
    """(the single-pulse detector's factor, the train detector's), as pd_cases' chain takes them"""
    return pd_cases.chain_alphas(cfar_alpha)


def chain_detect(y, L, alpha_train):
    """train detections [(cpi, gate, bin)] of pd_ref + cfar_ref on a compressed stream folded at the integer pri L from
    origin 0, and the best cell power per interval"""
    r = pd_cases.chain_replica()
    C, T = pd_cases.CHAIN_CFAR["block_cells"], pd_cases.CHAIN_CFAR["train_blocks"]
    G = -(-r.size // C)
    found, peaks = [], []
    for c, A in enumerate(pd_ref.intervals(y, len(y), True, 0, L, L, CHAIN_K)):
        bp, bh = pd_ref.best(pd_ref.power(pd_ref.transform(A, None, CHAIN_K, True)), CHAIN_K, True)
        det, _ = cfar_ref.detect(bp.astype(np.float32), L, True, C=C, G=G, T=T, alpha=alpha_train, merge_gap=r.size, hyp=bh)
        found += [(c, int(d["peak_index"]), int(d["hypothesis"])) for d in det]
        peaks.append(float(bp.max()))
    return found, peaks


def chain_regridded(y, period_q32=CHAIN_Q, origin=0):
    """the compressed stream laid on rows of CHAIN_ROW samples by the restatement"""
    _, out = R.regrid(y, 0, period_q32, CHAIN_ROW, origin)
    return out
