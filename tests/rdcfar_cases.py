"""The inputs the range-Doppler CFAR tests share: noise maps with raised cells, maps whose float64 sums depend on their
order, exact ties inside and outside a peak box, non-finite cells, and the pulse-Doppler chain with a second, weaker
train in the same gate.  test_rdcfar_cpu.py asserts on the restatement alone that each design is what
test_gpu_rdcfar.py takes it for.  A support module, not a test."""
import numpy as np

import mf_ref
import pd_cases
import pd_ref
import rdcfar_ref as R

TILE = 256   # plan.tile_gates (test_rdcfar_cpu.py holds it to pfb_rdcfar_describe)


def noise_maps(n, ND, Rg, seed, share=0.01, level=300.0):
    """unit exponential noise, `share` of the cells raised by `level`"""
    rng = np.random.default_rng(seed)
    p = rng.exponential(1.0, (n, ND, Rg))
    p[rng.random((n, ND, Rg)) < share] *= level
    return p.astype(np.float32)


# -- order dependence ---------------------------------------------------------------------------------------------
BIG = np.float32(2.0 ** 90)   # BIG + s == BIG in float64 for every s of order 1
ORDER_GATES = dict(Wd=0, Gr=1, Tr=8, Pd=0, alpha=4.0)   # Tr a multiple of 4: every window holds as many +BIG as -BIG
ORDER_ROWS = dict(Wd=1, Gr=0, Tr=3, Pd=1, alpha=4.0)


def order_map_gates(ND=5, Rg=2 * TILE + 3, seed=3):
    """along the gates +BIG, s, -BIG, s', ...: a window's sum is what the small values leave after the cancellations,
    and that depends on where the walk begins; each row starts at another phase"""
    rng = np.random.default_rng(seed)
    p = rng.uniform(0.5, 1.5, (ND, Rg)).astype(np.float32)
    d, r = np.meshgrid(np.arange(ND), np.arange(Rg), indexing="ij")
    ph = (d + r) % 4
    p[ph == 0] = BIG
    p[ph == 2] = -BIG
    return p


def order_map_rows(ND=9, Rg=TILE + 1, seed=4):
    """down the rows +BIG, s, -BIG with period 3 (ND a multiple of 3), for Wd = 1: A is 0 or s by the order of j"""
    rng = np.random.default_rng(seed)
    p = rng.uniform(0.5, 1.5, (ND, Rg)).astype(np.float32)
    d, r = np.meshgrid(np.arange(ND), np.arange(Rg), indexing="ij")
    ph = (d + r) % 3
    p[ph == 0] = BIG
    p[ph == 2] = -BIG
    return p


# -- ties and the peak box ----------------------------------------------------------------------------------------
TIE = dict(Wd=1, Gr=2, Tr=8, Pd=1, alpha=5.0)
TIE_SHAPE = (16, 2 * TILE + 90)
# pairs of equal cells inside one peak box: the lower (row, gate) is reported
TIE_INSIDE = [((3, TILE - 1), (3, TILE)),        # two tiles
              ((7, 63), (7, 64)),                # two waves
              ((5, 10), (5, 12)),                # two lanes, Gr apart
              ((7, 300), (8, 300)),              # two row bands (tile_rows = 8)
              ((0, 400), (15, 400)),             # rows 0 and ND-1: the box wraps; (0, 400) is the lower
              ((11, 2 * TILE - 1), (12, 2 * TILE + 1))]   # a diagonal over a tile and a row
# pairs of equal cells just outside each other's box: both are reported
TIE_OUTSIDE = [((3, 100), (3, 103)),             # Gr + 1 gates apart
               ((10, 200), (12, 200)),           # Pd + 1 rows apart
               ((1, 350), (14, 350))]            # three rows apart through the wrap


def tie_map():
    p = np.ones(TIE_SHAPE, np.float32)
    for a, b in TIE_INSIDE + TIE_OUTSIDE:
        p[a] = p[b] = 100.0
    return p


# -- non-finite cells ---------------------------------------------------------------------------------------------
NONFINITE = dict(Wd=1, Gr=2, Tr=4, Pd=1, alpha=6.0)


def nonfinite_map(ND=8, Rg=TILE + 40, seed=9):
    """NaN, +Inf and -Inf as test cell, as training cell of a raised cell and as its peak-box neighbour"""
    rng = np.random.default_rng(seed)
    p = rng.exponential(1.0, (ND, Rg)).astype(np.float32)
    for k, v in enumerate((np.nan, np.inf, -np.inf)):
        g = 30 + 60 * k
        p[2, g] = v            # the test cell itself
        p[5, g] = 500.0
        p[5, g + 4] = v        # in the lag set of (5, g)
        p[6, g + 20] = 500.0
        p[7, g + 21] = v       # in the peak box of (6, g + 20)
        p[0, g + 40] = 500.0
        p[ND - 1, g + 40] = v  # a Doppler neighbour through the wrap: in the column sums of (0, g + 40 +- ...)
    p[3, 250] = p[3, 252] = np.inf   # equal infinities in one box: a tie
    return p


# -- the chain: pd_cases.CHAIN with a second train in gate 700 on another Doppler bin ------------------------------
CHAIN2_BIN = 9            # the second train turns by CHAIN2_BIN / (K L) of a cycle per sample
CHAIN2_RATIO = 0.95       # its amplitude over the first train's
# Gr = len(replica).  The compressed noise is correlated over a chip (8 gates), so 128 gates per side are about 16
# independent ones per row.  Over the three intervals the largest noise cell is 11.9 times its noise and the weakest of
# the six peaks 53.5 times: 25 puts every noise cell under half its threshold and every peak over twice its own.
CHAIN_RD = dict(Wd=1, Tr=128, Pd=1)
CHAIN_ALPHA = 25.0


def chain2_stream():
    """pd_cases.chain_stream() plus the noiseless train once more, CHAIN2_RATIO of it, turned by CHAIN2_BIN: float64,
    rounded once to (n, 2) float32"""
    c = pd_cases.CHAIN
    iq = pd_cases.chain_stream()
    r = pd_cases.chain_replica().astype(np.complex128)
    n = len(iq)
    second = np.zeros(n, np.complex128)
    for s in range(c["first_pulse"], n - r.size + 1, c["pri"]):
        second[s:s + r.size] = r
    KL = pd_cases.CHAIN_K * c["pri"]
    second *= CHAIN2_RATIO * np.exp(2j * np.pi * ((CHAIN2_BIN * np.arange(n)) % KL) / KL)
    z = iq[:, 0].astype(np.float64) + 1j * iq[:, 1] + second
    return np.stack([z.real, z.imag], axis=1).astype(np.float32)


def chain_maps(iq, window=None):
    """the float64 chain's power maps, centered rows, as float32 (intervals, K, L)"""
    L, K = pd_cases.CHAIN["pri"], pd_cases.CHAIN_K
    y = mf_ref.compress(mf_ref.unpack(iq, "cf32", 16), pd_cases.chain_replica(), True)
    return np.stack([pd_ref.power(pd_ref.transform(A, window, K, True)).astype(np.float32)
                     for A in pd_ref.intervals(y, len(y), True, 0, L, L, K)])


def chain_default_alpha(cfar_alpha):
    """detect_targets' factor for the default pfa"""
    return float(np.float32(cfar_alpha(1e-6, 2 * CHAIN_RD["Tr"] * (2 * CHAIN_RD["Wd"] + 1))))


def chain_hann():
    return np.hanning(pd_cases.CHAIN_K + 2)[1:-1].astype(np.float32)


def chain_detect(maps, alpha):
    Gr = pd_cases.chain_replica().size
    return R.detect(maps, CHAIN_RD["Wd"], Gr, CHAIN_RD["Tr"], CHAIN_RD["Pd"], R.CA, alpha, 0.0)
