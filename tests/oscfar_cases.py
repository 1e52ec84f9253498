"""The inputs the ordered-statistic CFAR tests share: noise maps with raised cells, maps quantised to four values so
that every rank boundary falls inside a run of equal values, non-finite cells at, below and above the rank, signed zeros
as the selected value, the masking scene that is the unit's purpose, and the pulse-Doppler chain with a second train in
the first one's training window.  test_oscfar_cpu.py asserts on the restatement alone that each design is what
test_gpu_oscfar.py takes it for.  A support module, not a test."""
import numpy as np

import oscfar_ref as O
import pd_cases
import rdcfar_cases
import rdcfar_ref as R

TILE = 256   # plan.tile_gates (test_oscfar_cpu.py holds it to pfb_oscfar_describe)
noise_maps = rdcfar_cases.noise_maps


def quantised_maps(n, ND, Rg, seed, raised=0.02):
    """cells drawn from {0, 1, 2, 3}, a few raised to 9: every order statistic is one of four values, so ties sit at
    every rank boundary"""
    rng = np.random.default_rng(seed)
    p = rng.integers(0, 4, (n, ND, Rg)).astype(np.float32)
    p[rng.random((n, ND, Rg)) < raised] = 9.0
    return p


# -- non-finite cells at the rank -----------------------------------------------------------------------------------
# Wd = 0: a cell's training set is 2 Tr gates of its own row.  Each designed cell stands at 500 with c of its training
# gates set to a special value; with rank 6 of 8, c = 2, 3, 4 copies of NaN or +Inf (sorted last) put the first of them
# one above, at and one below the rank; c = 5, 6, 7 copies of -Inf (sorted first) put the last of them one below, at
# and one above it.
NONFINITE = dict(Wd=0, Gr=2, Tr=4, Pd=1, rank=6, alpha=6.0)
NONFINITE_ROWS = (1, 4)     # the rows rdcfar_cases.nonfinite_map() leaves as noise
NONFINITE_DESIGN = [(v, c) for v, cs in ((np.nan, (2, 3, 4)), (np.inf, (2, 3, 4)), (-np.inf, (5, 6, 7))) for c in cs]


def nonfinite_gate(i):
    """25 apart, and clear of the peak boxes of what rdcfar_cases.nonfinite_map() put into the rows next to them"""
    return 12 + 25 * i


def nonfinite_map():
    """rdcfar_cases.nonfinite_map() (NaN, +Inf and -Inf as test cell, training cell and peak-box neighbour) with the
    designed cells in two more rows"""
    p = rdcfar_cases.nonfinite_map()
    c = NONFINITE
    for row in NONFINITE_ROWS:
        for i, (v, copies) in enumerate(NONFINITE_DESIGN):
            g = nonfinite_gate(i)
            window = [g + c["Gr"] + 1 + t for t in range(c["Tr"])] + [g - c["Gr"] - 1 - t for t in range(c["Tr"])]
            p[row, g] = 500.0
            p[row, window[:copies]] = v
    return p


# -- signed zeros ---------------------------------------------------------------------------------------------------
ZEROS = dict(Wd=1, Gr=1, Tr=2, Pd=0, rank=5, alpha=2.0)


def zeros_map(ND=6, Rg=TILE + 20):
    """three rows of -0.0 and three of +0.0 (Wd = 1: the cells of rows 1 and 4 train on one sign alone, the others on
    both), with cells of 1 and of 5: the selected value is a zero of either sign, or 1 where enough ones stand in the
    window"""
    p = np.zeros((ND, Rg), np.float32)
    p[0:3] = -0.0
    rng = np.random.default_rng(8)
    p[rng.random((ND, Rg)) < 0.2] = 1.0
    p[rng.random((ND, Rg)) < 0.03] = 5.0
    p[3:6, 100:130] = 1.0    # a stretch where the selected value is 1
    p[4, 115] = 5.0
    return p


# -- the masking scene ----------------------------------------------------------------------------------------------
# Three targets ten gates apart in one row, each inside the others' training windows, and one on its own.  The mean of
# 32 cells with a 200 among them is raised sevenfold; the 24th smallest of 32 does not move.
MASK = dict(Wd=0, Gr=2, Tr=16, Pd=0)
MASK_RANK = 24
MASK_PFA = 1e-6
MASK_TARGETS = [(3, 300), (3, 310), (3, 320), (5, 100)]
MASK_MISSED = (3, 310)


def mask_map():
    rng = np.random.default_rng(0)
    p = rng.exponential(1.0, (8, 600)).astype(np.float32)
    p[3, 300], p[3, 310], p[3, 320], p[5, 100] = 200.0, 180.0, 220.0, 200.0
    return p


def mask_alphas():
    """(the CA factor, the ordered-statistic factor) for MASK_PFA as float32 values, from the formulas"""
    N = O.full_cells(MASK["Wd"], MASK["Tr"])
    return (float(np.float32(N * (MASK_PFA ** (-1.0 / N) - 1.0))), float(np.float32(O.alpha_ref(MASK_PFA, N, MASK_RANK))))


# -- the chain: pd_cases.CHAIN with a second, far stronger train on the same Doppler bin -------------------------------
# The second train stands CHAIN_OFFSET gates behind the first: outside its guard (Gr = len(replica) = 104), inside its
# lag window (Tr = 128).  Its compressed peak and its range sidelobes (Barker 13: 1/169 of the peak over 103 gates either
# side) fill about 104 + 1 of the first train's 768 training cells and raise their mean fortyfold.
# On the float64 reference, over the three intervals: under CA (factor 25, as rdcfar_cases) the first train stands at
# 0.05 to 0.08 of its threshold and is missed.  Under rank 384 of 768 it stands 61.7 to 96.2 times its noise while the
# largest cell that is neither train (nor inside a train's guard) stands 18.6 times its own: a ratio of 3.3, and
# 3.3 at rank 576 and 3.0 at rank 192 too.  The compressed noise is correlated over a chip, so the chain's SNR allows no
# factor with 2 on both sides (that needs a ratio of 4).  33 puts the weaker train at >= 1.8 times its threshold and
# every other cell at <= 0.57 of its own; test_oscfar_cpu.py holds 1.7 and 0.6.  The scene that carries a factor of 2 on
# both sides is the map-level one above.
CHAIN_OFFSET = 232
CHAIN_RATIO = 12.0        # the second train's amplitude over the first's
CHAIN_RD = dict(Wd=1, Tr=128, Pd=1)
CHAIN_RANK = 384          # N / 2 of 768
CHAIN_CA_ALPHA = rdcfar_cases.CHAIN_ALPHA
CHAIN_OS_ALPHA = 33.0


def chain_stream():
    """pd_cases.chain_stream() plus the noiseless train once more, CHAIN_RATIO of it, CHAIN_OFFSET samples later:
    float64, rounded once to (n, 2) float32"""
    c = pd_cases.CHAIN
    iq = pd_cases.chain_stream()
    r = pd_cases.chain_replica().astype(np.complex128)
    n = len(iq)
    second = np.zeros(n, np.complex128)
    for s in range(c["first_pulse"] + CHAIN_OFFSET, n - r.size + 1, c["pri"]):
        second[s:s + r.size] = r
    z = iq[:, 0].astype(np.float64) + 1j * iq[:, 1] + CHAIN_RATIO * second
    return np.stack([z.real, z.imag], axis=1).astype(np.float32)


chain_maps = rdcfar_cases.chain_maps


def chain_detect_ca(maps):
    Gr = pd_cases.chain_replica().size
    return R.detect(maps, CHAIN_RD["Wd"], Gr, CHAIN_RD["Tr"], CHAIN_RD["Pd"], R.CA, CHAIN_CA_ALPHA, 0.0)


def chain_detect_os(maps):
    Gr = pd_cases.chain_replica().size
    return O.detect(maps, CHAIN_RD["Wd"], Gr, CHAIN_RD["Tr"], CHAIN_RD["Pd"], CHAIN_RANK, CHAIN_OS_ALPHA, 0.0)
