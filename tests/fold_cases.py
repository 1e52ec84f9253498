"""The inputs the PRI-search tests share: the order-sensitive stream, the shape grid, and the chain of pd_cases folded
over the candidates around its PRI.  test_fold_cpu.py asserts on the restatement alone that each design is what
test_gpu_fold.py takes it for.  A support module, not a test."""
import functools

import numpy as np

import fold_ref as R
import mf_ref
import pd_cases

BIN_CELLS = (1, 2, 3, 4, 5, 8, 16, 64)
GRID_BINS = (1, 2, 63, 64, 65, 255, 256, 257, 513)
DIRECT = {1: "pfb_fold_direct<1>", 2: "pfb_fold_direct<2>", 3: "pfb_fold_direct<3>", 4: "pfb_fold_direct<4>"}
TILE_DEFAULT = (8, 16, 32, 64)       # the widths fold_tile runs by the library's choice


def direct_name(C):
    return DIRECT.get(C, "pfb_fold_direct<n>")


def kernel_name(C):
    """plan.kernel: the tier the library chooses for bin_cells = C"""
    return f"pfb_fold_tile<{C}>" if C in TILE_DEFAULT else direct_name(C)


def grid_periods(C):
    """the candidates of one handle: NB bins with L mod C in {0, 1, C-1}, one period twice, and the largest legal
    profile for this C where the grid's streams are shorter than its period (bins_used < num_bins)"""
    out = []
    for NB in GRID_BINS:
        for rem in sorted({0, min(1, C - 1), C - 1}):
            out.append(NB * C + rem)
    out.append(out[7])                         # a duplicate, a candidate of its own
    if C == 1:
        out.append(65536)                      # NB = 65536
    if C == 64:
        out.append(1 << 22)                    # the largest NB-legal shape: NB = 65536, L = 2^22
    return out


def grid_checkpoints(C, periods):
    """every N of {0, 1, C, L-1, L, L+1, 2L + C + 1, 5L + 3} of every period of the grid proper, ascending"""
    small = [L for L in periods if L // C <= max(GRID_BINS)]
    return sorted({n for L in small for n in (0, 1, C, L - 1, L, L + 1, 2 * L + C + 1, 5 * L + 3)})


def cut_periods(C):
    """the candidates of the cutting tests: short periods, so that one call spans many of them"""
    return [NB * C + rem for NB in (2, 63, 65, 257) for rem in sorted({0, min(1, C - 1), C - 1})]


def cut_stream(C):
    """40 periods of the longest candidate and a ragged end, order-sensitive"""
    return R.spread_stream(40 * max(cut_periods(C)) + 7, 100 + C)


ORDER_SHAPES = ((37, 1), (37, 4), (131, 4), (640, 5), (1000, 16), (4159, 64))


def order_stream(L):
    """what the cuttings run on, for one period: 40 periods and a ragged end of cells whose sum depends on its order"""
    return R.spread_stream(40 * L + 7, L)


class Walk:
    """the restatement taken along a stream cut at any points: profiles held per candidate, records on demand"""

    def __init__(self, periods, C):
        self.periods, self.C, self.N = [int(L) for L in periods], C, 0
        self.F = [np.zeros(L // C, np.float32) for L in self.periods]

    def take(self, p):
        self.F = [R.fold(p, L, self.C, self.N, F) for L, F in zip(self.periods, self.F)]
        self.N += len(p)

    def records(self):
        return np.array([R.score(F, self.N, L, self.C) for F, L in zip(self.F, self.periods)], R.SCORE)

    def bounds(self):
        return [R.sums_bound(F, self.N, L, self.C) for F, L in zip(self.F, self.periods)]


# -- the chain: pd_cases' train under the single-pulse threshold, compressed, folded around its PRI ----------------
CHAIN_C = 4
CHAIN_PERIODS = list(range(1984, 2113)) + [1024, 4096, 6144]
CHAIN_EXTRA = (1024, 4096, 6144)
CHAIN_FIRST_PULSE = pd_cases.CHAIN["first_pulse"]
CHAIN_CELLS = pd_cases.CHAIN_CPIS * pd_cases.CHAIN_K * pd_cases.CHAIN["pri"] - (pd_cases.CHAIN["pw"] - 1)


@functools.lru_cache(maxsize=1)
def chain_powers():
    """the float64 matched filter's powers of the chain's stream, rounded to float32 once"""
    y = mf_ref.compress(mf_ref.unpack(pd_cases.chain_stream(), "cf32", 16), pd_cases.chain_replica(), True)
    p = (y.real ** 2 + y.imag ** 2).astype(np.float32)
    p.setflags(write=False)
    return p


def chain_reference(p):
    """(records, profiles) of the chain's candidates over the powers p"""
    return R.scores(p, CHAIN_PERIODS, CHAIN_C)
