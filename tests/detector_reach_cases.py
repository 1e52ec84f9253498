"""The inputs with which the three detector units (pfb_cfar_*, pfb_rdcfar_*, pfb_oscfar_*) are taken past the caps of
their grids: sequences of maps so long that a workgroup of *_cells<lds> takes a second and third (map, band, tile), and
streams so dense in detections that cfar_runs goes over its list of starts more than once.  The kernel constants the
designs rest on stand here; test_detector_reach_cpu.py holds them to the sources and asserts on the restatements alone
that each design is what test_gpu_detector_reach.py takes it for.  A support module, not a test."""
import numpy as np

import rdcfar_cases

GRID_CAP = 1 << 16      # kMaxGrid in pfb_cfar.hip and in pfb_rdmap.hpp (pfb_rdcfar.hip, pfb_oscfar.hip)
RUN_GRID = 1024         # workgroups of the cfar_runs launch in launch_step (pfb_cfar.hip), one wave and one run each
STEP_CELLS = 1 << 24    # kStepCells in pfb_cfar.hip and pfb_rdmap.hpp: cells of a step at most
STEP_WORDS = 1 << 18    # kStepWords in pfb_rdmap.hpp: words of 64 gates of a step at most
TILE = 256              # kTileGates in pfb_rdmap.hpp (plan.tile_gates)

noise_maps = rdcfar_cases.noise_maps


# -- long sequences of small maps -----------------------------------------------------------------------------------
# A call's maps repeat DISTINCT different ones, so the restatement runs over those alone (tiled_records).  DISTINCT is
# a prime: with NB = NT = 1 the units u and u + GRID_CAP of one workgroup are the maps m and m + GRID_CAP, and
# GRID_CAP % 61 = 22, so they never hold the same cells.  With 64 they always would, and a block left in LDS by the
# first unit would serve the second one unnoticed.
DISTINCT = 61

# maps: what one call takes; `what` for the reader.  A step takes step_maps(ND, R) maps.
CASES_2D = {
    # one step; every workgroup takes 2 or 3 units; NB = NT = 1
    "A": dict(ND=1, R=24, Wd=0, Gr=1, Tr=3, Pd=0, maps=2 * GRID_CAP + 100, alpha=4.0, share=0.05, seed=101),
    # a full step of 87381 maps and a short one: halo rows wrapped on re-staging, nb = 3 < band_rows = 4, map0 > 0
    "B": dict(ND=3, R=24, Wd=1, Gr=1, Tr=3, Pd=1, maps=87381 + 19, alpha=4.5, share=0.03, seed=102),
    # a full step of 29127 maps, 87381 units, and a short one; NT = 3 and GRID_CAP % 3 = 1: a workgroup's second unit
    # is the next gate tile of another map
    "C": dict(ND=1, R=520, Wd=0, Gr=2, Tr=8, Pd=0, maps=29127 + 40, alpha=5.0, share=0.02, seed=103),
}
# (case, unit, method or rank): "ca" / "go" for RangeDopplerCfar, an integer rank for OsCfar
VARIANTS_2D = [("A", "rdcfar", "ca"), ("A", "oscfar", 4),       # rank 4 of N = 6
               ("B", "rdcfar", "ca"), ("B", "rdcfar", "go"), ("B", "oscfar", 12),   # rank 12 of N = 18
               ("C", "rdcfar", "ca"), ("C", "oscfar", 12)]      # rank 12 of N = 16


def step_maps(ND, R):
    """maps of one step: the step rule of rdcfar_step and oscfar_step"""
    return max(1, min(STEP_CELLS // (ND * R), STEP_WORDS // (ND * -(-R // 64))))


def distinct_maps(case):
    c = CASES_2D[case]
    return noise_maps(DISTINCT, c["ND"], c["R"], seed=c["seed"], share=c["share"])


def tiled(distinct, n):
    """n maps: the D distinct ones over and over, map m holding distinct[m % D]"""
    return np.ascontiguousarray(distinct[np.arange(n) % len(distinct)])


def tiled_records(ref_records, ref_stats, D, n, rem_stats=None, first_map=0):
    """(records, stats) of tiled(distinct, n) taken as maps first_map .. first_map + n - 1, from the restatement's
    records and stats of the D distinct maps (first_map 0).  Maps are decided each on its own and the records ascend in
    (map, row, gate), so map m's records are those of map m % D with the map field moved: repeat them, add k D to the
    k-th copy, cut at map n.  The stats are n // D times those of the D maps plus `rem_stats`, the restatement's of the
    first n % D of them (needed unless D divides n)."""
    reps = -(-n // D)
    rec = np.tile(ref_records, reps)
    rec["map"] += np.repeat(np.arange(reps, dtype=np.uint64) * np.uint64(D), len(ref_records))
    rec = rec[rec["map"] < n]
    rec["map"] += np.uint64(first_map)
    q, rem = divmod(n, D)
    assert rem == 0 or rem_stats is not None
    stats = {k: q * v + (rem_stats[k] if rem else 0) for k, v in ref_stats.items()}
    assert stats["maps_in"] == n
    return rec, stats


def unit_block(case, plan_rows, u, distinct=None):
    """what the workgroup of unit u of the case's first step stages: (m % D, the block's cells with the halo of rows
    wrapped and the halo of gates clipped to zeros), decoded as u = (m NB + b) NT + t"""
    c = CASES_2D[case]
    distinct = distinct_maps(case) if distinct is None else distinct
    ND, R, GT, H = c["ND"], c["R"], c["Gr"] + c["Tr"], max(c["Wd"], c["Pd"])
    NT, NB = -(-R // TILE), -(-ND // plan_rows)
    t, b, m = u % NT, (u // NT) % NB, u // (NT * NB)
    d0 = b * plan_rows
    nb = min(plan_rows, ND - d0)
    rows = (d0 - H + np.arange(nb + 2 * H)) % ND
    gates = t * TILE - GT + np.arange(TILE + 2 * GT)
    ok = (gates >= 0) & (gates < R)
    block = np.where(ok[None, :], distinct[m % DISTINCT][rows][:, np.where(ok, gates, 0)], np.float32(0.0))
    return m, block


# -- a dense map for the cell-averaging detector ----------------------------------------------------------------------
# the map of test_gpu_oscfar.test_maps_that_are_mostly_detections; (Gr, Pd) -> (detections, over cells) of the
# restatement, of 2 * 8 * 326 = 5216 cells
DENSE = dict(n=2, ND=8, R=TILE + 70, seed=13, share=0.01, Wd=1, Tr=3, alpha=0.5)
DENSE_RD = {(0, 0): (2770, 2770), (1, 1): (508, 2764)}
DENSE_OS = dict(Gr=1, rank=1, Pd=(0, 1))


def dense_maps():
    d = DENSE
    return noise_maps(d["n"], d["ND"], d["R"], seed=d["seed"], share=d["share"])


# -- streams that are mostly detections -----------------------------------------------------------------------------
# configs: (C, G, T); gaps: merge_gap -> (runs after the flush, the least whole multiple of RUN_GRID that the
# candidates of the one unflushed call exceed: cfar_runs makes factor + 1 passes at least); over: over cells after the
# flush, whatever the gap
def alternating():
    p = np.ones(6 * 1024 + 37, np.float32)
    p[1::2] = 1000.0
    return p


def every_third():
    p = np.ones(9000, np.float32)
    p[::3] = 1000.0
    return p


def random_half():
    return np.random.default_rng(1).exponential(1.0, 40000).astype(np.float32)


def all_over():
    return np.ones(50000, np.float32)


CASES_1D = {
    # 32 starts in every word; runs of one cell
    "alternating": dict(make=alternating, alpha=1.5, configs=[(16, 1, 2), (256, 0, 1)], gaps={0: (3090, 2)}, over=3090),
    # two cells of not-over between over cells: a new run at gaps 0 and 1, none at 2 (i - prev > g + 1)
    "every_third": dict(make=every_third, alpha=2.0, configs=[(16, 1, 2)], gaps={0: (3000, 2), 1: (3000, 2), 2: (1, 0)},
                        over=3000),
    "random_half": dict(make=random_half, alpha=0.7, configs=[(64, 1, 4)],
                        gaps={0: (10014, 9), 1: (5068, 4), 2: (2531, 2), 5: (315, 0)}, over=19857),
    # one run as long as the stream, every cell equal: the peak stays at index 0 over every call seam
    "all_over": dict(make=all_over, alpha=0.5, configs=[(64, 1, 2)], gaps={0: (1, 0)}, over=50000),
}
ALL_OVER_CUTS = [7000, 13000, 1, 20000, 50000 - 40001]
TRUNCATION = dict(case="alternating", config=(16, 1, 2), capacity=1500, cuts=[3100, 6 * 1024 + 37 - 3100])


def cuttings(n, C, k=3):
    """the two cuttings every stream is taken in besides the one call"""
    return [[n // 3, 1, n - n // 3 - 1], [C + 1] * k + [n - k * (C + 1)]]


def hypotheses(n):
    return np.arange(n, dtype=np.int32) * 11 - 7
