"""The long lists of deint_scale_cases without a GPU: on the numpy restatement (deint_ref) alone, that every list is
what test_gpu_deint_scale.py takes it for -- that it reaches the path of pfb_deint.hip it is named for -- and that the
restatement can be trusted there: held to the literal loops on the slices of the long lists they can afford, and on
every one of the small lists with runs of duplicates."""
import importlib
import os
import re

import numpy as np

import deint_cases as DC
import deint_ref as R
import deint_scale_cases as SC

di = importlib.import_module("sdr_channelizer_amd.deinterleave")   # the module, not the function of the same name
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def round_up(v, to=256):
    return (v + to - 1) // to * to


def doubling_rounds(t, c, tau):
    """the doubling rounds chains() runs on a whole list: the smallest r with 2^r >= min(n - 1, span / (tau - e))"""
    most = min(len(t) - 1, (int(t[-1]) - int(t[0])) // (tau - c.e))
    r = 0
    while (1 << r) < most:
        r += 1
    return r, most


# -- the boundaries ----------------------------------------------------------------------------------------------------
def test_the_boundaries_hold_one_another_and_the_source():
    assert SC.TILE * SC.SCAN_WAVE == SC.ARGMAX_STRIDE == 1 << 18
    assert SC.MAX_PULSES == di.MAX_PULSES == 1 << SC.MAX_ROUNDS == 4 * SC.ARGMAX_STRIDE
    assert SC.MAX_PULSES // SC.TILE == 4 * SC.SCAN_WAVE       # one workgroup of four waves scans every tile's count
    src, core = (re.sub(r"//.*", "", open(os.path.join(ROOT, "sdr_channelizer_amd", "csrc", name)).read())
                 for name in ("pfb_deint.hip", "pfb_list.hpp"))
    assert "kMaxPulses = 1u << 20" in src and f"kMaxRounds = {SC.MAX_ROUNDS};" in src
    assert f"kTile = {SC.TILE};" in src and "kThreads = 256;" in core and '#include "pfb_list.hpp"' in src
    assert "deint_argmax, dim3(std::min((alive + kThreads - 1) / kThreads, 1024u)), dim3(kThreads)" in src
    # the scan of the tiles' counts is the list units' shared kernel, launched here
    scan = core[core.index("void __launch_bounds__(kThreads) list_scan("):core.index("enum {")]
    assert scan.count("const uint32_t i = threadIdx.x * 4 + k;") == 2 and "list_scan<false>, dim3(1), dim3(kThreads)" in src
    assert SC.SCAN_EDGES == (4097, 1 << 18, (1 << 18) + 1, (2 << 18) + 1, (3 << 18) + 1)
    assert [-(-n // SC.TILE) for n in SC.SCAN_EDGES] == [5, 256, 257, 513, 769]


def test_the_longest_list_is_accepted_and_its_scratch_reported():
    for c in (DC.SMALL, SC.FOUR, SC.FOUR_WIDE):
        plan = di.describe_deinterleaver(c.pmin, c.pmax, c.W, num_pulses=SC.MAX_PULSES, **c.settings())
        cap = SC.MAX_PULSES
        # the carving of pfb_deint.hip's scratch: 68 bytes a pulse in 256-byte pieces, the tiles' counts, the histogram,
        # the 64-byte control block; then level_bytes(): kMaxRounds jump tables of 4 bytes a pulse
        layout = sum(round_up(cap * b) for b in (8, 4, 8, 4, 4, 4, 4, 16, 16)) + round_up(cap // SC.TILE * 4) \
            + round_up(c.NB * 4) + round_up(64)
        assert plan.scratch_bytes >= layout + SC.MAX_ROUNDS * cap * 4
        assert plan.num_bins == c.NB


# -- 1. one chain ------------------------------------------------------------------------------------------------------
def test_one_chain_of_the_longest_list():
    t, c = SC.case("one_chain_max")
    rec, labels, stats = SC.expected("one_chain_max")
    n = SC.MAX_PULSES
    assert len(t) == n and len(rec) == 1 and not labels.any()
    assert (rec[0]["pulses"], rec[0]["periods"], rec[0]["candidate_period"], rec[0]["period"]) == (n, n - 1, SC.CHAIN_TAU, 100.0)
    assert stats == dict(rounds=1, candidates_tried=1, candidates_refused=0, pulses_assigned=n)
    assert doubling_rounds(t, c, SC.CHAIN_TAU) == (SC.MAX_ROUNDS, n - 1)     # every table level_bytes() allocates
    # around 2^18 the rounds go from 18 to 19; with 2^18 + 1 pulses the hops are 2^rounds itself
    got = [doubling_rounds(DC.train(SC.CHAIN_TAU, m, 11), c, SC.CHAIN_TAU) for m in SC.chain_edge_lengths()]
    assert got == [(18, (1 << 18) - 2), (18, (1 << 18) - 1), (18, 1 << 18), (19, (1 << 18) + 1)]


# -- 2. four trains ----------------------------------------------------------------------------------------------------
def test_four_trains_in_the_longest_list():
    t, c = SC.case("four_trains_max")
    rec, labels, stats = SC.expected("four_trains_max")
    assert len(t) == SC.MAX_PULSES and (np.diff(t.astype(np.int64)) >= 0).all()
    assert len(rec) == 4 and stats["rounds"] == 5 and stats["candidates_tried"] - stats["candidates_refused"] == 4
    assert sorted(np.rint(rec["period"]).astype(int).tolist()) == list(SC.FOUR_PERIODS)
    left = int((labels < 0).sum())
    print("records", rec[["pulses", "periods", "candidate_period"]], "unassigned", left, stats)
    assert 15000 <= left <= 25000 and stats["pulses_assigned"] == SC.MAX_PULSES - left
    # one record a round, so the alive set of each round follows from the labels
    assert stats["candidates_refused"] == 0
    before = None
    for r in range(1, 6):
        idx = SC.alive_before_round(labels, r)
        assert len(idx) == SC.MAX_PULSES - int(rec["pulses"][:r - 1].sum())
        # compaction reads the labels of all the caller's tiles every round: the scan's fourth wave has counts to add
        assert idx[-1] // SC.TILE + 1 > 3 * SC.SCAN_WAVE
        counts = np.bincount(idx // SC.TILE, minlength=SC.MAX_PULSES // SC.TILE)
        if r >= 2:
            assert counts.min() < counts.max() and counts.min() > 0     # a real scan: no constant stride between tiles
            assert len(idx) < before
        before = len(idx)
    # the histograms of the tier test: 8001 bins for the LDS tier, 65536 for the global one alone
    assert SC.FOUR_W1.NB == 8001 <= DC.LDS_BINS < SC.FOUR_WIDE.NB == 65536
    h = SC.expected_histogram("four_trains_max", SC.FOUR_W1)
    assert h.max() > 1 << 16 and h.sum() > 8 * SC.MAX_PULSES


# -- 3. the scan's edges -----------------------------------------------------------------------------------------------
def test_the_scan_edges_compact_dead_pulses():
    for n in SC.SCAN_EDGES:
        t, c = SC.case(f"scan_edge_{n}")
        rec, labels, stats = SC.expected(f"scan_edge_{n}")
        assert len(t) == n and t.tobytes() == SC.four_trains()[:n].tobytes()
        assert stats["rounds"] >= 2 and len(rec) >= 1 and (labels == 0).any()     # the second round compacts with dead pulses
        assert (labels[-SC.TILE:] < 0).any() and (labels[:SC.TILE] >= 0).any()


# -- 4. the winner -----------------------------------------------------------------------------------------------------
def test_the_late_and_the_early_winner():
    for name, first in (("late_winner", SC.LATE_LONG), ("early_winner", 0)):
        t, c = SC.case(name)
        rec, labels, stats = SC.expected(name)
        assert len(t) == SC.LATE_LONG + 2 * SC.LATE_PAIR > 2 * SC.ARGMAX_STRIDE and (np.diff(t.astype(np.int64)) > 0).all()
        got = [(int(r["pulses"]), int(r["candidate_period"]), int(r["first_pulse"])) for r in rec]
        assert got == [(SC.LATE_PAIR, 1003, first), (SC.LATE_PAIR, 1003, first + 1), (SC.LATE_LONG, 1777, SC.LATE_LONG - first)]
        assert rec["period"].tolist() == [1003.0, 1003.0, 1777.0] and (labels >= 0).all()
        # the first candidate has two chains of one length: the lower index wins, in the argmax's second stride or its first
        succ, step, ln = R.lengths(t, c, 1003)
        assert ln[first] == ln[first + 1] == ln.max() == SC.LATE_PAIR and int(np.argmax(ln)) == first
        if name == "late_winner":
            assert SC.ARGMAX_STRIDE <= rec["first_pulse"][0] < 2 * SC.ARGMAX_STRIDE
            assert ln[:SC.ARGMAX_STRIDE].max() == 1                 # the first stride alone knows no chain at all
        else:
            assert rec["first_pulse"][0] < SC.ARGMAX_STRIDE and ln[SC.ARGMAX_STRIDE:].max() < SC.LATE_PAIR


# -- 5. successors far on ----------------------------------------------------------------------------------------------
def test_the_dense_lists_reach_the_gallop_and_the_end():
    me = np.arange(SC.DENSE_N)
    # the gallop adds 16, 32, .. to the 8 probed entries: a successor more than 8 + 16 + .. + 16384 entries on has
    # walked every width up to 32768
    for tau, lo, hi in zip(SC.DENSE_A_TAUS, (550, 5500, 8 + 32752), (800, 6500, 45000)):
        succ, step, ln = SC.expected_lengths("dense_a", tau)
        far = (succ - me)[succ >= 0]
        none = int((succ < 0).sum())
        print("tau", tau, "successors", far.min(), "to", far.max(), "entries on; none for the last", none)
        assert lo < far.min() and far.max() < hi
        assert lo < none < hi and (succ[-none:] < 0).all() and (succ[:-none] >= 0).all()      # the clamp at n
        assert set(np.unique(step)) == {0, 1}
    # 'b': gaps up to 59 ticks against windows of 9, 17, .. ticks: the first seven can be empty, the eighth (65) never
    # is; 'c': gaps up to 99, and every step 0 .. X + 1 occurs
    steps = {w: np.bincount(SC.expected_lengths("dense_" + w, SC.DENSE_B_TAU)[1], minlength=SC.DENSE.X + 2) for w in "bc"}
    print("steps", steps)
    assert (steps["b"][:8] > 0).all() and not steps["b"][9:].any()
    assert len(steps["c"]) == SC.DENSE.X + 2 and (steps["c"] >= 14).all()


def test_the_restatement_on_slices_of_the_dense_lists():
    """on lists this long only the vectorised successors are affordable; the first and last 3000 pulses are lists of
    their own, and short enough for the literal loop"""
    for which, tau in (("a", SC.DENSE_A_TAUS[0]), ("b", SC.DENSE_B_TAU), ("c", SC.DENSE_B_TAU)):
        for part in (slice(0, SC.SLICE), slice(-SC.SLICE, None)):
            a = SC.dense(which)[part]
            got, lit = R.successors(a, SC.DENSE, tau), R.literal_successors(a, SC.DENSE, tau)
            assert got[0].tobytes() == lit[0].tobytes() and got[1].tobytes() == lit[1].tobytes(), (which, part)
            assert (lit[0] >= 0).sum() > SC.SLICE // 2


# -- 6. runs of duplicates ---------------------------------------------------------------------------------------------
def test_the_runs_of_duplicates():
    lists = SC.duplicate_lists()
    assert len(lists) == len(SC.DUP_FILLS) * len(SC.DUP_RUNS) * len(SC.DUP_OFFS) == 224
    for (fill, run, off), t, ref, lit in lists:
        assert (np.diff(t.astype(np.int64)) >= 0).all() and len(t) == 1 + fill + run + 1 + 3
        assert ref[0].tobytes() == lit[0].tobytes() and ref[1].tobytes() == lit[1].tobytes(), (fill, run, off)
        # pulse 0's successor is the lowest of the run, `fill` entries on: under the target (off < 0) it is what the
        # second search returns, past its 8 probes from fill = 8 on and by `run` entries of bisection
        assert (ref[0][0], ref[1][0]) == (1 + fill, 1) and t[1 + fill] == SC.DUP_TAU + off
        assert (t[1 + fill:1 + fill + run] == t[1 + fill]).all() and (fill == 0 or t[fill] < SC.DUP_TAU - SC.DUP.e)
        assert R.run(t, SC.DUP)[2]["rounds"] >= 1


def literal_successor_of(a, c, tau, i):
    for m in range(c.X + 1):
        target, w = int(a[i]) + (m + 1) * tau, (m + 1) * c.e
        best = None
        for j in range(i + 1, len(a)):
            if int(a[j]) > target + w:
                break
            if int(a[j]) >= target - w and (best is None or abs(int(a[j]) - target) < abs(int(a[best]) - target)):
                best = j
        if best is not None:
            return best, m + 1
    return -1, 0


def test_a_long_run_of_duplicates_far_on():
    t, tau, i, j = SC.dense_run()
    assert (np.diff(t.astype(np.int64)) >= 0).all() and SC.DENSE.e * (2 * SC.DENSE.X + 3) < tau
    succ, step, ln = SC.expected_lengths("dense_run", tau)
    assert (succ[i], step[i]) == (j, 1) == literal_successor_of(t, SC.DENSE, tau, i)
    assert t[j] == t[i] + tau - 1 and (j == 0 or t[j - 1] < t[j])                     # under the target, the lowest
    assert (t[j:j + SC.RUN_LEN] == t[j]).all() and t[j + SC.RUN_LEN + 4] > t[j] + 1 + SC.DENSE.e
    assert i + SC.RUN_AHEAD - 4 <= j <= i + SC.RUN_AHEAD                              # past the widths 16 .. 8192
    for k in (i - 1, i + 1, i + 500):                                                 # its neighbours see the run too
        assert (succ[k], step[k]) == literal_successor_of(t, SC.DENSE, tau, k)
