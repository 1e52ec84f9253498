"""The deinterleaver on the device at the list sizes it accepts: the lists of deint_scale_cases -- 2^18 to 2^20 pulses,
each the smallest that reaches one path of pfb_deint.hip that a short list never takes -- against the numpy restatement
(deint_ref), byte for byte: the histogram, then successors, steps and lengths at chosen periods, then records, labels,
count and stats.  What each list is and why the restatement can be trusted on it is shown without a GPU in
test_deint_scale_cpu.py."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import deint_cases as DC  # noqa: E402
import deint_ref as R  # noqa: E402
import deint_scale_cases as SC  # noqa: E402
from gpu_support import cuda_torch  # noqa: E402
from sdr_channelizer_amd import Deinterleaver  # noqa: E402
from sdr_channelizer_amd import _lib as L  # noqa: E402
from sdr_channelizer_amd.deinterleave import EMITTER_DTYPE, records_to_numpy  # noqa: E402


@pytest.fixture(scope="module")
def torch():
    return cuda_torch()


def make(c: R.Cfg) -> Deinterleaver:
    return Deinterleaver(c.pmin, c.pmax, c.W, **c.settings())


def on_device(torch, t):
    return torch.from_numpy(np.array(t, np.uint64).view(np.int64)).cuda()


def both(torch, t):
    """(where the call reads the list, its name): host memory, then device memory"""
    return ((t, "host"), (on_device(torch, t), "device"))


def set_tier(d, hist, mark):
    assert L.load().pfb_deint_set_tier(d._h, hist, mark) == L.PFB_OK


def same(got, want, what):
    for g, r, name in zip(got, want, ("succ", "step", "len")):
        assert g.dtype == np.int32 and g.tobytes() == r.tobytes(), (what, name, np.nonzero(g != r)[0][:8])


def check(d, x, name, taus=(), what=""):
    """every entry point on one named list (x: its ticks where the call reads them) against the restatement's shared
    results; returns the run's records"""
    what = (name, what)
    assert d.histogram(x).tobytes() == SC.expected_histogram(name).tobytes(), what
    for tau in taus:
        same(d.successors(x, tau), SC.expected_lengths(name, tau), (what, tau))
    rec, labels, stats = SC.expected(name)
    got_rec, got_labels = d.run(x)
    got_rec = records_to_numpy(got_rec)
    got_labels = got_labels if isinstance(got_labels, np.ndarray) else got_labels.cpu().numpy()
    assert got_rec.dtype == EMITTER_DTYPE and len(got_rec) == len(rec), (what, got_rec, rec)
    assert got_rec.tobytes() == rec.tobytes(), (what, got_rec, rec)
    assert got_labels.dtype == np.int32 and got_labels.tobytes() == labels.tobytes(), (what, np.nonzero(got_labels != labels)[0][:8])
    assert d.stats == stats, (what, d.stats, stats)
    return got_rec


def one_chain(got, n, what):
    """(succ, step, len) of a perfect train of n pulses"""
    succ, step, ln = got
    assert np.array_equal(ln, np.arange(n, 0, -1, dtype=np.int32)), what
    assert np.array_equal(succ[:-1], np.arange(1, n, dtype=np.int32)) and succ[-1] == -1, what
    assert (step[:-1] == 1).all() and step[-1] == 0, what


# -- 1. the doubling rounds and the kept tables at their limit ---------------------------------------------------------
@pytest.mark.parametrize("mark", (1, 2))
def test_one_chain_of_the_longest_list(torch, mark):
    """2^20 pulses in one chain: 20 doubling rounds, every kept table read, at both marking tiers"""
    t, c = SC.case("one_chain_max")
    n = len(t)
    assert n == SC.MAX_PULSES
    with make(c) as d:
        set_tier(d, 0, mark)
        for x, where in both(torch, t):
            rec = check(d, x, "one_chain_max", what=(where, mark))
            assert ("pfb_deint_mark_walk", "pfb_deint_mark_tables")[mark - 1] in d.last_kernel.split("+")
            assert "pfb_deint_double" in d.last_kernel.split("+")
            assert len(rec) == 1 and (rec[0]["pulses"], rec[0]["periods"], rec[0]["first_pulse"]) == (n, n - 1, 0)
            one_chain(d.successors(x, SC.CHAIN_TAU), n, where)


def test_the_doubling_rounds_around_2_18(torch):
    with make(DC.SMALL) as d:
        for n in SC.chain_edge_lengths():
            t = DC.train(SC.CHAIN_TAU, n, 11)
            for x, where in both(torch, t):
                one_chain(d.successors(x, SC.CHAIN_TAU), n, (n, where))


# -- 2. four trains in 2^20 pulses -------------------------------------------------------------------------------------
def test_four_trains_in_the_longest_list(torch):
    """five rounds over all 1024 tiles: the scan of the tiles' counts through its four waves, round after round"""
    t, c = SC.case("four_trains_max")
    with make(c) as d:
        for x, where in both(torch, t):
            rec = check(d, x, "four_trains_max", what=where)
            assert len(rec) == 4 and d.stats["rounds"] == 5
            assert {"pfb_deint_compact", "pfb_deint_hist_lds", "pfb_deint_argmax", "pfb_deint_mark_tables"} <= set(d.last_kernel.split("+"))


def test_successors_in_the_longest_list(torch):
    t, c = SC.case("four_trains_max")
    with make(c) as d:
        for tau in (SC.FOUR_PERIODS[0], c.pmax):
            want = SC.expected_lengths("four_trains_max", tau)
            for x, where in both(torch, t):
                same(d.successors(x, tau), want, (tau, where))


def test_the_histogram_of_the_longest_list_in_both_tiers(torch):
    """1024 workgroups: the LDS tier's flush of their private histograms and the global tier's adds into few bins"""
    t, _ = SC.case("four_trains_max")
    x = on_device(torch, t)
    c = SC.FOUR_W1
    assert c.NB == 8001 <= DC.LDS_BINS
    want = SC.expected_histogram("four_trains_max", c)
    assert int(want.max()) > 1 << 16          # a bin that every one of the 1024 workgroups adds into
    with make(c) as d:
        for hist, kernel in ((0, "pfb_deint_hist_lds"), (2, "pfb_deint_hist_global")):
            set_tier(d, hist, 0)
            for src in (t, x):
                assert d.histogram(src).tobytes() == want.tobytes(), (hist, src is x)
                assert d.last_kernel == "pfb_deint_compact+" + kernel
    c = SC.FOUR_WIDE
    assert c.NB == 65536
    want = SC.expected_histogram("four_trains_max", c)
    with make(c) as d:
        for src in (t, x):
            assert d.histogram(src).tobytes() == want.tobytes(), src is x
        assert d.last_kernel == "pfb_deint_compact+pfb_deint_hist_global"


# -- 3. the scan's edges -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SC.SCAN_EDGES)
def test_the_scan_at_its_lane_and_wave_edges(torch, n):
    name = f"scan_edge_{n}"
    t, c = SC.case(name)
    assert len(t) == n
    with make(c) as d:
        for x, where in both(torch, t):
            check(d, x, name, what=where)
            assert d.stats["rounds"] >= 2


# -- 4. the argmax past its first stride -------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("late_winner", "early_winner"))
def test_the_winner_of_a_list_longer_than_the_argmax_grid(torch, name):
    t, c = SC.case(name)
    assert len(t) > 2 * SC.ARGMAX_STRIDE
    with make(c) as d:
        for x, where in both(torch, t):
            rec = check(d, x, name, what=where)
            first = SC.LATE_LONG if name == "late_winner" else 0
            assert rec["first_pulse"].tolist() == [first, first + 1, SC.LATE_LONG - first]


# -- 5. successors far on ----------------------------------------------------------------------------------------------
def test_successors_far_on_and_past_the_end(torch):
    """the gallop's widths up to 32768, its clamp at the list's end, and every step up to X + 1"""
    with make(SC.DENSE) as d:
        for which, taus in (("a", SC.DENSE_A_TAUS), ("b", (SC.DENSE_B_TAU,)), ("c", (SC.DENSE_B_TAU,))):
            t = SC.dense(which)
            for x, where in both(torch, t):
                for tau in taus:
                    same(d.successors(x, tau), SC.expected_lengths("dense_" + which, tau), (which, tau, where))
                assert d.last_kernel == "pfb_deint_compact+pfb_deint_succ+pfb_deint_double"


# -- 6. the lowest of a run of duplicates ------------------------------------------------------------------------------
def test_the_lowest_of_a_run_of_duplicates(torch):
    c = SC.DUP
    with make(c) as d:
        for key, t, ref, lit in SC.duplicate_lists():
            want = R.run(t, c)
            for x, where in both(torch, t):
                got = d.successors(x, SC.DUP_TAU)
                same(got, ref, (key, where))
                assert got[0].tobytes() == lit[0].tobytes() and got[1].tobytes() == lit[1].tobytes(), (key, where)
                rec, labels = d.run(x)
                labels = labels if isinstance(labels, np.ndarray) else labels.cpu().numpy()
                assert records_to_numpy(rec).tobytes() == want[0].tobytes() and labels.tobytes() == want[1].tobytes(), (key, where)
                assert d.stats == want[2], (key, where)


def test_a_long_run_of_duplicates_far_on(torch):
    t, tau, i, j = SC.dense_run()
    want = SC.expected_lengths("dense_run", tau)
    with make(SC.DENSE) as d:
        for x, where in both(torch, t):
            got = d.successors(x, tau)
            same(got, want, where)
            assert (got[0][i], got[1][i]) == (j, 1)


# -- 7. growth on one handle -------------------------------------------------------------------------------------------
def test_a_longer_list_after_a_shorter_one_on_one_handle(torch):
    short, c = SC.case("short_on_long_handle")
    long_ = SC.case("four_trains_max")[0]
    with make(c) as d:                                   # the scratch and the kept tables grow together, then stay
        for name in ("short_on_long_handle", "four_trains_max", "short_on_long_handle"):
            check(d, SC.case(name)[0], name, what="host, in turn")
    x = on_device(torch, long_)
    with make(c) as d:
        check(d, on_device(torch, short), "short_on_long_handle", what="before the growth")
        # the scratch grows and the tables do not ...
        assert d.histogram(x).tobytes() == SC.expected_histogram("four_trains_max").tobytes()
        check(d, x, "four_trains_max", what="the tables grow")    # ... until the run
        check(d, short, "short_on_long_handle", what="after the growth")
