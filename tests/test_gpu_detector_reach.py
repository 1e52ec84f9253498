"""The three detector units where a workgroup takes more than one unit of work, byte for byte against cfar_ref,
rdcfar_ref and oscfar_ref (designs and their proofs: detector_reach_cases, test_detector_reach_cpu.py).

2-D units: sequences of small maps whose first step has more (map, band, tile) units than the grid's cap of 2^16, so
that every workgroup of rdcfar_cells<lds> / oscfar_cells<lds> decodes, re-stages and decides a second and a third
unit; a capacity that ends in the middle of such a call's output; a map that is mostly detections for the
cell-averaging detector, with a capacity that ends inside a full word in the middle of a tile, and the same cut on the
ordered-statistic detector's dense map.

1-D unit: streams on which most cells are over, so that cfar_runs (1024 workgroups, a run each) goes over the list of
starts up to ten times, every word holds up to 32 starts, one run is as long as the stream and its carried peak ties
at every call seam, and the capacity of an async call ends past the first pass.

Not reachable, so not tested here: the <direct> tier of the 2-D kernels cannot reach the cap inside a step (it needs
Gr + Tr > 1042, so a map has at least 7 x 1026 cells and a step holds about 2336 maps of 5 units); *_tile_counts and
*_emit take at most 1024 tiles of a step's 2^18 words; in the 1-D unit a step of 2^24 cells gives cfar_sum and
cfar_mask 2^14 workgroups and cfar_tile_last 1024; fold_direct's cap equals its largest grid.

Wall time on one MI355X, per test: the long sequences 0.31 s (A, rdcfar, the module's first), 0.06 s (A, oscfar), 0.04
to 0.05 s (B and C, either unit, case C's 61 MB included: it stays for oscfar too); the dense maps 0.05 and 0.12 s;
alternating 0.03 s each, every third cell 0.01 to 0.02 s, the random half 0.38, 0.17, 0.11 and 0.06 s, every cell over
0.03 s, the truncation 0.01 s.  20 tests in 3.8 s, 1.7 s of it the first use of the device."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import cfar_ref  # noqa: E402
import detector_reach_cases as K  # noqa: E402
import oscfar_ref as O  # noqa: E402
import rdcfar_ref as R  # noqa: E402
from gpu_support import cuda_torch  # noqa: E402
from rdmap_support import SENTINEL, place, run_async  # noqa: E402
from sdr_channelizer_amd import Cfar, OsCfar, RangeDopplerCfar  # noqa: E402
from sdr_channelizer_amd import cfar, rd_cfar  # noqa: E402

METHOD = {"ca": R.CA, "go": R.GO}


@pytest.fixture(scope="module")
def torch():
    return cuda_torch()


# -- the 2-D units --------------------------------------------------------------------------------------------------
def detector(unit, how, ND, Rg, Wd, Gr, Tr, Pd, alpha):
    if unit == "rdcfar":
        return RangeDopplerCfar(ND, Rg, Wd, Gr, Tr, alpha, peak_half_width=Pd, method=how)
    return OsCfar(ND, Rg, Wd, Gr, Tr, how, alpha, peak_half_width=Pd)


def restatement(unit, how, maps, Wd, Gr, Tr, Pd, alpha):
    if unit == "rdcfar":
        return R.detect(maps, Wd, Gr, Tr, Pd, METHOD[how], alpha)
    return O.detect(maps, Wd, Gr, Tr, Pd, how, alpha)


def truncated(torch, det, x, want, wstats):
    """one async call with room for half the records and one: the first ones, nothing behind them, the rest counted"""
    det.reset()
    cap = len(want) // 2 + 1
    got, count = run_async(torch, det, x, cap)
    assert count == len(want) and len(got) == cap and got.tobytes() == want[:cap].tobytes()
    assert det.stats == dict(wstats, dropped=len(want) - cap) and det.next_map == len(x)


@pytest.mark.parametrize("case,unit,how", K.VARIANTS_2D)
def test_long_sequences_of_small_maps(torch, case, unit, how):
    """Cases A, B and C of detector_reach_cases: the async route with guard rows and the synchronous route; on case A
    also a capacity that ends in the middle of the strided launch's output."""
    c = K.CASES_2D[case]
    geometry = (c["Wd"], c["Gr"], c["Tr"], c["Pd"], c["alpha"])
    D, n = K.DISTINCT, c["maps"]
    distinct = K.distinct_maps(case)
    ref, rstats = restatement(unit, how, distinct, *geometry)
    _, rem = restatement(unit, how, distinct[:n % D], *geometry)
    want, wstats = K.tiled_records(ref, rstats, D, n, rem)
    assert len(want) > n // 2 and int(want["map"][-1]) > n - D
    x = place(torch, K.tiled(distinct, n))
    with detector(unit, how, c["ND"], c["R"], *geometry) as det:
        got, count = run_async(torch, det, x, len(want) + 3)
        assert det.last_kernel == f"pfb_{unit}_cells<lds>"
        assert count == len(want)
        if got.tobytes() != want.tobytes():
            bad = int(np.flatnonzero(got != want)[0])
            raise AssertionError((case, unit, how, "first differing record", bad, got[bad], want[bad]))
        assert det.stats == wstats and det.next_map == n
        det.reset()
        again = rd_cfar.records(det.process(x))                      # the synchronous call, the same bytes
        assert again.tobytes() == want.tobytes() and det.stats == wstats and det.next_map == n
        if case == "A":
            truncated(torch, det, x, want, wstats)


def test_a_map_that_is_mostly_detections_for_the_cell_averaging_detector(torch):
    """(Gr, Pd) = (0, 0): every over cell is a detection, more than half the cells; (1, 1): the peak box thins them"""
    d = K.DENSE
    maps = K.dense_maps()
    x = place(torch, maps)
    for (Gr, Pd), (dets, over) in K.DENSE_RD.items():
        want, wstats = R.detect(maps, d["Wd"], Gr, d["Tr"], Pd, R.CA, d["alpha"])
        assert (len(want), wstats["cells_over"]) == (dets, over) and over > maps.size // 2
        with RangeDopplerCfar(d["ND"], d["R"], d["Wd"], Gr, d["Tr"], d["alpha"], peak_half_width=Pd) as det:
            got, count = run_async(torch, det, x, len(want) + 3)
            assert count == len(want) and got.tobytes() == want.tobytes(), (Gr, Pd)
            assert det.stats == wstats and det.next_map == len(maps)
            det.reset()
            assert rd_cfar.records(det.process(x)).tobytes() == want.tobytes() and det.stats == wstats
            if (Gr, Pd) == (0, 0):
                truncated(torch, det, x, want, wstats)


def test_the_ordered_statistic_detectors_dense_map_truncated(torch):
    d, o = K.DENSE, K.DENSE_OS
    maps = K.dense_maps()
    x = place(torch, maps)
    sorts = [O.sorted_training(P, d["Wd"], o["Gr"], d["Tr"]) for P in maps]
    for Pd in o["Pd"]:
        want, wstats = O.detect(maps, d["Wd"], o["Gr"], d["Tr"], Pd, o["rank"], d["alpha"], sorts=sorts)
        assert wstats["cells_over"] > maps.size // 2
        with OsCfar(d["ND"], d["R"], d["Wd"], o["Gr"], d["Tr"], o["rank"], d["alpha"], peak_half_width=Pd) as det:
            truncated(torch, det, x, want, wstats)


# -- the 1-D unit ---------------------------------------------------------------------------------------------------
def as_cells(p, hyp):
    if hyp is None:
        return np.ascontiguousarray(p, np.float32)
    c = np.zeros(len(p), cfar_ref.CELL)
    c["power"], c["hypothesis"] = p, hyp
    return c.view(np.float32).reshape(-1, 2)


class Reference:
    """cfar_ref.detect of one stream and one setting, each (cell count, flushed) computed once"""

    def __init__(self, p, kw, hyp=None):
        self.p, self.kw, self.seen = p, dict(kw, hyp=hyp), {}

    def __call__(self, n, flushed):
        if (n, flushed) not in self.seen:
            self.seen[n, flushed] = cfar_ref.detect(self.p, n, flushed, **self.kw)
        return self.seen[n, flushed]


def stream(torch, det, ref, cuts, hyp=None, host=False):
    """One stream through `det` (reset first), cut into calls of the lengths `cuts`: what has come out after each call,
    and after the flush, is what the restatement says has closed by then, and so are the stats (the logic of
    test_gpu_cfar.stream)."""
    det.reset()
    x = as_cells(ref.p, hyp)
    got, pos = [np.zeros(0, cfar.DET_DTYPE)], 0
    for m in cuts:
        part = x[pos:pos + m]
        got.append(cfar.records(det.process(part if host else torch.from_numpy(part).cuda())))
        pos += m
        assert det.next_index == pos
        want, wstats = ref(pos, False)
        assert np.concatenate(got).tobytes() == want.tobytes() and det.stats == wstats, (pos, cuts, det.stats, wstats)
    got.append(cfar.records(det.flush()))
    want, wstats = ref(pos, True)
    assert np.concatenate(got).tobytes() == want.tobytes() and det.stats == wstats, (cuts, det.stats, wstats)
    return np.concatenate(got)


def settings(name, config, gap, element="power"):
    case = K.CASES_1D[name]
    C_, G, T = config
    det = Cfar(C_, G, T, case["alpha"], element=element, merge_gap=gap)
    return det, dict(C=C_, G=G, T=T, alpha=case["alpha"], merge_gap=gap)


@pytest.mark.parametrize("config", K.CASES_1D["alternating"]["configs"])
def test_alternating_cells(torch, config):
    """3090 runs of one cell, 32 starts in every word, three passes of cfar_runs; also as bank cells and from host
    memory"""
    p = K.alternating()
    n = len(p)
    det, kw = settings("alternating", config, 0)
    ref = Reference(p, kw)
    with det:
        for cuts in [[n]] + K.cuttings(n, config[0]):
            out = stream(torch, det, ref, cuts)
            assert len(out) == 3090 and (out["first_index"] == out["last_index"]).all()
        stream(torch, det, ref, [n], host=True)
    hyp = K.hypotheses(n)
    det, kw = settings("alternating", config, 0, element="cell")
    with det:
        out = stream(torch, det, Reference(p, kw, hyp), [n], hyp=hyp)
        assert np.array_equal(out["hypothesis"], hyp[1::2])


@pytest.mark.parametrize("gap", list(K.CASES_1D["every_third"]["gaps"]))
def test_every_third_cell(torch, gap):
    """two cells of not-over between over cells: 3000 runs at gaps 0 and 1, one run at 2"""
    p = K.every_third()
    n = len(p)
    config = K.CASES_1D["every_third"]["configs"][0]
    det, kw = settings("every_third", config, gap)
    ref = Reference(p, kw)
    with det:
        for cuts in [[n]] + K.cuttings(n, config[0]):
            out = stream(torch, det, ref, cuts)
            assert len(out) == K.CASES_1D["every_third"]["gaps"][gap][0]


@pytest.mark.parametrize("gap", list(K.CASES_1D["random_half"]["gaps"]))
def test_a_random_half_of_the_cells(torch, gap):
    """19857 of 40000 cells over: 10014, 5068, 2531 and 315 runs, up to ten passes of cfar_runs"""
    p = K.random_half()
    n = len(p)
    config = K.CASES_1D["random_half"]["configs"][0]
    det, kw = settings("random_half", config, gap)
    ref = Reference(p, kw)
    rng = np.random.default_rng(3)
    cuttings = [[n]] + K.cuttings(n, config[0])
    for _ in range(3):
        edges = np.sort(rng.integers(0, n + 1, 9))
        cuttings.append(np.diff(np.concatenate([[0], edges, [n]])).tolist())
    with det:
        for cuts in cuttings:
            out = stream(torch, det, ref, cuts)
            assert len(out) == K.CASES_1D["random_half"]["gaps"][gap][0]


def test_every_cell_over(torch):
    """one run 0 .. 49999 of equal cells: the carried peak keeps index 0 over every call seam"""
    p = K.all_over()
    n = len(p)
    config = K.CASES_1D["all_over"]["configs"][0]
    det, kw = settings("all_over", config, 0)
    ref = Reference(p, kw)
    with det:
        for cuts in [[n], K.ALL_OVER_CUTS] + K.cuttings(n, config[0]):
            out = stream(torch, det, ref, cuts)
            assert [(int(d["first_index"]), int(d["last_index"]), int(d["peak_index"]), int(d["cells_over"]))
                    for d in out] == [(0, n - 1, 0, n)]


def test_truncation_past_the_first_pass(torch):
    """the alternating stream in two async calls with room for 1500 records each: the first 1500 of each call, nothing
    behind them, the excess counted"""
    t = K.TRUNCATION
    p = K.alternating()
    det, kw = settings(t["case"], t["config"], 0)
    ref = Reference(p, kw)
    cap = t["capacity"]
    x = torch.from_numpy(p).cuda()
    edges = np.cumsum([0] + t["cuts"]).tolist()
    closed = [len(ref(e, False)[0]) for e in edges]
    with det:
        outs = [torch.full((cap + 2, 6), SENTINEL, dtype=torch.int64, device="cuda") for _ in t["cuts"]]
        counts = torch.full((len(t["cuts"]), 3), SENTINEL, dtype=torch.int64, device="cuda")
        for k, (lo, hi) in enumerate(zip(edges[:-1], edges[1:])):
            det.process_async(x[lo:hi], outs[k][1:cap + 1], counts[k][1:2])
        det.sync()
        got = counts.cpu().numpy()
        assert got[:, 1].tolist() == np.diff(closed).tolist() and (got[:, [0, 2]] == SENTINEL).all()
        assert min(np.diff(closed)) > cap
        for k in range(len(t["cuts"])):
            rec = outs[k].cpu().numpy()
            assert (rec[0] == SENTINEL).all() and (rec[cap + 1] == SENTINEL).all()
            want = ref(edges[k + 1], False)[0][closed[k]:closed[k] + cap]
            assert cfar.records(rec[1:cap + 1]).tobytes() == want.tobytes(), k
        wstats = ref(edges[-1], False)[1]
        assert det.stats == dict(wstats, dropped=int(sum(c - cap for c in np.diff(closed))))
        assert det.stats["detections"] == closed[-1]
