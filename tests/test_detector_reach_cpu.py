"""The designs of detector_reach_cases without a GPU, on the restatements and the host-only describe calls alone: the
kernel constants the designs rest on are the literals in the sources (if a cap moves, this fails instead of the GPU
tests silently no longer reaching the loop), every 2-D case's first step has more units than the grid's cap and runs
the <lds> kernel, the two units of one workgroup stage different cells, tiled_records is the restatement on the tiled
maps, and every 1-D case has the runs, over counts, starts per word and passes of cfar_runs it was made for."""
import os
import re

import numpy as np
import pytest

import cfar_ref
import detector_reach_cases as K
import oscfar_ref as O
import rdcfar_ref as R
from sdr_channelizer_amd import os_cfar, rd_cfar

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
METHOD = {"ca": R.CA, "go": R.GO}


def source(name):
    with open(os.path.join(ROOT, "sdr_channelizer_amd", "csrc", name)) as f:
        return f.read()


def shifts(pattern, text):
    """the numbers every match of `pattern` captures: one definition, one number"""
    return [int(m) for m in re.findall(pattern, text)]


def test_the_constants_are_the_sources():
    # the 1-D unit has its constants; the two 2-D units have theirs in the core they share, and no other
    for name in ("pfb_cfar.hip", "pfb_rdmap.hpp"):
        text = source(name)
        assert shifts(r"constexpr unsigned kMaxGrid = 1u << (\d+);", text) == [16], name
        assert shifts(r"constexpr uint64_t kStepCells = \(uint64_t\)1 << (\d+);", text) == [24], name
        # the clamp is one function of the host plumbing, and every grid of the unit takes the unit's cap through it
        assert text.count("grid_for(") == text.count(", kMaxGrid)") > 0 and "unsigned grid_for" not in text, name
    clamp = "std::min<uint64_t>(std::max<uint64_t>((items + per_block - 1) / per_block, 1), cap)"
    assert source("pfb_host.cpp").count(clamp) == 1
    assert len(re.findall(r"^unsigned grid_for\(uint64_t items, unsigned per_block, unsigned cap\) \{", source("pfb_host.cpp"), re.M)) == 1
    assert K.GRID_CAP == 1 << 16 and K.STEP_CELLS == 1 << 24 and K.STEP_WORDS == 1 << 18
    core = source("pfb_rdmap.hpp")
    assert shifts(r"constexpr uint64_t kStepWords = \(uint64_t\)1 << (\d+);", core) == [18]
    assert shifts(r"constexpr int kTileGates = (\d+);", core) == [K.TILE]
    assert core.count("std::min(kStepCells / h->map_cells, kStepWords / h->map_words)") == 1
    assert len(re.findall(r"const unsigned units = grid_for\(\(uint64_t\)m \* p\.NB \* p\.NT, 1, kMaxGrid\)", core)) == 1
    assert core.count("const char* kernel = h->cells(p, units);") == 1     # the units launch on that grid
    for name, cells in (("pfb_rdcfar.hip", "rdcfar_cells"), ("pfb_oscfar.hip", "oscfar_cells")):
        text = source(name)
        for constant in ("kMaxGrid", "kStepCells", "kStepWords", "kTileGates"):
            assert not re.search(r"constexpr \w+ %s\b" % constant, text), (name, constant)
        assert "grid_for(" not in text, name
        assert "for (long long u = blockIdx.x; u < units; u += gridDim.x)" in text
        assert len(re.findall(cells + r"<(?:true|false)>, dim3\(units\), dim3\(kTileGates\)", text)) == 2, name
        assert re.search(r"const char\* cells\(\w+& p, unsigned units\) const \{", text), name
    runs = re.findall(r"hipLaunchKernelGGL\(\(cfar_runs<E>\), dim3\((\d+)\), dim3\((\d+)\)", source("pfb_cfar.hip"))
    assert runs == [(str(K.RUN_GRID), "64")]
    assert "for (int c = blockIdx.x; c < sc.candidates; c += gridDim.x)" in source("pfb_cfar.hip")


def plan_of(case, unit, how):
    c = K.CASES_2D[case]
    if unit == "rdcfar":
        return rd_cfar.describe_rdcfar(c["ND"], c["R"], c["Wd"], c["Gr"], c["Tr"], c["Pd"], c["alpha"], how)
    return os_cfar.describe_oscfar(c["ND"], c["R"], c["Wd"], c["Gr"], c["Tr"], how, c["Pd"], c["alpha"])


def first_step_units(case, plan):
    c = K.CASES_2D[case]
    first = min(c["maps"], K.step_maps(c["ND"], c["R"]))
    return first * -(-c["ND"] // plan.tile_rows) * -(-c["R"] // plan.tile_gates)


@pytest.mark.parametrize("case,unit,how", K.VARIANTS_2D)
def test_every_2d_case_is_past_the_cap_in_its_first_step(case, unit, how):
    c = K.CASES_2D[case]
    plan = plan_of(case, unit, how)
    assert plan.tile_gates == K.TILE and plan.kernel.decode() == f"pfb_{unit}_cells<lds>"
    units = first_step_units(case, plan)
    assert units > K.GRID_CAP
    steps = -(-c["maps"] // K.step_maps(c["ND"], c["R"]))
    NB, NT = -(-c["ND"] // plan.tile_rows), -(-c["R"] // K.TILE)
    if case == "A":
        assert steps == 1 and units == c["maps"] > 2 * K.GRID_CAP and (NB, NT) == (1, 1)   # 2 or 3 units each
    if case == "B":
        assert steps == 2 and units == K.step_maps(3, 24) == 87381 and (NB, NT) == (1, 1)
        assert c["ND"] < plan.tile_rows and c["maps"] - 87381 == 19                    # nb < band_rows
    if case == "C":
        assert steps == 2 and K.step_maps(1, 520) == 29127 and units == 87381 and (NB, NT) == (1, 3)
        assert K.GRID_CAP % NT != 0


@pytest.mark.parametrize("case,unit,how", K.VARIANTS_2D)
def test_the_units_of_one_workgroup_stage_different_cells(case, unit, how):
    plan = plan_of(case, unit, how)
    units = first_step_units(case, plan)
    distinct = K.distinct_maps(case)
    rng = np.random.default_rng(5)
    sample = [0, 1, 2, units - K.GRID_CAP - 1] + rng.integers(0, units - K.GRID_CAP, 60).tolist()
    for u in sample:
        m0, first = K.unit_block(case, plan.tile_rows, u, distinct)
        m1, second = K.unit_block(case, plan.tile_rows, u + K.GRID_CAP, distinct)
        assert m0 != m1 and m0 % K.DISTINCT != m1 % K.DISTINCT, u
        assert first.shape == second.shape and not np.array_equal(first, second), u
    assert K.GRID_CAP % K.DISTINCT != 0 and (2 * K.GRID_CAP) % K.DISTINCT != 0
    assert len({distinct[k].tobytes() for k in range(K.DISTINCT)}) == K.DISTINCT


def detect_2d(case, unit, how, maps, first_map=0):
    c = K.CASES_2D[case]
    if unit == "rdcfar":
        return R.detect(maps, c["Wd"], c["Gr"], c["Tr"], c["Pd"], METHOD[how], c["alpha"], 0.0, first_map=first_map)
    return O.detect(maps, c["Wd"], c["Gr"], c["Tr"], c["Pd"], how, c["alpha"], 0.0, first_map=first_map)


@pytest.mark.parametrize("case,unit,how", K.VARIANTS_2D)
def test_tiled_records_are_the_restatement_on_the_tiled_maps(case, unit, how):
    D = K.DISTINCT
    distinct = K.distinct_maps(case)
    ref, stats = detect_2d(case, unit, how, distinct)
    assert len(ref) > D and len(np.unique(ref["map"])) > 3 * D // 4   # detections all along the sequence
    n = 3 * D + 5
    _, rem = detect_2d(case, unit, how, distinct[:n % D])
    for first_map in (0, 7):
        want, wstats = detect_2d(case, unit, how, K.tiled(distinct, n), first_map=first_map)
        got, gstats = K.tiled_records(ref, stats, D, n, rem, first_map=first_map)
        assert got.dtype == want.dtype and got.tobytes() == want.tobytes() and gstats == wstats
    got, gstats = K.tiled_records(ref, stats, D, 2 * D)          # D divides n: no remainder needed
    want, wstats = detect_2d(case, unit, how, K.tiled(distinct, 2 * D))
    assert got.tobytes() == want.tobytes() and gstats == wstats
    assert np.array_equal(K.tiled(distinct, n)[D + 3], distinct[3])


def test_the_dense_maps_are_mostly_over():
    d = K.DENSE
    maps = K.dense_maps()
    assert maps.size == 5216
    for (Gr, Pd), (dets, over) in K.DENSE_RD.items():
        want, stats = R.detect(maps, d["Wd"], Gr, d["Tr"], Pd, R.CA, d["alpha"])
        assert (len(want), stats["cells_over"]) == (dets, over) and over > maps.size // 2
        # half the records end inside a full word in the middle of a tile
        assert 64 < len(want) // 2 + 1 < len(want) - 64
    o = K.DENSE_OS
    for Pd in o["Pd"]:
        want, stats = O.detect(maps, d["Wd"], o["Gr"], d["Tr"], Pd, o["rank"], d["alpha"])
        assert stats["cells_over"] > maps.size // 2 and len(want) > 200


def starts_per_word(over, gap):
    """the over cells of every 64-cell word that start a run: the over cell before them lies more than gap + 1 back"""
    idx = np.flatnonzero(over)
    start = np.concatenate([[True], np.diff(idx) > gap + 1])
    return np.bincount(idx[start] // 64, minlength=-(-len(over) // 64))


@pytest.mark.parametrize("name", list(K.CASES_1D))
def test_every_1d_case_is_what_it_was_made_for(name):
    case = K.CASES_1D[name]
    p = case["make"]()
    n = len(p)
    for C_, G, T in case["configs"]:
        for gap, (runs, factor) in case["gaps"].items():
            kw = dict(C=C_, G=G, T=T, alpha=case["alpha"], merge_gap=gap)
            want, stats = cfar_ref.detect(p, n, True, **kw)
            assert (len(want), stats["cells_over"]) == (runs, case["over"]), (name, C_, gap)
            assert int(want["cells_over"].astype(np.int64).sum()) == case["over"]
            # the one unflushed call: its candidates are what closes and the run left open
            one, ostats = cfar_ref.detect(p, n, False, **kw)
            candidates = len(one) + ostats["open_run"]
            assert candidates > factor * K.RUN_GRID, (name, C_, gap, candidates)
            assert factor > 0 or candidates <= K.RUN_GRID
            over, _, _ = cfar_ref.decide(p, n, False, C_, G, T, cfar_ref.CA, case["alpha"], 0.0)
            per_word = starts_per_word(over, gap)
            assert int(per_word.sum()) == candidates
            if name == "alternating":
                assert (want["cells_over"] == 1).all() and (per_word[:-1] == 32).all()
            if name == "every_third" and gap < 2:
                assert set(per_word[:-1].tolist()) == {21, 22} and (want["cells_over"] == 1).all()
            if name == "random_half":
                assert per_word.max() >= (12, 8, 5, 2)[[0, 1, 2, 5].index(gap)]
            if name == "all_over" or (name == "every_third" and gap == 2):
                assert int(want["first_index"][0]) == 0 and int(want["peak_index"][0]) == 0
                assert int(want["last_index"][0]) == (n - 1 if name == "all_over" else n - 3)
    assert all(sum(cuts) == n and min(cuts) > 0 for cuts in K.cuttings(n, case["configs"][0][0]))
    assert name != "all_over" or (sum(K.ALL_OVER_CUTS) == n and min(K.ALL_OVER_CUTS) > 0)


def test_the_truncated_calls_close_more_than_their_capacity():
    t = K.TRUNCATION
    case = K.CASES_1D[t["case"]]
    p = case["make"]()
    C_, G, T = t["config"]
    kw = dict(C=C_, G=G, T=T, alpha=case["alpha"], merge_gap=0)
    assert sum(t["cuts"]) == len(p)
    done = 0
    for pos in np.cumsum(t["cuts"]):
        closed = len(cfar_ref.detect(p, int(pos), False, **kw)[0])
        assert closed - done > t["capacity"] > K.RUN_GRID      # the capacity edge lies in the second pass of cfar_runs
        done = closed
