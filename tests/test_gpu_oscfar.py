"""The ordered-statistic CFAR detector on the GPU against the numpy restatement (oscfar_ref), byte for byte: records,
counts and stats.  The shape grid crosses every ND with three (Gr, Tr) pairs, both Wd and the ranks 1, N/2 and N (one
sort of the training cells serves the three ranks); the pitch, the peak box and the pointer's offset from a 256-byte
boundary are drawn per shape by a hash.  Then both tiers, wrap and clip with the rank rule at the gate edges, ties at
the rank, non-finite cells and signed zeros, maps that are mostly detections, the cuttings of a sequence of maps into
calls, capacity and async semantics, and the two scenes the unit exists for: three targets in each other's training
windows, and the chain from I/Q with a second train in the first one's window."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import oscfar_cases as K  # noqa: E402
import oscfar_ref as O  # noqa: E402
import pd_cases  # noqa: E402
import rdcfar_cases  # noqa: E402
import rdcfar_ref as R  # noqa: E402
from gpu_support import Busy, cuda_torch  # noqa: E402
from rdmap_support import SENTINEL, place, run_async  # noqa: E402
from sdr_channelizer_amd import (MatchedFilter, OsCfar, cfar_alpha, detect_maps, detect_maps_os, detect_targets,  # noqa: E402
                                 os_cfar_alpha, range_doppler, targets_to_pdws)
from sdr_channelizer_amd import _lib as L  # noqa: E402
from sdr_channelizer_amd import os_cfar, rd_cfar  # noqa: E402
from sdr_channelizer_amd.rd_cfar import DET_DTYPE, TARGET_DTYPE, records  # noqa: E402

@pytest.fixture(scope="module")
def torch():
    return cuda_torch()


def cells(det):
    return [(int(d["row"]), int(d["gate"])) for d in det]


def check(torch, maps, Wd, Gr, Tr, Pd, ranks, alpha=4.0, min_power=0.0, pitch=0, offset=0, kernel=None):
    """the device against the restatement for every rank of `ranks` (an int, or a list: one sort serves them all);
    `alpha` a number or a function of the rank; returns the restatement's records of the last rank"""
    ranks = [ranks] if isinstance(ranks, int) else list(ranks)
    n, ND, Rg = maps.shape
    sorts = [O.sorted_training(P, Wd, Gr, Tr) for P in maps]
    x = place(torch, maps, pitch, offset)
    want = None
    for rank in ranks:
        a = alpha(rank) if callable(alpha) else alpha
        want, wstats = O.detect(maps, Wd, Gr, Tr, Pd, rank, a, min_power, sorts=sorts)
        with OsCfar(ND, Rg, Wd, Gr, Tr, rank, a, peak_half_width=Pd, min_power=min_power, pitch=pitch) as det:
            got, count = run_async(torch, det, x, len(want) + 3)
            where = (maps.shape, Wd, Gr, Tr, Pd, rank, pitch, offset)
            assert count == len(want) and got.tobytes() == want.tobytes(), where
            assert det.stats == wstats and det.next_map == n, where
            if kernel:
                assert det.last_kernel == f"pfb_oscfar_cells<{kernel}>" == det.plan.kernel.decode()
            det.reset()
            again = records(det.process(x))                            # the synchronous call, the same bytes
            assert again.tobytes() == want.tobytes() and det.stats == wstats, where
    return want


GRID = [(ND, Gr, Tr, Wd) for ND in (1, 3, 8, 64, 1024) for Gr, Tr in ((0, 1), (2, 4), (104, 16)) for Wd in (0, 1)
        if 2 * Wd + 1 <= ND]


@pytest.mark.parametrize("ND,Gr,Tr,Wd", GRID)
def test_shape_grid(torch, ND, Gr, Tr, Wd):
    """ranks 1, ceil(N / 2) and N; the factor is the design factor for a rate of 1e-2 (1e-3 on the large maps), so that
    every rank decides about as many cells over and both the counting and the select path run"""
    N = O.full_cells(Wd, Tr)
    T = K.TILE
    gate_counts = [2 * T + 90] if ND == 1024 else sorted({1, Gr + 1, Gr + Tr, 2 * (Gr + Tr) + 1, T - 1, T + 1, 2 * T + 90})
    for i, Rg in enumerate(gate_counts):
        h = ((i + 1) * 2654435761 + ND * 40503 + Gr * 97 + Wd * 7) >> 5
        Pd = min((ND - 1) // 2, (h >> 3) % 3)
        pitch = Rg + (h >> 7) % 5 if (h >> 10) & 1 else 0
        offset = (h >> 11) & 3
        big = ND * Rg > 1 << 16
        n = 1 if big else 2
        maps = K.noise_maps(n, ND, Rg, seed=i + ND, share=0.004 if big else 0.05)
        pfa = 1e-3 if big else 1e-2
        check(torch, maps, Wd, Gr, Tr, Pd, [1, (N + 1) // 2, N], alpha=lambda k: float(np.float32(O.alpha_ref(pfa, N, k))),
              min_power=0.25, pitch=pitch, offset=offset)


@pytest.mark.parametrize("Pd,kernel", [(2, "lds"), (3, "direct")])
def test_the_widest_windows_on_one_short_map(torch, Pd, kernel):
    """Gr = 1024, Tr = 100, Wd = 2: one row's block with a halo of two rows fits the LDS budget, with three it does not.
    The unit has these two tiers and no other; last_kernel names each."""
    N = O.full_cells(2, 100)
    for Rg in (1025, 2600):
        maps = K.noise_maps(1, 7, Rg, seed=Rg, share=0.003)
        check(torch, maps, 2, 1024, 100, Pd, 3 * N // 4, alpha=3.0, offset=Rg % 4, kernel=kernel)
    assert os_cfar.describe_oscfar(7, 2600, 2, 1024, 100, 1, Pd).kernel.decode() == f"pfb_oscfar_cells<{kernel}>"


def test_the_largest_window_reads_through_the_caches(torch):
    """Tr = 256 with Wd = 2 and Pd = 3: N = 2560 cells, the direct tier"""
    maps = K.noise_maps(1, 7, 1280, seed=4, share=0.003)
    check(torch, maps, 2, 1024, 256, 3, [1, 1920], alpha=lambda k: 500.0 if k == 1 else 3.0, kernel="direct")


def test_wrap_and_clip(torch):
    ND = 12
    kw = dict(Wd=2, Gr=3, Tr=6, Pd=2)
    N = O.full_cells(2, 6)
    for row, seen_from in ((0, ND - 1), (ND - 1, 0)):
        p = np.ones((1, ND, K.TILE + 30), np.float32)
        p[0, row, 100] = 900.0             # in the training sets of rows row-2 .. row+2 through the wrap, and in their boxes
        p[0, seen_from, 101] = 800.0       # beaten by it through the wrap
        want = check(torch, p, ranks=[N // 2, N], alpha=5.0, **kw)
        assert cells(want) == [(row, 100)]
    for Rg in (1, 5, 8, 2 * (3 + 6) + 1):  # R = 1, R < Gr + Tr, and the first R with one fully trained gate
        maps = K.noise_maps(2, ND, Rg, seed=Rg, share=0.1)
        check(torch, maps, ranks=[1, 37, N], alpha=2.0, **kw)
    for Rg in (1, 3, 4):                   # R <= Gr + 1: nothing detects, every cell is counted without noise
        p = np.full((2, ND, Rg), 7.0, np.float32)
        with OsCfar(ND, Rg, 2, 3, 6, 37, 1.0, peak_half_width=2) as det:
            assert len(det.process(p)) == 0
            assert det.stats == {"maps_in": 2, "cells_over": 0, "cells_without_noise": 2 * ND * Rg, "detections": 0,
                                 "dropped": 0}


def test_the_rank_rule_at_every_gate_of_both_edges(torch):
    """rank 7 of 36 (Wd = 1, Tr = 6): k' = ceil(7 n / 36) for n = 18, 21 .. 36; with a low factor every edge gate
    reports a cell in some row, so every n and k' of the edges is compared"""
    ND, Rg, Wd, Gr, Tr = 12, K.TILE + 30, 1, 1, 6
    maps = K.noise_maps(1, ND, Rg, seed=3, share=0.0)
    want = check(torch, maps, Wd, Gr, Tr, 0, 7, alpha=1.2)
    edge = [g for g in range(Rg) if g < Gr + Tr or g >= Rg - Gr - Tr]
    assert set(edge) <= {int(d["gate"]) for d in want}
    assert {int(d["training_cells"]) for d in want} == {3 * n for n in range(6, 13)}
    assert {int(d["flags"]) for d in want if int(d["gate"]) in edge} == {R.ONE_SIDED}


def test_ties_at_the_rank(torch):
    """maps of the values 0, 1, 2, 3: the k-th smallest lies in a run of equal values for every rank 1 .. N"""
    for Wd, Tr in ((0, 4), (1, 2)):
        N = O.full_cells(Wd, Tr)
        maps = K.quantised_maps(2, 5, K.TILE + 40, seed=N)
        check(torch, maps, Wd, 1, Tr, 1, range(1, N + 1), alpha=1.5, pitch=K.TILE + 44, offset=1)


def test_ties_and_the_peak_box(torch):
    c = rdcfar_cases.TIE
    want = check(torch, rdcfar_cases.tie_map()[None], c["Wd"], c["Gr"], c["Tr"], c["Pd"], [24, 36], alpha=c["alpha"])
    assert cells(want) == sorted([min(a, b) for a, b in rdcfar_cases.TIE_INSIDE]
                                 + [x for pair in rdcfar_cases.TIE_OUTSIDE for x in pair])


def test_non_finite_cells_and_signed_zeros(torch):
    c = K.NONFINITE
    p = K.nonfinite_map()
    check(torch, p[None], c["Wd"], c["Gr"], c["Tr"], c["Pd"], range(1, 9), alpha=c["alpha"])
    check(torch, p[None], 1, c["Gr"], c["Tr"], c["Pd"], [1, 12, 18, 24], alpha=c["alpha"], offset=3)
    c = K.ZEROS
    want = check(torch, K.zeros_map()[None], c["Wd"], c["Gr"], c["Tr"], c["Pd"], [1, c["rank"]], alpha=c["alpha"])
    zero = want[want["noise"] == 0]
    assert len(zero) > 100 and not zero["noise"].view(np.uint32).any()     # +0.0, whichever zero was selected


def test_maps_that_are_mostly_detections(torch):
    """rank 1 and a factor of a half: more than half the cells are over, so every lane of a wave selects"""
    maps = K.noise_maps(2, 8, K.TILE + 70, seed=13, share=0.01)
    for Pd in (0, 1):
        sorts = [O.sorted_training(P, 1, 1, 3) for P in maps]
        _, stats = O.detect(maps, 1, 1, 3, Pd, 1, 0.5, sorts=sorts)
        assert stats["cells_over"] > maps.size // 2
        check(torch, maps, 1, 1, 3, Pd, 1, alpha=0.5)


def test_cuttings(torch):
    ND, Rg, n = 8, K.TILE + 5, 7
    kw = dict(peak_half_width=1, min_power=0.5)
    maps = K.noise_maps(n, ND, Rg, seed=11, share=0.01)
    want, wstats = O.detect(maps, 1, 2, 4, 1, 18, 5.0, 0.5)
    assert len(want) > 20
    x = torch.from_numpy(maps).cuda()
    rng = np.random.default_rng(0)
    cuts = [[0, n], list(range(n + 1)), [0, 0, 3, 3, n, n]]
    cuts += [[0] + sorted(rng.integers(0, n + 1, 3).tolist()) + [n] for _ in range(3)]
    cuts.append(cuts[-1])                  # the same cutting twice
    with OsCfar(ND, Rg, 1, 2, 4, 18, 5.0, **kw) as det:
        empty = det.process(x[:0])
        assert len(empty) == 0 and det.next_map == 0
        for cut in cuts:
            det.reset()
            got = [records(det.process(x[a:b])) for a, b in zip(cut[:-1], cut[1:])]
            assert np.concatenate(got).tobytes() == want.tobytes(), cut
            assert det.stats == wstats and det.next_map == n
        det.reset()                         # host memory, one map per call and all at once
        got = [records(det.process(maps[k:k + 1])) for k in range(n)]
        assert np.concatenate(got).tobytes() == want.tobytes()
        det.reset()
        assert records(det.process(maps)).tobytes() == want.tobytes() and det.stats == wstats
    assert detect_maps_os(x, 1, 2, 4, 18, 5.0, **kw).tobytes() == want.tobytes()
    assert detect_maps_os(maps, 1, 2, 4, 18, 5.0, **kw).tobytes() == want.tobytes()


def test_host_memory_over_three_staging_steps(torch):
    """maps of 1024 rows of three gates: a step takes 2^18 words of 64 gates, 256 such maps, so 517 are three steps"""
    n = 2 * 256 + 5
    maps = K.noise_maps(n, 1024, 3, seed=5, share=0.005, level=100.0)
    want, wstats = O.detect(maps, 1, 0, 1, 1, 5, 20.0)
    assert len(want) > 1000 and int(want["map"][-1]) > 512
    with OsCfar(1024, 3, 1, 0, 1, 5, 20.0, peak_half_width=1) as det:
        got = records(det.process(maps))
        assert got.tobytes() == want.tobytes() and det.stats == wstats
        det.reset()
        assert records(det.process(torch.from_numpy(maps).cuda())).tobytes() == want.tobytes()


def test_a_capacity_one_short_changes_nothing(torch):
    ND, Rg = 8, K.TILE + 5
    maps = K.noise_maps(4, ND, Rg, seed=21, share=0.01)
    first, fstats = O.detect(maps[:1], 1, 2, 4, 1, 18, 5.0)
    rest, _ = O.detect(maps[1:], 1, 2, 4, 1, 18, 5.0, first_map=1)
    whole, wstats = O.detect(maps, 1, 2, 4, 1, 18, 5.0)
    assert len(rest) > 4
    lib = L.load()
    x = torch.from_numpy(maps).cuda()
    with OsCfar(ND, Rg, 1, 2, 4, 18, 5.0, peak_half_width=1) as det:
        assert records(det.process(x[:1])).tobytes() == first.tobytes()
        for mem, src in ((L.PFB_MEM_DEVICE, x[1:]), (L.PFB_MEM_HOST, maps[1:])):
            cap = len(rest) - 1
            count = C.c_uint64(0)
            if mem == L.PFB_MEM_DEVICE:         # guard records before and behind the room given
                buf = torch.full((cap + 2, 4), SENTINEL, dtype=torch.int64, device="cuda")
                ptr, data = buf[1:].data_ptr(), src.data_ptr()
            else:
                buf = np.full((cap + 2, 4), SENTINEL, np.int64)
                ptr, data = buf[1:].ctypes.data, src.ctypes.data
            rc = lib.pfb_oscfar_process(det._h, C.c_void_p(data), 3, C.c_void_p(ptr), cap, C.byref(count), mem)
            assert rc == L.PFB_ERR_CAPACITY and count.value == len(rest)
            assert (buf[0] == SENTINEL).all() and (buf[cap + 1] == SENTINEL).all()
            assert det.next_map == 1 and det.stats == fstats
        assert records(det.process(x[1:])).tobytes() == rest.tobytes()
        assert det.stats == wstats and det.next_map == 4 and len(whole) == len(first) + len(rest)


def test_async_across_a_stream_switch_with_truncation(torch):
    ND, Rg = 8, K.TILE + 5
    maps = K.noise_maps(6, ND, Rg, seed=31, share=0.01)
    a, _ = O.detect(maps[:3], 1, 2, 4, 1, 18, 5.0)
    b, _ = O.detect(maps[3:], 1, 2, 4, 1, 18, 5.0, first_map=3)
    _, wstats = O.detect(maps, 1, 2, 4, 1, 18, 5.0)
    assert len(b) > 4
    x = torch.from_numpy(maps).cuda()
    busy = Busy(torch)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    cap_b = len(b) - 4
    out_a = torch.full((len(a) + 2, 4), SENTINEL, dtype=torch.int64, device="cuda")
    out_b = torch.full((cap_b + 1, 4), SENTINEL, dtype=torch.int64, device="cuda")
    counts = torch.full((2,), SENTINEL, dtype=torch.int64, device="cuda")
    with OsCfar(ND, Rg, 1, 2, 4, 18, 5.0, peak_half_width=1) as det:
        det.set_stream(s1.cuda_stream)
        busy.queue(s1)
        det.process_async(x[:3], out_a, counts[0:1])
        det.set_stream(s2.cuda_stream)        # what s1 still holds comes first
        det.process_async(x[3:], out_b[:cap_b], counts[1:2])
        det.sync()
        s1.synchronize()
        assert counts.tolist() == [len(a), len(b)]
        assert records(out_a[:len(a)]).tobytes() == a.tobytes() and (out_a[len(a):] == SENTINEL).all()
        assert records(out_b[:cap_b]).tobytes() == b[:cap_b].tobytes() and (out_b[cap_b] == SENTINEL).all()
        assert det.stats == dict(wstats, dropped=4) and det.next_map == 6


def test_pointers_off_a_256_byte_boundary_with_a_pitch(torch):
    maps = K.noise_maps(2, 8, K.TILE + 9, seed=41, share=0.01)
    for offset in (1, 2, 3):
        check(torch, maps, 1, 3, 5, 1, 23, alpha=5.0, pitch=K.TILE + 9 + offset, offset=offset)


def test_the_masking_scene(torch):
    """three targets ten gates apart and one alone: the cell-averaging detector at its factor for 1e-6 misses the middle
    one, the ordered statistic at its own factor for the same rate reports all four"""
    p, c = K.mask_map(), K.MASK
    a_ca, a_os = K.mask_alphas()
    ref_ca, _ = R.detect(p[None], c["Wd"], c["Gr"], c["Tr"], c["Pd"], R.CA, a_ca)      # the reference first
    ref_os, _ = O.detect(p[None], c["Wd"], c["Gr"], c["Tr"], c["Pd"], K.MASK_RANK, a_os)
    assert cells(ref_ca) == [t for t in K.MASK_TARGETS if t != K.MASK_MISSED] and cells(ref_os) == K.MASK_TARGETS
    x = torch.from_numpy(p).cuda()
    ca = detect_maps(x, c["Wd"], c["Gr"], c["Tr"], pfa=K.MASK_PFA, peak_half_width=c["Pd"])
    assert len(ca) == 3 and K.MASK_MISSED not in cells(ca) and ca.tobytes() == ref_ca.tobytes()
    assert float(np.float32(cfar_alpha(K.MASK_PFA, 32))) == a_ca
    assert float(np.float32(os_cfar_alpha(K.MASK_PFA, 32, K.MASK_RANK))) == a_os
    found = detect_maps_os(x, c["Wd"], c["Gr"], c["Tr"], K.MASK_RANK, pfa=K.MASK_PFA, peak_half_width=c["Pd"])
    assert len(found) == 4 and cells(found) == K.MASK_TARGETS and found.tobytes() == ref_os.tobytes()
    assert (found["power"] > 2 * np.float32(a_os) * found["noise"]).all()


def test_the_chain_a_second_train_in_the_training_window(torch, monkeypatch):
    """pd_cases.CHAIN with a second train twelve times the first one's amplitude 232 gates behind it on the same
    Doppler bin: detect_targets (cell averaging) reports only the strong train, detect_targets(rank=...) both, in every
    interval; its records are the restatement's over the device's own maps"""
    c, Kp = pd_cases.CHAIN, pd_cases.CHAIN_K
    host = K.chain_stream()
    r = pd_cases.chain_replica()
    row, g1 = Kp // 2, c["first_pulse"]
    g2 = g1 + K.CHAIN_OFFSET
    maps = K.chain_maps(host)                                        # the reference first
    ref_ca, _ = K.chain_detect_ca(maps)
    ref_os, _ = K.chain_detect_os(maps)
    both = [(m, row, g) for m in range(pd_cases.CHAIN_CPIS) for g in (g1, g2)]
    assert [(int(d["map"]), int(d["row"]), int(d["gate"])) for d in ref_ca] == [t for t in both if t[2] == g2]
    assert [(int(d["map"]), int(d["row"]), int(d["gate"])) for d in ref_os] == both
    iq = torch.from_numpy(host).cuda()
    kw = dict(train_gates=K.CHAIN_RD["Tr"], doppler_half_width=K.CHAIN_RD["Wd"], peak_half_width=K.CHAIN_RD["Pd"],
              normalize=True, fs=c["fs"], chunk_samples=100000)
    with monkeypatch.context() as mp:                                # without a rank the new unit is not touched
        def refuse(*a, **k):
            raise AssertionError("OsCfar made without a rank")
        mp.setattr(os_cfar, "OsCfar", refuse)
        old = detect_targets(iq, r, c["pri"], Kp, alpha=K.CHAIN_CA_ALPHA, **kw)
        assert detect_targets(iq, r, c["pri"], Kp, alpha=K.CHAIN_CA_ALPHA, rank=None, **kw).tobytes() == old.tobytes()
    assert [(int(d["cpi"]), int(d["row"]), int(d["gate"])) for d in old] == [t for t in both if t[2] == g2]    # the gap
    found = detect_targets(iq, r, c["pri"], Kp, alpha=K.CHAIN_OS_ALPHA, rank=K.CHAIN_RANK, **kw)
    assert found.dtype == TARGET_DTYPE
    assert [(int(d["cpi"]), int(d["row"]), int(d["gate"])) for d in found] == both
    assert (found["doppler_bin"] == 0).all() and (found["power"] > np.float32(K.CHAIN_OS_ALPHA) * found["noise"]).all()
    assert np.allclose(found["power"], ref_os["power"], rtol=1e-3) and np.allclose(found["noise"], ref_os["noise"], rtol=2e-3)
    assert detect_targets(host, r, c["pri"], Kp, alpha=K.CHAIN_OS_ALPHA, rank=K.CHAIN_RANK, **kw).tobytes() == found.tobytes()
    pdws = targets_to_pdws(found[found["gate"] == g1], c["fs"], 915e6, 0.0, c["pri"], Kp, Kp)
    assert np.array_equal(pdws["toa"], (np.arange(3) * Kp * c["pri"] + g1 + 1) / c["fs"]) and (pdws["bin"] == 0).all()
    # default pfa (the ordered-statistic factor): the records are the restatement's over the device's own maps
    with MatchedFilter(r, "cf32", 16, "complex", True) as mf:
        y = mf.process(iq)
    dev_maps = range_doppler(y, c["pri"], Kp, output="power", centered=True, flush=True)
    assert tuple(dev_maps.shape) == (pd_cases.CHAIN_CPIS, Kp, c["pri"])
    dflt = detect_targets(iq, r, c["pri"], Kp, normalize=True, fs=c["fs"], chunk_samples=len(host), train_gates=16, rank=72)
    alpha = float(np.float32(os_cfar_alpha(1e-6, 2 * 16 * 3, 72)))
    ref_d, _ = O.detect(dev_maps.cpu().numpy(), 1, r.size, 16, 1, 72, alpha, 0.0)
    assert len(ref_d) >= 2 * pd_cases.CHAIN_CPIS
    for name, field in (("cpi", "map"), ("row", "row"), ("gate", "gate"), ("power", "power"), ("noise", "noise")):
        assert dflt[name].tobytes() == ref_d[field].astype(dflt[name].dtype).tobytes(), name
    assert rd_cfar.DET_DTYPE == DET_DTYPE
