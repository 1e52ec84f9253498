"""The range-Doppler CFAR detector on the GPU against the numpy restatement (rdcfar_ref), byte for byte: records, counts
and stats.  The shape grid crosses every ND with the gate counts around the tile and three (Gr, Tr) pairs; Wd, the
method, the pitch and the pointer's offset from a 256-byte boundary are drawn per shape by a hash, so each occurs with
every ND and R class.  Then wrap and clip, the order of the sums, ties, non-finite cells, the cuttings of a sequence of
maps into calls, and the chain from I/Q to two trains in one gate."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import pd_cases  # noqa: E402
import rdcfar_cases as K  # noqa: E402
import rdcfar_ref as R  # noqa: E402
from gpu_support import Busy, cuda_torch  # noqa: E402
from rdmap_support import SENTINEL, place, run_async  # noqa: E402
from sdr_channelizer_amd import (MatchedFilter, RangeDopplerCfar, cfar_alpha, detect_maps, detect_pulse_train,  # noqa: E402
                                 detect_targets, fit_event, range_doppler, targets_to_pdws)
from sdr_channelizer_amd import _lib as L  # noqa: E402
from sdr_channelizer_amd.rd_cfar import DET_DTYPE, TARGET_DTYPE, records  # noqa: E402

METHODS = {R.CA: "ca", R.GO: "go", R.SO: "so"}


@pytest.fixture(scope="module")
def torch():
    return cuda_torch()


def check(torch, maps, Wd, Gr, Tr, Pd, method=R.CA, alpha=4.0, min_power=0.0, pitch=0, offset=0, kernel=None):
    want, wstats = R.detect(maps, Wd, Gr, Tr, Pd, method, alpha, min_power)
    n, ND, Rg = maps.shape
    x = place(torch, maps, pitch, offset)
    with RangeDopplerCfar(ND, Rg, Wd, Gr, Tr, alpha, peak_half_width=Pd, method=METHODS[method], min_power=min_power,
                          pitch=pitch) as det:
        got, count = run_async(torch, det, x, len(want) + 3)
        assert count == len(want) and got.tobytes() == want.tobytes(), (maps.shape, Wd, Gr, Tr, Pd, method, pitch, offset)
        assert det.stats == wstats and det.next_map == n
        if kernel:
            assert det.last_kernel == f"pfb_rdcfar_cells<{kernel}>"
        det.reset()
        again = records(det.process(x))                            # the synchronous call, the same bytes
        assert again.tobytes() == want.tobytes() and det.stats == wstats
    return want


def gate_counts(Gr, Tr):
    T = K.TILE
    return sorted({1, max(Gr, 1), Gr + 1, Gr + Tr, 2 * (Gr + Tr) + 1, T - 1, T, T + 1, 2 * T + 3})


@pytest.mark.parametrize("Gr,Tr", [(0, 1), (2, 4), (104, 16)])
@pytest.mark.parametrize("ND", [1, 3, 8, 64, 1000, 1024])
def test_shape_grid(torch, ND, Gr, Tr):
    widths = sorted({0, min(1, (ND - 1) // 2), min((ND - 1) // 2, 16)})
    for i, Rg in enumerate(gate_counts(Gr, Tr)):
        h = ((i + 1) * 2654435761 + ND * 40503 + Gr * 97) >> 5
        Wd = widths[h % len(widths)]
        Pd = min((ND - 1) // 2, (h >> 3) % 3)
        method = (R.CA, R.GO, R.SO)[(h >> 5) % 3]
        pitch = Rg + (h >> 7) % 5 if (h >> 10) & 1 else 0
        offset = (h >> 11) & 3
        n = 2 if ND * Rg <= 1 << 16 else 1
        maps = K.noise_maps(n, ND, Rg, seed=i + ND, share=0.004 if ND * Rg > 4096 else 0.05)
        check(torch, maps, Wd, Gr, Tr, Pd, method, alpha=6.0, min_power=0.25, pitch=pitch, offset=offset)


@pytest.mark.parametrize("Wd,Pd,kernel", [(1, 1, "lds"), (2, 2, "direct")])
def test_the_widest_window_on_one_short_map(torch, Wd, Pd, kernel):
    """Gr = 1024, Tr = 256: the block with its halo fits LDS for one row of halo, and does not for two"""
    for Rg in (1024, 1025, 1280, 2561, 2600):
        maps = K.noise_maps(1, 6, Rg, seed=Rg, share=0.003)
        check(torch, maps, Wd, 1024, 256, Pd, (R.CA, R.GO, R.SO)[Rg % 3], alpha=5.0, offset=Rg % 4, kernel=kernel)


def test_every_method_on_every_halo(torch):
    maps = K.noise_maps(2, 40, K.TILE + 9, seed=77, share=0.01)
    for method in (R.CA, R.GO, R.SO):
        for Wd, Pd in ((0, 0), (1, 0), (0, 2), (16, 3), (3, 16)):
            check(torch, maps, Wd, 3, 5, Pd, method, alpha=5.0, pitch=K.TILE + 12, offset=1)


def test_wrap_and_clip(torch):
    ND, Rg = 12, K.TILE + 30
    kw = dict(Wd=2, Gr=3, Tr=6, Pd=2, alpha=5.0)
    for row, seen_from in ((0, ND - 1), (ND - 1, 0)):
        p = np.ones((1, ND, Rg), np.float32)
        p[0, row, 100] = 900.0             # raises A of rows row-2 .. row+2 through the wrap, and sits in their boxes
        p[0, seen_from, 101] = 800.0       # beaten by it through the wrap
        p[0, seen_from, 107] = 100.0       # trains on gates 98 .. 103: over only if the wrap left the 900 out of A
        want = check(torch, p, **kw)
        assert [(int(d["row"]), int(d["gate"])) for d in want] == [(row, 100)]
    p = np.ones((1, ND, Rg), np.float32)
    p[0, 4, 0] = p[0, 5, Rg - 1] = 300.0
    want = check(torch, p, **kw)
    assert [(int(d["gate"]), int(d["flags"]), int(d["training_cells"])) for d in want] == [(0, 1, 30), (Rg - 1, 1, 30)]
    for Rg in (1, 3, 4):                   # R <= Gr + 1: nothing detects, every cell is counted without noise
        p = np.full((2, ND, Rg), 7.0, np.float32)
        with RangeDopplerCfar(ND, Rg, 2, 3, 6, 1.0, peak_half_width=2) as det:
            assert len(det.process(p)) == 0
            assert det.stats == {"maps_in": 2, "cells_over": 0, "cells_without_noise": 2 * ND * Rg, "detections": 0,
                                 "dropped": 0}


def test_the_sums_are_walked_in_the_defined_order(torch):
    c = K.ORDER_GATES
    check(torch, K.order_map_gates()[None], c["Wd"], c["Gr"], c["Tr"], c["Pd"], R.CA, c["alpha"])
    check(torch, K.order_map_gates()[None], c["Wd"], c["Gr"], c["Tr"], c["Pd"], R.GO, c["alpha"], offset=3)
    c = K.ORDER_ROWS
    check(torch, K.order_map_rows()[None], c["Wd"], c["Gr"], c["Tr"], c["Pd"], R.CA, c["alpha"])
    check(torch, K.order_map_rows()[None], c["Wd"], c["Gr"], c["Tr"], c["Pd"], R.SO, c["alpha"], pitch=K.TILE + 6)


def test_ties_and_the_peak_box(torch):
    want = check(torch, K.tie_map()[None], method=R.CA, **K.TIE)
    got = [(int(d["row"]), int(d["gate"])) for d in want]
    assert got == sorted([min(a, b) for a, b in K.TIE_INSIDE] + [c for pair in K.TIE_OUTSIDE for c in pair])
    Gr = K.TIE["Gr"]                       # two spikes Gr and Gr + 1 gates apart
    for gap, n in ((Gr, 1), (Gr + 1, 2)):
        p = np.ones((1, 4, K.TILE + 20), np.float32)
        p[0, 2, K.TILE - 1] = 400.0
        p[0, 2, K.TILE - 1 + gap] = 300.0
        assert len(check(torch, p, **K.TIE)) == n


def test_non_finite_cells(torch):
    p = K.nonfinite_map()
    for method in (R.CA, R.GO, R.SO):
        check(torch, p[None], method=method, **K.NONFINITE)


def test_cuttings(torch):
    ND, Rg, n = 8, K.TILE + 5, 9
    kw = dict(peak_half_width=1, min_power=0.5)
    maps = K.noise_maps(n, ND, Rg, seed=11, share=0.01)
    want, wstats = R.detect(maps, 1, 2, 4, 1, R.CA, 5.0, 0.5)
    x = torch.from_numpy(maps).cuda()
    rng = np.random.default_rng(0)
    cuts = [[0, n], list(range(n + 1)), [0, 0, 3, 3, n, n]]
    cuts += [[0] + sorted(rng.integers(0, n + 1, 3).tolist()) + [n] for _ in range(3)]
    cuts.append(cuts[-1])                  # the same cutting twice
    with RangeDopplerCfar(ND, Rg, 1, 2, 4, 5.0, **kw) as det:
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
    assert detect_maps(x, 1, 2, 4, 5.0, **kw).tobytes() == want.tobytes()
    assert detect_maps(maps, 1, 2, 4, 5.0, **kw).tobytes() == want.tobytes()


def test_host_memory_over_three_staging_steps(torch):
    """maps of 1024 rows of three gates: a step takes 2^18 words of 64 gates, 256 such maps, so 517 are three steps"""
    n = 2 * 256 + 5
    maps = K.noise_maps(n, 1024, 3, seed=5, share=0.005, level=100.0)
    want, wstats = R.detect(maps, 1, 0, 1, 1, R.SO, 20.0)
    assert len(want) > 1000 and int(want["map"][-1]) > 512
    with RangeDopplerCfar(1024, 3, 1, 0, 1, 20.0, peak_half_width=1, method="so") as det:
        got = records(det.process(maps))
        assert got.tobytes() == want.tobytes() and det.stats == wstats
        det.reset()
        assert records(det.process(torch.from_numpy(maps).cuda())).tobytes() == want.tobytes()


def test_a_capacity_one_short_changes_nothing(torch):
    ND, Rg = 8, K.TILE + 5
    maps = K.noise_maps(4, ND, Rg, seed=21, share=0.01)
    first, fstats = R.detect(maps[:1], 1, 2, 4, 1, R.CA, 5.0)
    rest, _ = R.detect(maps[1:], 1, 2, 4, 1, R.CA, 5.0, first_map=1)
    whole, wstats = R.detect(maps, 1, 2, 4, 1, R.CA, 5.0)
    lib = L.load()
    x = torch.from_numpy(maps).cuda()
    with RangeDopplerCfar(ND, Rg, 1, 2, 4, 5.0, peak_half_width=1) as det:
        assert records(det.process(x[:1])).tobytes() == first.tobytes()
        for mem, src in ((L.PFB_MEM_DEVICE, x[1:]), (L.PFB_MEM_HOST, maps[1:])):
            cap = len(rest) - 1
            count = C.c_uint64(0)
            if mem == L.PFB_MEM_DEVICE:
                buf = torch.zeros((cap, 4), dtype=torch.int64, device="cuda")
                ptr, data = buf.data_ptr(), src.data_ptr()
            else:
                buf = np.zeros(cap, DET_DTYPE)
                ptr, data = buf.ctypes.data, src.ctypes.data
            rc = lib.pfb_rdcfar_process(det._h, C.c_void_p(data), 3, C.c_void_p(ptr), cap, C.byref(count), mem)
            assert rc == L.PFB_ERR_CAPACITY and count.value == len(rest)
            assert det.next_map == 1 and det.stats == fstats
        assert records(det.process(x[1:])).tobytes() == rest.tobytes()
        assert det.stats == wstats and det.next_map == 4


def test_async_across_a_stream_switch_with_truncation(torch):
    ND, Rg = 8, K.TILE + 5
    maps = K.noise_maps(6, ND, Rg, seed=31, share=0.01)
    a, _ = R.detect(maps[:3], 1, 2, 4, 1, R.CA, 5.0)
    b, _ = R.detect(maps[3:], 1, 2, 4, 1, R.CA, 5.0, first_map=3)
    _, wstats = R.detect(maps, 1, 2, 4, 1, R.CA, 5.0)
    x = torch.from_numpy(maps).cuda()
    busy = Busy(torch)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    cap_b = len(b) - 4
    out_a = torch.full((len(a) + 2, 4), SENTINEL, dtype=torch.int64, device="cuda")
    out_b = torch.full((cap_b + 1, 4), SENTINEL, dtype=torch.int64, device="cuda")
    counts = torch.full((2,), SENTINEL, dtype=torch.int64, device="cuda")
    with RangeDopplerCfar(ND, Rg, 1, 2, 4, 5.0, peak_half_width=1) as det:
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


def test_the_chain_two_trains_in_one_gate(torch):
    """pd_cases.CHAIN with a second, weaker train in gate 700 on Doppler bin 9: detect_pulse_train collapses the rows
    and returns one record per interval; detect_targets returns both trains in every interval."""
    c, Kp = pd_cases.CHAIN, pd_cases.CHAIN_K
    host = K.chain2_stream()
    r = pd_cases.chain_replica()
    gate, rows = c["first_pulse"], (Kp // 2, Kp // 2 + K.CHAIN2_BIN)
    maps = K.chain_maps(host)                                        # the reference first
    ref, _ = K.chain_detect(maps, K.CHAIN_ALPHA)
    want = [(m, row, gate) for m in range(pd_cases.CHAIN_CPIS) for row in rows]
    assert [(int(d["map"]), int(d["row"]), int(d["gate"])) for d in ref] == want
    iq = torch.from_numpy(host).cuda()
    old = detect_pulse_train(iq, r, c["pri"], Kp, normalize=True, fs=c["fs"], chunk_samples=100000)
    assert [(int(d["cpi"]), int(d["gate"])) for d in old] == [(m, gate) for m in range(pd_cases.CHAIN_CPIS)]   # the gap
    kw = dict(alpha=K.CHAIN_ALPHA, train_gates=K.CHAIN_RD["Tr"], doppler_half_width=K.CHAIN_RD["Wd"],
              peak_half_width=K.CHAIN_RD["Pd"], normalize=True, fs=c["fs"], chunk_samples=100000)
    found = detect_targets(iq, r, c["pri"], Kp, **kw)
    assert found.dtype == TARGET_DTYPE
    assert [(int(d["cpi"]), int(d["row"]), int(d["gate"])) for d in found] == want
    assert [int(d["doppler_bin"]) for d in found] == [0, K.CHAIN2_BIN] * pd_cases.CHAIN_CPIS
    assert np.allclose(found["frequency"], found["doppler_bin"] * c["fs"] / (Kp * c["pri"]), rtol=1e-12, atol=0)
    assert (found["power"] > np.float32(K.CHAIN_ALPHA) * found["noise"]).all()
    assert np.allclose(found["power"], ref["power"], rtol=1e-3) and np.allclose(found["noise"], ref["noise"], rtol=1e-3)
    assert detect_targets(host, r, c["pri"], Kp, **kw).tobytes() == found.tobytes()      # the same from host memory
    second = found[found["doppler_bin"] == K.CHAIN2_BIN]
    pdws = targets_to_pdws(second, c["fs"], 915e6, 0.0, c["pri"], Kp, Kp)
    assert np.array_equal(pdws["toa"], (np.arange(3) * Kp * c["pri"] + gate + 1) / c["fs"]) and (pdws["bin"] == K.CHAIN2_BIN).all()
    t_peak, snr_peak, coef = fit_event(pdws)
    assert pdws["toa"][0] < t_peak < pdws["toa"][2] and coef[2] < 0
    # under a Hann window, default pfa: the records are the restatement's over the device's own maps
    w = K.chain_hann()
    with MatchedFilter(r, "cf32", 16, "complex", True) as mf:
        y = mf.process(iq)
    dev_maps = range_doppler(y, c["pri"], Kp, window=w, output="power", centered=True, flush=True)
    assert tuple(dev_maps.shape) == (pd_cases.CHAIN_CPIS, Kp, c["pri"])
    hann = detect_targets(iq, r, c["pri"], Kp, window=w, normalize=True, fs=c["fs"], chunk_samples=len(host))
    alpha = float(np.float32(cfar_alpha(1e-6, 2 * 64 * 3)))
    ref_h, _ = R.detect(dev_maps.cpu().numpy(), 1, r.size, 64, 1, R.CA, alpha, 0.0)
    assert len(ref_h) >= 2 * pd_cases.CHAIN_CPIS
    for name, field in (("cpi", "map"), ("row", "row"), ("gate", "gate"), ("power", "power"), ("noise", "noise")):
        assert hann[name].tobytes() == ref_h[field].astype(hann[name].dtype).tobytes(), name
