"""The deinterleaver on the device: histogram, successors, steps and lengths, records, labels, count and stats against
the numpy restatement (deint_ref), byte for byte -- over the small lists of deint_cases that sit on one sentence of the
definition each, at the tile, workgroup and tier boundaries, through both histogram and both marking tiers, from host
and device memory, at an odd pointer and between guard bytes, across a stream switch, on the designed scene with its
companions, and along the chain: two pulse trains added sample by sample, detected and told apart."""
import ctypes as C
import importlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import deint_cases as DC  # noqa: E402
import deint_ref as R  # noqa: E402
from gpu_support import cuda_torch  # noqa: E402
from sdr_channelizer_amd import (Deinterleaver, PulseTrain, deinterleave, deinterleave_detections,  # noqa: E402
                                 deinterleave_pdws, detect_pulses, replica_from_pulse_train)
from sdr_channelizer_amd import _lib as L  # noqa: E402
from sdr_channelizer_amd.pdw import PDW_DTYPE  # noqa: E402

di = importlib.import_module("sdr_channelizer_amd.deinterleave")   # the module, not the function of the same name
GUARD = 0x5A


@pytest.fixture(scope="module")
def torch():
    return cuda_torch()


def make(c: R.Cfg) -> Deinterleaver:
    return Deinterleaver(c.pmin, c.pmax, c.W, **c.settings())


def on_device(torch, t):
    return torch.from_numpy(np.ascontiguousarray(t, np.uint64).view(np.int64)).cuda()


def periods_of(t, c):
    """periods worth a successor search: the first candidates of the whole list's histogram, and pmax"""
    taus = [c.pmax]
    if len(t) >= 2:
        taus += [tau for _, tau, _ in R.candidates(R.histogram(t, c), c, int(t[-1]) - int(t[0]))[:2]]
    return [tau for tau in taus if c.e * (2 * c.X + 3) < tau]


def check(d, x, t, c, want=None, taus=None, what=""):
    """every entry point on one list (x: t where the call reads it) against the restatement; returns the run's records"""
    assert d.histogram(x).tobytes() == R.histogram(t, c).tobytes(), what
    for tau in periods_of(t, c) if taus is None else taus:
        got, ref = d.successors(x, tau), R.lengths(t, c, tau)
        for g, r, name in zip(got, ref, ("succ", "step", "len")):
            assert g.dtype == np.int32 and g.tobytes() == r.tobytes(), (what, tau, name)
    rec, labels, stats = R.run(t, c) if want is None else want
    got_rec, got_labels = d.run(x)
    got_rec = di.records_to_numpy(got_rec)
    got_labels = got_labels if isinstance(got_labels, np.ndarray) else got_labels.cpu().numpy()
    assert got_rec.dtype == di.EMITTER_DTYPE and len(got_rec) == len(rec), (what, got_rec, rec)
    assert got_rec.tobytes() == rec.tobytes(), (what, got_rec, rec)
    assert got_labels.dtype == np.int32 and got_labels.tobytes() == labels.tobytes(), what
    assert d.stats == stats, (what, d.stats, stats)
    return got_rec


# -- the small lists ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(DC.CASES))
def test_the_designed_lists(torch, name):
    t, c = DC.CASES[name]()
    want = DC.expected(name)
    with make(c) as d:
        assert d.last_kernel == "" and d.stats == dict.fromkeys(di.STATS_FIELDS, 0)
        rec = check(d, t, t, c, want, what=name)
        tier = "pfb_deint_hist_lds" if c.NB <= DC.LDS_BINS else "pfb_deint_hist_global"
        assert d.plan.histogram_kernel.decode() == tier and d.num_bins == c.NB
        if len(t) >= c.min_pulses:
            assert tier in d.last_kernel.split("+"), d.last_kernel
        d.histogram(t)
        assert d.last_kernel == ("pfb_deint_compact+" + tier if len(t) else "")
        if len(t):
            check(d, on_device(torch, t), t, c, want, what=name + " from device memory")
    # what each case is there for
    if name.startswith("train_"):
        assert len(rec) == (1 if len(t) >= c.min_pulses else 0)
    if name == "train_5":
        assert (rec[0]["pulses"], rec[0]["periods"], rec[0]["period"], rec[0]["first_tick"], rec[0]["last_tick"]) == (5, 4, 100.0, 7, 407)
    if name.startswith("bins_") or name == "one_bin":
        assert len(rec) >= 1
    if name == "bins_65536":
        assert R.histogram(t, c)[-3:].any()                    # the top bins are in use
    if name == "equal_chains":
        assert len(rec) == 2 and rec["first_pulse"].tolist() == [0, 1] and rec["pulses"].tolist() == [10, 10]
    if name == "duplicates":
        assert len(rec) == 2 and rec["first_pulse"].tolist() == [0, 1]
    if name == "fill_at_boundary":
        assert (rec[0]["candidate_period"], rec[0]["pulses"], rec[0]["periods"]) == (100, 7, 8)      # 600 >= 75 * 8
    if name == "fill_refused":
        assert want[2]["candidates_refused"] == 1 and rec[0]["candidate_period"] == 200                 # 600 < 76 * 8
    if name == "fill_one_hit_better":
        assert (rec[0]["candidate_period"], rec[0]["pulses"], rec[0]["periods"]) == (100, 8, 8)
    if name in ("wide", "under_2_62"):
        assert len(rec) == 2 and int(t[-1]) - int(t[0]) > 1 << 32 and rec["period"].tolist() == list(DC.WIDE_PERIODS) and c.NB == 65536
    if name == "under_2_62":
        assert int(t[-1]) == (1 << 62) - 1
    if name == "max_emitters":
        assert len(rec) == 2 and len(DC.expected("scene")[0]) == 4
    if name == "level_256":
        assert (np.diff(t[:1000].astype(np.int64)) * 256 < c.pmax).all()


def test_the_difference_at_the_edges_of_the_period_range(torch):
    c = R.Cfg(pmin=1000, pmax=1999, W=100, Lv=2, min_pulses=3, X=1, tol=5)
    t = DC.edge_list(c)
    want = R.literal_histogram(t, c)
    assert want[0] >= 1 and want[-1] >= 1 and want.sum() < 2 * (len(t) - 1)     # some pairs fall outside on each side
    with make(c) as d:
        assert d.histogram(t).tobytes() == want.tobytes() == d.histogram(on_device(torch, t)).tobytes()


@pytest.mark.parametrize("X", (0, 2, 8))
def test_the_window_edges_and_the_ties(torch, X):
    c = R.Cfg(pmin=50, pmax=400, W=1, Lv=4, min_pulses=3, X=X, tol=2)
    with make(c) as d:
        for t in DC.window_lists(c, 100):
            got, ref, lit = d.successors(t, 100), R.lengths(t, c, 100), R.literal_successors(t, c, 100)
            assert got[0].tobytes() == ref[0].tobytes() == lit[0].tobytes(), t
            assert got[1].tobytes() == ref[1].tobytes() == lit[1].tobytes() and got[2].tobytes() == ref[2].tobytes(), t


def test_the_doubling_rounds(torch):
    c = DC.SMALL
    with make(c) as d:
        for t in DC.chain_lists():
            succ, step, ln = d.successors(t, 100)
            n = len(t)
            assert ln.tolist() == list(range(n, 0, -1)) and succ.tolist() == list(range(1, n)) + [-1], n
            assert step.tolist() == [1] * (n - 1) + [0]
        t = DC.chain_lists()[-1]                           # 1026 pulses in one chain, through the search
        rec = check(d, t, t, c, what="one long chain")
        assert len(rec) == 1 and rec[0]["pulses"] == len(t) == 1026


# -- the tiers ---------------------------------------------------------------------------------------------------------
def test_both_tiers_give_the_same_bytes(torch):
    lib = L.load()
    for name in ("scene", "bins_8192", "tile_2051"):
        t, c = (DC.NAMED[name] if name in DC.NAMED else DC.CASES[name])()
        want = DC.expected(name)
        with make(c) as d:
            seen = {}
            for hist, mark in ((0, 0), (1, 1), (2, 1), (1, 2), (2, 2)):
                assert lib.pfb_deint_set_tier(d._h, hist, mark) == L.PFB_OK
                rec = check(d, t, t, c, want, what=(name, hist, mark))
                ran = d.last_kernel.split("+")
                assert ("pfb_deint_hist_global" if hist == 2 else "pfb_deint_hist_lds") in ran
                assert ("pfb_deint_mark_walk" if mark == 1 else "pfb_deint_mark_tables") in ran
                seen[hist, mark] = rec.tobytes()
            assert len(set(seen.values())) == 1
            for bad in ((3, 0), (-1, 0), (0, 3), (0, -1)):
                assert lib.pfb_deint_set_tier(d._h, *bad) == L.PFB_ERR_BAD_ARG
    t, c = DC.CASES["bins_8193"]()
    with make(c) as d:
        assert lib.pfb_deint_set_tier(d._h, 1, 0) == L.PFB_ERR_UNSUPPORTED      # the LDS tier's bound
        assert lib.pfb_deint_set_tier(d._h, 2, 2) == L.PFB_OK
        check(d, t, t, c, DC.expected("bins_8193"), what="tables over the global tier")


# -- the calls ---------------------------------------------------------------------------------------------------------
def raw_run(d, ptr, n, mem, cap, torch=None):
    """pfb_deint_run between guard bytes: (status, count, records' buffer, labels' buffer) as numpy bytes"""
    lib = L.load()
    rb, lb = 48 * cap + 128, 4 * n + 128
    count = C.c_uint64(77)
    if mem == L.PFB_MEM_HOST:
        rec, lab = np.full(rb, GUARD, np.uint8), np.full(lb, GUARD, np.uint8)
        rc = lib.pfb_deint_run(d._h, C.c_void_p(ptr), n, mem, C.c_void_p(rec.ctypes.data + 64), cap, C.byref(count),
                               C.c_void_p(lab.ctypes.data + 64))
        return rc, count.value, rec, lab
    rec = torch.full((rb,), GUARD, dtype=torch.uint8, device="cuda")
    lab = torch.full((lb,), GUARD, dtype=torch.uint8, device="cuda")
    rc = lib.pfb_deint_run(d._h, C.c_void_p(ptr), n, mem, C.c_void_p(rec.data_ptr() + 64), cap, C.byref(count),
                           C.c_void_p(lab.data_ptr() + 64))
    torch.cuda.synchronize()
    return rc, count.value, rec.cpu().numpy(), lab.cpu().numpy()


def test_a_capacity_one_short_and_the_guard_bytes(torch):
    t, c = DC.NAMED["scene"]()
    rec, labels, stats = DC.expected("scene")
    x = on_device(torch, t)
    with make(c) as d:
        for mem, ptr in ((L.PFB_MEM_HOST, t.ctypes.data), (L.PFB_MEM_DEVICE, x.data_ptr())):
            rc, count, rb, lb = raw_run(d, ptr, len(t), mem, 4, torch)
            assert (rc, count) == (L.PFB_OK, 4)
            assert rb[64:64 + 192].tobytes() == rec.tobytes() and lb[64:64 + 4 * len(t)].tobytes() == labels.tobytes()
            assert (rb[:64] == GUARD).all() and (rb[64 + 192:] == GUARD).all()
            assert (lb[:64] == GUARD).all() and (lb[64 + 4 * len(t):] == GUARD).all()
            assert d.stats == stats
            # one record short: the true count, nothing written, the stats of the run before
            small = DC.train(100, 3)
            assert raw_run(d, small.ctypes.data, 3, L.PFB_MEM_HOST, 4)[:2] == (L.PFB_OK, 0) and d.stats["rounds"] == 0
            rc, count, rb, lb = raw_run(d, ptr, len(t), mem, 3, torch)
            assert (rc, count) == (L.PFB_ERR_CAPACITY, 4)
            assert (rb == GUARD).all() and (lb == GUARD).all() and d.stats["rounds"] == 0
            rc, count, rb, lb = raw_run(d, ptr, len(t), mem, 0, torch)
            assert (rc, count) == (L.PFB_ERR_CAPACITY, 4) and (rb == GUARD).all() and (lb == GUARD).all()
        with pytest.raises(L.PfbError) as e:
            d.run(t, capacity=3)
        assert e.value.status == L.PFB_ERR_CAPACITY


def test_a_list_out_of_order_is_refused_with_nothing_written(torch):
    lib = L.load()
    t, c = DC.CASES["tile_2051"]()
    with make(c) as d:
        for at, value in ((1, int(t[0]) - 1 if t[0] else None), (1500, int(t[1499]) - 1), (len(t) - 1, int(t[-2]) - 1),
                          (0, 1 << 62), (len(t) - 1, 1 << 62), (len(t) - 1, (1 << 64) - 1)):
            if value is None:
                continue
            bad = t.copy()
            bad[at] = value
            x = on_device(torch, bad)
            for mem, ptr in ((L.PFB_MEM_HOST, bad.ctypes.data), (L.PFB_MEM_DEVICE, x.data_ptr())):
                rc, count, rb, lb = raw_run(d, ptr, len(t), mem, 8, torch)
                assert (rc, count) == (L.PFB_ERR_BAD_ARG, 77) and (rb == GUARD).all() and (lb == GUARD).all(), (at, value)
            out = np.full(c.NB + 4, 0x5A5A5A5A, np.uint32)
            assert lib.pfb_deint_histogram(d._h, C.c_void_p(bad.ctypes.data), len(t), L.PFB_MEM_HOST,
                                           C.c_void_p(out.ctypes.data), c.NB) == L.PFB_ERR_BAD_ARG
            assert (out == 0x5A5A5A5A).all()
            with pytest.raises(L.PfbError):
                d.successors(bad, 1210)
        check(d, t, t, c, DC.expected("tile_2051"), what="after the refusals")
        # what is checked before the device
        p = C.c_void_p(t.ctypes.data)
        u = C.c_uint64(77)
        BAD = L.PFB_ERR_BAD_ARG
        lab = np.zeros(len(t), np.int32)
        lp, n = C.c_void_p(lab.ctypes.data), len(t)
        rec = np.zeros(8, di.EMITTER_DTYPE)
        rp = C.c_void_p(rec.ctypes.data)
        assert lib.pfb_deint_run(d._h, p, n, 2, rp, 8, C.byref(u), lp) == BAD
        assert lib.pfb_deint_run(d._h, p, (1 << 20) + 1, 0, rp, 8, C.byref(u), lp) == BAD
        assert lib.pfb_deint_run(d._h, None, n, 0, rp, 8, C.byref(u), lp) == BAD
        assert lib.pfb_deint_run(d._h, p, n, 0, None, 8, C.byref(u), lp) == BAD
        assert lib.pfb_deint_run(d._h, p, n, 0, rp, 8, None, lp) == lib.pfb_deint_run(d._h, p, n, 0, rp, 8, C.byref(u), None) == BAD
        x = on_device(torch, t)
        dl = torch.zeros(n + 2, dtype=torch.int32, device="cuda")
        dr = torch.zeros(8 * 48 + 16, dtype=torch.uint8, device="cuda")
        xp, dlp, drp = x.data_ptr(), dl.data_ptr(), dr.data_ptr()
        assert lib.pfb_deint_run(d._h, C.c_void_p(xp + 4), n - 1, 1, C.c_void_p(drp), 8, C.byref(u), C.c_void_p(dlp)) == BAD
        assert lib.pfb_deint_run(d._h, C.c_void_p(xp), n, 1, C.c_void_p(drp + 4), 8, C.byref(u), C.c_void_p(dlp)) == BAD
        assert lib.pfb_deint_run(d._h, C.c_void_p(xp), n, 1, C.c_void_p(drp), 8, C.byref(u), C.c_void_p(dlp + 2)) == BAD
        assert lib.pfb_deint_histogram(d._h, p, n, 0, None, c.NB) == BAD
        assert lib.pfb_deint_histogram(d._h, p, n, 0, lp, c.NB - 1) == L.PFB_ERR_CAPACITY
        for period in (0, 1 << 32, c.e * (2 * c.X + 3)):
            assert lib.pfb_deint_successors(d._h, p, n, 0, period, lp, lp, lp) == BAD
        assert lib.pfb_deint_successors(d._h, p, n, 0, 1210, None, lp, lp) == BAD
        assert u.value == 77 and not lab.any() and not dl.any().item() and not dr.any().item()


def test_host_memory_an_odd_device_pointer_and_the_same_call_twice(torch):
    t, c = DC.NAMED["scene"]()
    want = DC.expected("scene")
    room = torch.zeros(len(t) + 1, dtype=torch.int64, device="cuda")
    assert room.data_ptr() % 256 == 0
    x = room[1:]
    x.copy_(on_device(torch, t))
    assert x.data_ptr() % 256 == 8
    with make(c) as d:
        first = check(d, t, t, c, want, what="host")
        again = check(d, x, t, c, want, what="device, 8 bytes off")
        assert check(d, x, t, c, want, what="twice").tobytes() == again.tobytes() == first.tobytes()
        rec, labels = d.run(x)
        assert labels.is_cuda and labels.dtype == torch.int32 and rec.is_cuda and tuple(rec.shape) == (4, 48)
        # a shorter list after a longer one, in the kept scratch
        short = DC.CASES["group_257"]()[0]           # its ticks alone, under the scene's settings
    with make(c) as d:
        d.run(t)
        got = d.run(short)
        ref = R.run(short, c)
        assert got[0].tobytes() == ref[0].tobytes() and got[1].tobytes() == ref[1].tobytes()


def test_a_stream_switch_between_runs(torch):
    t, c = DC.NAMED["scene"]()
    want = DC.expected("scene")
    x = on_device(torch, t)
    side = torch.cuda.Stream()
    with make(c) as d:
        check(d, x, t, c, want, what="the null stream")
        d.set_stream(side.cuda_stream)
        with torch.cuda.stream(side):
            y = x.clone()
        check(d, y, t, c, want, what="a side stream")
        d.sync()
        d.set_stream(0)
        check(d, t, t, c, want, what="back on the null stream")


# -- the scene ---------------------------------------------------------------------------------------------------------
def test_the_designed_scene_and_its_companions(torch):
    t, who = DC.scene()
    for name in ("scene", "scene_no_fill"):
        c = DC.NAMED[name]()[1]
        rec, labels, stats = want = DC.expected(name)
        if name == "scene":                 # the conditions on the input, before the comparison that uses it
            rows, strays = DC.quality(who, rec, labels)
            assert len(rec) == 4 and all(p >= 0.98 and s >= 0.90 for _, p, s in rows) and strays <= 5
        else:
            assert len(rec) > 4 and rec[0]["candidate_period"] == 1202
        with make(c) as d:
            check(d, t, t, c, want, what=name)
            check(d, on_device(torch, t), t, c, want, what=name + " from device memory")
    # twice the period is a candidate of the first round, and the period is what the first record holds
    c = DC.SCENE
    k2 = (4096 - c.pmin) // c.W
    with make(c) as d:
        C_ = d.histogram(t)
        assert R.is_candidate(C_, c, int(t[-1]) - int(t[0]), k2)
        assert di.records_to_numpy(d.run(t)[0])[0]["bin"] == (2048 - c.pmin) // c.W
    # the one-shot forms
    rec, labels = deinterleave(t, c.pmin, c.pmax, c.W, **c.settings())
    assert rec.tobytes() == DC.expected("scene")[0].tobytes() and labels.tobytes() == DC.expected("scene")[1].tobytes()
    pdws = np.zeros(len(t), PDW_DTYPE)
    shuffle = np.random.default_rng(3).permutation(len(t))
    pdws["toa"] = 10.0 + t[shuffle].astype(np.float64) / 2.0e6      # frames of a 2 MHz clock, in any order
    rec2, labels2 = deinterleave_pdws(pdws, 2.0e6, c.pmin, c.pmax, c.W, t0=10.0, **c.settings())
    ticks, order = R.ticks_from_toa(pdws["toa"], 10.0, 2.0e6)
    ref = R.run(ticks, c)
    back = np.full(len(t), -1, np.int32)
    back[order] = ref[1]
    assert rec2.tobytes() == ref[0].tobytes() and labels2.tobytes() == back.tobytes() and len(rec2) == 4


# -- the chain ---------------------------------------------------------------------------------------------------------
def test_the_chain_tells_two_pulse_trains_apart(torch):
    """two Barker-13 trains, PRI 2048 and 3000 samples, added sample by sample with their noise; detect_pulses finds
    the pulses of both in one list, deinterleave_detections returns the two trains"""
    kw = dict(sample_format="cf32", barker13=True, barker_degrees=True, phase_from_zero=True, f0=31250.0, fs=2.0e6, pw=104,
              amplitude=0.3, bit_width=16)
    trains = ((2048, 700), (3000, 1900))
    n = 40 * 3000
    r = replica_from_pulse_train(pri=2048, **kw)
    iq = None
    for seed, (pri, first) in enumerate(trains):
        with PulseTrain(first_pulse=first, pri=pri, noise_sigma=0.02, seed=seed + 1, **kw) as pt:
            part = pt.generate(n)
        iq = part if iq is None else iq + part
    found = detect_pulses(iq, r, normalize=True)
    ticks = np.ascontiguousarray(found.records["peak_index"], np.uint64)
    known = [np.arange(first, n - 104, pri) for pri, first in trains]
    # a detection belongs to a train when it lies on one of its pulses and off the other train's pulses
    near = [np.abs(ticks.astype(np.int64)[:, None] - k[None, :]).min(axis=1) for k in known]
    who = np.where((near[0] <= 2) & (near[1] > 104), 0, np.where((near[1] <= 2) & (near[0] > 104), 1, -1))
    # a pulse within 104 samples of the other train's is nobody's: 208 / 3000 = 7 % of the first train's pulses and
    # 208 / 2048 = 10 % of the second's on average, so three quarters of each must be left
    print("detections %d: %d of %d and %d of %d pulses attributed" % (len(ticks), (who == 0).sum(), len(known[0]),
                                                                       (who == 1).sum(), len(known[1])))
    assert (who == 0).sum() >= 0.75 * len(known[0]) and (who == 1).sum() >= 0.75 * len(known[1])
    c = R.Cfg(pmin=1000, pmax=7000, W=4, Lv=8, detect=30, min_pulses=8, X=3, tol=4, fill=50, max_emitters=8)
    # the reference first, on the same detections
    rec, labels, _ = R.run(ticks, c)
    assert len(rec) == 2
    for e in range(2):
        train = int(np.bincount(who[(labels == e) & (who >= 0)]).argmax())
        assert abs(rec[e]["period"] - trains[train][0]) <= 1e-3 * trains[train][0]
        assert (labels[who == train] == e).all() and (who[labels == e] != 1 - train).all()
    got, got_labels = deinterleave_detections(found, c.pmin, c.pmax, c.W, **c.settings())
    assert got.tobytes() == rec.tobytes() and got_labels.tobytes() == labels.tobytes()
    assert deinterleave_detections(found.records, c.pmin, c.pmax, c.W, **c.settings())[0].tobytes() == rec.tobytes()
