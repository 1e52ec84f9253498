"""The PDW association on the device: labels, records, count, stats (without rounds) and links against the numpy
restatement (assoc_ref), byte for byte -- over the designed lists of assoc_cases that sit on one sentence of the
definition each, at the tile and tier boundaries, through both tiers, from host and device memory, between guard bytes,
across a stream switch, on one list of 2^20 items, and along the chain: a chirp train through the channelizer and the
extractor, several rows a pulse, fused to one and handed to the deinterleaver."""
import ctypes as C
import importlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import assoc_cases as AC  # noqa: E402
import assoc_ref as R  # noqa: E402
from gpu_support import cuda_torch  # noqa: E402
from sdr_channelizer_amd import (Channelizer, PulseAssociator, PulseTrain, associate, associate_pdws,  # noqa: E402
                                 deinterleave, fuse_pdws)
from sdr_channelizer_amd import _lib as L  # noqa: E402
from sdr_channelizer_amd.pdw import PDW_DTYPE, extract_pdws  # noqa: E402

am = importlib.import_module("sdr_channelizer_amd.associate")   # the module, not the function of the same name
GUARD = 0x5A
LDS, GLOBAL = "pfb_assoc_link_lds", "pfb_assoc_link_global"


@pytest.fixture(scope="module")
def torch():
    return cuda_torch()


def make(c: R.Cfg) -> PulseAssociator:
    return PulseAssociator(**c.settings())


def on_device(torch, it):
    return torch.from_numpy(np.ascontiguousarray(it).view(np.uint8).reshape(-1, 24).copy()).cuda()


def check(a, x, want, what=""):
    """both entry points on one list (x: the items where the call reads them) against the restatement; returns the
    records"""
    rec, labels, stats, (first, count) = want
    got_first, got_count = a.links(x)
    assert got_first.dtype == got_count.dtype == np.int32, what
    assert got_first.tobytes() == first.tobytes() and got_count.tobytes() == count.tobytes(), what
    got_rec, got_labels = a.run(x)
    got_rec = am.groups_to_numpy(got_rec)
    got_labels = got_labels if isinstance(got_labels, np.ndarray) else got_labels.cpu().numpy()
    assert got_rec.dtype == am.GROUP_DTYPE and len(got_rec) == len(rec), (what, len(got_rec), len(rec))
    assert got_rec.tobytes() == rec.tobytes(), (what, got_rec[:8], rec[:8])
    assert got_labels.dtype == np.int32 and got_labels.tobytes() == labels.tobytes(), what
    got_stats = a.stats
    rounds = got_stats.pop("rounds")
    assert got_stats == stats, (what, got_stats, stats)
    assert rounds <= 64 and (rounds >= 1) == (stats["edges"] > 0), (what, rounds)
    return got_rec


# -- the designed lists ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(AC.CASES))
def test_the_designed_lists(torch, name):
    it, c = AC.inputs(name)
    want = AC.expected(name)
    tier = LDS if c.K <= AC.LDS_WINDOW else GLOBAL
    with make(c) as a:
        assert a.last_kernel == "" and a.stats == dict.fromkeys(am.STATS_FIELDS, 0)
        assert (a.plan.tile_items, a.plan.lds_window, a.plan.link_kernel.decode()) == (AC.TILE, AC.LDS_WINDOW, tier)
        check(a, it, want, what=name)
        if len(it):
            ran = a.last_kernel.split("+")
            assert ran[:2] == ["pfb_assoc_prep", tier] and ran[-2:] == ["pfb_assoc_number", "pfb_assoc_gather"], ran
            assert ("pfb_assoc_hook" in ran) == ("pfb_assoc_jump" in ran) == (want[2]["edges"] > 0)
            a.links(it)
            assert a.last_kernel == "pfb_assoc_prep+" + tier
            check(a, on_device(torch, it), want, what=name + " from device memory")
        else:
            assert a.last_kernel == ""
    if name == "backward":
        with make(c) as a:
            a.run(it)
            print("backward: the device went round %d times" % a.stats["rounds"])


def test_both_tiers_give_the_same_bytes(torch):
    lib = L.load()
    for name in ("tiles_3_plus_1", "lds_window_at_k", "lds_window_at_k_plus_1", "star", "staircase", "random_dense"):
        it, c = AC.inputs(name)
        want = AC.expected(name)
        with make(c) as a:
            seen = []
            for tier, kernel in ((0, LDS), (2, GLOBAL), (1, LDS), (2, GLOBAL)):
                assert lib.pfb_assoc_set_tier(a._h, tier) == L.PFB_OK
                seen.append(check(a, it, want, what=(name, tier)).tobytes())
                assert kernel in a.last_kernel.split("+") and (LDS in a.last_kernel) != (GLOBAL in a.last_kernel)
            assert len(set(seen)) == 1
            for bad in (3, -1):
                assert lib.pfb_assoc_set_tier(a._h, bad) == L.PFB_ERR_BAD_ARG
    it, c = AC.inputs("global_window_at_k")
    with make(c) as a:
        assert lib.pfb_assoc_set_tier(a._h, 1) == L.PFB_ERR_UNSUPPORTED          # the LDS tier's bound
        assert lib.pfb_assoc_set_tier(a._h, 2) == L.PFB_OK
        check(a, it, AC.expected("global_window_at_k"), what="over the LDS tier's bound")


# -- the calls ---------------------------------------------------------------------------------------------------------
def raw_run(a, ptr, n, mem, cap, torch=None):
    """pfb_assoc_run between guard bytes: (status, count, records' buffer, labels' buffer) as numpy bytes"""
    lib = L.load()
    rb, lb = 48 * cap + 128, 4 * n + 128
    count = C.c_uint64(77)
    if mem == L.PFB_MEM_HOST:
        rec, lab = np.full(rb, GUARD, np.uint8), np.full(lb, GUARD, np.uint8)
        rc = lib.pfb_assoc_run(a._h, C.c_void_p(ptr), n, mem, C.c_void_p(rec.ctypes.data + 64), cap, C.byref(count),
                               C.c_void_p(lab.ctypes.data + 64))
        return rc, count.value, rec, lab
    rec = torch.full((rb,), GUARD, dtype=torch.uint8, device="cuda")
    lab = torch.full((lb,), GUARD, dtype=torch.uint8, device="cuda")
    rc = lib.pfb_assoc_run(a._h, C.c_void_p(ptr), n, mem, C.c_void_p(rec.data_ptr() + 64), cap, C.byref(count),
                           C.c_void_p(lab.data_ptr() + 64))
    torch.cuda.synchronize()
    return rc, count.value, rec.cpu().numpy(), lab.cpu().numpy()


def raw_links(a, ptr, n, mem, torch=None):
    """pfb_assoc_links between guard bytes: (status, first's buffer, count's buffer)"""
    lib = L.load()
    nb = 4 * n + 128
    if mem == L.PFB_MEM_HOST:
        f, k = np.full(nb, GUARD, np.uint8), np.full(nb, GUARD, np.uint8)
        rc = lib.pfb_assoc_links(a._h, C.c_void_p(ptr), n, mem, C.c_void_p(f.ctypes.data + 64), C.c_void_p(k.ctypes.data + 64))
        return rc, f, k
    f = torch.full((nb,), GUARD, dtype=torch.uint8, device="cuda")
    k = torch.full((nb,), GUARD, dtype=torch.uint8, device="cuda")
    rc = lib.pfb_assoc_links(a._h, C.c_void_p(ptr), n, mem, C.c_void_p(f.data_ptr() + 64), C.c_void_p(k.data_ptr() + 64))
    torch.cuda.synchronize()
    return rc, f.cpu().numpy(), k.cpu().numpy()


def test_a_capacity_one_short_and_the_guard_bytes(torch):
    it, c = AC.inputs("tiles_3_plus_1")
    rec, labels, stats, (first, count) = AC.expected("tiles_3_plus_1")
    G, n = len(rec), len(it)
    x = on_device(torch, it)
    with make(c) as a:
        for mem, ptr in ((L.PFB_MEM_HOST, it.ctypes.data), (L.PFB_MEM_DEVICE, x.data_ptr())):
            rc, got, rb, lb = raw_run(a, ptr, n, mem, G, torch)
            assert (rc, got) == (L.PFB_OK, G)
            assert rb[64:64 + 48 * G].tobytes() == rec.tobytes() and lb[64:64 + 4 * n].tobytes() == labels.tobytes()
            assert (rb[:64] == GUARD).all() and (rb[64 + 48 * G:] == GUARD).all()
            assert (lb[:64] == GUARD).all() and (lb[64 + 4 * n:] == GUARD).all()
            rc, fb, kb = raw_links(a, ptr, n, mem, torch)
            assert rc == L.PFB_OK and fb[64:64 + 4 * n].tobytes() == first.tobytes() and kb[64:64 + 4 * n].tobytes() == count.tobytes()
            for b in (fb, kb):
                assert (b[:64] == GUARD).all() and (b[64 + 4 * n:] == GUARD).all()
            got_stats = a.stats
            assert {k: got_stats[k] for k in R.STATS} == stats
            # one record short: the true count, nothing written, the stats of the run before
            lone = AC.inputs("n_1")[0]
            assert raw_run(a, lone.ctypes.data, 1, L.PFB_MEM_HOST, 4)[:2] == (L.PFB_OK, 1) and a.stats["groups"] == 1
            rc, got, rb, lb = raw_run(a, ptr, n, mem, G - 1, torch)
            assert (rc, got) == (L.PFB_ERR_CAPACITY, G)
            assert (rb == GUARD).all() and (lb == GUARD).all() and a.stats["groups"] == 1
            rc, got, rb, lb = raw_run(a, ptr, n, mem, 0, torch)
            assert (rc, got) == (L.PFB_ERR_CAPACITY, G) and (rb == GUARD).all() and (lb == GUARD).all()
        with pytest.raises(L.PfbError) as e:
            a.run(it, capacity=G - 1)
        assert e.value.status == L.PFB_ERR_CAPACITY


def test_a_list_out_of_order_is_refused_with_nothing_written(torch):
    lib = L.load()
    it, c = AC.inputs("tiles_3_plus_1")
    n = len(it)
    top = 1 << 62
    with make(c) as a:
        # one inversion in the first tile and in a later one, at a tile's first item, a start or an end + g at 2^62
        changes = [(1, "start", int(it["start"][0]) - 1 if it["start"][0] else None), (100, "start", int(it["start"][99]) - 1),
                   (2 * AC.TILE, "start", int(it["start"][2 * AC.TILE - 1]) - 1), (2 * AC.TILE + 77, "start", int(it["start"][2 * AC.TILE + 76]) - 1),
                   (n - 1, "start", int(it["start"][n - 2]) - 1), (n - 1, "start", top), (n - 1, "start", (1 << 64) - 1),
                   (n - 1, "start", top - int(it["length"][n - 1]))]
        for at, field, value in changes:
            if value is None:
                continue
            bad = it.copy()
            bad[field][at] = value
            assert not R.acceptable(bad, c)
            x = on_device(torch, bad)
            for mem, ptr in ((L.PFB_MEM_HOST, bad.ctypes.data), (L.PFB_MEM_DEVICE, x.data_ptr())):
                rc, got, rb, lb = raw_run(a, ptr, n, mem, n, torch)
                assert (rc, got) == (L.PFB_ERR_BAD_ARG, 77) and (rb == GUARD).all() and (lb == GUARD).all(), (at, value)
                rc, fb, kb = raw_links(a, ptr, n, mem, torch)
                assert rc == L.PFB_ERR_BAD_ARG and (fb == GUARD).all() and (kb == GUARD).all(), (at, value)
        # the largest end + g that passes
        edge = it.copy()
        edge["start"][n - 1] = top - int(it["length"][n - 1]) - 1
        assert R.acceptable(edge, c) and raw_run(a, edge.ctypes.data, n, L.PFB_MEM_HOST, n)[0] == L.PFB_OK
        check(a, it, AC.expected("tiles_3_plus_1"), what="after the refusals")
        # what is checked before the device
        p = C.c_void_p(it.ctypes.data)
        u = C.c_uint64(77)
        BAD = L.PFB_ERR_BAD_ARG
        lab = np.zeros(n, np.int32)
        lp = C.c_void_p(lab.ctypes.data)
        rec = np.zeros(n, am.GROUP_DTYPE)
        rp = C.c_void_p(rec.ctypes.data)
        assert lib.pfb_assoc_run(a._h, p, n, 2, rp, n, C.byref(u), lp) == BAD
        assert lib.pfb_assoc_run(a._h, p, (1 << 20) + 1, 0, rp, n, C.byref(u), lp) == BAD
        assert lib.pfb_assoc_run(a._h, None, n, 0, rp, n, C.byref(u), lp) == BAD
        assert lib.pfb_assoc_run(a._h, p, n, 0, None, n, C.byref(u), lp) == BAD
        assert lib.pfb_assoc_run(a._h, p, n, 0, rp, n, None, lp) == lib.pfb_assoc_run(a._h, p, n, 0, rp, n, C.byref(u), None) == BAD
        assert lib.pfb_assoc_links(a._h, p, n, 2, lp, lp) == lib.pfb_assoc_links(a._h, None, n, 0, lp, lp) == BAD
        assert lib.pfb_assoc_links(a._h, p, n, 0, None, lp) == lib.pfb_assoc_links(a._h, p, n, 0, lp, None) == BAD
        # misaligned device pointers
        x = torch.zeros(24 * n + 8, dtype=torch.uint8, device="cuda")
        dl = torch.zeros(n + 2, dtype=torch.int32, device="cuda")
        dr = torch.zeros(n * 48 + 16, dtype=torch.uint8, device="cuda")
        xp, dlp, drp = x.data_ptr(), dl.data_ptr(), dr.data_ptr()
        assert lib.pfb_assoc_run(a._h, C.c_void_p(xp + 4), n, 1, C.c_void_p(drp), n, C.byref(u), C.c_void_p(dlp)) == BAD
        assert lib.pfb_assoc_run(a._h, C.c_void_p(xp), n, 1, C.c_void_p(drp + 4), n, C.byref(u), C.c_void_p(dlp)) == BAD
        assert lib.pfb_assoc_run(a._h, C.c_void_p(xp), n, 1, C.c_void_p(drp), n, C.byref(u), C.c_void_p(dlp + 2)) == BAD
        assert lib.pfb_assoc_links(a._h, C.c_void_p(xp + 4), n, 1, C.c_void_p(dlp), C.c_void_p(dlp)) == BAD
        assert lib.pfb_assoc_links(a._h, C.c_void_p(xp), n, 1, C.c_void_p(dlp + 2), C.c_void_p(dlp)) == BAD
        assert lib.pfb_assoc_links(a._h, C.c_void_p(xp), n, 1, C.c_void_p(dlp), C.c_void_p(dlp + 2)) == BAD
        assert u.value == 77 and not lab.any() and not rec.view(np.uint8).any() and not dl.any().item() and not dr.any().item()


def test_host_memory_an_odd_device_pointer_the_same_call_twice_and_a_handle_that_grows(torch):
    it, c = AC.inputs("tiles_3_plus_1")
    want = AC.expected("tiles_3_plus_1")
    room = torch.zeros(24 * len(it) + 8, dtype=torch.uint8, device="cuda")
    assert room.data_ptr() % 256 == 0
    x = room[8:]
    x.copy_(on_device(torch, it).reshape(-1))
    assert x.data_ptr() % 256 == 8
    with make(c) as a:
        check(a, AC.inputs("n_2")[0], AC.expected("n_2"), what="a short list first")
        first = check(a, it, want, what="host, in a scratch that grew")
        again = check(a, x, want, what="device, 8 bytes off")
        assert check(a, x, want, what="twice").tobytes() == again.tobytes() == first.tobytes()
        rec, labels = a.run(x)
        assert labels.is_cuda and labels.dtype == torch.int32 and rec.is_cuda and tuple(rec.shape) == (len(want[0]), 48)
        big, _ = AC.scene(5 * 1024 + 3)            # over the scratch's granule again
        check(a, big, R.run(big, c) + (R.links(big, c),), what="a longer list")
        check(a, AC.inputs("tile")[0], AC.expected("tile"), what="a shorter list after a longer one")
    rec, labels = associate(it, **c.settings())
    assert rec.tobytes() == want[0].tobytes() and labels.tobytes() == want[1].tobytes()
    rec, labels = associate(on_device(torch, it), **c.settings())
    assert rec.tobytes() == want[0].tobytes() and labels.cpu().numpy().tobytes() == want[1].tobytes()


def test_a_stream_switch_between_runs(torch):
    it, c = AC.inputs("tiles_3_plus_1")
    want = AC.expected("tiles_3_plus_1")
    x = on_device(torch, it)
    side = torch.cuda.Stream()
    with make(c) as a:
        check(a, x, want, what="the null stream")
        a.set_stream(side.cuda_stream)
        with torch.cuda.stream(side):
            y = x.clone()
        check(a, y, want, what="a side stream")
        a.sync()
        a.set_stream(0)
        check(a, it, want, what="back on the null stream")


# -- the one large list ------------------------------------------------------------------------------------------------
def test_a_list_of_2_20_items(torch):
    it, c = AC.inputs("big")
    rec, labels, stats, _ = want = AC.expected("big")
    assert len(it) == 1 << 20 and c.K == 8
    # the conditions on the input, before the comparison that uses it: the measured 15 / 10 pattern, every pulse whole
    # but the last, which the cut at 2^20 may leave with a single row
    assert rec["members"][:-1].tolist() == ([AC.CHIRP_ROWS, AC.TONE_ROWS] * (len(rec) // 2 + 1))[:len(rec) - 1]
    assert stats["largest_group"] == AC.CHIRP_ROWS and stats["linked_items"] >= (1 << 20) - 1 and stats["clipped"] > 0
    with make(c) as a:
        check(a, it, want, what="2^20 items")
        check(a, on_device(torch, it), want, what="2^20 items from device memory")
        assert L.load().pfb_assoc_set_tier(a._h, 2) == L.PFB_OK
        check(a, it, want, what="2^20 items through the global tier")


# -- the chain ---------------------------------------------------------------------------------------------------------
def test_the_chain_from_a_channelized_chirp_train_to_one_emitter(torch):
    """a chirp train through the 56-channel bank and the channelized extractor gives several rows a pulse; the
    association gives one group a pulse, and the deinterleaver, fed the groups' first ticks, one emitter at the PRI"""
    M, fs, pri, pw, pulses = 56, 56.0e6, 22400, 2240, 24
    first = 5600
    with PulseTrain(sample_format="cf32", first_pulse=first, pri=pri, pw=pw, f0=0.5e6, lfm_extent_hz=5.0e6, fs=fs,
                    amplitude=0.3, noise_sigma=0.003, seed=3, bit_width=16) as pt:
        iq = pt.generate(pulses * pri)
    with Channelizer(M, sample_format="cf32", fftshift=True) as ch:
        y = ch(iq)
        pdws = extract_pdws(y, fs, 0.0, 0.0, decimation=M, snr_threshold_db=15.0, matlab_quirks=False)
    rate = fs / M                                  # a tick is a frame
    print("%d PDWs for %d pulses" % (len(pdws), pulses))
    assert len(pdws) >= 3 * pulses                 # several rows a pulse
    # the reference first, on the same table
    items, order = R.items_from_pdws(pdws, 0.0, rate)
    rec, sorted_labels, stats = R.run(items, R.Cfg(1, 0, 64))
    frames = np.arange(pulses) * (pri // M) + first // M
    assert len(rec) == pulses and stats["clipped"] == 0
    assert (np.abs(rec["first_tick"].astype(np.int64) - frames) <= 12).all()
    assert (np.abs(rec["end_tick"].astype(np.int64) - (frames + pw // M)) <= 12).all() and (rec["members"] >= 3).all()
    labels = np.full(len(pdws), -1, np.int32)
    labels[order] = sorted_labels
    got, got_labels = associate_pdws(pdws, rate, cell_reach=1, slack_ticks=0, window_items=64, t0=0.0)
    assert got.tobytes() == rec.tobytes() and got_labels.tobytes() == labels.tobytes()
    fused = fuse_pdws(pdws, rate, t0=0.0)
    assert fused.dtype == PDW_DTYPE and len(fused) == pulses
    srt = pdws[order]
    assert (fused["toa"] == srt["toa"][rec["first_item"]]).all() and (fused["bin"] == rec["best_cell"]).all()
    assert (fused["mag"] == srt["mag"][rec["best_item"]]).all() and (fused["freq"] == srt["freq"][rec["best_item"]]).all()
    assert np.allclose(fused["pw"], (rec["end_tick"] - rec["first_tick"]) / rate, rtol=0, atol=1e-12)
    sat = np.zeros(pulses, np.int32)
    np.maximum.at(sat, labels, (pdws["sat"] != 0).astype(np.int32))
    assert (fused["sat"] == sat).all() and (fused["snr"] == srt["snr"][rec["best_item"]]).all()
    # one emitter at the train's PRI in frames
    emitters, who = deinterleave(rec["first_tick"], 100, 2000, 1, min_pulses=8, tolerance=3)
    assert len(emitters) == 1 and emitters[0]["pulses"] >= pulses - 1 and abs(emitters[0]["period"] - pri / M) <= 0.5
