"""The PRI search on the device: profiles and score records against the numpy restatement (fold_ref), byte for byte
but for the two float64 sums, which are held to fold_ref.sums_bound -- over the shape grid, under cuttings of an
order-sensitive stream, at odd pointers and between guard bytes, on NaN, Inf and exact ties, through the host staging
steps, across a stream switch, and along the chain: the train no single-pulse detector finds, its PRI found by folding
and handed to detect_pulse_train."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import fold_cases as FC  # noqa: E402
import fold_ref as R  # noqa: E402
import mf_ref  # noqa: E402
import pd_cases as P  # noqa: E402
from gpu_support import Busy, cuda_torch  # noqa: E402
from sdr_channelizer_amd import (MatchedFilter, PriFold, PulseTrain, cfar_alpha, detect_pulse_train, find_pri,  # noqa: E402
                                 replica_from_pulse_train)
from sdr_channelizer_amd import _lib as L  # noqa: E402
from sdr_channelizer_amd.pri_search import FOUND_DTYPE, SCORE_DTYPE, fold_z  # noqa: E402

SENTINEL = 0x7FC54321   # a NaN no kernel writes


@pytest.fixture(scope="module")
def torch():
    return cuda_torch()


def check(fold, walk, what=""):
    """the handle's records and every profile are the restatement's"""
    got, want, bounds = fold.scores(), walk.records(), walk.bounds()
    assert got.dtype == SCORE_DTYPE and fold.next_index == walk.N
    for k in range(len(want)):
        assert R.same_record(got[k], want[k], bounds[k]), (what, k, got[k], want[k], bounds[k])
        assert R.same_floats(fold.profile(k), walk.F[k]), (what, k)
    return got


# -- the shape grid --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C_", FC.BIN_CELLS)
def test_the_shape_grid(torch, C_):
    periods = FC.grid_periods(C_)
    points = FC.grid_checkpoints(C_, periods)
    assert len(periods) > len(set(periods)) and max(L_ // C_ for L_ in periods) == (65536 if C_ in (1, 64) else 513)
    x = R.spread_stream(points[-1], 7 * C_)
    xd = torch.from_numpy(x).cuda()
    walk = FC.Walk(periods, C_)
    with PriFold(periods, C_) as fold:
        assert fold.plan.total_bins == sum(L_ // C_ for L_ in periods) > 4 * 256     # the prefix table crosses workgroups
        assert fold.last_kernel == "" and fold.plan.kernel.decode() == FC.kernel_name(C_)
        check(fold, walk, "N = 0")
        at = 0
        for i, n in enumerate(points):
            fold.process(xd[at:n] if i % 2 else x[at:n])      # device and host memory in turn; n == at: an empty call
            walk.take(x[at:n])
            at = n
            got = check(fold, walk, f"N = {n}")
            if n > 0:
                assert fold.last_kernel == FC.kernel_name(C_)
        big = int(np.argmax(periods))
        if C_ in (1, 64):
            assert got[big]["num_bins"] == 65536 > got[big]["bins_used"] > 0
        for k in range(len(periods)):
            assert np.array_equal(fold.counts(k), R.counts(at, periods[k], C_))
        dup = [k for k, L_ in enumerate(periods) if L_ == periods[-1 if C_ not in (1, 64) else -2]]
        assert len(dup) == 2 and bytes(got[dup[0]]) == bytes(got[dup[1]])


# -- cuttings --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C_", FC.BIN_CELLS)
def test_cuttings_give_the_same_bits(torch, C_):
    """one call over 40 periods and more (the kernel's batched loads), random cuttings, the same cutting twice"""
    periods = FC.cut_periods(C_)
    x = FC.cut_stream(C_)
    xd = torch.from_numpy(x).cuda()
    walk = FC.Walk(periods, C_)
    walk.take(x)
    rng = np.random.default_rng(C_)
    with PriFold(periods, C_) as fold:
        fold.process(xd)
        whole = check(fold, walk, "one call")
        assert fold.last_kernel == FC.kernel_name(C_)
        cutting = np.sort(rng.integers(0, len(x) + 1, 9))
        for cuts in (cutting, cutting, np.sort(rng.integers(0, len(x) + 1, 40)), [len(x) // 2] * 3):
            fold.reset()
            assert fold.next_index == 0 and not fold.profile(0).any()
            edges = [0] + [int(c) for c in cuts] + [len(x)]
            for a, b in zip(edges[:-1], edges[1:]):
                fold.process(xd[a:b])
                fold.scores()                                   # changes nothing
            got = fold.scores()
            for k in range(len(periods)):
                assert fold.profile(k).tobytes() == walk.F[k].tobytes(), (cuts, k)
                assert bytes(got[k]) == bytes(whole[k])          # the same kernel on the same profile: the sums too


@pytest.mark.parametrize("C_", (8, 16, 32, 64))
def test_both_tiers_give_the_same_bytes(torch, C_):
    """fold_direct and fold_tile (pfb_fold_set_tier, the dev header) on the same inputs: the grid's candidates and the
    cuttings' in one handle, one call over 40 periods of the longest and more, and a random cutting"""
    lib = L.load()
    periods = FC.cut_periods(C_) + FC.grid_periods(C_)[:28]
    x = FC.cut_stream(C_)
    xd = torch.from_numpy(x).cuda()
    walk = FC.Walk(periods, C_)
    walk.take(x)
    cuts = [0] + sorted(int(c) for c in np.random.default_rng(C_).integers(0, len(x) + 1, 7)) + [len(x)]
    seen = {}
    with PriFold(periods, C_) as fold:
        for tier, name in ((1, FC.direct_name(C_)), (2, f"pfb_fold_tile<{C_}>")):
            assert lib.pfb_fold_set_tier(fold._h, tier) == L.PFB_OK
            fold.reset()
            fold.process(xd)
            assert fold.last_kernel == name
            check(fold, walk, name)
            seen[tier] = [fold.profile(k).tobytes() for k in range(len(periods))]
            fold.reset()
            for a, b in zip(cuts[:-1], cuts[1:]):
                fold.process(xd[a:b]) if a % 2 else fold.process(x[a:b])
            assert [fold.profile(k).tobytes() for k in range(len(periods))] == seen[tier]
        assert seen[1] == seen[2]
        assert lib.pfb_fold_set_tier(fold._h, 3) == lib.pfb_fold_set_tier(fold._h, -1) == L.PFB_ERR_BAD_ARG
        assert lib.pfb_fold_set_tier(fold._h, 0) == L.PFB_OK
        fold.reset()
        fold.process(xd)
        assert fold.last_kernel == fold.plan.kernel.decode() == FC.kernel_name(C_)
    with PriFold((2048,), 5) as fold:
        assert lib.pfb_fold_set_tier(fold._h, 2) == L.PFB_ERR_UNSUPPORTED and lib.pfb_fold_set_tier(None, 1) == L.PFB_ERR_BAD_ARG


def test_one_cell_at_a_time(torch):
    """across a bin edge, a period end and the widened last bin; empty calls and scores() in between"""
    for C_, periods in ((4, (11, 8, 9, 4, 7)), (1, (1, 2, 3)), (5, (14, 5, 9)), (64, (127, 64, 191))):
        n = 3 * max(periods) + 2
        x = R.spread_stream(n, 50 + C_)
        xd = torch.from_numpy(x).cuda()
        walk = FC.Walk(periods, C_)
        with PriFold(periods, C_) as fold:
            for i in range(n):
                fold.process(xd[i:i + 1] if i % 3 else x[i:i + 1])
                walk.take(x[i:i + 1])
                fold.process(xd[i:i]) if i % 2 else fold.process(x[i:i])
                if i < 2 * periods[0] + 2 or i == n - 1:
                    check(fold, walk, f"cell {i}")
            check(fold, walk)


# -- pointers --------------------------------------------------------------------------------------------------------
def test_pointers_and_guards(torch):
    lib = L.load()
    C_, periods = 4, (259, 64, 1030, 7)
    x = R.spread_stream(5000, 9)
    walk = FC.Walk(periods, C_)
    walk.take(x)
    want, bounds = walk.records(), walk.bounds()
    for off in (0, 1, 2, 3):                                    # cells off a 256-byte boundary
        buf = torch.zeros(len(x) + 64 + off, dtype=torch.float32, device="cuda")
        base = (-buf.data_ptr() // 4) % 64                      # first cell of buf on a 256-byte boundary
        view = buf[base + off: base + off + len(x)]
        assert view.data_ptr() % 256 == 4 * off
        view.copy_(torch.from_numpy(x))
        with PriFold(periods, C_) as fold:
            fold.process(view)
            check(fold, walk, f"{off} cells off")
    with PriFold(periods, C_) as fold:
        h = fold._h
        fold.process(x)
        NC = len(periods)
        words = NC * 7
        # score records between guard words, device and host
        dev = torch.full((words + 4,), SENTINEL, dtype=torch.int64, device="cuda")
        assert lib.pfb_fold_scores(h, C.c_void_p(dev.data_ptr() + 16), NC, L.PFB_MEM_DEVICE) == L.PFB_OK
        got = dev.cpu().numpy()
        assert (got[:2] == SENTINEL).all() and (got[-2:] == SENTINEL).all()
        rec = got[2:-2].copy().view(SCORE_DTYPE)
        host = np.full(words + 4, SENTINEL, np.int64)
        assert lib.pfb_fold_scores(h, C.c_void_p(host.ctypes.data + 16), NC + 5, L.PFB_MEM_HOST) == L.PFB_OK
        assert (host[:2] == SENTINEL).all() and (host[-2:] == SENTINEL).all()
        assert host[2:-2].tobytes() == rec.tobytes()
        for k in range(NC):
            assert R.same_record(rec[k], want[k], bounds[k])
        # capacity one short: PFB_ERR_CAPACITY, nothing written, nothing changed
        dev.fill_(SENTINEL)
        host[:] = SENTINEL
        assert lib.pfb_fold_scores(h, C.c_void_p(dev.data_ptr() + 16), NC - 1, L.PFB_MEM_DEVICE) == L.PFB_ERR_CAPACITY
        assert lib.pfb_fold_scores(h, C.c_void_p(host.ctypes.data + 16), NC - 1, L.PFB_MEM_HOST) == L.PFB_ERR_CAPACITY
        assert (dev.cpu().numpy() == SENTINEL).all() and (host == SENTINEL).all()
        assert lib.pfb_fold_scores(h, C.c_void_p(dev.data_ptr() + 4), NC, L.PFB_MEM_DEVICE) == L.PFB_ERR_BAD_ARG
        assert lib.pfb_fold_scores(h, C.c_void_p(dev.data_ptr()), NC, 2) == L.PFB_ERR_BAD_ARG
        # a profile between guard words
        for k, L_ in enumerate(periods):
            NB = L_ // C_
            devf = torch.full((NB + 2,), -7.0, dtype=torch.float32, device="cuda")
            assert lib.pfb_fold_profile(h, k, C.c_void_p(devf.data_ptr() + 4), NB, L.PFB_MEM_DEVICE) == L.PFB_OK
            g = devf.cpu().numpy()
            assert g[0] == g[-1] == -7.0 and g[1:-1].tobytes() == walk.F[k].tobytes()
            hostf = np.full(NB + 2, -7.0, np.float32)
            assert lib.pfb_fold_profile(h, k, C.c_void_p(hostf.ctypes.data + 4), NB - 1, L.PFB_MEM_HOST) == L.PFB_ERR_CAPACITY
            assert lib.pfb_fold_profile(h, k, C.c_void_p(devf.data_ptr() + 4), NB - 1, L.PFB_MEM_DEVICE) == L.PFB_ERR_CAPACITY
            assert (hostf == -7.0).all()
            assert lib.pfb_fold_profile(h, k, C.c_void_p(hostf.ctypes.data + 4), NB + 1, L.PFB_MEM_HOST) == L.PFB_OK
            assert hostf[0] == hostf[-1] == -7.0 and hostf[1:-1].tobytes() == walk.F[k].tobytes()
        assert lib.pfb_fold_profile(h, NC, C.c_void_p(hostf.ctypes.data), 1 << 20, L.PFB_MEM_HOST) == L.PFB_ERR_BAD_ARG
        assert lib.pfb_fold_profile(h, 0, C.c_void_p(devf.data_ptr() + 2), 1 << 20, L.PFB_MEM_DEVICE) == L.PFB_ERR_BAD_ARG
        # per-call refusals leave the state alone
        xd = torch.from_numpy(x).cuda()
        BAD = L.PFB_ERR_BAD_ARG
        assert lib.pfb_fold_process(h, C.c_void_p(xd.data_ptr() + 2), 8, L.PFB_MEM_DEVICE) == BAD
        assert lib.pfb_fold_process_async(h, C.c_void_p(xd.data_ptr() + 1), 8) == BAD
        assert lib.pfb_fold_process(h, C.c_void_p(xd.data_ptr()), 8, 2) == lib.pfb_fold_process(h, None, 8, L.PFB_MEM_HOST) == BAD
        assert lib.pfb_fold_process(h, C.c_void_p(xd.data_ptr()), (1 << 62) - 4999, L.PFB_MEM_DEVICE) == BAD
        assert lib.pfb_fold_process(h, None, 0, L.PFB_MEM_DEVICE) == lib.pfb_fold_process_async(h, None, 0) == L.PFB_OK
        check(fold, walk, "after the refusals")
        with pytest.raises(TypeError):
            fold.process(xd.double())
        with pytest.raises(TypeError):
            fold.process(x.astype(np.float64))
        with pytest.raises(IndexError):
            fold.profile(NC)


# -- special values ----------------------------------------------------------------------------------------------------
def test_special_values_and_ties(torch):
    C_, periods = 4, (64, 65, 128, 9)
    nan, inf = np.float32(np.nan), np.float32(np.inf)
    base = R.spread_stream(3 * 64 + 20, 21)
    peak = int(R.score(R.fold(base, 64, C_), len(base), 64, C_)["peak_bin"])   # of the first candidate, undisturbed
    assert peak != 0                                            # or two of the cases below would be one
    for name, edits in (("NaN in the peak bin", {64 + 4 * peak + 1: nan}), ("NaN in the first used bin", {2: nan}),
                        ("NaN elsewhere", {4 * ((peak + 5) % 16): nan}), ("+Inf in the peak bin", {4 * peak: inf}),
                        ("+Inf in the first used bin", {0: inf}), ("-Inf in the peak bin", {4 * peak + 3: -inf}),
                        ("-Inf in the first used bin", {1: -inf}), ("+Inf and -Inf in one bin", {8: inf, 64 + 9: -inf}),
                        ("every bin NaN", {i: nan for i in range(0, 64, 4)}), ("Inf elsewhere", {4 * ((peak + 3) % 16): inf})):
        x = base.copy()
        for i, v in edits.items():
            x[i] = v
        walk = FC.Walk(periods, C_)
        walk.take(x)
        with PriFold(periods, C_) as fold:
            fold.process(torch.from_numpy(x).cuda())
            got = check(fold, walk, name)
        if name == "NaN in the first used bin":
            assert got[0]["peak_bin"] == 0 and np.isnan(got[0]["peak_mean"]) and np.isnan(got[0]["sum_means"])
        if name == "NaN in the peak bin":
            assert got[0]["peak_bin"] != peak and np.isfinite(got[0]["peak_mean"]) and np.isnan(got[0]["sum_means"])
        if name == "+Inf in the peak bin":
            assert got[0]["peak_bin"] == peak and got[0]["peak_mean"] == inf
    # exact ties: equal sums with equal counts go to the lowest bin ...
    x = np.zeros(2 * 64, np.float32)
    x[[4 * 9 + 1, 64 + 4 * 3 + 2, 4 * 12]] = 5.0
    walk = FC.Walk((64,), C_)
    walk.take(x)
    with PriFold((64,), C_) as fold:
        fold.process(x)
        got = check(fold, walk, "equal sums")
        assert got[0]["peak_bin"] == 3 and got[0]["peak_sum"] == 5.0 and got[0]["peak_cells"] == 8
    # ... and so do equal means from different counts: L = 9 has bins of 4 and 5 cells
    for sums, want in (((8.0, 10.0), 0), ((8.0, 10.5), 1), ((10.0, 12.5), 0)):
        x = np.zeros(9, np.float32)
        x[0], x[4] = sums
        walk = FC.Walk((9,), C_)
        walk.take(x)
        with PriFold((9,), C_) as fold:
            fold.process(x)
            got = check(fold, walk, "equal means")
            assert got[0]["peak_bin"] == want and fold_z(got)[0] == 0.0     # two bins: no z


# -- routes ----------------------------------------------------------------------------------------------------------
def test_three_staging_steps_from_host_memory(torch):
    n = 2 * (1 << 24) + 5
    periods, C_ = ((1 << 22), (1 << 22) + 63), 64
    rng = np.random.default_rng(2)
    x = (rng.random(n, dtype=np.float32) + np.float32(0.5)) * np.float32(2.0) ** rng.integers(-12, 13, n).astype(np.float32)
    walk = FC.Walk(periods, C_)
    walk.take(x)
    with PriFold(periods, C_) as fold:
        fold.process(x)
        check(fold, walk, "host")
        fold.reset()
        fold.process(torch.from_numpy(x).cuda())                # the same through three launches of device cells
        check(fold, walk, "device")


def test_async_calls_across_a_stream_switch(torch):
    C_ = 4
    periods = FC.cut_periods(C_)
    x = FC.cut_stream(C_)
    xd = torch.from_numpy(x).cuda()
    walk = FC.Walk(periods, C_)
    walk.take(x)
    cuts = [0, 1000, 1001, 1001, len(x) // 2, len(x)]
    with PriFold(periods, C_) as fold:
        side = torch.cuda.Stream()
        busy = Busy(torch)
        torch.cuda.synchronize()
        busy.queue(torch.cuda.default_stream(), copies=2)       # the host runs ahead of the device
        for k, (a, b) in enumerate(zip(cuts[:-1], cuts[1:])):
            if k == 3:
                fold.set_stream(side.cuda_stream)               # what is queued on the old stream comes first
            fold.process_async(xd[a:b])
        assert fold.next_index == len(x)
        fold.sync()
        check(fold, walk, "async")
        fold.set_stream(0)
        fold.reset()
        check(fold, FC.Walk(periods, C_), "reset")
        fold.process_async(xd)
        check(fold, walk, "after reset")
        with pytest.raises(TypeError):
            fold.process_async(x)


# -- the chain -------------------------------------------------------------------------------------------------------
def test_the_chain_finds_the_pri_of_a_train_under_the_single_pulse_threshold(torch):
    c = P.CHAIN
    kw = dict(P.CHAIN_SYNTH, **{k: c[k] for k in ("fs", "pw", "pri", "amplitude", "bit_width")})
    r = replica_from_pulse_train(**kw)
    n = P.CHAIN_CPIS * P.CHAIN_K * c["pri"]
    with PulseTrain(first_pulse=c["first_pulse"], noise_sigma=c["noise_sigma"], seed=c["seed"], **kw) as pt:
        iq = pt.generate(n)
    host = iq.cpu().numpy()
    assert host.tobytes() == P.chain_stream().tobytes() and r.tobytes() == P.chain_replica().tobytes()
    # the reference first: the float64 chain ranks 2048 first, at the train's first pulse
    ref, _ = FC.chain_reference(FC.chain_powers())
    order = R.ranked(ref, FC.CHAIN_C)
    assert ref[order[0]]["period"] == 2048 and ref[order[0]]["peak_bin"] == 175 and R.z(ref)[order[0]] >= 8
    # the device's records are the restatement's over the device's own compressed stream (float32 arithmetic, one call)
    with MatchedFilter(r, "cf32", 12, "power", True) as mf:
        p = mf.process(iq).cpu().numpy().reshape(-1)
    assert len(p) == FC.CHAIN_CELLS        # a power within TOL of an amplitude on each factor, and its own rounding
    assert np.abs(p - FC.chain_powers()).max() <= 3 * mf_ref.TOL * FC.chain_powers().max()
    want, prof = R.scores(p, FC.CHAIN_PERIODS, FC.CHAIN_C)
    found = find_pri(iq, r, 1984, 2112, extra_periods=FC.CHAIN_EXTRA, normalize=True)
    assert found.dtype == FOUND_DTYPE and len(found) == len(FC.CHAIN_PERIODS)
    rank = R.ranked(want, FC.CHAIN_C)
    for k, i in enumerate(rank):
        assert R.same_record(found[k], want[i], R.sums_bound(prof[i], len(p), FC.CHAIN_PERIODS[i], FC.CHAIN_C)), (k, i)
    assert np.array_equal(found["origin"], found["peak_bin"] * 4) and (np.diff(found["z"]) <= 0).all()
    assert np.allclose(found["z"], R.z(want)[rank], rtol=1e-9, atol=0)
    assert found[0]["period"] == 2048 and found[0]["origin"] // 4 == 175 and found[0]["z"] >= 8
    print("device: z(2048) %.2f, runner-up %d at %.2f" % (found[0]["z"], found[1]["period"], found[1]["z"]))
    # ... and that period, handed on, finds the train: one detection per interval, at a gate inside the peak bin
    got = detect_pulse_train(iq, r, pri=int(found[0]["period"]), num_pulses=P.CHAIN_K, normalize=True, fs=c["fs"],
                             chunk_samples=100000)
    assert [(int(d["cpi"]), int(d["doppler_bin"])) for d in got] == [(k, 0) for k in range(P.CHAIN_CPIS)]
    assert (got["gate"] // 4 == found[0]["origin"] // 4).all() and (got["gate"] == c["first_pulse"]).all()
    _, a_train = P.chain_alphas(cfar_alpha)
    assert (got["peak_power"] > a_train * got["noise"]).all()
    # the same from host memory
    again = find_pri(host, r, 1984, 2112, extra_periods=FC.CHAIN_EXTRA, normalize=True)
    assert again.tobytes() == found.tobytes()
