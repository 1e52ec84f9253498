"""The fractional-PRI search and the regridder on the device: profiles and score records against the numpy restatement
(qfold_ref), byte for byte but for the two float64 sums, which are held to qfold_ref.sums_bound; regridded streams as
bytes -- over the period grid, in whole batches of periods, under cuttings, across step boundaries, from start indices
past 2^32 and 2^56, at odd pointers and between guard words, on NaN, Inf and exact ties, through the host staging
steps, across a stream switch, against pfb_fold_* at whole periods, and along the chain: a train at 2048.37 samples that
the integer search and the integer integrator miss."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import fold_ref  # noqa: E402
import pd_cases as P  # noqa: E402
import qfold_cases as QC  # noqa: E402
import qfold_ref as R  # noqa: E402
from gpu_support import Busy, cuda_torch  # noqa: E402
from sdr_channelizer_amd import (FinePriFold, PriFold, Regrid, cfar_alpha, detect_pulse_train, detect_pulse_train_fine,  # noqa: E402
                                 find_pri, find_pri_fine, refine_pri, regrid)
from sdr_channelizer_amd import _lib as L  # noqa: E402
from sdr_channelizer_amd.pri_fine import QFOUND_DTYPE, QSCORE_DTYPE, grid_q32  # noqa: E402
from sdr_channelizer_amd.pulse_doppler import TRAIN_DET_DTYPE  # noqa: E402

SENTINEL = 0x7FC54321   # a NaN no kernel writes
M32 = (1 << 32) - 1


@pytest.fixture(scope="module")
def torch():
    return cuda_torch()


def pq(Pi, Pf=0):
    return (Pi << 32) | Pf


def q64(periods):
    return np.array(list(periods), np.uint64)


def check(fold, walk, what=""):
    """the handle's records and every profile are the restatement's"""
    got, want, bounds = fold.scores(), walk.records(), walk.bounds()
    assert got.dtype == QSCORE_DTYPE and fold.next_index == walk.N
    for k in range(len(want)):
        assert R.same_record(got[k], want[k], bounds[k]), (what, k, got[k], want[k], bounds[k])
        assert R.same_floats(fold.profile(k), walk.F[k]), (what, k)
    return got


def profiles(fold):
    return [fold.profile(k).tobytes() for k in range(len(fold.periods_q32))]


def tiers(C_):
    """(tier, the kernel's name) of every tier that exists for C"""
    out = [(1, QC.direct_name(C_))]
    return out + [(2, f"pfb_qfold_tile<{C_}>")] if C_ in QC.TILE_DEFAULT else out


def batch_periods(C_):
    """periods per batch of the kernels of C: the direct tier's and the tile tier's"""
    direct = {1: 32, 2: 16, 3: 8, 4: 8}.get(C_)
    return [P_ for P_ in (direct, 64 // C_ if C_ in QC.TILE_DEFAULT else None) if P_]


# -- the period grid -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C_", QC.BIN_CELLS)
def test_the_period_grid(torch, C_):
    """Pf in {0, 1, 2^31, 2^32 - 1}; Pi = C (one bin), k C and k C + C - 1; 1, 63, 64, 65 and 513 bins; records and every
    profile after each of N = 0, 1, C, Pi - 1, Pi, Pi + 1, start(2) - 1, start(2), start(2) + 1 and 5 periods + 3 of every
    period of the grid, device and host memory in turn"""
    periods = QC.grid_periods(C_)
    points = QC.grid_checkpoints(C_, periods)
    assert all(n in points for q in periods for n in QC.checkpoints(C_, q))
    assert len(periods) > len(set(periods)) and {(q >> 32) // C_ for q in periods} == set(QC.GRID_BINS)
    assert {q & M32 for q in periods} == set(QC.FRACTIONS) and pq(C_) in periods
    x = R.spread_stream(points[-1], 7 * C_)
    xd = torch.from_numpy(x).cuda()
    walk = R.Walk(periods, C_)
    with FinePriFold(q64(periods), C_) as fold:
        assert fold.plan.total_bins == sum((q >> 32) // C_ for q in periods) > 4 * 256   # the prefix table crosses workgroups
        assert fold.last_kernel == "" and fold.plan.kernel.decode() == QC.kernel_name(C_)
        check(fold, walk, "N = 0")
        at = 0
        for i, n in enumerate(points):
            fold.process(xd[at:n] if i % 2 else x[at:n])      # n == at: an empty call
            walk.take(x[at:n])
            at = n
            got = check(fold, walk, f"N = {n}")
            if n > 0:
                assert fold.last_kernel == QC.kernel_name(C_)
        for k in range(len(periods)):
            assert np.array_equal(fold.counts(k), R.counts(at, periods[k], C_))
        dup = [k for k, q in enumerate(periods) if q == periods[-1]]
        assert len(dup) == 2 and bytes(got[dup[0]]) == bytes(got[dup[1]])
        fold.reset()
        check(fold, R.Walk(periods, C_), "reset")


# -- batches, cuttings, tiers ----------------------------------------------------------------------------------------
def cut_periods(C_):
    """short periods, so that one call spans many of them: 2, 63, 65 and 257 bins, the last bin C (and C + 1 in a long
    period) or 2 C - 1 (and 2 C) cells, three fractions"""
    return [pq(NB * C_ + rem, Pf) for NB in (2, 63, 65, 257) for rem in sorted({0, C_ - 1}) for Pf in (1 << 31, M32, 0x5eb851eb)]


@pytest.mark.parametrize("C_", QC.BIN_CELLS)
def test_batches_cuttings_and_tiers(torch, C_):
    """every tier on one handle, each named by last_kernel: whole batches of P periods plus 1 and P - 1 leftover periods
    (at Pf = 2^31 long and short periods alternate, so both variants of the widened last bin fall inside a batch), one
    call over 40 periods, random cuttings and the same cutting twice; all the same bytes"""
    lib = L.load()
    periods = cut_periods(C_)
    longest = max(periods)
    x = R.spread_stream(R.start(40, longest) + 7, 100 + C_)
    xd = torch.from_numpy(x).cuda()
    walk = R.Walk(periods, C_)
    walk.take(x)
    rng = np.random.default_rng(C_)
    cutting = np.sort(rng.integers(0, len(x) + 1, 9))
    lengths = sorted({R.start(whole + 1, longest) + 1 for P_ in batch_periods(C_) for whole in (2 * P_ + 1, 3 * P_ - 1)})
    short = {}
    for n in lengths:                                           # first period, `whole` whole periods, one cell of the last
        w = R.Walk(periods, C_)
        w.take(x[:n])
        short[n] = w
    seen = {}
    with FinePriFold(q64(periods), C_) as fold:
        for tier, name in tiers(C_):
            assert lib.pfb_qfold_set_tier(fold._h, tier, 0) == L.PFB_OK
            for n in lengths:
                fold.reset()
                fold.process(xd[:n])
                assert fold.last_kernel == name
                check(fold, short[n], f"{name}, {n} cells")
            fold.reset()
            fold.process(xd)
            whole = check(fold, walk, name)
            seen[tier] = profiles(fold)
            for cuts in (cutting, cutting, np.sort(rng.integers(0, len(x) + 1, 40)), [len(x) // 2] * 3):
                fold.reset()
                assert fold.next_index == 0 and not fold.profile(0).any()
                edges = [0] + [int(c) for c in cuts] + [len(x)]
                for a, b in zip(edges[:-1], edges[1:]):
                    fold.process(xd[a:b]) if a % 2 else fold.process(x[a:b])
                    fold.scores()                               # changes nothing
                got = fold.scores()
                assert profiles(fold) == seen[tier], (name, cuts)
                for k in range(len(periods)):
                    assert bytes(got[k]) == bytes(whole[k])      # the same kernel on the same profile: the sums too
        assert all(v == seen[1] for v in seen.values())
        assert lib.pfb_qfold_set_tier(fold._h, 3, 0) == lib.pfb_qfold_set_tier(fold._h, -1, 0) == L.PFB_ERR_BAD_ARG
        assert lib.pfb_qfold_set_tier(fold._h, 0, (1 << 24) + 1) == L.PFB_ERR_BAD_ARG
        if C_ not in QC.TILE_DEFAULT:
            assert lib.pfb_qfold_set_tier(fold._h, 2, 0) == L.PFB_ERR_UNSUPPORTED
        assert lib.pfb_qfold_set_tier(fold._h, 0, 0) == L.PFB_OK
        fold.reset()
        fold.process(xd)
        assert fold.last_kernel == fold.plan.kernel.decode() == QC.kernel_name(C_) and profiles(fold) == seen[1]


def test_one_cell_at_a_time(torch):
    """across a bin edge, a short-period end, a long-period end and the widened last bin; empty calls and scores() in
    between"""
    for C_, periods in ((4, (pq(11, 1 << 31), pq(8, M32), pq(9, 1), pq(4, 1 << 31), pq(7))), (1, (pq(1, 1 << 31), pq(2, 1), pq(3, M32))),
                        (5, (pq(14, 1 << 31), pq(5, 1 << 30), pq(9, M32))), (64, (pq(127, 1 << 31), pq(64, M32), pq(191, 1)))):
        n = R.start(3, max(periods)) + 2
        x = R.spread_stream(n, 50 + C_)
        xd = torch.from_numpy(x).cuda()
        walk = R.Walk(periods, C_)
        with FinePriFold(q64(periods), C_) as fold:
            for i in range(n):
                fold.process(xd[i:i + 1] if i % 3 else x[i:i + 1])
                walk.take(x[i:i + 1])
                fold.process(xd[i:i]) if i % 2 else fold.process(x[i:i])
                if i < R.start(2, periods[0]) + 2 or i == n - 1:
                    check(fold, walk, f"cell {i}")
            check(fold, walk)


@pytest.mark.parametrize("C_", (4, 5, 16))
def test_steps_of_4096_cells(torch, C_):
    """the step boundary (pfb_qfold_set_tier's step_cells): periods shorter and longer than a step, one call over three
    steps and more, and cuts on, one before and one after a boundary; every tier"""
    lib = L.load()
    periods = [pq(NB * C_ + rem, Pf) for NB, rem in ((3, 0), (65, C_ - 1), (5000 // C_, 0), (9000 // C_, C_ - 1))
               for Pf in (1 << 31, M32)]
    x = R.spread_stream(3 * 4096 + 777, 60 + C_)
    xd = torch.from_numpy(x).cuda()
    walk = R.Walk(periods, C_)
    walk.take(x)
    with FinePriFold(q64(periods), C_) as fold:
        for tier, name in tiers(C_):
            assert lib.pfb_qfold_set_tier(fold._h, tier, 4096) == L.PFB_OK
            for cuts in ((), (4095, 8193), (4096, 8192), (4097, 8191, 12288), (1, 4096, 4096, 12289)):
                fold.reset()
                edges = [0] + list(cuts) + [len(x)]
                for k, (a, b) in enumerate(zip(edges[:-1], edges[1:])):
                    fold.process(xd[a:b]) if k % 2 else fold.process(x[a:b])
                check(fold, walk, f"{name}, cuts {cuts}")
                assert fold.last_kernel == name


# -- the start index -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C_", (4, 8))
def test_set_index(torch, C_):
    """to 2^32 - 3, 2^56 + 5, 2^62 - 2^20 and into the middle of a period, where the used bins are not the leading
    ones; reset after each"""
    lib = L.load()
    periods = [pq(2048, 0x5eb851eb), pq(65 * C_ + C_ - 1, M32), pq(63 * C_, 1 << 31), pq(C_, 1), pq(513 * C_ + 1)]
    mid = R.start(3, periods[0]) + 5 * C_ + 1
    x = R.spread_stream(3000, 70 + C_)
    xd = torch.from_numpy(x).cuda()
    with FinePriFold(q64(periods), C_) as fold:
        for tier, name in tiers(C_):
            assert lib.pfb_qfold_set_tier(fold._h, tier, 0) == L.PFB_OK
            for N0 in ((1 << 32) - 3, (1 << 56) + 5, (1 << 62) - (1 << 20), mid):
                fold.process(xd[:100])                          # something to clear
                fold.set_index(N0)
                walk = R.Walk(periods, C_, N0)
                check(fold, walk, f"at {N0}")
                for a, b in ((0, C_), (C_, 1111), (1111, 1111), (1111, 3000)):
                    fold.process(xd[a:b]) if a else fold.process(x[a:b])
                    walk.take(x[a:b])
                    got = check(fold, walk, f"{name} from {N0}, {b} cells")
                    if N0 == mid and b == C_:
                        assert got[0]["bins_used"] == 2 and got[0]["peak_bin"] in (5, 6) and got[0]["cells"] == C_
                for k in range(len(periods)):
                    assert np.array_equal(fold.counts(k), R.counts(N0 + 3000, periods[k], C_, N0))
                fold.reset()
                check(fold, R.Walk(periods, C_), "reset")
        assert lib.pfb_qfold_set_index(fold._h, (1 << 62) + 1) == L.PFB_ERR_BAD_ARG
        fold.set_index(1 << 62)
        assert lib.pfb_qfold_process(fold._h, C.c_void_p(xd.data_ptr()), 1, L.PFB_MEM_DEVICE) == L.PFB_ERR_BAD_ARG
        assert fold.next_index == 1 << 62


# -- whole periods: pfb_fold_* on the same cells ------------------------------------------------------------------------
@pytest.mark.parametrize("C_", QC.BIN_CELLS)
def test_whole_periods_give_the_integer_folder_s_bytes(torch, C_):
    ints = sorted({NB * C_ + rem for NB in (1, 2, 63, 65, 257) for rem in (0, min(1, C_ - 1), C_ - 1)})
    x = fold_ref.spread_stream(40 * max(ints) + 7, 30 + C_)
    xd = torch.from_numpy(x).cuda()
    with PriFold(ints, C_) as old, FinePriFold(ints, C_) as new:
        assert new.periods_q32.tolist() == [L_ << 32 for L_ in ints]
        for a, b in ((0, 1), (1, 3 * max(ints) + 2), (3 * max(ints) + 2, len(x))):
            old.process(xd[a:b])
            new.process(xd[a:b])
            want, got = old.scores(), new.scores()
            for k in range(len(ints)):
                assert new.profile(k).tobytes() == old.profile(k).tobytes(), (k, b)
                for name in R.SHARED:
                    assert got[k][name].tobytes() == want[k][name].astype(got[k][name].dtype).tobytes(), (k, b, name)
                bound = fold_ref.sums_bound(old.profile(k), b, ints[k], C_)
                assert abs(got[k]["sum_means"] - want[k]["sum_means"]) <= 2 * bound[0]
                assert abs(got[k]["sum_sq_means"] - want[k]["sum_sq_means"]) <= 2 * bound[1]


# -- pointers --------------------------------------------------------------------------------------------------------
def test_pointers_and_guards(torch):
    lib = L.load()
    C_, periods = 4, (pq(259, 1 << 31), pq(64, M32), pq(1030, 1), pq(7, 0x5eb851eb))
    x = R.spread_stream(5000, 9)
    walk = R.Walk(periods, C_)
    walk.take(x)
    want, bounds = walk.records(), walk.bounds()
    for off in (0, 1, 2, 3):                                    # cells off a 256-byte boundary
        buf = torch.zeros(len(x) + 64 + off, dtype=torch.float32, device="cuda")
        base = (-buf.data_ptr() // 4) % 64
        view = buf[base + off: base + off + len(x)]
        assert view.data_ptr() % 256 == 4 * off
        view.copy_(torch.from_numpy(x))
        with FinePriFold(q64(periods), C_) as fold:
            fold.process(view)
            check(fold, walk, f"{off} cells off")
    with FinePriFold(q64(periods), C_) as fold:
        h = fold._h
        fold.process(x)
        NC = len(periods)
        words = NC * 8
        dev = torch.full((words + 4,), SENTINEL, dtype=torch.int64, device="cuda")
        assert lib.pfb_qfold_scores(h, C.c_void_p(dev.data_ptr() + 16), NC, L.PFB_MEM_DEVICE) == L.PFB_OK
        got = dev.cpu().numpy()
        assert (got[:2] == SENTINEL).all() and (got[-2:] == SENTINEL).all()
        rec = got[2:-2].copy().view(QSCORE_DTYPE)
        host = np.full(words + 4, SENTINEL, np.int64)
        assert lib.pfb_qfold_scores(h, C.c_void_p(host.ctypes.data + 16), NC + 5, L.PFB_MEM_HOST) == L.PFB_OK
        assert (host[:2] == SENTINEL).all() and (host[-2:] == SENTINEL).all()
        assert host[2:-2].tobytes() == rec.tobytes()
        for k in range(NC):
            assert R.same_record(rec[k], want[k], bounds[k])
        # capacity one short: PFB_ERR_CAPACITY, nothing written, nothing changed
        dev.fill_(SENTINEL)
        host[:] = SENTINEL
        assert lib.pfb_qfold_scores(h, C.c_void_p(dev.data_ptr() + 16), NC - 1, L.PFB_MEM_DEVICE) == L.PFB_ERR_CAPACITY
        assert lib.pfb_qfold_scores(h, C.c_void_p(host.ctypes.data + 16), NC - 1, L.PFB_MEM_HOST) == L.PFB_ERR_CAPACITY
        assert (dev.cpu().numpy() == SENTINEL).all() and (host == SENTINEL).all()
        assert lib.pfb_qfold_scores(h, C.c_void_p(dev.data_ptr() + 4), NC, L.PFB_MEM_DEVICE) == L.PFB_ERR_BAD_ARG
        assert lib.pfb_qfold_scores(h, C.c_void_p(dev.data_ptr()), NC, 2) == L.PFB_ERR_BAD_ARG
        for k, q in enumerate(periods):                         # a profile between guard words
            NB = (q >> 32) // C_
            devf = torch.full((NB + 2,), -7.0, dtype=torch.float32, device="cuda")
            assert lib.pfb_qfold_profile(h, k, C.c_void_p(devf.data_ptr() + 4), NB, L.PFB_MEM_DEVICE) == L.PFB_OK
            g = devf.cpu().numpy()
            assert g[0] == g[-1] == -7.0 and g[1:-1].tobytes() == walk.F[k].tobytes()
            hostf = np.full(NB + 2, -7.0, np.float32)
            assert lib.pfb_qfold_profile(h, k, C.c_void_p(hostf.ctypes.data + 4), NB - 1, L.PFB_MEM_HOST) == L.PFB_ERR_CAPACITY
            assert lib.pfb_qfold_profile(h, k, C.c_void_p(devf.data_ptr() + 4), NB - 1, L.PFB_MEM_DEVICE) == L.PFB_ERR_CAPACITY
            assert (hostf == -7.0).all()
            assert lib.pfb_qfold_profile(h, k, C.c_void_p(hostf.ctypes.data + 4), NB + 1, L.PFB_MEM_HOST) == L.PFB_OK
            assert hostf[0] == hostf[-1] == -7.0 and hostf[1:-1].tobytes() == walk.F[k].tobytes()
        assert lib.pfb_qfold_profile(h, NC, C.c_void_p(hostf.ctypes.data), 1 << 20, L.PFB_MEM_HOST) == L.PFB_ERR_BAD_ARG
        assert lib.pfb_qfold_profile(h, 0, C.c_void_p(devf.data_ptr() + 2), 1 << 20, L.PFB_MEM_DEVICE) == L.PFB_ERR_BAD_ARG
        xd = torch.from_numpy(x).cuda()                         # per-call refusals leave the state alone
        BAD = L.PFB_ERR_BAD_ARG
        assert lib.pfb_qfold_process(h, C.c_void_p(xd.data_ptr() + 2), 8, L.PFB_MEM_DEVICE) == BAD
        assert lib.pfb_qfold_process_async(h, C.c_void_p(xd.data_ptr() + 1), 8) == BAD
        assert lib.pfb_qfold_process(h, C.c_void_p(xd.data_ptr()), 8, 2) == lib.pfb_qfold_process(h, None, 8, L.PFB_MEM_HOST) == BAD
        assert lib.pfb_qfold_process(h, C.c_void_p(xd.data_ptr()), (1 << 62) - 4999, L.PFB_MEM_DEVICE) == BAD
        assert lib.pfb_qfold_process(h, None, 0, L.PFB_MEM_DEVICE) == lib.pfb_qfold_process_async(h, None, 0) == L.PFB_OK
        check(fold, walk, "after the refusals")
        with pytest.raises(TypeError):
            fold.process(xd.double())
        with pytest.raises(IndexError):
            fold.profile(NC)


# -- special values ----------------------------------------------------------------------------------------------------
def test_special_values_and_ties(torch):
    C_ = 4
    periods = (pq(64, 1 << 31), pq(65, M32), pq(128, 1), pq(9, 1 << 31))
    q = periods[0]
    nan, inf = np.float32(np.nan), np.float32(np.inf)
    N0 = R.start(1, q) + 9                                      # bins 0 and 1 of the first candidate see nothing before period 2
    n = R.start(2, q) - N0 - 3                                  # ... and this stream ends before it: the first used bin is bin 2
    base = R.spread_stream(n, 21)
    cell = lambda j, u=0: R.start(1, q) + 4 * j + u - N0        # noqa: E731  stream position of cell u of bin j, period 1
    rec0 = R.score(R.fold(base, q, C_, N0), N0 + n, q, C_, N0)
    peak = int(rec0["peak_bin"])
    assert rec0["bins_used"] == 14 and 4 < peak < 15 and R.counts(N0 + n, q, C_, N0)[:3].tolist() == [0, 0, 3]
    for name, edits in (("NaN in the peak bin", {cell(peak, 1): nan}), ("NaN in the first used bin", {cell(2, 2): nan}),
                        ("NaN elsewhere", {cell(3): nan}), ("+Inf in the peak bin", {cell(peak): inf}),
                        ("+Inf in the first used bin", {cell(2, 1): inf}), ("-Inf in the peak bin", {cell(peak, 3): -inf}),
                        ("-Inf in the first used bin", {cell(2, 3): -inf}), ("+Inf and -Inf in one bin", {cell(4): inf, cell(4, 1): -inf}),
                        ("every bin NaN", {cell(j, 3 if j < 15 else 0): nan for j in range(2, 16)}),
                        ("Inf elsewhere", {cell(3, 2): inf})):
        x = base.copy()
        for i, v in edits.items():
            x[i] = v
        walk = R.Walk(periods, C_, N0)
        walk.take(x)
        with FinePriFold(q64(periods), C_) as fold:
            fold.set_index(N0)
            fold.process(torch.from_numpy(x).cuda())
            got = check(fold, walk, name)
        if name == "NaN in the first used bin":
            assert got[0]["peak_bin"] == 2 and np.isnan(got[0]["peak_mean"]) and np.isnan(got[0]["sum_means"])
        if name == "NaN in the peak bin":
            assert got[0]["peak_bin"] != peak and np.isfinite(got[0]["peak_mean"]) and np.isnan(got[0]["sum_means"])
        if name == "+Inf in the peak bin":
            assert got[0]["peak_bin"] == peak and got[0]["peak_mean"] == inf
        if name == "every bin NaN":
            assert got[0]["peak_bin"] == 2
    # exact ties: equal sums with equal counts go to the lowest bin ...
    q = pq(64, 1 << 31)                                         # periods of 65 and 64 cells: the last bin has 5 + 4 = 9 cells
    x = np.zeros(R.start(2, q), np.float32)
    x[[4 * 9 + 1, 65 + 4 * 3 + 2, 4 * 12]] = 5.0
    walk = R.Walk((q,), C_)
    walk.take(x)
    with FinePriFold(q64((q,)), C_) as fold:
        fold.process(x)
        got = check(fold, walk, "equal sums")
        assert got[0]["peak_bin"] == 3 and got[0]["peak_sum"] == 5.0 and got[0]["peak_cells"] == 8
    # ... and so do equal means from different counts: bins of 8 and of 9 cells
    for sums, want in (((8.0, 9.0), 0), ((8.0, 9.5), 15), ((16.0, 18.0), 0)):
        x = np.zeros(R.start(2, q), np.float32)
        x[0], x[63] = sums
        walk = R.Walk((q,), C_)
        walk.take(x)
        with FinePriFold(q64((q,)), C_) as fold:
            fold.process(x)
            got = check(fold, walk, "equal means")
            assert got[0]["peak_bin"] == want and got[0]["peak_cells"] == (9 if want else 8)


# -- routes ----------------------------------------------------------------------------------------------------------
def test_three_staging_steps_from_host_memory(torch):
    lib = L.load()
    step = 1 << 18
    n = 2 * step + 5
    periods, C_ = (pq(1 << 16, 1 << 31), pq((1 << 16) + 63, M32), pq(300, 1)), 64
    x = R.spread_stream(n, 2)
    walk = R.Walk(periods, C_)
    walk.take(x)
    with FinePriFold(q64(periods), C_) as fold:
        assert lib.pfb_qfold_set_tier(fold._h, 0, step) == L.PFB_OK
        fold.process(x)
        check(fold, walk, "host")
        fold.reset()
        fold.process(torch.from_numpy(x).cuda())                # the same through three launches of device cells
        check(fold, walk, "device")


def test_async_calls_across_a_stream_switch(torch):
    C_ = 4
    periods = cut_periods(C_)
    x = R.spread_stream(R.start(40, max(periods)) + 7, 104)
    xd = torch.from_numpy(x).cuda()
    walk = R.Walk(periods, C_)
    walk.take(x)
    cuts = [0, 1000, 1001, 1001, len(x) // 2, len(x)]
    with FinePriFold(q64(periods), C_) as fold:
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
        check(fold, R.Walk(periods, C_), "reset")
        fold.process_async(xd)
        check(fold, walk, "after reset")
        with pytest.raises(TypeError):
            fold.process_async(x)


# -- the regridder ---------------------------------------------------------------------------------------------------
def regrid_input(n, dtype, seed):
    rng = np.random.default_rng(seed)
    words = rng.integers(0, 1 << 32, n * (2 if dtype == np.complex64 else 1), dtype=np.uint64).astype(np.uint32)
    return words.view(dtype)                                    # any bit pattern, NaNs included: the copy is bit for bit


@pytest.mark.parametrize("dtype", (np.complex64, np.float32))
@pytest.mark.parametrize("R_", (1, 2, 255, 256, 257, 300))
def test_regrid(torch, R_, dtype):
    """rows of R of a period of 300.37 samples (R = 300 = Pi), origins on and off 16 bytes: one call, cuttings where a
    row straddles two and three calls and a call lies wholly between two rows, host and device memory, bytes"""
    q = R.q32("300.37")
    n = R.start(12, q) + 50
    x = regrid_input(n, dtype, R_)
    xd = torch.from_numpy(x).cuda()
    for origin in (0, 1, 2, 3, 77):
        t0, want = R.regrid(x, 0, q, R_, origin)
        assert t0 == 0 and len(want) >= 11 * R_
        row3 = origin + R.start(3, q)
        cuts = [0, row3 + 1, row3 + R_ // 2 + 1, row3 + R_, R.start(4, q) + origin, R.start(7, q) + origin + R_ // 3, n]
        with Regrid(np.uint64(q), R_, origin, dtype) as rg:
            assert rg.outputs_for(n) == len(want) and rg.outputs_for(origin) == 0
            got = rg.process(xd)
            assert got.is_cuda and got.cpu().numpy().tobytes() == want.tobytes() and rg.next_index == n
            assert rg.outputs_for(5 * n) == R.regrid_before(6 * n, q, R_, origin) - len(want)
            rg.reset()
            assert rg.process(x).tobytes() == want.tobytes()
            for route in ("device", "host"):
                rg.reset()
                parts = []
                for a, b in zip(cuts[:-1], cuts[1:]):
                    t, w = R.regrid(x[a:b], a, q, R_, origin)
                    assert rg.outputs_for(b - a) == len(w)
                    out = rg.process(xd[a:b]) if route == "device" else rg.process(x[a:b])
                    out = out.cpu().numpy() if route == "device" else out
                    assert out.tobytes() == w.tobytes(), (route, a, b)
                    parts.append(out)
                if R_ < 300:                                    # the rows leave a gap: the call [row 3's end, row 4) gives nothing
                    assert len(parts[3]) == 0
                assert 0 < len(parts[1]) < R_ or R_ <= 2        # row 3 in three calls
                assert np.concatenate(parts).tobytes() == want.tobytes()
    assert regrid(x, np.uint64(q), R_, 5).tobytes() == R.regrid(x, 0, q, R_, 5)[1].tobytes()


def test_regrid_capacity_async_and_large_origins(torch):
    lib = L.load()
    q, R_ = R.q32("300.37"), 256
    x = regrid_input(4000, np.complex64, 5)
    xd = torch.from_numpy(x).cuda()
    _, want = R.regrid(x, 0, q, R_, 3)
    with Regrid(np.uint64(q), R_, 3) as rg:
        h = rg._h
        # a capacity one short: the count needed, nothing written, no state changed -- host, device and async
        cnt = C.c_uint64(0)
        host = np.full(len(want) + 2, SENTINEL + 0j, np.complex64)
        assert lib.pfb_regrid_process(h, C.c_void_p(x.ctypes.data), len(x), C.c_void_p(host.ctypes.data + 8), len(want) - 1,
                                      C.byref(cnt), L.PFB_MEM_HOST) == L.PFB_ERR_CAPACITY
        assert cnt.value == len(want) and rg.next_index == 0 and (host == SENTINEL + 0j).all()
        dev = torch.full((len(want) + 2,), 7.0 + 0j, dtype=torch.complex64, device="cuda")
        dcnt = torch.full((1,), -5, dtype=torch.int64, device="cuda")
        assert lib.pfb_regrid_process(h, C.c_void_p(xd.data_ptr()), len(x), C.c_void_p(dev.data_ptr() + 8), len(want) - 1,
                                      C.byref(cnt), L.PFB_MEM_DEVICE) == L.PFB_ERR_CAPACITY
        assert lib.pfb_regrid_process_async(h, C.c_void_p(xd.data_ptr()), len(x), C.c_void_p(dev.data_ptr() + 8), len(want) - 1,
                                            C.c_void_p(dcnt.data_ptr())) == L.PFB_ERR_CAPACITY
        torch.cuda.synchronize()
        assert rg.next_index == 0 and (dev.cpu().numpy() == 7.0).all() and int(dcnt.item()) == -5
        # the Python handle grows its buffer and calls again
        assert rg.process(x, capacity=1).tobytes() == want.tobytes() and rg.next_index == len(x)
        # between guard elements, the exact capacity, the async route behind a busy stream, in three calls
        rg.reset()
        busy = Busy(torch)
        torch.cuda.synchronize()
        busy.queue(torch.cuda.default_stream(), copies=2)
        at = 1
        counts = torch.full((3,), -5, dtype=torch.int64, device="cuda")
        for k, (a, b) in enumerate(((0, 1000), (1000, 1000), (1000, 4000))):
            need = rg.outputs_for(b - a)
            rg.process_async(xd[a:b], dev[at:at + need], counts[k:k + 1])
            at += need
        assert rg.next_index == len(x)
        rg.sync()
        g = dev.cpu().numpy()
        assert at == len(want) + 1 and g[0] == g[-1] == 7.0 and g[1:-1].tobytes() == want.tobytes()
        assert counts.cpu().tolist() == [rg_count for rg_count in (R.regrid_before(1000, q, R_, 3), 0,
                                                                  len(want) - R.regrid_before(1000, q, R_, 3))]
        # refusals
        BAD = L.PFB_ERR_BAD_ARG
        assert lib.pfb_regrid_process(h, C.c_void_p(xd.data_ptr() + 4), 8, C.c_void_p(dev.data_ptr()), 8, C.byref(cnt), L.PFB_MEM_DEVICE) == BAD
        assert lib.pfb_regrid_process(h, C.c_void_p(xd.data_ptr()), 8, C.c_void_p(dev.data_ptr()), 8, C.byref(cnt), 2) == BAD
        assert lib.pfb_regrid_process(h, C.c_void_p(xd.data_ptr()), 8, C.c_void_p(dev.data_ptr()), 8, None, L.PFB_MEM_DEVICE) == BAD
        assert lib.pfb_regrid_set_index(h, (1 << 62) + 1) == BAD and rg.next_index == len(x)
        with pytest.raises(TypeError):
            rg.process(np.zeros(8, np.complex128))
    # an origin at 2^40 (and off 16 bytes), float32: the stream enters at an index before it
    for origin in (1 << 40, (1 << 40) + 3):
        s = origin - 123
        xf = regrid_input(3000, np.float32, 6)
        t0, want = R.regrid(xf, s, q, 255, origin)
        with Regrid(np.uint64(q), 255, origin, np.float32) as rg:
            rg.set_index(s)
            a = rg.process(torch.from_numpy(xf[:1500]).cuda()).cpu().numpy()
            b = rg.process(xf[1500:])
            assert t0 == 0 and np.concatenate([a, b]).tobytes() == want.tobytes() and rg.next_index == s + 3000
    # rows far from the origin: row 2^33 and on, Al and the start need 128 bits on the host
    k0 = (1 << 33) + 5
    s = R.start(k0, q) - 7
    t0, want = R.regrid(xf, s, q, 257, 0)
    with Regrid(np.uint64(q), 257, 0, np.float32) as rg:
        rg.set_index(s)
        assert t0 == k0 * 257 and rg.process(torch.from_numpy(xf).cuda()).cpu().numpy().tobytes() == want.tobytes()


# -- the chain -------------------------------------------------------------------------------------------------------
def test_the_chain_finds_a_train_at_a_fractional_pri(torch):
    """the CPU module's scene, from host and from device memory: the restatement's answer first, then the device's"""
    c = P.CHAIN
    host = QC.chain_stream()
    iq = torch.from_numpy(np.array(host)).cuda()
    r = P.chain_replica()
    a_single, a_train = QC.chain_alphas(cfar_alpha)
    # the references: no integer period over 6, the true period at 8 or more in the train's bin; nothing at pri 2048,
    # one detection per interval at the gate and row after the regrid
    p = QC.chain_powers()
    zi = fold_ref.z(fold_ref.scores(p, list(range(2040, 2057)), QC.CHAIN_FOLD_C)[0])
    zq, rec = QC.scene_z(p, [QC.CHAIN_Q])
    assert zi.max() <= 6 and zq[0] >= 8 and rec[0]["peak_bin"] == QC.CHAIN_FIRST // QC.CHAIN_FOLD_C
    want = [(k, QC.CHAIN_FIRST, QC.CHAIN_BIN) for k in range(QC.CHAIN_CPIS)]
    y = QC.chain_compressed()
    assert [f for f in QC.chain_detect(y, 2048, a_train)[0] if f[0] < QC.CHAIN_CPIS] == []
    assert QC.chain_detect(QC.chain_regridded(y), QC.CHAIN_ROW, a_train)[0] == want
    # the integer search ranks nothing
    found = find_pri(iq, r, 2040, 2056, normalize=True)
    assert found["z"].max() <= 6
    # the fine search puts the true period first within one step, at the train's bin: the restatement's answer first
    step, lo, hi = QC.CHAIN_STEP, 2048.30, 2048.44
    grid = [int(v) for v in grid_q32(lo, hi, step)]
    zg, recg = QC.scene_z(p, grid)
    best = int(np.argmax(zg))
    assert len(grid) == 8 and abs(grid[best] / 2.0 ** 32 - float(QC.CHAIN_PERIOD)) <= step and zg[best] >= 8
    assert recg[best]["peak_bin"] == QC.CHAIN_FIRST // QC.CHAIN_FOLD_C
    for src in (iq, host):
        fine = find_pri_fine(src, r, lo, hi, step, normalize=True)
        assert fine.dtype == QFOUND_DTYPE and len(fine) == len(grid) and (np.diff(fine["z"]) <= 0).all()
        assert abs(fine[0]["period"] - float(QC.CHAIN_PERIOD)) <= step and fine[0]["z"] >= 8
        assert fine[0]["period_q32"] == grid[best] and fine[0]["origin"] // 4 == QC.CHAIN_FIRST // 4
        assert sorted(fine["period_q32"].tolist()) == grid
    print("device: z %.2f at %.4f (restatement %.2f), integer search at most %.2f" % (
        fine[0]["z"], fine[0]["period"], zg[best], found["z"].max()))
    # refine_pri on the powers alone gives the same answer
    again = refine_pri(torch.from_numpy(p).cuda(), 2048.36, 0.06, step)
    assert len(again) == 7 and again[0]["period_q32"] == grid[best]
    # the integer integrator misses the train, the fine chain finds it once per interval at its gate and row
    miss = detect_pulse_train(iq, r, 2048, QC.CHAIN_K, normalize=True, fs=c["fs"])
    assert [d for d in miss if d["cpi"] < QC.CHAIN_CPIS] == []
    for src in (iq, host):
        got = detect_pulse_train_fine(src, r, QC.CHAIN_PERIOD, QC.CHAIN_K, normalize=True, fs=c["fs"], chunk_samples=100000)
        assert got.dtype == TRAIN_DET_DTYPE
        assert [(int(d["cpi"]), int(d["gate"]), int(d["doppler_bin"])) for d in got] == want
        assert np.allclose(got["frequency"], QC.CHAIN_BIN * c["fs"] / (QC.CHAIN_K * float(QC.CHAIN_PERIOD)), rtol=1e-12, atol=0)
        assert (got["peak_power"] > a_train * got["noise"]).all()
    # the period the search found, handed on, finds it too
    got = detect_pulse_train_fine(iq, r, fine[0]["period"], QC.CHAIN_K, normalize=True, fs=c["fs"])
    got = got[got["cpi"] < QC.CHAIN_CPIS]           # at a shorter period a 193rd row begins: an interval of zeros but for it
    assert [(int(d["cpi"]), int(d["doppler_bin"])) for d in got] == [(k, QC.CHAIN_BIN) for k in range(QC.CHAIN_CPIS)]
    # a period off by d walks the pulses of interval c by d K c .. d K (c + 1) samples: the gate lies within that of 700
    walk = abs(float(QC.CHAIN_PERIOD) - fine[0]["period"]) * QC.CHAIN_K * (got["cpi"] + 1.0)
    assert (np.abs(got["gate"].astype(np.int64) - QC.CHAIN_FIRST) <= np.ceil(walk)).all()
