"""The fractional-PRI search and regridder without a GPU: the numpy restatement (qfold_ref) against the literal per-cell
loop, the period arithmetic, the counts against np.bincount and pfb_qfold_counts, agreement with fold_ref at whole
periods, every argument check that comes before the device, the struct layouts, the exports, and -- on the restatements
alone -- the two scenes test_gpu_qfold.py relies on."""
import ctypes as C
import os
import re
import shutil
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import fold_ref
import qfold_cases as QC
import qfold_ref as R
from abi_symbols import declared_symbols
from sdr_channelizer_amd import _lib as L
from sdr_channelizer_amd import cfar
from sdr_channelizer_amd import pri_fine as pf
from sdr_channelizer_amd import pri_search as ps

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
QFOLD_EXPORTS = {"pfb_qfold_" + n for n in (
    "describe", "counts", "create", "destroy", "reset", "set_index", "set_stream", "sync", "get_device", "next_index",
    "process", "process_async", "scores", "profile", "last_kernel")}
REGRID_EXPORTS = {"pfb_regrid_" + n for n in (
    "create", "destroy", "reset", "set_index", "set_stream", "sync", "get_device", "next_index", "outputs_for", "process",
    "process_async", "doppler_frequencies")}
M32 = (1 << 32) - 1


def pq(Pi, Pf=0):
    return (Pi << 32) | Pf


# -- the definition, sentence by sentence -------------------------------------------------------------------------
@pytest.mark.parametrize("Pi,C_", [(1, 1), (7, 1), (7, 2), (7, 3), (8, 4), (9, 4), (11, 4), (13, 5), (64, 64), (127, 64),
                                   (100, 7), (33, 16)])
def test_restatement_is_the_literal_loop(Pi, C_):
    rng = np.random.default_rng(Pi * 100 + C_)
    for Pf in (0, 1, 1 << 31, M32, 0x5eb851eb):
        q = pq(Pi, Pf)
        s2 = R.start(2, q)
        for n in (0, 1, C_, Pi - 1, Pi, Pi + 1, s2 + 1, R.start(5, q) + 3):
            for first in (0, 3, Pi - 1, s2 + 1, (1 << 40) + 5):
                p = R.spread_stream(n, int(rng.integers(1 << 30)))
                F, cnt, js = R.literal_fold(p, q, C_, first)
                assert R.fold(p, q, C_, first).tobytes() == F.tobytes()
                assert np.array_equal(R.bins(first, n, q, C_), js)
                assert np.array_equal(np.bincount(js, minlength=Pi // C_).astype(np.uint64), cnt)
                assert np.array_equal(R.counts(first + n, q, C_, first), cnt), (Pf, n, first)


def test_every_period_is_pi_or_pi_plus_one_long():
    for Pi in (1, 7, 2048, 1 << 24):
        for Pf in (0, 1, 1 << 31, M32, 0x5eb851eb):
            q = pq(Pi, Pf) if Pi < 1 << 24 else pq(Pi)
            for m0 in (0, 1, 1000, (1 << 38) + 3):
                s = [R.start(m, q) for m in range(m0, m0 + 70)]
                d = np.diff(np.array(s, dtype=object))
                assert set(d.tolist()) <= {Pi, Pi + 1} and (d > 0).all()
                assert (q & M32) or set(d.tolist()) == {Pi}
                for m, a, b in zip(range(m0, m0 + 69), s[:-1], s[1:]):
                    assert R.period_of(a, q) == m == R.period_of(b - 1, q) and (a == 0 or R.period_of(a - 1, q) == m - 1)
    assert [R.start(m, pq(3, 1 << 31)) for m in range(5)] == [0, 4, 7, 11, 14]
    assert R.q32(Fraction(204837, 100)) == pf.period_q32(Fraction(204837, 100)) == round(Fraction(204837, 100) * 2 ** 32)


def test_a_cut_stream_and_a_start_index_in_mid_period():
    p = R.spread_stream(700, 3)
    for q, C_ in ((pq(37, 1 << 31), 4), (pq(64, M32), 16), (pq(101, 1), 5)):
        whole = R.fold(p, q, C_)
        for cuts in ((0, 1, 2, 3, 700), (0, 36, 37, 38, 300, 300, 700), tuple(range(0, 701, 7))):
            F = None
            for a, b in zip(cuts[:-1], cuts[1:]):
                F = R.fold(p[a:b], q, C_, a, F)
            assert F.tobytes() == whole.tobytes()
        # from the middle of period 1: the used bins are not the leading ones
        N0 = R.start(1, q) + 2 * C_ + 1
        rec = R.score(R.fold(p[:C_], q, C_, N0), N0 + C_, q, C_, N0)
        n = R.counts(N0 + C_, q, C_, N0)
        assert n[:2].sum() == 0 and n[2] == C_ - 1 and n[3] == 1 and rec["bins_used"] == 2 and rec["cells"] == C_
        assert rec["peak_bin"] in (2, 3) and rec["peak_cells"] == n[rec["peak_bin"]]


def test_whole_periods_are_the_integer_fold():
    """with Pf = 0: bins, profiles, counts and every shared score field equal fold_ref's"""
    p = R.spread_stream(700, 9)
    for C_ in range(1, 65):
        for L_ in range(max(7, C_), 128):
            q = pq(L_)
            assert np.array_equal(R.bins(0, 700, q, C_), fold_ref.bins(np.arange(700), L_, C_))
            for N in (0, 1, L_, 3 * L_ + 2, 700):
                F = R.fold(p[:N], q, C_)
                assert F.tobytes() == fold_ref.fold(p[:N], L_, C_).tobytes()
                assert np.array_equal(R.counts(N, q, C_), fold_ref.counts(N, L_, C_))
                a, b = R.score(F, N, q, C_), fold_ref.score(F, N, L_, C_)
                assert a["period_q32"] == L_ << 32
                for name in R.SHARED + ["sum_means", "sum_sq_means"]:
                    assert a[name] == b[name] or (np.isnan(a[name]) and np.isnan(b[name])), (C_, L_, N, name)


def test_the_score_record():
    nan, inf = np.nan, np.inf
    q = pq(16, 1 << 31)
    for F, want in (([1, 5, 5, 2], 1), ([3, nan, 9, 9], 2), ([nan, 9, 1, 1], 0), ([1, -inf, inf, inf], 2),
                    ([-inf, -inf, -inf, -inf], 0), ([1, 2, nan, nan], 1)):
        assert R.score(np.array(F, np.float32), 16, q, 4)["peak_bin"] == want, F
    # a start index after bin 0: the first used bin is bin 1, and a NaN there stays
    assert R.score(np.array([0, nan, 9, 1], np.float32), 16, q, 4, N0=4)["peak_bin"] == 1
    assert R.score(np.array([0, 3, 9, 9], np.float32), 16, q, 4, N0=4)["peak_bin"] == 2
    rng = np.random.default_rng(8)
    for _ in range(200):
        F = rng.choice(np.array([nan, inf, -inf, 0.0, -0.0, 1.0, 2.0, 3.0], np.float32), 12)
        N0 = int(rng.integers(0, 20))
        n = R.counts(48, pq(48), 4, N0)
        used = [j for j in range(12) if n[j] > 0]
        with np.errstate(all="ignore"):
            m = F.astype(np.float64) / np.maximum(n, 1)
        assert R.score(F, 48, pq(48), 4, N0)["peak_bin"] == R.literal_peak(m, used), (F, N0)
    zero = R.score(np.zeros(9, np.float32), 5, pq(37, 7), 4, N0=5)
    assert bytes(zero) == bytes(np.array((pq(37, 7), 9, 0, 0, 0, 0, 0, 0, 0, 0, 0), R.SCORE))
    assert R.SCORE == pf.QSCORE_DTYPE and R.SCORE.itemsize == C.sizeof(L.PfbQfoldScore) == 64
    for (name, _), (cname, _) in zip(R.SCORE.descr, L.PfbQfoldScore._fields_):
        assert name == cname and R.SCORE.fields[name][1] == getattr(L.PfbQfoldScore, cname).offset
    # fold_z reads the new records unchanged
    rec = np.zeros(2, pf.QSCORE_DTYPE)
    rec["bins_used"], rec["peak_mean"], rec["sum_means"], rec["sum_sq_means"] = (16, 7), 5.0, 16.0, 32.0
    assert ps.fold_z(rec).tolist() == [4.0, 0.0] == R.z(rec).tolist()
    found = pf.rank_fine(rec, 4)
    assert found.dtype == pf.QFOUND_DTYPE and found["z"].tolist() == [4.0, 0.0]


def test_period_conversions():
    assert pf.period_q32(2048) == 2048 << 32 and pf.period_q32(np.int64(7)) == 7 << 32
    assert pf.period_q32(Fraction(1, 3)) == round(Fraction(1 << 32, 3)) and pf.period_q32(0.5) == 1 << 31
    assert pf.period_q32(2048.37) == round(Fraction(2048.37) * 2 ** 32)      # the float's exact value, to nearest
    assert abs(pf.period_samples(pf.period_q32(2048.37)) - 2048.37) <= 2.0 ** -33 and pf.period_samples(pq(2048, 1 << 30)) == 2048.25
    assert pf.period_samples((5 << 32) | (1 << 31)) == 5.5
    for bad in (-1, -0.5, Fraction(-1, 3)):
        with pytest.raises(ValueError):
            pf.period_q32(bad)
    with pytest.raises(TypeError):
        pf.period_q32(True)
    g = pf.grid_q32(2048, 2049, 0.25)
    assert g.dtype == np.uint64 and g.tolist() == [pq(2048), pq(2048, 1 << 30), pq(2048, 1 << 31), pq(2048, 3 << 30), pq(2049)]
    assert len(pf.grid_q32(2048.35, 2048.39, 0.002)) == 21
    assert [len(x) for x in pf._loads([pq(65536)] * 600, 1)] == [256, 256, 88]
    assert [len(x) for x in pf._loads([pq(64)] * 5000, 1)] == [4096, 904]


# -- the arguments ---------------------------------------------------------------------------------------------------
def config(periods=(pq(2048, 5), pq(2049)), C_=4, NC=None, flags=0, size=None, device=-1, null=False):
    p = np.ascontiguousarray(periods, np.uint64)
    cfg = L.PfbQfoldConfig(C.sizeof(L.PfbQfoldConfig) if size is None else size, C_, len(p) if NC is None else NC, flags,
                           None if null else p.ctypes.data_as(C.POINTER(C.c_uint64)), device, 0)
    cfg._keep = p
    return cfg


def both(**kw):
    """the status of pfb_qfold_describe and of pfb_qfold_create for one config, their outputs untouched on failure"""
    lib = L.load()
    cfg = config(**kw)
    plan, h = L.PfbQfoldPlan(), C.c_void_p()
    C.memset(C.byref(plan), 0x5a, C.sizeof(plan))
    d = lib.pfb_qfold_describe(C.byref(cfg), C.byref(plan))
    c = lib.pfb_qfold_create(C.byref(cfg), C.byref(h))
    assert d == L.PFB_OK or bytes(plan) == b"\x5a" * C.sizeof(plan)
    assert not h.value or c == L.PFB_OK
    if h.value:
        lib.pfb_qfold_destroy(h)
    return d, c


def test_arguments_are_checked_before_the_device_and_in_order():
    lib = L.load()
    BAD, UNS = L.PFB_ERR_BAD_ARG, L.PFB_ERR_UNSUPPORTED
    plan, h = L.PfbQfoldPlan(), C.c_void_p()
    cfg = config()
    assert lib.pfb_qfold_describe(None, C.byref(plan)) == lib.pfb_qfold_describe(C.byref(cfg), None) == BAD
    assert lib.pfb_qfold_create(None, C.byref(h)) == lib.pfb_qfold_create(C.byref(cfg), None) == BAD
    # one case per refusal, in the header's order: null list, struct_size, C, NC, a period, flags
    bad = [dict(null=True), dict(size=28), dict(size=40), dict(C_=0), dict(C_=65), dict(C_=1 << 31)]
    bad += [dict(NC=0), dict(periods=[pq(2048)] * 4097), dict(NC=1 << 31)]
    bad += [dict(periods=(pq(2048), pq(3, M32))), dict(periods=(0,)), dict(periods=(M32,), C_=1)]
    bad += [dict(periods=(pq(1 << 24, 1),), C_=64), dict(periods=((1 << 64) - 1,), C_=64)]
    bad += [dict(periods=(pq(65537),), C_=1), dict(periods=(pq(2048), pq(65536 * 4 + 4, 9)))]
    bad += [dict(flags=1), dict(flags=1 << 31)]
    for kw in bad:
        assert both(**kw) == (BAD, BAD), kw
        assert both(device=1 << 20, **kw) == (BAD, BAD), kw    # before the device is looked at
    assert both(C_=0, periods=[pq(2048)] * 4097, flags=1) == (BAD, BAD)
    # the profiles: 64 MiB allowed, one bin more refused -- after every BAD_ARG check
    full = [pq(65536, 77)] * 256
    assert both(periods=full + [pq(1)], C_=1, device=1 << 20) == (UNS, UNS)
    assert both(periods=full + [pq(1)], C_=1, flags=1, device=1 << 20) == (BAD, BAD)
    assert lib.pfb_qfold_describe(C.byref(config(periods=full, C_=1)), C.byref(plan)) == L.PFB_OK
    assert (plan.profile_bytes, plan.total_bins, plan.max_bins) == (64 << 20, 1 << 24, 65536)
    # the largest legal shapes: Pi = 2^24 exactly, and 65536 bins at C = 64 with the fraction full
    assert lib.pfb_qfold_describe(C.byref(config(periods=(pq(1 << 24), pq((1 << 22) + 63, M32)), C_=64 * 4)), C.byref(plan)) == BAD
    assert lib.pfb_qfold_describe(C.byref(config(periods=(pq((1 << 22) + 63, M32), pq(1 << 22)), C_=64)), C.byref(plan)) == L.PFB_OK
    assert (plan.total_bins, plan.max_bins) == (2 << 16, 65536)
    assert both(periods=(pq(1 << 24),), C_=64, device=1 << 20) == (BAD, BAD)          # 2^18 bins
    # null handles and pointers
    u = C.c_uint64(7)
    buf = np.zeros(64, np.float32)
    p = C.c_void_p(buf.ctypes.data)
    assert lib.pfb_qfold_destroy(None) == lib.pfb_qfold_reset(None) == lib.pfb_qfold_sync(None) == BAD
    assert lib.pfb_qfold_set_index(None, 0) == lib.pfb_qfold_set_tier(None, 0, 0) == BAD
    assert lib.pfb_qfold_set_stream(None, None) == lib.pfb_qfold_get_device(None, None) == BAD
    assert lib.pfb_qfold_next_index(None, C.byref(u)) == BAD and u.value == 7
    for mem in (L.PFB_MEM_HOST, L.PFB_MEM_DEVICE, 2):
        assert lib.pfb_qfold_process(None, p, 16, mem) == lib.pfb_qfold_scores(None, p, 2, mem) == BAD
        assert lib.pfb_qfold_profile(None, 0, p, 64, mem) == BAD
    assert lib.pfb_qfold_process_async(None, p, 16) == BAD
    assert lib.pfb_qfold_last_kernel(None) == b""
    assert not buf.any()
    with pytest.raises(ValueError):
        pf.describe_fine_fold([-1.5])
    with pytest.raises(ValueError):
        pf.describe_fine_fold([1 << 32])


def regrid_config(period=pq(2048, 5), R_=256, origin=0, elem=8, flags=0, size=None, device=-1):
    return L.PfbRegridConfig(C.sizeof(L.PfbRegridConfig) if size is None else size, R_, period, origin, elem, flags, device, 0)


def test_regrid_arguments_are_checked_before_the_device_and_in_order():
    lib = L.load()
    BAD = L.PFB_ERR_BAD_ARG
    h = C.c_void_p()
    assert lib.pfb_regrid_create(None, C.byref(h)) == lib.pfb_regrid_create(C.byref(regrid_config()), None) == BAD
    bad = [dict(size=36), dict(size=48), dict(period=M32), dict(period=0), dict(period=pq(1 << 24, 1)),
           dict(origin=(1 << 62) + 1), dict(R_=0), dict(R_=2049), dict(R_=1 << 31), dict(elem=0), dict(elem=2), dict(elem=16),
           dict(flags=1)]
    for kw in bad:
        for dev in (-1, 1 << 20):
            cfg = regrid_config(device=dev, **kw)
            assert lib.pfb_regrid_create(C.byref(cfg), C.byref(h)) == BAD and not h.value, kw
    assert lib.pfb_regrid_create(C.byref(regrid_config(period=M32, origin=1 << 63, R_=0, elem=3, flags=1)), C.byref(h)) == BAD
    u = C.c_uint64(7)
    assert lib.pfb_regrid_destroy(None) == lib.pfb_regrid_reset(None) == lib.pfb_regrid_sync(None) == BAD
    assert lib.pfb_regrid_set_index(None, 0) == lib.pfb_regrid_set_stream(None, None) == BAD
    assert lib.pfb_regrid_get_device(None, None) == lib.pfb_regrid_next_index(None, C.byref(u)) == BAD
    assert lib.pfb_regrid_outputs_for(None, 5, C.byref(u)) == BAD and u.value == 7
    assert lib.pfb_regrid_process(None, None, 0, None, 0, C.byref(u), 0) == BAD
    assert lib.pfb_regrid_process_async(None, None, 0, None, 0, None) == BAD
    with pytest.raises(TypeError):
        pf.Regrid(2048.5, 256, dtype=np.float64)


def test_a_valid_config_needs_a_device():
    if L.load().pfb_device_count() > 0:
        pytest.skip("a GPU is present")
    for kw in (dict(), dict(periods=(pq(1),), C_=1), dict(periods=(pq(64, M32),), C_=64), dict(periods=[pq(65536, 1)] * 256, C_=1),
               dict(periods=(pq(2048, 3),) * 3), dict(periods=(pq((1 << 22) + 63, M32),), C_=64)):
        assert both(**kw) == (L.PFB_OK, L.PFB_ERR_NO_DEVICE), kw
    with pytest.raises(L.PfbError) as e:
        pf.FinePriFold([2048.37, 2049])
    assert e.value.status == L.PFB_ERR_NO_DEVICE
    with pytest.raises(L.PfbError) as e:
        pf.Regrid(2048.37, 2048)
    assert e.value.status == L.PFB_ERR_NO_DEVICE
    with pytest.raises(L.PfbError) as e:
        pf.find_pri_fine(np.ones((1000, 2), np.float32), np.ones(13, np.complex64), 100, 101, 0.5)
    assert e.value.status == L.PFB_ERR_NO_DEVICE
    with pytest.raises(ValueError):
        pf.find_pri_fine(np.broadcast_to(np.int8(1), ((1 << 27) + 1, 2)), np.ones(13, np.complex64), 100, 101, 0.5,
                         sample_format="int8")                     # refused by its length, before anything is allocated


def test_describe():
    periods = [640.25, Fraction(6411, 10), 1000, np.float64(640.25)]
    for C_ in (1, 2, 3, 4, 5, 7, 8, 12, 16, 32, 63, 64):
        plan = pf.describe_fine_fold(periods, C_)
        nb = [640 // C_, 641 // C_, 1000 // C_, 640 // C_]
        assert (plan.total_bins, plan.profile_bytes, plan.max_bins) == (sum(nb), 4 * sum(nb), max(nb))
        assert plan.kernel.decode() == QC.kernel_name(C_)
    assert pf.describe_fine_fold(np.array([pq(640, 9)], np.uint64), 4).total_bins == 160


def test_counts_are_the_closed_form():
    lib = L.load()
    periods = np.array([pq(9, 1), pq(37, 1 << 31), pq(64, M32), pq(2048, 0x5eb851eb), pq(127)], np.uint64)
    for C_ in (1, 3, 4, 5):
        for k, q in enumerate(periods.tolist()):
            Pi = q >> 32
            for N in (0, 1, C_, Pi - 1, Pi, Pi + 1, R.start(2, q) + C_ + 1, R.start(5, q) + 3, (1 << 32) - 3, (1 << 40) + 12345,
                      (1 << 56) + 5, (1 << 62) - 12345, 1 << 62):
                got = pf.fine_fold_counts(periods, C_, k, N)
                assert got.dtype == np.uint64 and np.array_equal(got, R.counts(N, q, C_)), (C_, q, N)
                assert int(got.sum()) == N
                for N0 in (0, N // 3, max(N - Pi - 2, 0), N):
                    got = pf.fine_fold_counts(periods, C_, k, N, N0)
                    assert np.array_equal(got, R.counts(N, q, C_, N0)) and int(got.sum()) == N - N0
    assert np.array_equal(pf.fine_fold_counts(periods, 4, 1, 300, 41), np.bincount(R.bins(41, 259, int(periods[1]), 4), minlength=9))
    out = np.full(16, 77, np.uint64)
    po = out.ctypes.data_as(C.POINTER(C.c_uint64))
    cfg = config(periods=(pq(9, 5), pq(37)))
    BAD = L.PFB_ERR_BAD_ARG
    assert lib.pfb_qfold_counts(None, 0, 0, 5, po) == lib.pfb_qfold_counts(C.byref(cfg), 0, 0, 5, None) == BAD
    assert lib.pfb_qfold_counts(C.byref(cfg), 2, 0, 5, po) == lib.pfb_qfold_counts(C.byref(cfg), 0, 0, (1 << 62) + 1, po) == BAD
    assert lib.pfb_qfold_counts(C.byref(cfg), 0, 6, 5, po) == BAD
    assert lib.pfb_qfold_counts(C.byref(config(periods=(pq(9), pq(3)))), 0, 0, 5, po) == BAD
    assert lib.pfb_qfold_counts(C.byref(config(periods=[pq(65536)] * 257, C_=1)), 0, 0, 5, po) == L.PFB_ERR_UNSUPPORTED
    assert (out == 77).all()
    assert lib.pfb_qfold_counts(C.byref(cfg), 0, 0, 5, po) == L.PFB_OK and out[:3].tolist() == [4, 1, 77]
    with pytest.raises(IndexError):
        pf.fine_fold_counts(periods, 4, 5, 10)


def test_regrid_restatement_and_doppler_frequencies():
    q = pq(5, 1 << 31)                                         # rows begin at 0, 6, 11, 17, 22, ...
    assert [R.regrid_source(t, q, 2, 100) for t in range(6)] == [100, 101, 106, 107, 111, 112]
    assert [R.regrid_before(X, q, 2, 100) for X in (0, 100, 101, 102, 106, 107, 108, 111)] == [0, 0, 1, 2, 2, 3, 4, 4]
    x = np.arange(40)
    whole = R.regrid(x, 90, q, 2, 100)[1]
    assert whole.tolist()[:6] == [10, 11, 16, 17, 21, 22]
    for cuts in ((0, 11, 12, 17, 40), (0, 13, 15, 16, 40), tuple(range(0, 41, 1))):      # a call between two rows gives nothing
        parts = [R.regrid(x[a:b], 90 + a, q, 2, 100) for a, b in zip(cuts[:-1], cuts[1:])]
        assert np.concatenate([v for _, v in parts]).tolist() == whole.tolist()
        assert [t for t, _ in parts] == np.cumsum([0] + [len(v) for _, v in parts])[:-1].tolist()
    assert len(R.regrid(x[13:15], 103, q, 2, 100)[1]) == 0
    for ND, centered in ((64, True), (64, False), (8, True), (1, False)):
        got = pf.regrid_doppler_frequencies(Fraction(204837, 100), ND, 2.0e6, centered)
        want = R.regrid_doppler(R.q32(Fraction(204837, 100)), ND, 2.0e6, centered)
        assert got.shape == (ND,) and np.allclose(got, want, rtol=1e-14, atol=0)
    assert pf.regrid_doppler_frequencies(2048, 64, 2.0e6, True).tolist() == ps_doppler(2048, 64, 2.0e6)
    lib = L.load()
    out = np.zeros(4)
    po = out.ctypes.data_as(C.POINTER(C.c_double))
    BAD = L.PFB_ERR_BAD_ARG
    assert lib.pfb_regrid_doppler_frequencies(pq(2048), 4, 0, 1.0, None) == BAD
    assert lib.pfb_regrid_doppler_frequencies(M32, 4, 0, 1.0, po) == lib.pfb_regrid_doppler_frequencies(pq(1 << 24, 1), 4, 0, 1.0, po) == BAD
    assert lib.pfb_regrid_doppler_frequencies(pq(2048), 0, 0, 1.0, po) == lib.pfb_regrid_doppler_frequencies(pq(2048), 65537, 0, 1.0, po) == BAD
    assert lib.pfb_regrid_doppler_frequencies(pq(2048), 4, 0, float("nan"), po) == BAD and not out.any()


def ps_doppler(L_, ND, fs):
    from sdr_channelizer_amd.pulse_doppler import doppler_frequencies
    return doppler_frequencies(L_, ND, fs, True).tolist()


def test_exports():
    lib = L.load()
    declared = declared_symbols()
    for prefix, want in (("pfb_qfold_", QFOLD_EXPORTS), ("pfb_regrid_", REGRID_EXPORTS)):
        assert {n for n in declared if n.startswith(prefix)} == want == {n for n in L.EXPORTS if n.startswith(prefix)}
        for name in want:
            assert hasattr(lib, name), name
    assert "pfb_qfold_set_tier" in L.DEV_EXPORTS and "pfb_qfold_set_tier" in declared_symbols(("pfb_channelizer_dev.h",))
    assert (C.sizeof(L.PfbQfoldConfig), C.sizeof(L.PfbQfoldPlan), C.sizeof(L.PfbQfoldScore), C.sizeof(L.PfbRegridConfig)) \
        == (32, 56, 64, 40)
    hdr = open(os.path.join(ROOT, "include", "pfb_channelizer.h")).read()
    assert "#define PFB_ABI_VERSION 2" in hdr and lib.pfb_abi_version() == 2
    assert hdr.index("pfb_qfold_describe(") > hdr.index("pfb_mop_pulses_from_pdw(")   # its own section, at the end
    assert "non-integer" not in hdr and hdr.count("staggered") >= 3
    import sdr_channelizer_amd as pkg
    names = ["FinePriFold", "describe_fine_fold", "period_q32", "period_samples", "refine_pri", "find_pri_fine", "Regrid",
             "regrid", "regrid_doppler_frequencies", "detect_pulse_train_fine", "QSCORE_DTYPE"]
    at = pkg.__all__.index("isolate_band") + 1
    assert pkg.__all__[at:at + len(names)] == names and pkg.__all__[at + len(names)] == "MOP_DTYPE"
    for name in names:
        assert getattr(pkg, name) is getattr(pf, name)


def test_the_struct_layouts_are_the_compilers(tmp_path):
    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.skip("no gcc")
    lines, want = [], []
    for cname, cls in (("pfb_qfold_config", L.PfbQfoldConfig), ("pfb_qfold_plan", L.PfbQfoldPlan),
                       ("pfb_qfold_score", L.PfbQfoldScore), ("pfb_regrid_config", L.PfbRegridConfig)):
        lines.append(f'  printf("%zu\\n", sizeof({cname}));')
        want.append(C.sizeof(cls))
        for name, _ in cls._fields_:
            lines.append(f'  printf("%zu\\n", offsetof({cname}, {name}));')
            want.append(getattr(cls, name).offset)
    src = tmp_path / "sizes.c"
    src.write_text('#include "pfb_channelizer.h"\n#include <stdio.h>\n#include <stddef.h>\nint main(void) {\n'
                   + "\n".join(lines) + "\n  return 0;\n}\n")
    exe = tmp_path / "sizes"
    subprocess.run([gcc, "-std=c99", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)],
                   check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert [int(v) for v in r.stdout.split()] == want and C.sizeof(L.PfbQfoldScore) == 64


def test_entry_points_sit_under_the_abi_guard():
    src = open(os.path.join(ROOT, "sdr_channelizer_amd", "csrc", "pfb_qfold.hip")).read()
    found = {}
    for m in re.finditer(r'^extern "C" int (\w+)\(', src, re.M):
        rest = src[m.start():]
        found[m.group(1)] = rest[: rest.index("\n}\n")]
    assert set(found) == ((QFOLD_EXPORTS | REGRID_EXPORTS) - {"pfb_qfold_last_kernel"}) | {"pfb_qfold_set_tier"}
    for name, body in found.items():
        assert "abi_guard" in body.split("{", 1)[1][:80], name
    assert src.count('extern "C"') == len(found) + 1
    from sdr_channelizer_amd import build
    assert "pfb_qfold.hip" in build.SOURCES
    create = src[src.index("int create_qfold("):]
    create = create[: create.index("\n}\n")]
    assert create.index("qfold_check(cfg") < create.index("resolve_device") < create.index("allocate_qfold(")
    code = re.sub(r"//.*", "", src).lower()
    for word in ("atomic", "asm", "mfma", "fma("):     # additions only, one writer per element
        assert word not in code, word


# -- the motivating scene, on the restatement alone -------------------------------------------------------------
SCENE_TRUE_Z, SCENE_OTHER_Z = 10.0, 8.0


def test_the_fractional_train_is_found_only_at_its_period():
    """512 pulses of +1.5 in exponential noise at 700 + ceil(k 2048.37), 2^20 cells, C = 4, seeds 1 .. 8.  The true period
    out-scores every integer candidate 2040 .. 2056 and every candidate 0.02 or more away; the margins asserted are those
    of DESIGN.md section 27 (the table printed here): z(true) >= 10, every integer and every candidate >= 0.02 away
    <= 8 and below the true period's, the peak in bin 175 = 700 / 4."""
    fr = [QC.SCENE_PERIOD + d for d in QC.SCENE_OFFSETS]
    cand = [R.q32(v) for v in QC.SCENE_INTEGERS + fr]
    k_true = len(QC.SCENE_INTEGERS)
    far = [k for k, v in enumerate(QC.SCENE_INTEGERS + fr) if abs(v - QC.SCENE_PERIOD) >= Fraction(2, 100)]
    assert cand[k_true] == QC.SCENE_Q and len(far) == len(QC.SCENE_INTEGERS) + 2
    print("integers: " + " ".join("%5d" % v for v in QC.SCENE_INTEGERS))
    print("seed  z(true)  best integer  z(-.02) z(+.02)  z(+-.002)      z(+-.004)      z(+-.01)")
    for seed in range(1, 9):
        z, rec = QC.scene_z(QC.scene(seed), cand)
        zi = z[:k_true]
        print("%4d  %7.2f  %7.2f @%d  %7.2f %7.2f  %6.2f %6.2f  %6.2f %6.2f  %6.2f %6.2f" % (
            seed, z[k_true], zi.max(), QC.SCENE_INTEGERS[int(zi.argmax())], z[-2], z[-1], *z[k_true + 1:k_true + 7]))
        print("      z(integers) " + " ".join("%5.2f" % v for v in zi))
        assert z[k_true] >= SCENE_TRUE_Z and rec[k_true]["peak_bin"] == 175
        assert all(z[k] <= SCENE_OTHER_Z and z[k] < z[k_true] for k in far), seed


# -- the chain scene, on mf_ref / pd_ref / cfar_ref alone ---------------------------------------------------------------
def test_the_chain_scene_needs_the_regrid():
    """a Barker-13 train under the single-pulse threshold at 2048.37 samples, Doppler row 5: integer folding ranks no
    integer period over 6, pd_ref at pri 2048 finds nothing, and after the regrid the train is found once per interval
    at its gate and row.  The loss from taking each pulse up to one sample late is printed."""
    a_single, a_train = QC.chain_alphas(cfar.cfar_alpha)
    y = QC.chain_compressed()
    p = QC.chain_powers()
    r = QC.pd_cases.chain_replica()
    single, _ = QC.cfar_ref.detect(p, len(p), True, C=64, G=-(-r.size // 64), T=8, alpha=a_single, merge_gap=r.size)
    assert len(single) == 0
    zi = fold_ref.z(fold_ref.scores(p, list(range(2040, 2057)), QC.CHAIN_FOLD_C)[0])
    zq, rec = QC.scene_z(p, [QC.CHAIN_Q])
    print("fold: z(2048.37) %.2f in bin %d, best integer %.2f" % (zq[0], rec[0]["peak_bin"], zi.max()))
    assert zi.max() <= 6 and zq[0] >= 8 and rec[0]["peak_bin"] == QC.CHAIN_FIRST // QC.CHAIN_FOLD_C
    found, peaks = QC.chain_detect(y, 2048, a_train)
    assert [f for f in found if f[0] < QC.CHAIN_CPIS] == []              # the train walks 24 gates in one interval
    found, peaks_q = QC.chain_detect(QC.chain_regridded(y), QC.CHAIN_ROW, a_train)
    assert found == [(c, QC.CHAIN_FIRST, QC.CHAIN_BIN) for c in range(QC.CHAIN_CPIS)]
    # the same train at a whole period: what the late alignment costs
    found_i, peaks_i = QC.chain_detect(QC.chain_compressed(2048 << 32), 2048, a_train)
    assert found_i[:QC.CHAIN_CPIS] == [(c, QC.CHAIN_FIRST, QC.CHAIN_BIN) for c in range(QC.CHAIN_CPIS)]
    loss = [10 * np.log10(a / b) for a, b in zip(peaks_q, peaks_i)]
    print("coherent peak, regridded 2048.37 against integer 2048: %s dB" % ", ".join("%.2f" % v for v in loss))
