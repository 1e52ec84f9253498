"""Modulation on pulse on the device against the numpy restatement (mop_ref): records and negatives byte for byte for
int8 and int16; for cf32 the counts, indices, flags and negatives byte for byte and the six doubles within the
header's bound.  Over every length at which the unit takes another path, one list through every tier, the list's edges,
more work than the capped grid has workgroups, odd pointers and guard bytes, full scale, NaN and Inf, the negatives'
list at its limits, pitched matrices, the host route in batches, async calls across a stream switch, and the chain:
pulse train -> extraction -> measurement -> figures, code, replica and matched filter."""
import ctypes as C
import importlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import mop_cases as MC  # noqa: E402
import mop_ref as R  # noqa: E402
import synth_ref as S  # noqa: E402
from gpu_support import cuda_torch  # noqa: E402
from sdr_channelizer_amd import (MatchedFilter, PulseModulation, PulseTrain, deinterleave, measure_pdws,  # noqa: E402
                                 measure_pulses, modulation_figures, modulation_from_iq_file, phase_code,
                                 replica_from_measurement)
from sdr_channelizer_amd import _lib as L  # noqa: E402
from sdr_channelizer_amd.pdw import extract_pdws_raw  # noqa: E402

pm = importlib.import_module("sdr_channelizer_amd.pulse_mod")
GUARD = 0x5A
FORMATS = (("int8", 8), ("int16", 12), ("cf32", 0))
ALL_TIERS = "mop_wave+mop_group+mop_split+mop_join"
TIER_NAMES = {1: "mop_wave", 2: "mop_group", 3: "mop_split+mop_join"}


@pytest.fixture(scope="module")
def torch():
    return cuda_torch()


def to_device(torch, x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def list_on_device(torch, plist):
    return torch.from_numpy(np.ascontiguousarray(plist).view(np.uint8)).cuda()


def as_numpy(rec, negs):
    if isinstance(rec, np.ndarray):
        return rec, negs
    return pm.records_to_numpy(rec), negs.cpu().numpy().view(np.uint32)


def agree(fmt, got, want, what=""):
    """(records, negs) of the device against (records, negs, bounds) of the restatement"""
    rec, negs = as_numpy(*got)
    assert rec.dtype == R.MOP and negs.dtype == np.uint32 and negs.shape == want[1].shape, what
    assert negs.tobytes() == want[1].tobytes(), what
    if fmt != "cf32":
        assert rec.tobytes() == want[0].tobytes(), (what, rec[rec != want[0]][:3], want[0][rec != want[0]][:3])
        return
    assert MC.same_exact(rec, want[0]), what
    ok, why = R.same_sums(rec, want[0], want[2])
    assert ok, (what, why)


def tier(m, t, grid_cap=0, stage_bytes=0):
    L.check(m._lib.pfb_mop_set_tier(m._h, t, grid_cap, stage_bytes), "pfb_mop_set_tier")


# -- lengths -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt,bw", FORMATS)
def test_every_length_at_which_the_path_changes(torch, fmt, bw):
    rows = MC.SPLIT_MIN + 3000
    x = MC.random_series(fmt, rows, 21)
    dx = to_device(torch, x)
    for trim in (0, 1, 7):
        lengths = MC.lengths_of_interest(trim) + [2 * trim, 2 * trim + 1] + ([1] if trim else [])
        plist = MC.spread(lengths, rows, 22 + trim)
        want = R.measure(x, plist, trim=trim, max_negatives=8)
        with PulseModulation(fmt, bw, trim, 8) as m:
            assert m.last_kernel == ""
            assert (m.plan.group_min, m.plan.split_min, m.plan.part_samples) == (MC.GROUP_MIN, MC.SPLIT_MIN, MC.PART)
            agree(fmt, m.measure(dx, plist), want, (fmt, trim))
            assert m.last_kernel == ALL_TIERS
            agree(fmt, m.measure(dx, list_on_device(torch, plist)), want, (fmt, trim, "device list"))
        assert set(want[0]["n"].tolist()) >= {0, 1, 2, 3, 63, 64, 65, 255, 256, 257, MC.GROUP_MIN - 1, MC.GROUP_MIN,
                                              MC.SPLIT_MIN - 1, MC.SPLIT_MIN, MC.SPLIT_MIN + 1}


@pytest.mark.parametrize("fmt,bw", [("int16", 16), ("cf32", 0)])
def test_the_longest_pulse_and_one_more(torch, fmt, bw):
    rows = (1 << 20) + 1
    x = MC.random_series(fmt, rows, 23)
    plist = R.pulses([1, 0, 0], [1 << 20, (1 << 20) + 1, 300])
    want = R.measure(x, plist, max_negatives=4)
    assert want[0]["flags"].tolist() == [R.NEGS_CLIPPED, R.NEGS_CLIPPED | R.TRUNCATED, R.NEGS_CLIPPED]
    assert want[0]["n"].tolist() == [1 << 20, 1 << 20, 300]
    with PulseModulation(fmt, bw, 0, 4) as m:
        agree(fmt, m.measure(to_device(torch, x), plist), want)
        assert m.last_kernel == "mop_wave+mop_split+mop_join"


def test_full_scale_int16_needs_both_limbs(torch):
    rows = 1 << 20
    x = np.full((rows, 2), -32768, np.int16)
    x[7::2, 0] = 32767                                    # mixed signs from sample 7 on; before it an exact tie of the peak
    plist = R.pulses([0, 0, 5, 0], [rows, 40000, 300, 7])
    want = R.measure(x, plist, max_negatives=2)
    assert want[0]["s2_re"][0] != 0 and abs(want[0]["s2_re"][0]) > 2.0 ** 64 and want[0]["peak_index"].tolist()[3] == 0
    with PulseModulation("int16", 16, 0, 2) as m:
        agree("int16", m.measure(to_device(torch, x), plist), want)
        for t in (1, 2, 3):
            tier(m, t)
            agree("int16", m.measure(to_device(torch, x), plist[1:]), tuple(w[1:] for w in want), t)


# -- tiers -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt,bw", FORMATS)
def test_one_list_through_every_tier(torch, fmt, bw):
    rows = 3 * MC.PART
    x = MC.random_series(fmt, rows, 31)
    lengths = [0, 1, 2, 3, 4, 5, 65, 600, MC.PART, MC.PART + 1, 2 * MC.PART - 5, 64, 256, MC.GROUP_MIN]
    plist = MC.spread(lengths, rows, 32)
    want = R.measure(x, plist, max_negatives=128)
    dx = to_device(torch, x)
    with PulseModulation(fmt, bw, 0, 128) as m:
        seen = []
        for t in (0, 1, 2, 3):
            tier(m, t)
            got = as_numpy(*m.measure(dx, plist))
            agree(fmt, got, want, t)
            seen.append(got[0].tobytes())
            assert m.last_kernel == (TIER_NAMES[t] if t else "mop_wave+mop_group")
        if fmt != "cf32":
            assert len(set(seen)) == 1                     # the same bytes whatever the tier
        assert m._lib.pfb_mop_set_tier(m._h, 4, 0, 0) == m._lib.pfb_mop_set_tier(m._h, -1, 0, 0) == L.PFB_ERR_BAD_ARG
        assert m._lib.pfb_mop_set_tier(m._h, 0, 65537, 0) == L.PFB_ERR_BAD_ARG


# -- the list's edges --------------------------------------------------------------------------------------------------
def test_list_edges(torch):
    rows, base = 5000, (1 << 32) + 12345
    x = MC.random_series("int16", rows, 41)
    dx = to_device(torch, x)
    starts = [base + 900, base + 10, base + 900, base + 950, base, base + rows - 40, base + rows - 39, base - 1,
              base + rows, base + rows, base + rows + 1, 0, (1 << 64) - 5, base + 100, 900]
    lengths = [700, 30, 700, 700, 40, 40, 40, 40, 0, 1, 0, 40, 40, 0xFFFFFFFF, 700]
    plist = R.pulses(starts, lengths)
    want = R.measure(x, plist, base=base, max_negatives=8)
    outside = [bool(f & R.OUTSIDE) for f in want[0]["flags"]]
    assert outside == [False] * 6 + [True, True, False, True, True, True, True, True, True]
    with PulseModulation("int16", 12, 0, 8) as m:
        agree("int16", m.measure(dx, plist, base_index=base), want)
        agree("int16", m.measure(x, plist, base_index=base), want, "host route")
        # the same list against base 0: all but the two pulses near 0 lie past 2^32, outside
        zero = R.measure(x, plist, base=0, max_negatives=8)
        assert [bool(f & R.OUTSIDE) for f in zero[0]["flags"]] == [True] * 11 + [False, True, True, False]
        agree("int16", m.measure(dx, plist), zero)
        rec, negs = m.measure(dx, plist[:0])
        assert len(rec) == 0 and negs.shape == (0, 8) and m.last_kernel == ""
    # column >= ld
    z = MC.random_series("cf32", 400, 42, ld=3)
    cols = R.pulses([10, 10, 10, 10], [100, 100, 100, 100], [0, 2, 3, 0xFFFFFFFF])
    want = R.measure(z, cols, max_negatives=8)
    assert [int(f & R.OUTSIDE) for f in want[0]["flags"]] == [0, 0, 1, 1]
    with PulseModulation("cf32", 0, 0, 8) as m:
        agree("cf32", m.measure(to_device(torch, z), cols), want)
        agree("cf32", m.measure(z, cols), want, "host route")


def test_more_units_of_work_than_the_grid_has_workgroups(torch):
    rows = 1 << 16
    x = MC.random_series("int16", rows, 51)
    dx = to_device(torch, x)
    rng = np.random.default_rng(52)
    with PulseModulation("int16", 12, 0, 2) as m:
        count = m.plan.grid_cap * 4 * 8 + 4469               # eight pulses a wave and a remainder; past one slice as well
        assert count > m.plan.slice_pulses
        lengths = rng.integers(3, 10, count)
        plist = R.pulses(rng.integers(0, rows - 9, count), lengths)
        want = R.measure_many(x, plist, 2)
        agree("int16", m.measure(dx, plist), want + (None,))
        assert m.last_kernel == "mop_wave"
        agree("int16", m.measure(dx, list_on_device(torch, plist)), want + (None,), "device list")
        # workgroups that loop, with the cap lowered through the dev switch: mop_group over 9 pulses with 2 workgroups,
        # and a split pulse whose 5 parts (and another's 3) exceed a grid of 3
        few = R.pulses([0, 100, 7, 7, 9000, 3, 0, 0, 40000], [600, 5, 3000, 3000, 64, 0, 2 * MC.PART, 70, 700])
        want = R.measure(x, few, max_negatives=2)
        tier(m, 2, grid_cap=2)
        agree("int16", m.measure(dx, few), want)
        long = R.pulses([3, 100], [4 * MC.PART + 9, 2 * MC.PART + 1])
        want = R.measure(x, long, max_negatives=2)
        tier(m, 3, grid_cap=3)
        agree("int16", m.measure(dx, long), want)
        assert m.last_kernel == "mop_split+mop_join"
        # more split pulses than one launch has slots, at the library's own cap: a launch of 256 slots is 256 x 64 =
        # 16384 units of work for 2048 workgroups, eight each (all but the first part of each are passed over)
        many = R.pulses(rng.integers(0, rows - 9, m.plan.split_slots + 40), rng.integers(3, 10, m.plan.split_slots + 40))
        want = R.measure_many(x, many, 2)
        tier(m, 3)
        agree("int16", m.measure(dx, many), want + (None,))


# -- pointers and numbers ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt,bw", FORMATS)
def test_odd_pointers_and_guard_bytes(torch, fmt, bw):
    rows = 3000
    x = MC.random_series(fmt, rows + 3, 61)
    dx = to_device(torch, x)
    assert dx.data_ptr() % 256 == 0
    plist = MC.spread([0, 3, 64, 700, 2000, rows], rows, 62)
    d_list = list_on_device(torch, plist)
    with PulseModulation(fmt, bw, 0, 5) as m:
        for off in (1, 2, 3):
            want = R.measure(x[off:off + rows], plist, max_negatives=5)
            part = dx[off:off + rows]
            assert part.data_ptr() % 256 == off * (2 if fmt == "int8" else 4 if fmt == "int16" else 8)
            agree(fmt, m.measure(part, plist), want, off)
            # records and negatives between guard bytes
            rec = torch.full((len(plist) + 2, 96), GUARD, dtype=torch.uint8, device="cuda")
            negs = torch.full((len(plist) + 2, 5), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
            L.check(m._lib.pfb_mop_measure(m._h, C.c_void_p(part.data_ptr()), rows, 1, 0, L.PFB_MEM_DEVICE,
                                           C.c_void_p(d_list.data_ptr()), len(plist), L.PFB_MEM_DEVICE,
                                           C.c_void_p(rec[1].data_ptr()), C.c_void_p(negs[1].data_ptr())), "pfb_mop_measure")
            agree(fmt, (rec[1:-1], negs[1:-1]), want, (off, "guards"))
            assert (rec[0] == GUARD).all() and (rec[-1] == GUARD).all()
            assert (negs[0] == 0x5A5A5A5A).all() and (negs[-1] == 0x5A5A5A5A).all()
        # misaligned device pointers are refused before the device is touched
        bad = L.PFB_ERR_BAD_ARG
        args = [C.c_void_p(dx.data_ptr()), rows, 1, 0, L.PFB_MEM_DEVICE, C.c_void_p(d_list.data_ptr()), len(plist),
                L.PFB_MEM_DEVICE, C.c_void_p(rec.data_ptr()), C.c_void_p(negs.data_ptr())]
        for k, by in ((0, 1), (5, 4), (8, 4), (9, 2)):
            off = list(args)
            off[k] = C.c_void_p(args[k].value + by)
            assert m._lib.pfb_mop_measure(m._h, *off) == bad, k
        assert m._lib.pfb_mop_measure(m._h, *args[:2], 0, *args[3:]) == bad                       # ld = 0
        assert m._lib.pfb_mop_measure(m._h, *args[:6], (1 << 24) + 1, *args[7:]) == bad
        if fmt != "cf32":
            assert m._lib.pfb_mop_measure(m._h, *args[:2], 2, *args[3:]) == bad                   # a pitch is cf32's
        else:
            assert m._lib.pfb_mop_measure(m._h, args[0], 1 << 62, 4, *args[3:]) == bad            # rows x ld overflows


def test_nan_and_inf_samples(torch):
    rows = 1200
    base = MC.random_series("cf32", rows, 71)
    plist = R.pulses([0, 100, 0, 0], [rows, 300, 40, 3])
    with PulseModulation("cf32", 0, 0, 16) as m:
        for name, edit in (("nan at the peak", lambda z: z.__setitem__(int(np.argmax(np.abs(z))), np.nan)),
                           ("nan in one term", lambda z: z.__setitem__(150, complex(np.nan, 1.0))),
                           ("nan everywhere", lambda z: z.fill(np.nan)),
                           ("+inf", lambda z: z.__setitem__(200, complex(np.inf, 0.0))),
                           ("-inf twice", lambda z: z.__setitem__(slice(210, 212), complex(0.0, -np.inf))),
                           ("an exact tie", lambda z: z.__setitem__(slice(0, rows, 7), 9.0 + 0j))):
            z = base.copy()
            edit(z)
            with np.errstate(all="ignore"):
                want = R.measure(z, plist, max_negatives=16)
            for t in (0, 2, 3):
                tier(m, t)
                agree("cf32", m.measure(to_device(torch, z), plist), want, (name, t))
            if name == "nan everywhere":
                assert (want[0]["peak_index"] == R.NONE).all() and (want[0]["peak_power"] == 0).all()
            if name == "an exact tie":
                assert want[0]["peak_index"].tolist() == [0, 5, 0, 0] and want[0]["peak_power"][0] == 81.0


# -- negatives ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt,bw", FORMATS)
def test_the_list_of_negatives_at_its_limits(torch, fmt, bw):
    rows = 3 * MC.PART + 100
    amp = 100.0 if fmt == "int8" else 1000.0
    four = [50, 200, 333, 1000]
    x = MC.carrier(fmt, rows, four + [1199], amp)           # pulse [0, 1200): 4 pairs and the single negative of a flip at the end
    edges = [MC.PART + 1, 2 * MC.PART + 1, 3 * MC.PART + 1]  # negatives on both sides of every part boundary
    y = MC.carrier(fmt, rows, edges, amp)
    dx, dy = to_device(torch, x), to_device(torch, y)
    plist = R.pulses([0, 0, 0], [1100, 1200, 40])
    want = R.measure(x, plist, max_negatives=8)
    assert want[0]["neg_count"].tolist() == [8, 9, 0] and want[0]["flags"].tolist() == [0, R.NEGS_CLIPPED, 0]
    assert want[1][0].tolist() == [48, 49, 198, 199, 331, 332, 998, 999] and want[0]["last_neg"][1] == 1197
    whole = R.pulses([0], [rows])
    split = R.measure(y, whole, max_negatives=128)
    assert split[1][0][:6].tolist() == [MC.PART - 1, MC.PART, 2 * MC.PART - 1, 2 * MC.PART, 3 * MC.PART - 1, 3 * MC.PART]
    with PulseModulation(fmt, bw, 0, 8) as m:
        for t in (0, 1, 2, 3):
            tier(m, t)
            agree(fmt, m.measure(dx, plist), want, t)
    with PulseModulation(fmt, bw, 0, 128) as m:
        for t in (1, 2, 3):
            tier(m, t)
            agree(fmt, m.measure(dy, whole), split, t)
    with PulseModulation(fmt, bw, 0, 2) as m:              # each part lists its first two: the join takes them in part order
        tier(m, 3)
        agree(fmt, m.measure(dy, whole), R.measure(y, whole, max_negatives=2), "two of six")
    # max_negatives = 0 with and without a pointer; max_negatives > 0 without one
    d_list = list_on_device(torch, plist)
    for maxneg in (0, 8):
        want = R.measure(x, plist, max_negatives=maxneg)
        with PulseModulation(fmt, bw, 0, maxneg) as m:
            if maxneg == 0:
                agree(fmt, m.measure(dx, plist), want)
            for negs in (None, torch.full((3, 8), 0x5A5A5A5A, dtype=torch.int32, device="cuda")):
                rec = torch.zeros((3, 96), dtype=torch.uint8, device="cuda")
                L.check(m._lib.pfb_mop_measure(m._h, C.c_void_p(dx.data_ptr()), rows, 1, 0, L.PFB_MEM_DEVICE,
                                               C.c_void_p(d_list.data_ptr()), 3, L.PFB_MEM_DEVICE, C.c_void_p(rec.data_ptr()),
                                               C.c_void_p(negs.data_ptr()) if negs is not None else None), "pfb_mop_measure")
                got = pm.records_to_numpy(rec)
                assert MC.same_exact(got, want[0]) and (fmt == "cf32" or got.tobytes() == want[0].tobytes())
                if negs is not None and maxneg == 0:
                    assert (negs == 0x5A5A5A5A).all()        # nothing is written


# -- cf32 with a pitch -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ld", [3, 56, 64])
def test_columns_of_a_matrix_where_they_lie(torch, ld):
    rows = 2 * MC.PART + 300
    z = MC.random_series("cf32", rows, 80 + ld, ld=ld)
    dz = to_device(torch, z)
    lengths = [5, 300, 700, 2 * MC.PART + 7]
    with PulseModulation("cf32", 0, 2, 16) as m:
        for col in (0, 1, ld - 1):
            plist = MC.spread(lengths, rows, 81 + col)
            plist["column"] = col
            want = R.measure(z, plist, trim=2, max_negatives=16)
            alone = np.ascontiguousarray(z[:, col])
            flat = R.measure(alone, R.pulses(plist["start"], plist["length"]), trim=2, max_negatives=16)
            for name in R.SUMS + ("peak_power", "n", "neg_count", "peak_index"):
                assert np.array_equal(want[0][name], flat[0][name])
            for t in (0, 3):
                tier(m, t)
                first = as_numpy(*m.measure(dz, plist))
                agree("cf32", first, want, (ld, col, t))
                again = as_numpy(*m.measure(dz, plist))
                assert first[0].tobytes() == again[0].tobytes() and first[1].tobytes() == again[1].tobytes()
                # the column copied out, measured as a stream: the same kernel in the same order, the same bytes
                copied = as_numpy(*m.measure(to_device(torch, alone), R.pulses(plist["start"], plist["length"])))
                for name in R.SUMS + ("peak_power",):
                    assert copied[0][name].tobytes() == first[0][name].tobytes(), (name, ld, col, t)
            agree("cf32", m.measure(z, plist), want, (ld, col, "host route"))


# -- routes ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt,bw", FORMATS)
def test_host_and_device_routes_give_the_same_bytes(torch, fmt, bw):
    rows = 40000
    x = MC.random_series(fmt, rows, 91)
    dx = to_device(torch, x)
    lengths = [1000, 24, 0, 1000, 1000, 3, 3000, 1000, 1000, 1, 600, 600, 2500, 8]
    plist = MC.spread(lengths, rows, 92)
    plist["start"][-1] = rows                                # outside: it takes no room in a batch
    want = R.measure(x, plist, trim=1, max_negatives=6)
    bps = 2 if fmt == "int8" else 4 if fmt == "int16" else 8
    with PulseModulation(fmt, bw, 1, 6) as m:
        device = as_numpy(*m.measure(dx, plist))
        agree(fmt, device, want, "device route")
        d_list = list_on_device(torch, plist)
        for chunk in (0, 2000 * bps, 998 * bps, 1):           # the default, batches of two pulses, of one, of one at most
            tier(m, 0, stage_bytes=chunk)
            for what, a, b in (("host, host", x, plist), ("host, device list", x, d_list), ("device, host list", dx, plist)):
                got = as_numpy(*m.measure(a, b))
                agree(fmt, got, want, (what, chunk))
                assert got[0].tobytes() == device[0].tobytes() and got[1].tobytes() == device[1].tobytes(), (what, chunk)


def test_async_calls_across_a_stream_switch(torch):
    rows = 30000
    x = MC.random_series("int16", rows, 95)
    dx = to_device(torch, x)
    lists = [MC.spread([700, 5, 64, 2000, 0, 300], rows, 96 + k) for k in range(4)]
    wants = [R.measure(x, p, max_negatives=4) for p in lists]
    d_lists = [list_on_device(torch, p) for p in lists]
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    with PulseModulation("int16", 12, 0, 4) as m:
        outs = []
        for k, d in enumerate(d_lists):
            m.set_stream((s1 if k % 2 == 0 else s2).cuda_stream)
            outs.append(m.measure_async(dx, d))
            assert m.last_kernel == "mop_wave+mop_group"     # the async form does not read which tiers have work
        m.sync()
        torch.cuda.synchronize()
        for got, want in zip(outs, wants):
            agree("int16", got, want)
        m.set_stream(0)
        tier(m, 3)                                           # forced, the async form splits as well
        got = m.measure_async(dx, d_lists[0])
        m.sync()
        agree("int16", got, wants[0])
        assert m.last_kernel == "mop_split+mop_join"
        with pytest.raises(TypeError):
            m.measure_async(x, d_lists[0])


# -- the chain ---------------------------------------------------------------------------------------------------------
def train_settings(kind, **over):
    kw = dict(sample_format="int16", bit_width=12, fs=MC.FS, f0=3e6, pri=4000, first_pulse=700, amplitude=0.5,
              noise_sigma=MC.CHAIN_SIGMA, seed=3)
    kw.update(dict(pw=1000, lfm_extent_hz=40e6) if kind == "lfm" else dict(pw=1001, barker13=True, barker_degrees=True))
    kw.update(over)
    return kw


def train(kind, pulses=6, **over):
    kw = train_settings(kind, **over)
    with PulseTrain(**kw) as pt:
        return pt.generate(700 + pulses * int(kw["pri"]))


def test_the_chain_reads_a_chirp(torch):
    """PulseTrain LFM (40 MHz over 1000 samples) at the CPU chain's noise -> extract_pdws_raw -> measure_pdws ->
    modulation_figures: the sweep and the mid frequency within the CPU table's tolerances (mop_cases), kind LFM; the
    replica made from the untrimmed measurement puts every pulse's matched-filter peak on its first sample, which the
    restatement's replica does through the float64 matched filter (mf_ref): asserted here first, and on the oracle's
    PDWs in test_mop_cpu.py::test_the_chain_on_the_restatement."""
    iq = train("lfm")
    pdws = extract_pdws_raw(iq, MC.FS, 1e9, 1000.0, bit_width=12, snr_threshold_db=MC.CHAIN_SNR_DB)
    assert len(pdws) == 6
    rec, negs = measure_pdws(iq, pdws, MC.FS, 1000.0, trim=8)
    # the reference first: the restatement on the same samples and pulses
    x = iq.cpu().numpy()
    want = R.measure(x, pm.pulses_from_pdws(pdws, MC.FS, 1000.0), trim=8, max_negatives=32)
    for f in R.figures(want[0], MC.FS):
        assert f[5] == 1
    agree("int16", (rec, negs), want)
    fig = modulation_figures(rec, MC.FS)
    for r, f in zip(rec, fig):
        assert abs(f["extent_hz"] - 40e6 * (int(r["n"]) - 1) / 999) <= MC.EXTENT_TOL_LFM40 and pm.KINDS[f["kind"]] == "lfm"
        assert abs(f["freq_hz"] - 23e6) <= MC.FREQ_TOL_LFM40       # the mid frequency: 3 MHz + half the sweep
    # the replica, the reference first: mop_ref's records at trim 0 -> replica -> mf_ref, the exact first samples
    want0 = R.measure(x, pm.pulses_from_pdws(pdws, MC.FS, 1000.0), max_negatives=32)
    assert MC.replica_peak_offsets(x, replica_from_measurement(want0[0], want0[1], MC.FS, 12)) == [0] * 6
    rec0, negs0 = measure_pdws(iq, pdws, MC.FS, 1000.0)
    agree("int16", (rec0, negs0), want0)
    replica = replica_from_measurement(rec0, negs0, MC.FS, 12)
    assert replica.dtype == np.complex64 and len(replica) == 1000 and abs(abs(replica[0]) - 0.5) < 0.01
    with MatchedFilter(replica, "int16", 12, "power") as mf:
        y = mf.process(iq).cpu().numpy()
    for k in range(6):
        lo = 700 + 4000 * k - 200
        assert int(np.argmax(y[lo:lo + 400])) == 200, k


def test_the_chain_reads_a_barker_code(torch):
    """the same for a Barker-13 train: 6 flips, chips of n / 13 samples, the Barker signs up to a global sign, and the
    replica's matched-filter peaks on the pulses' first samples -- each asserted on the restatement first (the replica
    through mf_ref), then on the device"""
    iq = train("barker")
    pdws = extract_pdws_raw(iq, MC.FS, 1e9, 1000.0, bit_width=12, snr_threshold_db=MC.CHAIN_SNR_DB)
    assert len(pdws) == 6
    rec, negs = measure_pdws(iq, pdws, MC.FS, 1000.0)
    want = R.measure(iq.cpu().numpy(), pm.pulses_from_pdws(pdws, MC.FS, 1000.0), max_negatives=32)
    for r, q in zip(want[0], want[1]):                           # the reference first
        chip, signs = phase_code(q, int(r["n"]))
        assert r["neg_count"] == 12 and abs(chip - 77.0) <= 0.5 and (signs * signs[0]).tolist() == list(S.BARKER_13)
    assert MC.replica_peak_offsets(iq.cpu().numpy(), replica_from_measurement(want[0], want[1], MC.FS, 12)) == [0] * 6
    agree("int16", (rec, negs), want)
    fig = modulation_figures(rec, MC.FS)
    for r, f, q in zip(rec, fig, negs):
        assert f["flips"] == 6.0 and pm.KINDS[f["kind"]] == "phase coded"
        chip, signs = phase_code(q, int(r["n"]))
        assert abs(chip - int(r["n"]) / 13) <= 0.5 and (signs * signs[0]).tolist() == list(S.BARKER_13)
    replica = replica_from_measurement(rec, negs, MC.FS, 12)
    with MatchedFilter(replica, "int16", 12, "power") as mf:
        y = mf.process(iq).cpu().numpy()
    for k in range(6):
        lo = 700 + 4000 * k - 200
        assert int(np.argmax(y[lo:lo + 400])) == 200, k


def test_a_record_on_disk(torch, tmp_path):
    """modulation_from_iq_file: the raw extraction of the record, then the host route, against the restatement on the
    record's samples and the pulses of its PDWs"""
    path = str(tmp_path / "train.iq")
    n = 700 + 6 * 4000
    with PulseTrain(**train_settings("lfm")) as pt:
        pt.write_iq(path, n)
        x = pt.generate(n).cpu().numpy()
    pdws, rec, negs, fig, record = modulation_from_iq_file(path, snr_threshold_db=MC.CHAIN_SNR_DB, trim=8, max_negatives=4)
    assert len(pdws) == 6 and record.iq.shape == (n, 2) and record.fs == MC.FS and np.array_equal(record.iq, x)
    want = R.measure(x, pm.pulses_from_pdws(pdws, MC.FS, record.sampleStartTime), trim=8, max_negatives=4)
    agree("int16", (rec, negs), want)
    assert (fig["kind"] == L.PFB_MOP_KIND_LFM).all() and (np.abs(fig["extent_hz"] - 40e6 * 983 / 999) <= MC.EXTENT_TOL_LFM40).all()


def test_two_emitters_on_one_grid_are_told_apart_by_their_inside(torch):
    """a chirped and a plain train with the same PRI of 8000 samples, half a PRI apart (the extractor's noise floor is
    a median: it wants the pulses to fill less than half the record), each with half the chain's noise power, twelve
    pulses each, all of them whole inside the record: 24 PDWs, one train of half the period to the deinterleaver, two
    kinds to modulation_figures"""
    n_pulses = 12
    both = dict(pri=8000, noise_sigma=MC.CHAIN_SIGMA / 2 ** 0.5)
    iq = train("lfm", n_pulses, seed=5, **both) + train("lfm", n_pulses, seed=6, lfm_extent_hz=0.0, first_pulse=4700, **both)
    pdws = extract_pdws_raw(iq, MC.FS, 1e9, 0.0, bit_width=12, snr_threshold_db=MC.CHAIN_SNR_DB)
    assert len(pdws) == 2 * n_pulses
    pulses = pm.pulses_from_pdws(pdws, MC.FS, 0.0)
    ticks = np.ascontiguousarray(pulses["start"], np.uint64)
    emitters, labels = deinterleave(ticks, 1000, 6000, 4, min_pulses=8)
    assert len(emitters) == 1 and abs(emitters[0]["period"] - 4000) < 1 and (labels == 0).all()
    rec, _ = measure_pulses(iq, pulses, trim=8)
    kinds = modulation_figures(rec, MC.FS)["kind"]
    chirped = (pulses["start"].astype(np.int64) - 700) % 8000 < 10
    assert chirped.sum() == n_pulses and (~chirped).sum() == n_pulses
    assert (kinds[chirped] == L.PFB_MOP_KIND_LFM).all() and (kinds[~chirped] == L.PFB_MOP_KIND_UNMODULATED).all()
