"""The trace / envelope unit on the MI355X where tests/test_gpu_trace.py does not reach: the full-rate kernel over more
than one pass of its capped grid; host-pointer calls of three and more staging steps, with steps bound by the records
and by the input, through the handle, the file reader and both full-rate outputs; calls queued behind one another
without a sync, across a stream switch with a bin open, a host-pointer call in the middle and a partials scratch that
grows on the way; cf32 under random cuttings and the same cutting twice; cf32 samples that are not finite; bit widths
1, 5 and 9 with samples wider than the width; bins of 67 partials on designed data; cf32 at 2^40 and 2^-40.  Everything
against tests/trace_ref.py with the tolerances of test_gpu_trace.py: integer records bit for bit, cf32 power_mean to
count * 2^-52, mag to 1 float32 ulp, phase to trace_ref.PHASE_TOL_DEG."""
import ctypes as C
import os
import time

import numpy as np
import pytest

import trace_ref as R
from gpu_support import Busy, cuda_torch
from sdr_channelizer_amd import _lib as L
from sdr_channelizer_amd import Trace, iqfile, trace
from trace_support import MEAN, GuardedFloats, Slots, note_mean, same, stream

pytestmark = pytest.mark.gpu
T = trace.TILE
S1 = (64 << 20) // 48                    # records per staging step when the records bind
LONGEST = 12 * 70001 + 40000             # the shared device streams: what the queued calls need at B = 70 001
FULL_RATE = {}                           # label -> (largest mag error in float32 ulp, largest phase error in degrees)
SECONDS = {}                             # host-staging tests: the call's own wall time


@pytest.fixture(scope="module")
def torch():
    t = cuda_torch()
    yield t
    # DESIGN.md section 14 quotes these
    for label, (ulp, deg) in FULL_RATE.items():
        print(f"\ntrace reach full-rate {label}: mag {ulp:.3f} ulp, phase {deg:.3e} deg (bound {R.PHASE_TOL_DEG:.3e})", end="")
    for label, frac in MEAN.items():
        print(f"\ntrace reach cf32 mean {label}: {frac:.4f} of the allowance", end="")
    for label, s in SECONDS.items():
        print(f"\ntrace reach host staging {label}: {s:.2f} s in the call", end="")
    print()


@pytest.fixture(scope="module")
def busy(torch):
    b = Busy(torch)
    yield b
    del b.src, b.dst
    torch.cuda.empty_cache()


def bytes_equal(got, want):
    got, want = trace.as_records(got), np.asarray(want)
    return got.shape == want.shape and got.tobytes() == want.tobytes()


def check_full_rate(label, mag, ph, m64, p64):
    err = float((np.abs(mag.astype(np.float64) - m64) / R.ulp32(m64)).max())
    deg = float(R.phase_diff(ph, p64).max())
    old = FULL_RATE.get(label, (0.0, 0.0))
    FULL_RATE[label] = (max(old[0], err), max(old[1], deg))
    print(f"{label}: mag {err:.3f} ulp, phase {deg:.3e} deg (bound {R.PHASE_TOL_DEG:.3e})")
    assert err <= 1.0, (label, err)
    assert deg <= R.PHASE_TOL_DEG, (label, deg)


def samples_into(tr, src, n, mag, ph):
    L.check(tr._lib.pfb_trace_samples(tr._h, C.c_void_p(src.data_ptr()), n, C.c_void_p(mag.ptr()) if mag else None,
                                      C.c_void_p(ph.ptr()) if ph else None, L.PFB_MEM_DEVICE), "pfb_trace_samples")


# ---- T1. the grid-stride loop of trace_samples_kernel ---------------------------------------------------------------

@pytest.mark.parametrize("fmt,bw", R.FORMATS)
def test_full_rate_trace_over_several_grid_passes(torch, fmt, bw):
    """Two whole passes of the capped grid, half a workgroup of a third and a scalar tail; from an aligned pointer into
    aligned outputs and from one sample in (a scalar head) into outputs one float past a 16-byte boundary."""
    cus = torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count
    pass_, n = R.grid_pass(fmt, cus)
    assert n > pass_                                  # more compute units: still more than one pass
    iq = R.phase_inputs(fmt, bw, n + 1, seed=21)
    d = torch.from_numpy(iq).cuda()
    assert d.data_ptr() % 16 == 0
    m64, p64 = R.mag_phase64(iq, fmt, bw)
    with Trace(64, fmt, bw) as tr:
        for off, lead in ((0, 4), (1, 5)):
            src = d[off:off + n]
            assert (src.data_ptr() % 16 == 0) == (off == 0)
            mag, ph, only = (GuardedFloats(torch, n, lead) for _ in range(3))
            assert mag.ptr() % 16 == ph.ptr() % 16 == (0 if off == 0 else 4)
            samples_into(tr, src, n, mag, ph)
            samples_into(tr, src, n, only, None)
            m, p = mag.values(), ph.values()          # the guards are checked here
            check_full_rate(f"{fmt}/{bw}", m, p, m64[off:off + n], p64[off:off + n])
            assert np.array_equal(only.values().view(np.uint32), m.view(np.uint32)), off


# ---- T2. host staging: three and more steps, steps bound by the records --------------------------------------------

_host = {}


def record_bound_samples():
    """int8, B = 1: the samples of the handle's and of the file's four-step call, and their records, made once"""
    if "a" not in _host:
        n = 3 * S1 + 17
        iq = np.random.default_rng(31).integers(-128, 128, size=(n, 2), dtype=np.int8)
        _host["a"] = (iq, R.envelope_fast(iq, "int8", 8, 1))
    return _host["a"]


def timed(label, call):
    t0 = time.perf_counter()
    got = call()
    SECONDS[label] = time.perf_counter() - t0
    print(f"{label}: {SECONDS[label]:.2f} s")
    return got


def test_host_steps_bound_by_the_records(torch):
    """B = 1 on host pointers: four steps of 64 MiB / 48 records each, both staging pairs used twice"""
    iq, want = record_bound_samples()
    assert len(iq) == 3 * S1 + 17 and S1 == 1398101 and S1 * 2 < 64 << 20    # the records bind, not the input
    with Trace(1, "int8", 8) as tr:
        got = timed("a: int8 B=1", lambda: tr.envelope(iq))
        assert tr.flush().size == 0
    assert bytes_equal(got, want)


def test_host_steps_of_whole_bins_leave_an_open_bin(torch):
    """B = 7: a step is 7 * (64 MiB / 48) samples, a multiple of B; the last step leaves three samples open"""
    n = 2 * 7 * S1 + 38
    iq = np.random.default_rng(32).integers(-128, 128, size=(n, 2), dtype=np.int8)
    with Trace(7, "int8", 8) as tr:
        got = timed("b: int8 B=7", lambda: tr.envelope(iq))
        last = tr.flush()
    assert got.size == n // 7 and last.size == 1 and last["count"][0] == n % 7 == 3
    assert bytes_equal(np.concatenate([got, last]), R.envelope_fast(iq, "int8", 8, 7))


def test_host_steps_that_cut_every_bin_they_end_in(torch):
    """cf32, B = 4099 (two partials per bin): steps of 2^23 samples bound by the input, none a multiple of B, so each
    step reads the carry record and writes the other one"""
    B, step = 4099, 1 << 23
    n = 2 * step + 3 * B + 5
    assert step == (64 << 20) // 8 and step % B and (2 * step) % B and n % B
    iq = R.random_iq("cf32", 12, n, seed=33)
    want = R.envelope_fast(iq, "cf32", 12, B)
    with Trace(B, "cf32", 12) as tr:
        got = timed("c: cf32 B=4099", lambda: tr.envelope(iq))
        got = np.concatenate([got, tr.flush()])
    note_mean("T2c host steps, B = 4099", got, want)
    assert same(got, want, "cf32")


def test_file_reader_steps_bound_by_the_records(torch, tmp_path):
    """the samples of the B = 1 call as an int8 record, max_bins = n: the reader's steps are bound by the records too"""
    iq, want = record_bound_samples()
    n = len(iq)
    path = os.path.join(tmp_path, "one_per_bin.iq")
    iqfile.write_iq(path, iq, 56e6, 0.0, 8)
    recs = np.zeros(n, R.BIN_DTYPE)
    f, b = C.c_uint64(), C.c_uint32()
    call = L.load().pfb_trace_envelope_from_iq_file
    rc = timed("d: int8 file B=1", lambda: call(path.encode(), n, C.c_void_p(recs.ctypes.data), n, C.byref(f), C.byref(b), None, -1))
    assert rc == L.PFB_OK and b.value == 1 and f.value == n
    assert bytes_equal(recs, want)


def test_full_rate_host_pointers_over_three_steps(torch):
    """pfb_trace_samples on host pointers: steps of 2^24 samples, three per output"""
    step = 1 << 24
    n = 2 * step + 4099
    iq = np.random.default_rng(34).integers(-128, 128, size=(n, 2), dtype=np.int8)
    iq[:16] = R.phase_inputs("int8", 8, 16, seed=1)
    with Trace(64, "int8", 8) as tr:
        hm, hp = timed("e: int8 full rate", lambda: tr.mag_phase(iq))
        dm, dp = tr.mag_phase(torch.from_numpy(iq).cuda())
        dm, dp = dm.cpu().numpy(), dp.cpu().numpy()
    assert hm.dtype == hp.dtype == np.float32 and hm.shape == hp.shape == (n,)
    assert np.array_equal(hm.view(np.uint32), dm.view(np.uint32)) and np.array_equal(hp.view(np.uint32), dp.view(np.uint32))
    for lo, hi in ((step - 4096, step + 4096), (2 * step - 4096, 2 * step + 4096), (n - 4099, n)):
        m64, p64 = R.mag_phase64(iq[lo:hi], "int8", 8)
        check_full_rate("int8/8 host steps", hm[lo:hi], hp[lo:hi], m64, p64)


# ---- T3. calls queued behind one another ------------------------------------------------------------------------------

@pytest.mark.parametrize("B", [5, 1000, T + 1, 70001])
@pytest.mark.parametrize("fmt,bw", R.FORMATS)
def test_calls_queued_behind_one_another(torch, busy, fmt, bw, B):
    """Ten calls on a side stream with no sync and no host read between them, behind unrelated work: the two carry
    records written in turn, a stream switch with a bin open, a host-pointer call behind the queued ones, and (B > T)
    a partials scratch that grows while earlier calls are queued."""
    n = 12 * B + 40000
    iq, d = stream(torch, fmt, bw, LONGEST)
    iq, d = iq[:n], d[:n]
    lengths = [1, 0, 3, B - 1, 2, 2 * B, 97, 5 * B + 3, 30011]
    lengths.append(n - sum(lengths))
    HOST = 6                                                   # the 97 samples go through host pointers
    starts = [int(s) for s in np.concatenate([[0], np.cumsum(lengths)])]
    counts = [(starts[k] % B + m) // B for k, m in enumerate(lengths)]
    if B > T:
        need = [R.call_segments(m, B, starts[k] % B) if m else 0 for k, m in enumerate(lengths)]
        grows = [k for k in range(len(need)) if need[k] > max([0] + need[:k])]
        assert len([k for k in grows if lengths[k] > B - 2]) >= 3, (need, grows)
    slots = Slots(torch, [0 if k == HOST else c for k, c in enumerate(counts)])
    first, second = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()                                   # the guard bytes are in place before other streams write
    with Trace(B, fmt, bw) as tr:
        tr.set_stream(first.cuda_stream)
        busy.queue(first)
        host_recs = None
        for k, m in enumerate(lengths):
            assert tr.bins_for(m) == counts[k], k
            if k == HOST:
                host_recs = tr.envelope(iq[starts[k]:starts[k] + m])
                assert host_recs.shape == (counts[k],)
            else:
                got = tr.envelope(d[starts[k]:starts[k] + m], out=slots.out(k), sync=False)
                assert got.shape == (counts[k], 48)
            if k == 2:
                assert tr.bins_for(B - 5) == 0 and tr.bins_for(B - 4) == 1      # a bin is open
                tr.set_stream(second.cuda_stream)
        tr.sync()
        last = tr.flush()
        tr.set_stream(0)
    pieces = slots.records()                                   # every slot's guards are checked here
    pieces[HOST] = host_recs
    assert [p.size for p in pieces] == counts and last.size == (1 if n % B else 0)
    assert same(np.concatenate(pieces + [last]), R.envelope_fast(iq, fmt, bw, B), fmt)


# ---- T4. cf32 under random cuttings -----------------------------------------------------------------------------------

@pytest.mark.parametrize("B", [3, 4096, 70001])
def test_cf32_under_random_cuttings(torch, B):
    """test_any_cutting_gives_the_same_bits for cf32: selections exact and the mean inside the summation bound under a
    seeded random cutting; and the same cutting from the same pointers a second time gives the same bytes."""
    fmt, bw, n = "cf32", 12, 200000
    iq, d = stream(torch, fmt, bw)
    iq, d = iq[:n], d[:n]
    want = R.envelope_fast(iq, fmt, bw, B)
    rng = np.random.default_rng(B)
    cuts, at, calls_in_bin, first = [], 0, {}, [1, 0, 1, 1, 2, 5]
    while at < n:
        m = first.pop(0) if first else int(rng.choice([0, 1, 2, 5, 97, 1023, 1024, T, T + 1, 9973, 30011]))
        m = min(m, n - at)
        cuts.append((at, m, rng.random() < 0.3, bool(rng.integers(2))))
        for b in range(at // B, (at + max(m, 1) - 1) // B + 1):
            calls_in_bin[b] = calls_in_bin.get(b, 0) + 1
        at += m
    assert max(calls_in_bin.values()) >= 3                    # a bin that straddles three calls and more
    with Trace(B, fmt, bw) as tr:
        whole = np.concatenate([trace.as_records(tr.envelope(d)), tr.flush()])
        note_mean("T4 one call", whole, want)
        assert same(whole, want, fmt)
        # reset: the origin is back at 0 and nothing is carried
        tr.envelope(d[:B + 1])
        runs = []
        for _ in range(2):
            tr.reset()
            pieces = []
            for at, m, refuse, sync in cuts:
                f = tr.bins_for(m)
                if f > 0 and refuse:                          # too little room: the number needed, and no state change
                    got = C.c_uint64()
                    rc = tr._lib.pfb_trace_envelope(tr._h, C.c_void_p(d[at:].data_ptr()), m, C.c_void_p(d.data_ptr()), f - 1,
                                                    C.byref(got), L.PFB_MEM_DEVICE)
                    assert rc == L.PFB_ERR_CAPACITY and got.value == f and tr.bins_for(m) == f
                pieces.append(trace.as_records(tr.envelope(d[at:at + m], sync=sync)))
                tr.sync()
            pieces.append(tr.flush())
            runs.append(np.concatenate(pieces))
        note_mean("T4 random cutting", runs[0], want)
        assert same(runs[0], want, fmt)
        assert runs[0].tobytes() == runs[1].tobytes()         # the same calls: the same bits, power_mean included
        # after the flush a new grid starts at the next sample, with the stream's indices going on
        again = np.concatenate([trace.as_records(tr.envelope(d[:B + 2])), tr.flush()])
        assert same(again, R.envelope_fast(iq[:B + 2], fmt, bw, B, origin=n), fmt)


# ---- T5. cf32 samples that are not finite -----------------------------------------------------------------------------

@pytest.mark.parametrize("B", [5, 300, T, 2 * T + 3, 66 * T + 3])
def test_non_finite_samples_stay_in_their_bins(torch, B):
    """A NaN, a +Inf and a -Inf (and, at B = 5, a bin of nothing but NaN) change the records of their own bins alone,
    with cuts before and after each of them and carry records that hold them; nothing is asserted of those bins."""
    fmt, bw = "cf32", 12
    n, more = 6 * B + 11, B + 2
    clean = R.random_iq(fmt, bw, n + more, seed=B)
    bad = clean.copy()
    bad[B, 0] = np.nan                                        # the first sample of bin 1
    bad[4 * B - 1, 1] = np.inf                                # the last sample of bin 3
    at_bad, cuts = [B, 4 * B - 1], {0, B, B + 1, 4 * B - 1, 4 * B, n}
    if B > T:
        bad[3 * B + T, 0] = -np.inf                           # the first sample of bin 3's second tile
        at_bad.append(3 * B + T)
        cuts |= {3 * B + T, 3 * B + T + 1}                    # the second cut leaves bin 3 open with the -Inf in the carry
    if B == 5:
        bad[20:25] = np.nan                                   # all of bin 4
        at_bad += list(range(20, 25))
        cuts |= {20, 22, 25}
    cuts = sorted(cuts)
    spoiled = R.bins_holding(at_bad, B, 0, n)
    assert spoiled.tolist() == ([1, 3, 4] if B == 5 else [1, 3])
    bins = -(-n // B)                                         # 7 with the flushed partial (9 at B = 5)
    keep = np.setdiff1d(np.arange(bins), spoiled)             # bins 0, 2, 5 and on, and 4 where B != 5
    assert {0, 2, 5, bins - 1} <= set(keep.tolist()) and (4 in keep) == (B != 5)
    assert np.isfinite(bad[:n][np.isin(np.arange(n) // B, keep)]).all()
    lengths = [b - a for a, b in zip(cuts[:-1], cuts[1:])]
    counts = [(a % B + m) // B for a, m in zip(cuts[:-1], lengths)]
    assert sum(counts) == n // B == bins - 1
    want = R.envelope_fast(clean[:n], fmt, bw, B)
    want_more = R.envelope_fast(clean[n:], fmt, bw, B, origin=n)
    d = torch.empty((n + more, 2), dtype=torch.float32, device="cuda")
    runs, traces = [], []
    with Trace(B, fmt, bw) as tr:
        for iq in (clean, bad):
            d.copy_(torch.from_numpy(iq))                     # the same pointers for both streams
            slots = Slots(torch, counts)
            tr.reset()
            for k, (a, m) in enumerate(zip(cuts[:-1], lengths)):
                assert tr.bins_for(m) == counts[k]
                tr.envelope(d[a:a + m], out=slots.out(k), sync=False)
            tr.sync()
            recs = np.concatenate(slots.records() + [tr.flush()])      # the guards are checked here
            assert recs.size == bins and recs["count"][keep].tolist() == [n % B if b == bins - 1 else B for b in keep]
            runs.append(recs)
            # a new grid behind the flush: clean samples, the stream's indices going on
            after = np.concatenate([trace.as_records(tr.envelope(d[n:])), tr.flush()])
            assert same(after, want_more, fmt)
            mag, ph = GuardedFloats(torch, n, 4), GuardedFloats(torch, n, 5)
            samples_into(tr, d[:n], n, mag, ph)
            traces.append((mag.values(), ph.values()))
    assert same(runs[0], want, fmt)
    note_mean("T5 clean run", runs[0], want)
    assert runs[0][keep].tobytes() == runs[1][keep].tobytes()
    assert same(runs[1][keep], want[keep], fmt)
    others = np.setdiff1d(np.arange(n), at_bad)
    for a, b in zip(traces[0], traces[1]):
        assert np.array_equal(a[others].view(np.uint32), b[others].view(np.uint32))


# ---- T6. bit widths, and samples wider than the width ----------------------------------------------------------------

@pytest.mark.parametrize("fmt,bw", [("int8", 1), ("int8", 5), ("int16", 1), ("int16", 9)])
def test_bit_widths_and_samples_wider_than_the_width(torch, fmt, bw):
    """p = u * 2^-(2(bit_width-1)) without clipping: data over the whole container at widths nothing else uses"""
    iq = R.wide_iq(fmt, 5 * (T + 1) + 3, seed=6)
    d = torch.from_numpy(iq).cuda()
    full = 128 if fmt == "int8" else 32768
    for B in (7, 1000, T + 1):
        n = 5 * B + 3
        with Trace(B, fmt, bw) as tr:
            got = np.concatenate([trace.as_records(tr.envelope(d[:n])), tr.flush()])
        assert bytes_equal(got, R.envelope_fast(iq[:n], fmt, bw, B)), B
        top = 2.0 * full * full * 2.0 ** (-2 * (bw - 1))       # 2^15 and 2^31 at bit_width 1
        assert got["power_max"][0] == top and got["peak_sample"][0] == 3
        assert got["peak_i"][0] == got["peak_q"][0] == -full * 2.0 ** -(bw - 1)
    n = 20003
    with Trace(64, fmt, bw) as tr:
        mag, ph = tr.mag_phase(d[:n])
    m64, p64 = R.mag_phase64(iq[:n], fmt, bw)
    check_full_rate(f"{fmt}/{bw} wide", mag.cpu().numpy(), ph.cpu().numpy(), m64, p64)


# ---- T7. deep folds on designed data ---------------------------------------------------------------------------------

@pytest.mark.parametrize("fmt,bw", [("int8", 8), ("int16", 12), ("cf32", 12)])
def test_deep_folds_on_designed_data(torch, fmt, bw):
    """Bins of 67 partials, so lanes 0 to 2 of the fold take two each: equal maxima in two partials of one lane and of
    two lanes, the minimum in a second-round partial; in one call and cut so that calls start deep inside a bin."""
    B = 66 * T + 3
    for iq, lower in zip(R.planted_fold_stream(fmt, bw, B, seed=7), (2, 10)):
        n = len(iq)
        want = R.envelope_fast(iq, fmt, bw, B)
        assert want["peak_sample"][1] == B + lower * T + 17 and want["power_min"][1] == 0
        d = torch.from_numpy(iq).cuda()
        # the third call of the cut streams starts in an open bin at its segment 65, or 64; the fourth inside bin 1
        for cutting, seg0 in (([n], None), ([T + 7, 64 * T + 1, B], 65), ([T + 7, 63 * T + 1, B], 64)):
            lengths = cutting + [n - sum(cutting)] if sum(cutting) < n else cutting
            assert seg0 is None or (sum(cutting[:2]) // T == seg0 and B < sum(cutting) < 2 * B)
            with Trace(B, fmt, bw) as tr:
                pieces, at = [], 0
                for m in lengths:
                    pieces.append(trace.as_records(tr.envelope(d[at:at + m])))
                    at += m
                pieces.append(tr.flush())
            got = np.concatenate(pieces)
            if fmt == "cf32":
                note_mean("T7 bins of 67 partials", got, want)
            assert same(got, want, fmt), (lower, cutting)


# ---- T8. cf32 away from unit scale -----------------------------------------------------------------------------------

@pytest.mark.parametrize("e", [40, -40])
def test_cf32_away_from_unit_scale(torch, e):
    """the streams times 2^40 and 2^-40: exact scalings, powers that stay normal doubles"""
    fmt, bw, scale = "cf32", 12, np.float32(2.0 ** e)
    iq = R.random_iq(fmt, bw, 6 * (T + 1) + 11, seed=8) * scale
    assert iq.dtype == np.float32
    d = torch.from_numpy(iq).cuda()
    for B in (5, T + 1):
        want = R.envelope_fast(iq, fmt, bw, B)
        with Trace(B, fmt, bw) as tr:
            got = np.concatenate([trace.as_records(tr.envelope(d)), tr.flush()])
        note_mean(f"T8 scale 2^{e}", got, want)
        assert same(got, want, fmt), B
        assert 2.0 ** (2 * e - 4) < got["power_max"].max() <= 2.0 ** (2 * e + 1)
    iq = R.phase_inputs(fmt, bw, 20003, seed=8) * scale
    with Trace(64, fmt, bw) as tr:
        mag, ph = tr.mag_phase(torch.from_numpy(iq).cuda())
    m64, p64 = R.mag_phase64(iq, fmt, bw)
    check_full_rate(f"cf32 times 2^{e}", mag.cpu().numpy(), ph.cpu().numpy(), m64, p64)
