"""Every row of the fused-kernel table under the launch a long, device-resident call gets (tuned run length, XCD remap,
whole rounds of workgroups, default-length slabs), and one row of every kernel family past 2^31 output elements.

One reference per row: the whole buffer in one call with the run length forced to two chunks, the launch
tests/test_gpu_plan_table.py holds against the oracle.  Frame f depends only on samples up to f D + offset, so a fresh
call on a prefix of the buffer must give the first rows of that reference bit for bit whatever run length, remap or
slab length the library picked for it.  Which launch each call got is what the library reports (pfb_last_launch); the
policy's arithmetic is not repeated here."""
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from plan_support import (BPS, FMT_NAME, REL_TOL, device_input, draw_bit_width, draw_switches, draw_taps,  # noqa: E402
                          family_rows, oracle_for, plan_handle)
from sdr_channelizer_amd import _lib as L  # noqa: E402

PLANS = L.fast_plans()
RUNGS = 12           # call lengths per row, geometric from a few chunks to the top
NWIN = 16            # frames per oracle window
TOP_SAMPLES = 1 << 24   # the shortest top call, in input samples: what a caller hands over as one record
ROUNDS = 3              # the top call has at least this many runs per compute unit: whole rounds of workgroups
# The schedules whose run length follows the call (shortened or evened out).  This list is the only thing the tests
# take from the policy, and only to demand more of those rows (two run lengths seen); the others must report one
# length on every rung.  Everything else -- the lengths, the remap, the slabs -- is read from pfb_last_launch.
PER_CALL_RUNS = (0, 6, 7, 11, 13)


def reached_tuned(rep, reps, d):
    """Does this call run the row's tuned length?  A reported run length is a whole number of chunks (asserted on
    every rung), so one at or above default_frames_per_block is at or above that figure rounded up to the chunk, or to
    whatever multiple of it the library rounds to.  A schedule with a fixed length reports that length on every rung:
    there the tuned length is the one the shortest rung reported."""
    if d.default_schedule in PER_CALL_RUNS:
        return rep.frames_per_block >= d.default_frames_per_block
    return rep.frames_per_block == reps[0].frames_per_block


def ragged(F, c):
    """F or the next count above it that is odd (so no multiple of 8) and no multiple of the chunk."""
    F |= 1
    while c > 1 and F % c == 0:
        F += 2
    return F


def ladder(top, c):
    lo = 4 * c + 3
    steps = [ragged(int(round(lo * (top / lo) ** (i / (RUNGS - 1)))), c) for i in range(RUNGS - 1)] + [top]
    return sorted(set(f for f in steps if f <= top))


def row_setup(row):
    d = PLANS[row]
    fmt = FMT_NAME[d.sample_format]
    rng = np.random.default_rng(52000 + row)
    bw = draw_bit_width(rng, fmt)
    h = draw_taps(rng, d.M, d.P)
    kw = draw_switches(rng, d)
    return d, fmt, bw, h, kw, rng


def window_error(oracle, iq, got, f0, d, fmt, bw, h, kw):
    """max|err| / max|want| over frames [f0, f0 + NWIN) of a frame-major result, the oracle evaluated on just the
    samples those frames depend on (from a frame whose derotation phase is zero, so local and global indices agree)."""
    M, P, D = d.M, d.P, d.D
    period = M // math.gcd(M, D)
    f_lo = max(0, f0 - (M * P + D - 1) // D - 1)
    f_lo -= f_lo % period
    seg = iq[f_lo * D:(f0 + NWIN) * D].cpu().numpy()
    want = oracle_for(oracle, seg, h, d, fmt, bw, kw)[-NWIN:]
    g = got[f0:f0 + NWIN].cpu().numpy()
    assert g.shape == want.shape
    return float(np.abs(g - want).max() / np.abs(want).max())


@pytest.mark.parametrize("row", range(len(PLANS)), ids=[d.name.decode() for d in PLANS])
def test_registered_plan_at_record_size(oracle, row):
    import torch
    d, fmt, bw, h, kw, rng = row_setup(row)
    name, M, D, c = d.name.decode(), d.M, d.D, d.chunk_frames
    bps = BPS[fmt]
    num_cus = torch.cuda.get_device_properties(0).multi_processor_count
    handles = []

    def handle(**extra):
        handles.append(plan_handle(d, fmt, bw, h, kw, **extra))
        return handles[-1]

    def call(ch, x, out):
        ch.reset()
        y = ch(x, out=out)
        assert ch.last_kernel == name, ch.last_kernel
        return y, ch.last_launch

    try:
        ch = handle()
        # -- how long must the top call be?  Ask the library: walk the ladder over zeros and read its reports, and double
        # the top until the top call runs the tuned length in three times the runs of the rung that first reported it
        # and in at least ROUNDS runs per compute unit.
        top = ragged(max(1 << 14, TOP_SAMPLES // D), c)
        zeros = scratch = None
        reps = []
        while True:
            zeros = scratch = None
            torch.cuda.empty_cache()
            n = top * D + D
            need = n * bps + 2 * top * M * 8   # the input, the reference and one output
            free = torch.cuda.mem_get_info()[0]
            if need * 1.1 > free:
                pytest.fail(f"{name}: the tuned regime needs a top call of {top} frames = {need >> 20} MiB, "
                            f"{free >> 20} MiB free; last reports {[(r.frames, r.frames_per_block, r.runs) for r in reps]}")
            zeros = torch.zeros((n, 2), dtype={"int8": torch.int8, "int16": torch.int16, "cf32": torch.float32}[fmt],
                                device="cuda")
            scratch = torch.empty(top * M, dtype=torch.complex64, device="cuda")
            lens = ladder(top, c)
            reps = [call(ch, zeros[:F * D + 1], scratch)[1] for F in lens]
            first = next((i for i, r in enumerate(reps) if reached_tuned(r, reps, d)), None)
            if (first is not None and reached_tuned(reps[-1], reps, d) and reps[-1].runs >= 3 * reps[first].runs
                    and reps[-1].runs >= ROUNDS * num_cus):
                break
            top = ragged(2 * top, c)
        zeros = None
        torch.cuda.empty_cache()

        tails = [int(rng.integers(1, D)) if D > 1 else 0 for _ in lens]
        iq = device_input(top * D + tails[-1], fmt, bw, int(rng.integers(1 << 30)))
        ref = handle()
        ref.set_option(L.PFB_OPT_FRAMES_PER_BLOCK, 2 * c)   # the shortest legal run
        want = ref(iq)
        short_rep = ref.last_launch
        assert ref.last_kernel == name and tuple(want.shape) == (top, M) and short_rep.frames_per_block == 2 * c

        # -- the ladder, frame-major at default options
        reps = []
        for F, r in zip(lens, tails):
            got, rep = call(ch, iq[:F * D + r], scratch)
            assert rep.fused == 1 and rep.frames == F and rep.by_slabs == 0 and rep.schedule == d.default_schedule, name
            assert rep.runs == -(-F // rep.frames_per_block)
            assert rep.frames_per_block % c == 0 or d.default_schedule not in PER_CALL_RUNS, (name, rep.frames_per_block)
            assert torch.equal(got, want[:F]), (name, F, rep.frames_per_block, rep.xcd_remap)
            reps.append(rep)
        print(f"{name}: top {top} frames; (frames, run length, runs, remap) = "
              f"{[(r.frames, r.frames_per_block, r.runs, r.xcd_remap) for r in reps]}")
        first = next(i for i, r in enumerate(reps) if reached_tuned(r, reps, d))
        top_rep = reps[-1]
        assert reached_tuned(top_rep, reps, d) and top_rep.runs >= 3 * reps[first].runs, name
        assert top_rep.runs >= ROUNDS * num_cus, (name, top_rep.runs, num_cus)
        if d.default_schedule in PER_CALL_RUNS:
            assert len({r.frames_per_block for r in reps}) >= 2, name
        else:
            assert len({r.frames_per_block for r in reps}) == 1, name
        # the row has the remap both on and off if the library reports it differently for the forced shortest runs
        # and for the tuned ones of the top call: then calls at default options must have seen both too
        if bool(short_rep.xcd_remap) != bool(top_rep.xcd_remap):
            assert {bool(r.xcd_remap) for r in reps} == {False, True}, name

        # -- the top call against the oracle: around the first, an interior and the last run boundary, around runs
        # 7 / 8 / 9 where the remap permutes, and on the first and last frames (got = the top call's output)
        fpb, runs = top_rep.frames_per_block, int(top_rep.runs)
        starts = {0, top - NWIN}
        for j in (1, runs // 2, runs - 1, 7, 8, 9):
            if 1 <= j < runs:
                starts.add(min(max(j * fpb - NWIN // 2, 0), top - NWIN))
        for f0 in sorted(starts):
            err = window_error(oracle, iq, got, f0, d, fmt, bw, h, kw)
            assert err < REL_TOL, (name, f0, err, fpb)

        # -- channel-major through the default route: the top and two lower rungs equal want.T, leading dimension =
        # the call's frames
        cm = handle(channel_major=True)
        cols = max(1, (1 << 27) // M)
        for i in (len(lens) - 1, len(lens) - 3, len(lens) // 2):
            F, r = lens[i], tails[i]
            got_cm, rep = call(cm, iq[:F * D + r], scratch)
            assert tuple(got_cm.shape) == (M, F) and got_cm.stride() == (F, 1)
            assert rep.by_slabs == (0 if d.channel_major_ok else 1), (name, rep.by_slabs)
            assert (rep.slab_frames > 0) == (not d.channel_major_ok)
            if i == len(lens) - 1:
                if rep.by_slabs:   # more than one slab: a later slab takes its history from the input in front of it
                    assert 0 < rep.slab_frames < F, (name, rep.slab_frames, F)
                print(f"{name}: channel-major top: slabs {rep.by_slabs}, slab frames {rep.slab_frames}, "
                      f"run length {rep.frames_per_block}, runs {rep.runs}")
            for f0 in range(0, F, cols):   # in blocks of frames: no third full-size buffer
                assert torch.equal(got_cm[:, f0:f0 + cols], want[f0:min(F, f0 + cols)].T), (name, F, f0)
        del got, got_cm, want, scratch
        torch.cuda.empty_cache()

        # -- magnitude at the top: the long runs of the magnitude schedule against the forced short runs
        mref = handle(magnitude=True)
        mref.set_option(L.PFB_OPT_FRAMES_PER_BLOCK, 2 * c)
        mag_want = mref(iq)
        mag = handle(magnitude=True)
        mag_got = mag(iq)
        assert mag.last_kernel == name and mref.last_kernel == name and mag_got.dtype == torch.float32
        rep = mag.last_launch
        assert rep.schedule == (d.magnitude_schedule if d.magnitude_schedule >= 0 else d.default_schedule), name
        print(f"{name}: magnitude top: schedule {rep.schedule}, run length {rep.frames_per_block}, runs {rep.runs}")
        assert torch.equal(mag_got, mag_want), name
        del mag_got, mag_want, iq
    finally:
        for hnd in handles:
            hnd.close()
        torch.cuda.empty_cache()


FAMILY_ROWS = family_rows(PLANS)


@pytest.mark.parametrize("row", FAMILY_ROWS, ids=[PLANS[i].name.decode() for i in FAMILY_ROWS])
def test_more_than_2_to_31_output_elements(oracle, row):
    """One device-resident call of just over 2^31 output elements (16 GiB complex; the input's byte offsets pass 2^32
    too) per kernel family -- the first row of each (default schedule, sample format, D == M) group: a 32-bit output or
    input index in any family's stores shows here.  Frame-major against the oracle around output element 2^29 (byte
    offset 2^32), element 2^31 (byte offset 2^34), the start and the end, and bit for bit against the forced-short-run
    launch; channel-major through the row's default route against the frame-major result."""
    import torch
    d, fmt, bw, h, kw, rng = row_setup(row)
    name, M, D, c = d.name.decode(), d.M, d.D, d.chunk_frames
    F = ragged((1 << 31) // M + 4 * NWIN + 64, c)
    assert F * M > (1 << 31) + NWIN * M
    n = F * D + (int(rng.integers(1, D)) if D > 1 else 0)
    need = n * BPS[fmt] + 2 * F * M * 8
    if torch.cuda.mem_get_info()[0] < need * 1.3:
        pytest.skip(f"needs {need >> 30} GiB of HBM")
    handles = []
    try:
        iq = device_input(n, fmt, bw, int(rng.integers(1 << 30)))
        nbytes = iq.numel() * iq.element_size()
        if D * BPS[fmt] >= 2 * M:   # two input bytes or more per output element
            assert nbytes > (1 << 32), (name, nbytes)
        else:
            assert nbytes > (1 << 31), (f"{name}: 2^31 outputs of a row with D = {D}, M = {M} at {BPS[fmt]} bytes a sample "
                                        f"take {nbytes} input bytes, short of 2^32: only its output offsets cross", nbytes)
        ch = plan_handle(d, fmt, bw, h, kw)
        handles.append(ch)
        y = ch(iq)
        rep = ch.last_launch
        assert ch.last_kernel == name and tuple(y.shape) == (F, M) and rep.frames == F
        print(f"{name}: {F} frames, run length {rep.frames_per_block}, runs {rep.runs}, remap {rep.xcd_remap}")
        rows = max(1, (1 << 27) // M)
        for f0 in range(0, F, rows):
            assert bool(torch.isfinite(torch.view_as_real(y[f0:f0 + rows])).all()), (name, f0)
        marks = {0, F - NWIN}
        for elem in (1 << 29, 1 << 31):
            marks.add(elem // M - NWIN // 2)
        for f0 in sorted(marks):
            err = window_error(oracle, iq, y, f0, d, fmt, bw, h, kw)
            assert err < REL_TOL, (name, f0, err)

        ref = plan_handle(d, fmt, bw, h, kw)
        handles.append(ref)
        ref.set_option(L.PFB_OPT_FRAMES_PER_BLOCK, 2 * c)
        other = ref(iq)
        assert ref.last_kernel == name
        for f0 in range(0, F, rows):
            assert torch.equal(y[f0:f0 + rows], other[f0:f0 + rows]), (name, f0)

        cm = plan_handle(d, fmt, bw, h, kw, channel_major=True)
        handles.append(cm)
        y_cm = cm(iq, out=other.reshape(-1))
        rep = cm.last_launch
        assert cm.last_kernel == name and tuple(y_cm.shape) == (M, F)
        assert rep.by_slabs == (0 if d.channel_major_ok else 1), name
        print(f"{name}: channel-major: slabs {rep.by_slabs}, slab frames {rep.slab_frames}, runs {rep.runs}")
        for f0 in range(0, F, rows):
            assert torch.equal(y_cm[:, f0:f0 + rows], y[f0:f0 + rows].T), (name, f0)
        del y, other, y_cm, iq
    finally:
        for hnd in handles:
            hnd.close()
        torch.cuda.empty_cache()
