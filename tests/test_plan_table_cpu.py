"""The fused-kernel table as the library lists it (pfb_fast_plan_count / pfb_fast_plan_info, host only): every row is
what its name says, the variants of a shape are numbered the way PFB_OPT_VARIANT counts them, every shape is fuzzed,
and the channel-major route of every plan is the one DESIGN.md names.  No GPU needed."""
import json
import os
import re

import pytest

from plan_support import FMT, SCHEDULES, SHAPES, sweep_lengths, top_frames, walk_lengths
from sdr_channelizer_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME_RE = re.compile(r"pfb_fast<M(\d+),P(\d+),D(\d+),(int8|int16|cf32)(?:,(\w+))?>")
# the plans a channel-major handle runs by frame-major slabs + the transpose kernel (kChannelMajorOk next to launch_fast in pfb_fast.hpp):
# the 16-wave plans and the three-pass plans on chunks of 4 or 2 frames, whose fused stores would be 32- / 16-byte runs
SLAB_PLANS = {
    "pfb_fast<M1024,P16,D1024,int16>", "pfb_fast<M1024,P16,D1024,int16,16w>",
    "pfb_fast<M1024,P16,D1024,cf32>", "pfb_fast<M1024,P16,D1024,cf32,16w>",
    "pfb_fast<M560,P12,D560,int16>", "pfb_fast<M560,P12,D560,int16,4f>",
    "pfb_fast<M560,P12,D560,int8>", "pfb_fast<M560,P12,D560,int8,4f>", "pfb_fast<M560,P12,D560,cf32>",
    "pfb_fast<M250,P12,D250,int16>", "pfb_fast<M250,P12,D250,int16,lockstep>",
    "pfb_fast<M500,P12,D500,int16>", "pfb_fast<M500,P12,D500,int16,lockstep>",
}


@pytest.fixture(scope="module")
def plans():
    return L.fast_plans()


def shape_of(d):
    return (d.M, d.P, d.D, d.sample_format)


def test_table_size(plans):
    shapes = {shape_of(d) for d in plans}
    print(f"{len(plans)} rows, {len(shapes)} shapes")
    assert len(plans) == 58 and len(shapes) == 46
    with open(os.path.join(ROOT, "README.md")) as f:
        assert "46 band-count / format combinations" in f.read()   # README's count of fused (M, P, D, format) shapes


def test_info_rejects_bad_arguments():
    lib = L.load()
    d = L.PfbFastPlanDesc()
    n = lib.pfb_fast_plan_count()
    assert lib.pfb_fast_plan_info(n, L.C.byref(d)) == L.PFB_ERR_BAD_ARG
    assert lib.pfb_fast_plan_info(-1, L.C.byref(d)) == L.PFB_ERR_BAD_ARG
    assert lib.pfb_fast_plan_info(0, None) == L.PFB_ERR_BAD_ARG
    assert lib.pfb_fast_plan_info(n - 1, L.C.byref(d)) == L.PFB_OK


def test_names_parse_back_to_their_own_shape(plans):
    names = [d.name.decode() for d in plans]
    assert len(set(names)) == len(names), "two rows report the same pfb_last_kernel name"
    for d, name in zip(plans, names):
        m = NAME_RE.fullmatch(name)
        assert m, name
        assert (int(m[1]), int(m[2]), int(m[3]), FMT[m[4]]) == shape_of(d), name
        # the default plan of a shape carries no suffix, the variants do
        assert (m[5] is None) == (d.variant == 0), name


def test_variants_count_rows_of_a_shape_in_table_order(plans):
    seen = {}
    for d in plans:
        k = shape_of(d)
        assert d.variant == seen.get(k, 0), d.name
        seen[k] = d.variant + 1


def test_schedules_and_chunks(plans):
    for d in plans:
        assert d.default_schedule in SCHEDULES and d.default_schedule >= 0, d.name
        assert d.magnitude_schedule == -1 or d.magnitude_schedule in SCHEDULES[1:], d.name
        assert d.chunk_frames >= 1 and d.channel_major_ok in (0, 1), d.name


def test_run_lengths_and_workgroup_sizes(plans):
    """default_frames_per_block and threads, appended to the descriptor: what the launch policy tunes a long call to.
    Pinned for the rows the README quotes rates for; sane for every row."""
    for d in plans:
        assert d.default_frames_per_block >= 2 * d.chunk_frames, d.name
        assert d.threads >= 64 and d.threads % 64 == 0 and d.threads <= 1024, d.name
    by_name = {d.name.decode(): (d.default_schedule, d.chunk_frames, d.default_frames_per_block, d.threads) for d in plans}
    assert by_name["pfb_fast<M64,P12,D64,int16>"] == (4, 8, 512, 64)
    assert by_name["pfb_fast<M64,P12,D64,int8>"] == (7, 8, 256, 64)
    assert by_name["pfb_fast<M128,P12,D64,int16>"] == (11, 8, 32, 64)
    assert by_name["pfb_fast<M256,P8,D256,int8>"] == (0, 4, 32, 64)
    assert by_name["pfb_fast<M1024,P16,D1024,int16>"] == (6, 4, 512, 512)
    assert by_name["pfb_fast<M1024,P16,D1024,int16,16w>"] == (0, 8, 256, 1024)
    assert by_name["pfb_fast<M1024,P16,D1024,int16,duo>"] == (13, 8, 256, 256)
    assert by_name["pfb_fast<M560,P12,D560,int8>"] == (6, 2, 512, 320)
    assert by_name["pfb_fast<M560,P12,D560,int16,9w>"] == (0, 7, 252, 576)
    assert by_name["pfb_fast<M8,P12,D8,cf32>"] == (0, 64, 1024, 64)
    # the struct grew at its end only: the fields in front keep their offsets
    offs = [getattr(L.PfbFastPlanDesc, f).offset for f, _ in L.PfbFastPlanDesc._fields_]
    assert offs == sorted(offs) and [f for f, _ in L.PfbFastPlanDesc._fields_][-2:] == ["default_frames_per_block", "threads"]
    assert L.PfbFastPlanDesc.channel_major_ok.offset == 44 and L.C.sizeof(L.PfbFastPlanDesc) == 56


def test_launch_report_needs_a_handle():
    """pfb_last_launch is host only: no handle (there is none without a device) or no destination is an argument error,
    and the mirror of the struct has the header's layout.  (That a new handle reports all zeros, and what it reports
    after a launch, is checked on the GPU: tests/test_gpu_async.py, tests/test_gpu_plan_at_size.py.)"""
    lib = L.load()
    rep = L.PfbLaunchReport()
    assert lib.pfb_last_launch(None, L.C.byref(rep)) == L.PFB_ERR_BAD_ARG
    assert lib.pfb_last_launch(None, None) == L.PFB_ERR_BAD_ARG
    assert L.C.sizeof(L.PfbLaunchReport) == 48 and L.PfbLaunchReport.frames.offset == 24


def test_launch_policy_gives_the_recorded_launches(plans):
    """tests/golden/launch_policy.json: what pfb_last_launch reported on an MI355X (its CU count is in the file) for
    every row of the table, at the commit named in the file -- the last one whose launch_frames decided the launch in
    its own body -- over default and forced options at call lengths from one frame to past eight tuned runs per CU.
    pfb_plan_launch, the function launch_frames now calls, gives every one of those reports field by field; and the
    recording leaves out no row, none of a row's schedules and neither channel-major route."""
    with open(os.path.join(ROOT, "tests", "golden", "launch_policy.json")) as f:
        gold = json.load(f)
    req_fields, rep_fields = gold["request"], gold["report"]
    assert req_fields == ["schedule", "frames_per_block", "xcd_remap", "slab_frames", "channel_major", "magnitude"]
    assert rep_fields == ["fused", "schedule", "frames_per_block", "xcd_remap", "by_slabs", "frames", "runs", "slab_frames"]
    assert len(gold["parent"]) == 40 and gold["num_cus"] > 0
    index = {d.name.decode(): i for i, d in enumerate(plans)}
    assert set(gold["rows"]) == set(index)
    nreq, played, entries = len(req_fields), set(), 0
    for name, rows in gold["rows"].items():
        d, seen, slabs = plans[index[name]], set(), set()
        for e in rows:
            assert len(e) == nreq + 1 + len(rep_fields), name
            req, frames, want = dict(zip(req_fields, e[:nreq])), e[nreq], dict(zip(rep_fields, e[nreq + 1:]))
            rep = L.plan_launch(index[name], frames, gold["num_cus"], **req)
            assert {f: getattr(rep, f) for f in rep_fields} == want and rep.reserved == 0, (name, req, frames)
            assert want["fused"] == 1 and want["frames"] == frames, (name, req, frames)
            seen.add(want["schedule"])
            slabs.add(want["by_slabs"])
            played.add(req["schedule"])
        entries += len(rows)
        # the row's own schedules, every schedule a frame-major handle can be forced to, and both routes
        own = {d.default_schedule} | ({d.magnitude_schedule} if d.magnitude_schedule >= 0 else set())
        assert seen >= own | {0, 2, 3, 4, 6, 7, 11, 13}, (name, seen)
        assert seen >= ({-1, 8} if d.channel_major_ok else set()), (name, seen)   # the fused channel-major launches
        assert slabs == {0, 1}, name
    assert played == set(SCHEDULES) | {9}
    print(f"{entries} recorded launches on {gold['num_cus']} CUs at {gold['parent'][:7]}")


def test_plan_launch_rejects_bad_arguments():
    lib = L.load()
    rq = L.PfbLaunchRequest(L.C.sizeof(L.PfbLaunchRequest), -1, 0, -1, 0, 0, 256, 0)
    rep = L.PfbLaunchReport()
    n = lib.pfb_fast_plan_count()
    assert lib.pfb_plan_launch(0, None, 100, L.C.byref(rep)) == L.PFB_ERR_BAD_ARG
    assert lib.pfb_plan_launch(0, L.C.byref(rq), 100, None) == L.PFB_ERR_BAD_ARG
    assert lib.pfb_plan_launch(n, L.C.byref(rq), 100, L.C.byref(rep)) == L.PFB_ERR_BAD_ARG
    assert lib.pfb_plan_launch(-1, L.C.byref(rq), 100, L.C.byref(rep)) == L.PFB_ERR_BAD_ARG
    for size in (0, L.C.sizeof(L.PfbLaunchRequest) - 8, L.C.sizeof(L.PfbLaunchRequest) + 8):
        rq.struct_size = size
        assert lib.pfb_plan_launch(0, L.C.byref(rq), 100, L.C.byref(rep)) == L.PFB_ERR_BAD_ARG
    rq.struct_size = L.C.sizeof(L.PfbLaunchRequest)
    assert lib.pfb_plan_launch(n - 1, L.C.byref(rq), 100, L.C.byref(rep)) == L.PFB_OK
    assert rep.fused == 1 and rep.frames == 100 and rep.runs == -(-100 // rep.frames_per_block)
    assert lib.pfb_plan_launch(0, L.C.byref(rq), 0, L.C.byref(rep)) == L.PFB_OK and rep.runs == 0   # no frames, no runs
    rq.channel_major, rq.schedule = 1, 9
    assert lib.pfb_plan_launch(0, L.C.byref(rq), 0, L.C.byref(rep)) == L.PFB_OK and rep.runs == 0 and rep.by_slabs == 1
    # the mirror has the header's layout: a uint32 and six ints, then the int64 on its own 8 bytes
    assert L.C.sizeof(L.PfbLaunchRequest) == 40 and L.PfbLaunchRequest.slab_frames.offset == 32


def test_every_shape_is_fuzzed(plans):
    fuzzed = {(M, P, D, FMT[f]) for M, P, D, fmts, _ in SHAPES for f in fmts}
    missing = sorted({shape_of(d) for d in plans} - fuzzed)
    assert not missing, f"registered but not in plan_support.SHAPES: {missing}"
    extra = sorted(fuzzed - {shape_of(d) for d in plans})
    assert not extra, f"in plan_support.SHAPES without a fused plan: {extra}"


def simulate_calls(lens, D):
    """(frames, carried phase at its start) of every call and the phases left behind: the stream arithmetic of
    pfb_frames_for, frames = (phase + n) // D, phase = (phase + n) % D."""
    phase, calls, left = 0, [], set()
    for n in lens:
        assert n >= 0
        calls.append(((phase + n) // D, phase))
        phase = (phase + n) % D
        left.add(phase)
    return calls, left


def test_short_call_walk_has_no_hole(plans):
    """The call lengths tests/test_gpu_plan_short_calls.py plays on every row (plan_support.walk_lengths): every frame
    count 0 ... K = 4 c + 3, every count up to 2 c + 1 both from a frame boundary and from a carried phase, a call that
    leaves phase D - 1, and the calls of 1, D - 1, history - 1 and history samples -- for every registered row, so that
    a plan registered tomorrow is not walked with a hole.  The schedule sweep's shorter walk (sweep_lengths): 0 ...
    2 c + 1 in both classes, and K."""
    for d in plans:
        D, c = d.D, d.chunk_frames
        K, hist = top_frames(c), d.M * d.P + D   # pfb_history_samples: the GPU tests read it from the handle
        assert K == 4 * c + 3
        lens = walk_lengths(D, K, hist)
        calls, left = simulate_calls(lens, D)
        assert {f for f, _ in calls} >= set(range(K + 1)), d.name
        assert {f for f, ph in calls if ph == 0} >= set(range(1, 2 * c + 2)), d.name
        assert {f for f, ph in calls if ph != 0} >= set(range(1, 2 * c + 2)), d.name
        assert D - 1 in left, d.name
        assert {1, D - 1, hist - 1, hist} <= set(lens), d.name
        assert K * (K + 1) // 2 <= sum(lens) // D <= K * (K + 1), d.name   # "about K (K + 1) / 2 frames"
        sweep = sweep_lengths(D, c, hist)
        calls, _ = simulate_calls(sweep, D)
        assert {f for f, ph in calls if ph == 0} >= set(range(1, 2 * c + 2)), d.name
        assert {f for f, ph in calls if ph != 0} >= set(range(1, 2 * c + 2)), d.name
        assert 0 in {f for f, _ in calls} and calls[-1] == (K, 0), d.name
        assert sum(sweep) <= sum(lens), d.name   # it is played on a prefix of the same stream


def test_channel_major_route_is_pinned(plans):
    by_slabs = {d.name.decode() for d in plans if not d.channel_major_ok}
    assert by_slabs == SLAB_PLANS
    # the 16-byte-run defaults measured slower fused than by slabs (profiles/r04_channel_major_routes.txt) stay on slabs
    assert {d.name.decode() for d in plans if d.variant == 0 and not d.channel_major_ok} == {
        "pfb_fast<M1024,P16,D1024,int16>", "pfb_fast<M1024,P16,D1024,cf32>", "pfb_fast<M560,P12,D560,int16>",
        "pfb_fast<M560,P12,D560,int8>", "pfb_fast<M560,P12,D560,cf32>", "pfb_fast<M250,P12,D250,int16>",
        "pfb_fast<M500,P12,D500,int16>"}


def test_design_names_the_slab_plans():
    """DESIGN.md section 5.2's paragraph on the slab route lists exactly the plans that take it."""
    with open(os.path.join(ROOT, "DESIGN.md")) as f:
        text = f.read()
    sec = text[text.index("### 5.2 "):text.index("### 5.2b")]
    start = sec.index("* **Frame-major slabs + a transpose kernel**")
    end = sec.find("\n* ", start + 1)
    para = sec[start:end if end > 0 else len(sec)]
    assert set(NAME_RE.findall(para)) and {m.group(0) for m in NAME_RE.finditer(para)} == SLAB_PLANS
