"""The fused-kernel table as the library lists it (pfb_fast_plan_count / pfb_fast_plan_info, host only): every row is
what its name says, the variants of a shape are numbered the way PFB_OPT_VARIANT counts them, every shape is fuzzed,
the channel-major route of every plan is the one DESIGN.md names, and every selection a handle can be put into
resolves to one named kernel entry (pfb_plan_entry).  No GPU needed."""
import json
import os
import re

import pytest

from plan_support import (ENTRY_CASES, FMT, SCHEDULES, SHAPES, entry_geometry, plan_entry_for, sweep_lengths, tag_parts,
                          top_frames, walk_lengths)
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


# ---- kernel entries: which kernel a launch resolves to (pfb_plan_entry: the policy, then the row's select) ------------

NUM_CUS = 256
FAMILY_SCHEDULE = {"sliding": 0, "seg": 0, "tile": 2, "shared": 3, "paired": 4, "teams": 6, "pairs_sliding": 7,
                   "tile_t": 8, "overlap": 11, "twin": 13}


# single-wave plans whose chunk buffer cannot hold the transposed chunk (kTileTOk, pfb_fast_tiles.hpp): their channel-major
# default is schedule 2
TILE_PLANS = {"pfb_fast<M50,P12,D50,int16>", "pfb_fast<M100,P12,D100,int16>", "pfb_fast<M120,P12,D120,int16>"}


def check_entry(d, e, rep, opts, where):
    """What every entry must satisfy, whatever was asked for."""
    # the two cases without a kernel -- a channel-major call on a plan without a channel-major instantiation, schedule 13
    # on a channel-major call -- are unreachable through the policy (it sends the first by slabs and hands a fused
    # channel-major call schedule -1, 0, 2 or 8), so here every entry has one
    assert e.kernel != 0 and e.reserved == 0, where
    family, _, roles = tag_parts(e.tag)
    assert FAMILY_SCHEDULE[family] == e.schedule, where
    if rep.schedule >= 0:   # the schedule asked for, or the plan lacks it: its sliding runs (the small banks: their one kernel)
        assert e.schedule == rep.schedule or (e.schedule == 0 and family in ("sliding", "seg")), where
    else:                   # a fused channel-major launch, the kernel's own pick
        assert e.schedule in (8, 2, 0) and opts.get("channel_major") and not rep.by_slabs, where
    cm = bool(opts.get("channel_major")) and not rep.by_slabs
    mag, nt = bool(opts.get("magnitude")), bool(opts.get("nontemporal"))
    assert ("cm" in roles) <= cm and ("mag" in roles) <= mag and ("c64" in roles) <= (not mag), where
    assert ("ms" in roles) <= (mag and opts.get("out_aligned16", True)) and ("nt" in roles) <= (nt and not mag), where
    if cm and family != "tile_t":   # (tile_t is channel-major by construction)
        assert "cm" in roles, where
    frames = min(rep.frames, rep.slab_frames) if rep.by_slabs else rep.frames
    per, threads = entry_geometry(e.tag, d, rep.frames_per_block)
    blocks = -(-frames // per)
    if family == "twin" and opts.get("grid", 0) > 0:
        blocks = min(blocks, opts["grid"])
    assert (e.threads, e.blocks) == (threads, blocks) and 64 <= e.threads <= 1024, where
    assert e.dyn_lds == (((opts.get("experiment", 0) >> 8) & 0xff) * 1024 if family == "shared" else 0), where


def test_every_selection_resolves_to_one_named_kernel(plans):
    """Every row, over every schedule pfb_set_option accepts, tile_waves 1 ... 16, both layouts, complex / magnitude /
    nontemporal output and run lengths from the default to 128 frames: the entry has a kernel, its schedule is the one
    asked for or the documented fall-back, its grid covers the call's frames with the workgroups its tag names, and
    within a row tag and kernel map one to one."""
    points = 0
    for i, d in enumerate(plans):
        by_tag, by_kernel = {}, {}
        for sched in SCHEDULES + (9,):
            for tw in (1, 4, 5, 6, 8, 16):
                for cm in (False, True):
                    for mag, nt in ((False, False), (True, False), (False, True)):
                        for fpb in (0, 2 * d.chunk_frames, 24, 32, 48, 64, 128):
                            opts = dict(schedule=sched, tile_waves=tw, channel_major=cm, magnitude=mag, nontemporal=nt,
                                        frames_per_block=fpb)
                            e = plan_entry_for(i, 2603, NUM_CUS, opts)
                            rep = L.plan_launch(i, 2603, NUM_CUS, schedule=sched, frames_per_block=fpb, channel_major=cm,
                                                magnitude=mag)
                            check_entry(d, e, rep, opts, (d.name, opts, e.fields()))
                            assert by_tag.setdefault(e.tag, e.kernel) == e.kernel, (d.name, e.tag)
                            assert by_kernel.setdefault(e.kernel, e.tag) == e.tag, (d.name, e.tag)
                            points += 1
        assert len(by_tag) == len(by_kernel) >= 2, d.name
    print(f"{points} selections over {len(plans)} rows")


def test_default_requests_run_the_rows_own_schedules(plans):
    for i, d in enumerate(plans):
        for frames in (1, 2603, 1 << 20):
            assert plan_entry_for(i, frames, NUM_CUS, {}).schedule == d.default_schedule, d.name
            want = d.magnitude_schedule if d.magnitude_schedule >= 0 else d.default_schedule
            assert plan_entry_for(i, frames, NUM_CUS, dict(magnitude=True)).schedule == want, d.name
            e = plan_entry_for(i, frames, NUM_CUS, dict(channel_major=True))
            rep = L.plan_launch(i, frames, NUM_CUS, channel_major=True)
            if rep.by_slabs:      # the frame-major kernel fills the slabs
                assert e.schedule == d.default_schedule and not d.channel_major_ok, d.name
            elif d.threads != 64:                    # multi-wave plans: channel-major sliding runs
                assert (e.schedule, e.tag) == (0, "sliding+cm"), (d.name, e.tag)
            elif tag_parts(e.tag)[0] == "seg":       # the small banks' one kernel
                assert (e.schedule, e.tag) == (0, "seg+cm+c64") and d.M <= 40, (d.name, e.tag)
            elif d.name.decode() in TILE_PLANS:      # one chunk per wave: 16 waves up to M = 64, 8 above
                assert (e.schedule, e.tag) == (2, "tile<16>+cm" if d.M <= 64 else "tile<8>+cm"), (d.name, e.tag)
            else:                                    # short runs transposed in LDS: 2 waves x 4 chunks up to M = 32, 4 x 2 above
                assert (e.schedule, e.tag) == (8, "tile_t<2,4>" if d.M <= 32 else "tile_t<4,2>"), (d.name, e.tag)


def test_pinned_entries(plans):
    """plan_support.ENTRY_CASES: the literals of the dispatch as the commit before select_fast had it."""
    index = {d.name.decode(): i for i, d in enumerate(plans)}
    for fam, name, opts, frames, schedule, tag in ENTRY_CASES:
        i = index[name]
        e = plan_entry_for(i, frames, NUM_CUS, opts)
        policy = {k: v for k, v in opts.items() if k in ("schedule", "frames_per_block", "channel_major", "magnitude")}
        rep = L.plan_launch(i, frames, NUM_CUS, **policy)
        where = (name, opts, e.fields())
        assert (e.schedule, e.tag) == (schedule, tag), where
        check_entry(plans[i], e, rep, opts, where)
        per, _ = entry_geometry(tag, plans[i], rep.frames_per_block)
        assert frames <= 2650 and frames % per != 0 and frames > 2 * per, where   # two whole workgroups and a partial one
        assert e.blocks == (opts["grid"] if "grid" in opts else -(-frames // per)) and (e.blocks >= 3 or "grid" in opts), where
        if "frames_per_block" in opts and tag_parts(tag)[0] not in ("sliding", "pairs_sliding") and "grid" not in opts:
            assert e.blocks == 3, where
    assert {c[0] for c in ENTRY_CASES} == {"cfg2", "m64", "m128", "m56", "m32", "m1024", "m8", "m256"}
    # the run length the report hands down is not the run length of the kernel that runs: 16 asked for, 8 x 64 run
    e = plan_entry_for(index["pfb_fast<M64,P12,D64,int16>"], 2603, NUM_CUS, dict(schedule=4, frames_per_block=16))
    rep = L.plan_launch(index["pfb_fast<M64,P12,D64,int16>"], 2603, NUM_CUS, schedule=4, frames_per_block=16)
    assert (rep.frames_per_block, rep.runs) == (16, -(-2603 // 16)) and (e.tag, e.blocks) == ("paired<8,64,4>+c64", -(-2603 // 512))
    # schedule 3's occupancy throttle: PFB_OPT_EXPERIMENT bits 8-15 are KiB of dynamic LDS
    e = plan_entry_for(index["pfb_fast<M64,P12,D64,int16>"], 483, NUM_CUS, dict(schedule=3, experiment=0x401))
    assert (e.tag, e.dyn_lds) == ("shared<8,24>", 4096)


def test_plan_entry_rejects_bad_arguments():
    lib = L.load()
    launch = L.PfbLaunchRequest(L.C.sizeof(L.PfbLaunchRequest), -1, 0, -1, 0, 0, NUM_CUS, 0)
    rq = L.PfbEntryRequest(L.C.sizeof(L.PfbEntryRequest), 0, launch, 8, 0, 0, 0, 1, 0, 100)
    e = L.PfbKernelEntry()
    assert lib.pfb_plan_entry(None, L.C.byref(e)) == L.PFB_ERR_BAD_ARG
    assert lib.pfb_plan_entry(L.C.byref(rq), None) == L.PFB_ERR_BAD_ARG
    assert lib.pfb_last_entry(None, L.C.byref(e)) == L.PFB_ERR_BAD_ARG and lib.pfb_last_entry(None, None) == L.PFB_ERR_BAD_ARG
    for size in (0, L.C.sizeof(L.PfbEntryRequest) - 8, L.C.sizeof(L.PfbEntryRequest) + 8):
        rq.struct_size = size
        assert lib.pfb_plan_entry(L.C.byref(rq), L.C.byref(e)) == L.PFB_ERR_BAD_ARG
    rq.struct_size = L.C.sizeof(L.PfbEntryRequest)
    rq.launch.struct_size = 0
    assert lib.pfb_plan_entry(L.C.byref(rq), L.C.byref(e)) == L.PFB_ERR_BAD_ARG
    rq.launch.struct_size = L.C.sizeof(L.PfbLaunchRequest)
    for row in (-1, lib.pfb_fast_plan_count()):
        rq.plan_index = row
        assert lib.pfb_plan_entry(L.C.byref(rq), L.C.byref(e)) == L.PFB_ERR_BAD_ARG
    rq.plan_index = 0
    assert lib.pfb_plan_entry(L.C.byref(rq), L.C.byref(e)) == L.PFB_OK and e.tag == "paired<8,64,4>+c64" and e.blocks == 1
    rq.frames = 0   # no frames: an entry with an empty grid (launching it is a no-op)
    assert lib.pfb_plan_entry(L.C.byref(rq), L.C.byref(e)) == L.PFB_OK and e.blocks == 0 and e.kernel != 0
    # the mirrors have the header's layout
    assert L.C.sizeof(L.PfbKernelEntry) == 40 and L.PfbKernelEntry.blocks.offset == 16 and L.PfbKernelEntry._tag.offset == 32
    assert L.C.sizeof(L.PfbEntryRequest) == 80 and L.PfbEntryRequest.launch.offset == 8 and L.PfbEntryRequest.frames.offset == 72
