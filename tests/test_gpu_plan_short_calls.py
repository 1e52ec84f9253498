"""Every row of the fused-kernel table on short calls and on the two launches of a time shard.

tests/test_gpu_plan_table.py holds every plan against the oracle on calls of 20 frames and more, and
tests/test_gpu_plan_at_size.py starts its ladder at K = 4 c + 3 frames (c = the plan's chunk).  Here every plan gets
every call length below that, so the two meet at K with no gap:

* the stream walk: one stream cut into calls of 0, 1, 2, ... K frames, every count up to 2 c + 1 both from a frame
  boundary and from a carried phase, calls of 1, D - 1, history - 1 and history samples (plan_support.walk_lengths; its
  coverage is checked on any machine by tests/test_plan_table_cpu.py) -- frame-major complex and magnitude,
  channel-major through the default route and by slabs, through host pointers in one-frame staging chunks, and every
  schedule on the calls of up to 2 c + 1 frames plus one of K (sweep_lengths);
* the fresh walk: a reset handle and ONE call of F frames, F = 1 ... K: no history, a first run that is the last;
* the split launch: pfb_process_shard_async on a world of one -- interior frames [head, F) with their history in the
  input, then the head frames over an input of the whole segment -- on segments from the smallest legal one up,
  against a plain call on a twin handle; and two ranks of the smallest legal segment for one row per kernel family.

One reference per row: the whole stream in one call with the run length forced to two chunks, held to the float64
oracle once (the project's bound, REL_TOL); everything else is bit equality against it.  What each launch was is read
from pfb_last_launch; the policy's arithmetic is not repeated.

Nothing was shortened: every row runs the full schedule sweep.  Measured on an MI355X: see SLOWEST below."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from gpu_support import Mailbox  # noqa: E402
from plan_support import (BPS, FMT_NAME, REL_TOL, SCHEDULES, draw_bit_width, draw_switches, draw_taps,  # noqa: E402
                          family_rows, host_input, oracle_for, plan_handle, rel, sweep_lengths, top_frames, walk_lengths)
from sdr_channelizer_amd import _lib as L  # noqa: E402

PLANS = L.fast_plans()
IDS = [d.name.decode() for d in PLANS]
FAMILY_ROWS = family_rows(PLANS)
# wall time of the slowest rows on an MI355X (pytest --durations): the three M = 8 rows (c = 64, K = 259)
SLOWEST = "stream walk 2.4 s (pfb_fast<M8,P12,D8,int8>; M = 10: 1.4 s); every other test of the module below 0.4 s; all 189: 21 s"


class Row:
    """One row's configuration, stream and references; built once and shared by the tests of the row."""

    def __init__(self, oracle, row):
        import torch
        d = self.d = PLANS[row]
        self.name, self.fmt = d.name.decode(), FMT_NAME[d.sample_format]
        M, P, D, c = d.M, d.P, d.D, d.chunk_frames
        rng = np.random.default_rng(73000 + row)
        self.kw = draw_switches(rng, d)
        self.bw = draw_bit_width(rng, self.fmt)
        self.h = draw_taps(rng, M, P)
        self.K = top_frames(c)
        with self.handle() as ch:
            self.hist = ch.history_samples
        self.lens = walk_lengths(D, self.K, self.hist)
        self.sweep = sweep_lengths(D, c, self.hist)
        n = sum(self.lens)
        assert n >= sum(self.sweep) and n >= self.K * D + D - 1
        self.iq = host_input(rng, n, self.fmt, self.bw)
        self.d_iq = torch.from_numpy(self.iq).cuda()
        self.fresh_tails = [int(x) for x in rng.integers(0, D, size=self.K + 1)]
        ref = oracle_for(oracle, self.iq, self.h, d, self.fmt, self.bw, self.kw)
        # the references: the whole stream in one call at the shortest legal run length, against the oracle.  (The run
        # length asserted below is the one handed down; the schedule-4 rows run their compiled-in 8 x 64-frame workgroups
        # whatever it says -- which kernel ran is pfb_last_entry, tests/test_gpu_kernel_entry.py)
        self.want = {}
        for mode, extra in (("complex", {}), ("magnitude", dict(magnitude=True))):
            with self.handle(**extra) as ch:
                ch.set_option(L.PFB_OPT_FRAMES_PER_BLOCK, 2 * c)
                y = ch(self.d_iq)
                assert ch.last_kernel == self.name and ch.last_launch.frames_per_block == 2 * c, self.name
            got = y.cpu().numpy()
            assert got.shape == ref.shape == (n // D, M), (self.name, got.shape, ref.shape)
            if mode == "complex":
                assert rel(got, ref) < REL_TOL, (self.name, self.kw)
            else:
                assert float(np.abs(got - np.abs(ref)).max()) / float(np.abs(ref).max()) < REL_TOL, (self.name, self.kw)
            self.want[mode, False] = y
            self.want[mode, True] = y.T   # channel-major = the transpose, bit for bit
        self.want_host = self.want["complex", False].cpu().numpy()

    def handle(self, **extra):
        return plan_handle(self.d, self.fmt, self.bw, self.h, self.kw, **extra)


_ROWS = {}


def row_of(oracle, row):
    if row not in _ROWS:
        _ROWS[row] = Row(oracle, row)
    return _ROWS[row]


def check_launch(ch, R, F, what, slabs=None, one_launch=True):
    """What include/pfb_channelizer_dev.h promises of pfb_last_launch, after a call of F > 0 frames."""
    d, rep = R.d, ch.last_launch
    assert ch.last_kernel == R.name, (ch.last_kernel, what)
    assert rep.fused == 1 and rep.frames_per_block % d.chunk_frames == 0, (what, rep.fused, rep.frames_per_block)
    if slabs is not None:
        assert rep.by_slabs == slabs, (what, rep.by_slabs)
    if not one_launch:   # a host-pointer call is one launch per staged chunk: the report is the last chunk's
        return
    assert rep.frames == F, (what, rep.frames)
    if rep.by_slabs:
        assert rep.slab_frames >= ch.shard_head_frames + 1 and rep.slab_frames % 64 == 0, (what, rep.slab_frames)
    else:
        assert rep.runs == -(-F // rep.frames_per_block), (what, rep.runs, rep.frames_per_block)


def play(ch, R, lens, mode, what, cm=False, host=False, slabs=None):
    """Reset the handle and play the calls; every part must be the reference's rows, bit for bit."""
    import torch
    D = R.d.D
    want = R.want_host if host else R.want[mode, cm]
    src = R.iq if host else R.d_iq
    ch.reset()
    pos = phase = done = 0
    for n in lens:
        F = (phase + n) // D
        where = (R.name, what, f"call of {F} frames = {n} samples at sample {pos}, carried phase {phase}")
        y = ch(src[pos:pos + n])
        assert tuple(y.shape) == ((R.d.M, F) if cm else (F, R.d.M)), where
        if F:
            check_launch(ch, R, F, where, slabs=slabs, one_launch=not host)
            if host:
                assert np.array_equal(y, want[done:done + F]), where
            else:
                assert torch.equal(y, want[:, done:done + F] if cm else want[done:done + F]), where
        pos, phase, done = pos + n, (phase + n) % D, done + F
    return done


@pytest.mark.parametrize("row", range(len(PLANS)), ids=IDS)
def test_stream_walk_of_short_calls(oracle, row):
    R = row_of(oracle, row)
    d = R.d
    route = 0 if d.channel_major_ok else 1
    handles = []

    def handle(**extra):
        handles.append(R.handle(**extra))
        return handles[-1]

    try:
        fm = handle()
        total = play(fm, R, R.lens, "complex", "frame-major complex", slabs=0)
        assert total == R.want["complex", False].shape[0] and total >= R.K * (R.K + 1) // 2
        play(handle(magnitude=True), R, R.lens, "magnitude", "frame-major magnitude", slabs=0)
        cm = handle(channel_major=True)
        play(cm, R, R.lens, "complex", "channel-major, default route", cm=True, slabs=route)
        cm.set_option(L.PFB_OPT_SCHEDULE, 9)
        cm.set_option(L.PFB_OPT_SLAB_FRAMES, 64)
        play(cm, R, R.lens, "complex", "channel-major by slabs of 64", cm=True, slabs=1)
        host = handle()
        host.set_option(L.PFB_OPT_HOST_CHUNK_SAMPLES, d.D)   # one-frame staging chunks
        play(host, R, R.lens, "complex", "host pointers, one-frame chunks", host=True, slabs=0)
        for s in SCHEDULES:
            fm.set_option(L.PFB_OPT_SCHEDULE, s)
            play(fm, R, R.sweep, "complex", f"frame-major complex, schedule {s}", slabs=0)
    finally:
        for ch in handles:
            ch.close()


@pytest.mark.parametrize("row", range(len(PLANS)), ids=IDS)
def test_fresh_handle_walk(oracle, row):
    """One call of F frames on a reset handle, F = 1 ... K: frame f depends only on samples up to f D + offset, so the
    result is the first F rows of the reference."""
    import torch
    R = row_of(oracle, row)
    d = R.d
    with R.handle() as fm, R.handle(channel_major=True) as cm:
        for ch, is_cm in ((fm, False), (cm, True)):
            want = R.want["complex", is_cm]
            for F in range(1, R.K + 1):
                n = F * d.D + R.fresh_tails[F]
                where = (R.name, "channel-major" if is_cm else "frame-major", f"fresh call of {F} frames = {n} samples")
                ch.reset()
                y = ch(R.d_iq[:n])
                check_launch(ch, R, F, where, slabs=(0 if d.channel_major_ok else 1) if is_cm else 0)
                assert torch.equal(y, want[:, :F] if is_cm else want[:F]), where


def shard_segments(d, head, hist, rng):
    c = d.chunk_frames
    lo = max(head, -(-hist // d.D))   # the smallest legal segment: it holds the history the handle keeps
    return [lo, head + 1, head + c, head + 2 * c + 1, int(rng.integers(150, 250))]


@pytest.mark.parametrize("row", range(len(PLANS)), ids=IDS)
def test_split_launch_of_a_shard(row):
    """pfb_process_shard_async on a world of one (no exchange, no threads; the head frames continue from the handle's
    own state): the interior launch [head, F) with f_begin > 0 and the head launch of `head` frames over an input of
    the whole segment give the bits of one plain call, and leave the segment's tail behind as state."""
    import torch
    d = PLANS[row]
    name, fmt, D = d.name.decode(), FMT_NAME[d.sample_format], d.D
    rng = np.random.default_rng(74000 + row)
    kw = draw_switches(rng, d)
    bw = draw_bit_width(rng, fmt)
    h = draw_taps(rng, d.M, d.P)
    handle = functools.partial(plan_handle, d, fmt, bw, h, kw)

    with handle() as probe:
        head, hist = probe.shard_head_frames, probe.history_samples
    segs = shard_segments(d, head, hist, rng)
    pre, after = head + 3, 3   # frames of the plain calls in front of the first segment and behind each
    d_iq = torch.from_numpy(host_input(rng, (pre + sum(segs) + after * len(segs)) * D, fmt, bw)).cuda()
    modes = (("frame-major complex", {}), ("frame-major magnitude", dict(magnitude=True)),
             ("channel-major complex", dict(channel_major=True)))
    for what, extra in modes:
        with handle(**extra) as ch, handle(**extra) as twin:
            ch.attach_shard(0, 1)
            # mid-stream: a non-zero history, phase 0, a non-zero frame index for the derotation
            assert torch.equal(ch(d_iq[:pre * D]), twin(d_iq[:pre * D])), (name, what)
            pos = pre * D
            for F in segs:
                where = (name, what, f"segment of {F} frames at sample {pos}, head {head}")
                seg = d_iq[pos:pos + F * D]
                got = ch.process_shard(seg)
                ch.sync()
                assert ch.last_kernel == name and ch.last_launch.fused == 1, where
                if "channel_major" in extra:
                    assert ch.last_launch.by_slabs == (0 if d.channel_major_ok else 1), where
                want = twin(seg)
                assert twin.last_kernel == name, where
                assert torch.equal(got, want), where
                pos += F * D
                tail = d_iq[pos:pos + after * D]   # the state left behind is the segment's tail
                assert torch.equal(ch(tail), twin(tail)), (where, "the plain call after it")
                pos += after * D


@pytest.mark.parametrize("row", FAMILY_ROWS, ids=[IDS[i] for i in FAMILY_ROWS])
def test_two_ranks_on_the_smallest_segments(row):
    """Two shards of the smallest legal length, the halo through the matched transport of tests/gpu_support.py:
    neither segment has an interior, rank 1's head frames read the landing zone; the stream of one handle, bit for bit."""
    import torch
    d = PLANS[row]
    name, fmt, D = d.name.decode(), FMT_NAME[d.sample_format], d.D
    rng = np.random.default_rng(75000 + row)
    kw = draw_switches(rng, d)
    bw = draw_bit_width(rng, fmt)
    h = draw_taps(rng, d.M, d.P)
    handle = functools.partial(plan_handle, d, fmt, bw, h, kw)

    for cm in (False, True):
        hs = [handle(channel_major=cm) for _ in range(2)]
        try:
            head, hist, halo = hs[0].shard_head_frames, hs[0].history_samples, hs[0].halo_samples
            F = max(head, -(-hist // D))
            d_iq = torch.from_numpy(host_input(rng, 2 * F * D, fmt, bw)).cuda()
            with handle(channel_major=cm) as one:
                want = one(d_iq)
                assert one.last_kernel == name
            box = Mailbox(2, halo * BPS[fmt])

            def call(g):
                def f():
                    hs[g].attach_shard(g, 2, box.exchange_for(g), ring=False)
                    hs[g].set_frame_index(g * F)
                    y = hs[g].process_shard(d_iq[g * F * D:(g + 1) * F * D])
                    hs[g].sync()
                    return y
                return f
            outs = box.run([call(0), call(1)])
            assert [x.last_kernel for x in hs] == [name, name]
            assert torch.equal(torch.cat(outs, dim=1 if cm else 0), want), (name, "channel-major" if cm else "frame-major", F)
        finally:
            for x in hs:
                x.release()
