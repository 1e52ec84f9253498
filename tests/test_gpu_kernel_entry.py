"""A forced option reaches the kernel it names: after one call, what the handle says it ran (pfb_last_entry) is what the
selection on its own says for the same row, options and frame count (pfb_plan_entry, walked over every row without a
device in tests/test_plan_table_cpu.py), its tag is the literal pinned from the dispatch's source
(plan_support.ENTRY_CASES), and its output is the bits of the same handle's plain sliding runs.  One call per case from
a reset handle, D * F + 5 samples: two whole workgroups of the entry and a partial third, the first with the history."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from plan_support import (ENTRY_CASES, FMT_NAME, device_input, draw_taps, plan_entry_for, plan_handle,  # noqa: E402
                          tag_parts)
from sdr_channelizer_amd import _lib as L  # noqa: E402

PLANS = L.fast_plans()
INDEX = {d.name.decode(): i for i, d in enumerate(PLANS)}
FAMILIES = sorted({c[0] for c in ENTRY_CASES})
OPTIONS = (("schedule", L.PFB_OPT_SCHEDULE, -1), ("frames_per_block", L.PFB_OPT_FRAMES_PER_BLOCK, 0),
           ("tile_waves", L.PFB_OPT_TILE_WAVES, 8), ("nontemporal", L.PFB_OPT_NONTEMPORAL, 0), ("grid", L.PFB_OPT_GRID, 0))


def set_options(ch, opts):
    for key, opt, default in OPTIONS:
        ch.set_option(opt, int(opts.get(key, default)))


@pytest.mark.parametrize("family", FAMILIES)
def test_forced_options_reach_the_kernel_they_name(family):
    import torch
    num_cus = torch.cuda.get_device_properties(0).multi_processor_count
    rng = np.random.default_rng(len(family))
    handles, inputs, refs = {}, {}, {}

    def handle(row, cm, mag):
        if (row, cm, mag) not in handles:
            d, fmt = PLANS[row], FMT_NAME[PLANS[row].sample_format]
            if row not in inputs:
                bw = {"int16": 12, "int8": 8, "cf32": 1}[fmt]
                inputs[row] = (device_input(d.D * 2650 + 5, fmt, bw, 100 + row), draw_taps(rng, d.M, d.P), bw)
            _, h, bw = inputs[row]
            handles[(row, cm, mag)] = plan_handle(d, fmt, bw, h, dict(channel_major=cm, magnitude=mag))
        return handles[(row, cm, mag)]

    try:
        for fam, name, opts, F, schedule, tag in ENTRY_CASES:
            if fam != family:
                continue
            row, d = INDEX[name], PLANS[INDEX[name]]
            cm, mag = bool(opts.get("channel_major")), bool(opts.get("magnitude"))
            ch = handle(row, cm, mag)
            iq = inputs[row][0][:d.D * F + 5]
            where = (name, opts, F)
            if (row, mag, F) not in refs:   # the same plan's sliding runs, frame-major
                ref = handle(row, False, mag)
                set_options(ref, dict(schedule=0))
                ref.reset()
                refs[(row, mag, F)] = ref(iq)
                assert ref.last_kernel == name and tag_parts(ref.last_entry.tag)[0] in ("sliding", "seg"), where
            want = refs[(row, mag, F)]
            out = None
            if not opts.get("out_aligned16", True):   # 8 bytes past a 16-byte boundary
                out = torch.empty(F * d.M + 2, dtype=want.dtype, device="cuda")[2:]
                assert out.data_ptr() % 16 == 8
            set_options(ch, opts)
            ch.reset()
            got = ch(iq, out=out)
            e = ch.last_entry
            where += (e.fields(),)
            assert ch.last_kernel == name and tuple(got.shape) == ((d.M, F) if cm else (F, d.M)), where
            assert e.fields() == plan_entry_for(row, F, num_cus, opts).fields(), where
            assert (e.schedule, e.tag) == (schedule, tag) and e.kernel != 0, where
            assert torch.equal(got.T if cm else got, want), where
    finally:
        for ch in handles.values():
            ch.close()


def test_entry_of_a_new_handle_and_of_the_generic_kernel():
    import torch
    from sdr_channelizer_amd import Channelizer
    with Channelizer(36, taps_per_band=12, bit_width=12) as ch:   # no fused plan for M = 36
        assert ch.last_entry.fields() == (0, 0, 0, 0, 0, "")       # all zeros and an empty tag before the first launch
        y = ch(torch.zeros((36 * 100, 2), dtype=torch.int16, device="cuda"))
        e, rep = ch.last_entry, ch.last_launch
        assert ch.last_kernel == "pfb_generic" and rep.fused == 0 and rep.frames == 100 and not bool(y.any())
        # its own grid: 256 threads, 16 frames per workgroup up to M = 256, both chunk buffers in dynamic LDS
        assert (e.schedule, e.tag, e.threads, e.blocks, e.dyn_lds) == (-1, "generic", 256, 7, 2 * 16 * 36 * 8) and e.kernel != 0
