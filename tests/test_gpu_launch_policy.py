"""What a launch stores in pfb_last_launch is what pfb_plan_launch says for the same row, options and device: the
export that tests/test_plan_table_cpu.py holds against the recorded launches is the function launch_frames calls.
Every row of the table on zero input, frame-major at 4 c + 3 and 2 c + 1 frames and channel-major at 4 c + 3 (c = the
plan's chunk): the smallest calls that reach the chunk-pair rounding and, on the slab plans, the slab clamp."""
import pytest

pytestmark = pytest.mark.gpu

from plan_support import FMT_NAME  # noqa: E402
from sdr_channelizer_amd import Channelizer  # noqa: E402
from sdr_channelizer_amd import _lib as L  # noqa: E402

PLANS = L.fast_plans()
FIELDS = [f for f, _ in L.PfbLaunchReport._fields_]


@pytest.mark.parametrize("row", range(len(PLANS)), ids=[d.name.decode() for d in PLANS])
def test_launch_report_is_the_policy_export(row):
    import torch
    d = PLANS[row]
    name, c, fmt = d.name.decode(), d.chunk_frames, FMT_NAME[d.sample_format]
    num_cus = torch.cuda.get_device_properties(0).multi_processor_count
    dtype = {"int8": torch.int8, "int16": torch.int16, "cf32": torch.float32}[fmt]
    zeros = torch.zeros(((4 * c + 3) * d.D, 2), dtype=dtype, device="cuda")
    for channel_major, counts in ((False, (4 * c + 3, 2 * c + 1)), (True, (4 * c + 3,))):
        with Channelizer(d.M, taps_per_band=d.P, decimation=d.D, sample_format=fmt, bit_width=1 if fmt == "cf32" else 8,
                         channel_major=channel_major) as ch:
            ch.set_option(L.PFB_OPT_KERNEL, 2)   # the fused plan or an error, never the generic kernel
            ch.set_option(L.PFB_OPT_VARIANT, d.variant)
            for F in counts:
                ch.reset()
                y = ch(zeros[:F * d.D])
                assert ch.last_kernel == name and tuple(y.shape) == ((d.M, F) if channel_major else (F, d.M))
                got, want = ch.last_launch, L.plan_launch(row, F, num_cus, channel_major=channel_major)
                assert [getattr(got, f) for f in FIELDS] == [getattr(want, f) for f in FIELDS], (name, channel_major, F)
                assert got.fused == 1 and got.frames == F and got.by_slabs == (channel_major and not d.channel_major_ok)
                assert not bool(y.any()), (name, channel_major, F)   # zeros in, zeros out
