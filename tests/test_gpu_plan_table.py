"""Every row of the fused-kernel table (pfb_fast_plan_info), reached through PFB_OPT_VARIANT, through every launch path
it has, against the float64 C oracle: complex, magnitude and power output in both layouts, every schedule, both
channel-major routes, and device buffers that are only sample-aligned.  The rows come from the library itself, so a
plan registered tomorrow is walked tomorrow (tests/test_plan_table_cpu.py pins the table's shape on any machine)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from plan_support import (FMT_NAME, REL_TOL, SCHEDULES, draw_bit_width, draw_switches, draw_taps, host_input,  # noqa: E402
                          oracle_for, plan_handle, rel)
from sdr_channelizer_amd import _lib as L  # noqa: E402

PLANS = L.fast_plans()
SLAB_FRAMES = (0, 64)   # 0: one slab for the whole call; 64: several, the later ones reading their history from the input


@pytest.mark.parametrize("row", range(len(PLANS)), ids=[d.name.decode() for d in PLANS])
def test_registered_plan_against_the_oracle(oracle, row):
    import torch
    d = PLANS[row]
    name, M, P, D, fmt = d.name.decode(), d.M, d.P, d.D, FMT_NAME[d.sample_format]
    rng = np.random.default_rng(31000 + row)
    frames = int(rng.integers(200, 400))
    n = frames * D + int(rng.integers(1, D))   # a ragged tail
    bw = draw_bit_width(rng, fmt)
    iq = host_input(rng, n + 1, fmt, bw)
    iq_pad, iq = iq, iq[1:]   # iq_pad on the device, one sample in, is the misaligned input of (d)
    h = draw_taps(rng, M, P)
    kw = draw_switches(rng, d)
    c1 = 2 * int(rng.integers(n // 10, n // 4)) + 1   # an odd sample
    cuts = [0, c1, int(rng.integers(c1 + D, n - D)), n]
    want = oracle_for(oracle, iq, h, d, fmt, bw, kw)
    mag_want = np.abs(want)
    peak = float(mag_want.max())

    def run(ch, channel_major=False):
        ch.reset()
        parts = []
        for a, b in zip(cuts[:-1], cuts[1:]):
            parts.append(ch(iq[a:b]))
            assert ch.last_kernel == name, (ch.last_kernel, a, b)
        return np.concatenate(parts, axis=1 if channel_major else 0)

    modes = {"complex": {}, "magnitude": dict(magnitude=True), "power": dict(power=True)}
    fm, handles = {}, {}
    try:
        for mode, extra in modes.items():
            handles[mode, False] = plan_handle(d, fmt, bw, h, kw, **extra)
            handles[mode, True] = plan_handle(d, fmt, bw, h, kw, channel_major=True, **extra)
        # (a) every output mode against the oracle, in both layouts; (c) the default channel-major route gives the
        # transposed frame-major bits
        for mode in modes:
            got = fm[mode] = run(handles[mode, False])
            cm = run(handles[mode, True], channel_major=True)
            assert np.array_equal(cm, got.T), (name, mode)
            if mode == "complex":
                assert got.shape == want.shape and got.dtype == np.complex64
                assert rel(got, want) < REL_TOL, (name, kw)
            elif mode == "magnitude":
                assert got.shape == want.shape and got.dtype == np.float32
                assert float(np.abs(got - mag_want).max()) / peak < REL_TOL, (name, kw)
            else:
                assert float(np.abs(got - mag_want ** 2).max()) / peak ** 2 < 2 * REL_TOL, (name, kw)
        assert np.all(np.abs(np.sqrt(fm["power"]) - fm["magnitude"]) <= np.spacing(fm["magnitude"])), name

        # (b) every schedule, frame-major: the default schedule's bits
        for mode in ("complex", "magnitude"):
            ch = handles[mode, False]
            for s in SCHEDULES:
                ch.set_option(L.PFB_OPT_SCHEDULE, s)
                assert np.array_equal(run(ch), fm[mode]), (name, mode, s)
            ch.set_option(L.PFB_OPT_SCHEDULE, -1)

        # (c) channel-major by slabs, one and several per call
        for mode in ("complex", "magnitude"):
            ch = handles[mode, True]
            ch.set_option(L.PFB_OPT_SCHEDULE, 9)
            for sf in SLAB_FRAMES:
                ch.set_option(L.PFB_OPT_SLAB_FRAMES, sf)
                assert np.array_equal(run(ch, channel_major=True), fm[mode].T), (name, mode, sf)

        # (d) device buffers one element in: the output (the magnitude's 4-byte offset takes the direct stores of the
        # staged-magnitude plans), and the input (the checked loads): the bits of aligned buffers, and the oracle's values
        dev_pad = torch.from_numpy(iq_pad).cuda()
        dev_in = dev_pad[1:]
        assert dev_in.data_ptr() % 16 != 0
        for mode in ("complex", "magnitude"):
            ch = handles[mode, False]
            ch.reset()
            aligned = ch(dev_in.clone())
            assert ch.last_kernel == name
            assert np.array_equal(aligned.cpu().numpy(), fm[mode]), (name, mode)   # device path = host path
            ch.reset()
            shifted_in = ch(dev_in)
            assert ch.last_kernel == name
            assert torch.equal(shifted_in, aligned), (name, mode)
            if mode == "complex":
                assert rel(shifted_in.cpu().numpy(), want) < REL_TOL, name
            else:
                assert float(np.abs(shifted_in.cpu().numpy() - mag_want).max()) / peak < REL_TOL, name
            ch.reset()
            buf = torch.empty(aligned.numel() + 1, dtype=aligned.dtype, device=aligned.device)
            shifted_out = ch(dev_in.clone(), out=buf[1:])
            assert ch.last_kernel == name
            assert torch.equal(shifted_out, aligned), (name, mode)
    finally:
        for ch in handles.values():
            ch.close()
