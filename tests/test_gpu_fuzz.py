"""Randomised cross-check of every fused shape against the generic kernel (same library, independent code path:
branches from global memory, radix-2 or plain DFT): random flags, input offsets, layouts, run lengths, schedules and
call boundaries.  Seeded, so a failure reproduces."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from plan_support import FMT, SHAPES  # noqa: E402
from sdr_channelizer_amd import Channelizer, synth  # noqa: E402
from sdr_channelizer_amd import _lib as L  # noqa: E402

PLANS = L.fast_plans()   # every row of the fused-kernel table (tests/test_plan_table_cpu.py checks SHAPES covers them)


def make_input(rng, n, fmt):
    if fmt == "cf32":
        return (rng.standard_normal((n, 2)) * 0.3).astype(np.float32), 1
    bw = 8 if fmt == "int8" else int(rng.choice([12, 16]))
    return synth.pulsed_iq_numpy(n, bw, np.int8 if fmt == "int8" else np.int16, seed=int(rng.integers(1 << 30))), bw


@pytest.mark.parametrize("case", range(int(os.environ.get("PFB_FUZZ_CASES", "384"))))  # 12 per shape over the 32 shapes; more with PFB_FUZZ_CASES=N
def test_fused_kernels_agree_with_the_generic_kernel(case):
    rng = np.random.default_rng(1000 + case)
    M, P, D, fmts, scheds = SHAPES[case % len(SHAPES)]
    fmt = fmts[int(rng.integers(len(fmts)))]
    frames = int(rng.integers(40, 2500))
    n = frames * D + int(rng.integers(0, D))
    iq, bw = make_input(rng, n, fmt)
    p_used = P if rng.random() < 0.7 else int(rng.integers(max(1, P - 5), P + 1))   # sometimes a shorter prototype
    h = (rng.standard_normal(M * p_used) / M).astype(np.float32)
    kw = dict(fftshift=bool(rng.integers(2)), conjugate_input=bool(rng.integers(2)), derotate=bool(rng.integers(2)),
              magnitude=bool(rng.integers(2)), channel_major=bool(rng.integers(2)),
              input_offset=int(rng.integers(-1, D)))
    kw["power"] = kw["magnitude"] and bool(rng.integers(2))   # |y|^2 instead of |y|
    cuts = sorted({0, n, *(int(c) for c in rng.integers(0, n, size=int(rng.integers(0, 3))))})
    with Channelizer(M, taps=h, decimation=D, sample_format=fmt, bit_width=bw, **kw) as ch:
        ch.set_option(L.PFB_OPT_KERNEL, 1)
        want = ch(iq)
        assert ch.last_kernel == "pfb_generic"
        ch.reset()
        ch.set_option(L.PFB_OPT_KERNEL, 2)
        if rng.random() < 0.6:
            ch.set_option(L.PFB_OPT_SCHEDULE, int(scheds[int(rng.integers(len(scheds)))]))
        if rng.random() < 0.5:
            ch.set_option(L.PFB_OPT_FRAMES_PER_BLOCK, int(rng.choice([8, 24, 40, 64, 100, 256, 1000])))
        if rng.random() < 0.3:
            ch.set_option(L.PFB_OPT_TILE_WAVES, int(rng.choice([4, 6, 8, 16])))
        if rng.random() < 0.3:
            ch.set_option(L.PFB_OPT_XCD_REMAP, int(rng.integers(0, 2)))
        if kw["channel_major"] and rng.random() < 0.3:   # frame-major slabs + transpose instead of the fused stores
            ch.set_option(L.PFB_OPT_SCHEDULE, 9)
            ch.set_option(L.PFB_OPT_SLAB_FRAMES, int(rng.choice([0, 64, 192, 1024])))
        parts = [ch(iq[a:b]) for a, b in zip(cuts[:-1], cuts[1:])]
        assert ch.last_kernel.startswith("pfb_fast")
        axis = 1 if kw["channel_major"] else 0
        got = np.concatenate([q for q in parts if q.size], axis=axis) if any(q.size for q in parts) else parts[0]
    assert got.shape == want.shape, (case, kw)
    scale = max(float(np.abs(want).max()), 1e-30)
    assert float(np.abs(got - want).max()) / scale < 3e-6, (case, M, fmt, kw)


# 14-15 per shape over the 32 shapes; more with PFB_ORACLE_FUZZ_CASES=N
@pytest.mark.parametrize("case", range(int(os.environ.get("PFB_ORACLE_FUZZ_CASES", "460"))))
def test_fused_kernels_agree_with_the_oracle(oracle, case):
    """The same seeded walk over shapes, formats, switches, output modes, registered plans, schedules, run lengths and call
    cuts -- against the float64 CPU oracle (oracle/pfb_oracle.c) instead of the generic kernel, at lengths the oracle
    finishes in a moment: the fast and the generic kernel share tables, mag_out and host code, the oracle shares nothing
    with either."""
    from oracle.pfb_oracle import OracleConfig
    rng = np.random.default_rng(7000 + case)
    rng2 = np.random.default_rng([7000 + case, 1])   # the draws added later, so that the older ones stay what they were
    M, P, D, fmts, scheds = SHAPES[case % len(SHAPES)]
    fmt = fmts[int(rng.integers(len(fmts)))]
    frames = int(rng.integers(30, 400 if M <= 256 else 120))
    n = frames * D + int(rng.integers(0, D))
    iq, bw = make_input(rng, n, fmt)
    h = (rng.standard_normal(M * P) / M).astype(np.float32)
    kw = dict(fftshift=bool(rng.integers(2)), conjugate_input=bool(rng.integers(2)), derotate=bool(rng.integers(2)),
              input_offset=int(rng.integers(-1, D)))
    channel_major = bool(rng.integers(2))
    cuts = sorted({0, n, *(int(c) for c in rng.integers(0, n, size=int(rng.integers(0, 3))))})
    magnitude = bool(rng2.integers(2))
    power = magnitude and bool(rng2.integers(2))   # |y|^2 instead of |y|
    plans = [d for d in PLANS if (d.M, d.P, d.D, d.sample_format) == (M, P, D, FMT[fmt])]
    plan = plans[int(rng2.integers(len(plans)))]   # any registered plan of the shape (PFB_OPT_VARIANT)
    with Channelizer(M, taps=h, decimation=D, sample_format=fmt, bit_width=bw, channel_major=channel_major,
                     magnitude=magnitude, power=power, **kw) as ch:
        ch.set_option(L.PFB_OPT_KERNEL, 2)
        ch.set_option(L.PFB_OPT_VARIANT, plan.variant)
        if rng.random() < 0.6:
            ch.set_option(L.PFB_OPT_SCHEDULE, int(scheds[int(rng.integers(len(scheds)))]))
        if rng.random() < 0.5:
            ch.set_option(L.PFB_OPT_FRAMES_PER_BLOCK, int(rng.choice([8, 12, 24, 32, 40, 64, 100, 256])))
        parts = [ch(iq[a:b]) for a, b in zip(cuts[:-1], cuts[1:])]
        assert ch.last_kernel == plan.name.decode()
        got = np.concatenate([q for q in parts if q.size], axis=1 if channel_major else 0) if any(q.size for q in parts) else parts[0]
    x = (iq[:, 0].astype(np.float64) + 1j * iq[:, 1].astype(np.float64)) if fmt == "cf32" else oracle.unpack(iq, bw)
    cfg = OracleConfig(M, P, D, fftshift=kw["fftshift"], conj_input=kw["conjugate_input"], derotate=kw["derotate"], off=kw["input_offset"])
    want = oracle.channelize(x, h.astype(np.float64), cfg, "fft" if (M & (M - 1)) == 0 else "polyphase")
    if channel_major:
        want = want.T
    assert got.shape == want.shape, (case, M, fmt, kw)
    scale = max(float(np.abs(want).max()), 1e-30)
    if power:   # the tolerances of test_fused_magnitude_output
        assert float(np.abs(got - np.abs(want) ** 2).max()) / scale ** 2 < 2e-5, (case, M, fmt, kw, plan.name)
    elif magnitude:
        assert float(np.abs(got - np.abs(want)).max()) / scale < 1e-5, (case, M, fmt, kw, plan.name)
    else:
        assert float(np.abs(got - want).max()) / scale < 1e-5, (case, M, fmt, kw, plan.name)   # the fp32 tolerance of the parity tests
