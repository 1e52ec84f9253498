"""What the tests that walk the fused-kernel table (pfb_fast_plan_info) share: the tolerance and the call of the float64
oracle, format and schedule tables, the fuzz shapes, the call-length walks, and what a walk builds a row from (draws
from the caller's generator, inputs, the handle).  Imported by basename; touches no device until a function needs one."""
import numpy as np

from oracle.pfb_oracle import OracleConfig
from sdr_channelizer_amd import Channelizer, synth
from sdr_channelizer_amd import _lib as L

REL_TOL = 1e-5  # north star: <= 1e-5 relative error
FMT = {"int8": L.PFB_FMT_INT8_IQ, "int16": L.PFB_FMT_INT16_IQ, "cf32": L.PFB_FMT_CF32}
FMT_NAME = {code: name for name, code in FMT.items()}
BPS = {"int8": 2, "int16": 4, "cf32": 8}   # bytes per input sample
# every schedule pfb_set_option accepts but 9 (channel-major by slabs, a route): a plan without one runs its sliding runs
SCHEDULES = (-1, 0, 2, 3, 4, 6, 7, 8, 11, 13)

# tests/test_gpu_fuzz.py's list: (M, P, D, formats, schedules worth forcing besides the default)
SHAPES = [
    (64, 12, 64, ("int16", "int8", "cf32"), (0, 2, 3, 4, 7, 8, 11)),
    (64, 16, 64, ("int16",), (0, 4, 7, 8)),
    (128, 12, 64, ("int16", "cf32"), (0, 2, 3, 7, 8, 11)),
    (256, 8, 256, ("int8", "int16", "cf32"), (0, 2, 8, 11)),
    (1024, 16, 1024, ("int16", "cf32"), (0, 6)),
    (56, 12, 56, ("int16", "int8", "cf32"), (0, 2, 3, 7, 8)),
    (560, 12, 560, ("int16", "int8", "cf32"), (0, 6)),
    (32, 12, 32, ("int16", "int8"), (0, 2, 7, 8)),
    (16, 12, 16, ("int16", "int8"), (0,)),
    (8, 12, 8, ("int16", "int8", "cf32"), (0,)),
    (10, 12, 10, ("int16",), (0,)),
    (20, 12, 20, ("int16",), (0,)),
    (40, 12, 40, ("int16",), (0,)),
    # csrc/pfb_kernels_mixed.hip: SegKernel shapes, single-wave two-pass shapes, multi-wave three-pass shapes (lockstep / teams)
    (12, 12, 12, ("int16",), (0,)), (24, 12, 24, ("int16",), (0,)), (25, 12, 25, ("int16",), (0,)), (30, 12, 30, ("int16",), (0,)),
    (48, 12, 48, ("int16",), (0, 7, 11, 8)), (50, 12, 50, ("int16",), (0, 7, 11)),
    (80, 12, 80, ("int16",), (0, 7, 11, 8)), (96, 12, 96, ("int16",), (0, 7, 11, 8)), (100, 12, 100, ("int16",), (0, 7, 11)),
    (112, 12, 112, ("int16",), (0, 7, 11, 8)), (120, 12, 120, ("int16",), (0, 7, 11)), (160, 12, 160, ("int16",), (0,)),
    (200, 12, 200, ("int16",), (0, 6)), (250, 12, 250, ("int16",), (0, 6)), (280, 12, 280, ("int16",), (0, 6)),
    (320, 12, 320, ("int16",), (0, 6)), (400, 12, 400, ("int16",), (0, 6)), (500, 12, 500, ("int16",), (0, 6)),
    (512, 12, 512, ("int16",), (0, 6)),
]


def rel(a, b):
    return float(np.abs(a - b).max() / np.abs(b).max())


def oracle_run(oracle, iq, h, M, P, D, bw, fmt="int", **kw):
    if fmt == "cf32":
        x = iq[:, 0].astype(np.float64) + 1j * iq[:, 1].astype(np.float64)
    else:
        x = oracle.unpack(iq, bw)
    method = "fft" if (M & (M - 1)) == 0 else "polyphase"
    return oracle.channelize(x, np.asarray(h, dtype=np.float64), OracleConfig(M, P, D, **kw), method)


def oracle_for(oracle, iq, h, d, fmt, bw, kw):
    """The oracle on table row d with the switches of draw_switches."""
    return oracle_run(oracle, iq, h, d.M, d.P, d.D, bw, "cf32" if fmt == "cf32" else "int", fftshift=kw["fftshift"],
                      conj_input=kw["conjugate_input"], derotate=kw["derotate"], off=kw["input_offset"])


def family(d):
    return (d.default_schedule, d.sample_format, d.D == d.M)


def family_rows(plans):
    """The first row of each (default schedule, sample format, D == M) group: one row per kernel family."""
    return [i for i, d in enumerate(plans) if family(d) not in {family(e) for e in plans[:i]}]


def draw_switches(rng, d):
    return dict(fftshift=bool(rng.integers(2)), conjugate_input=bool(rng.integers(2)),
                derotate=(d.D != d.M) and bool(rng.integers(2)), input_offset=int(rng.integers(-1, d.D)))


def draw_bit_width(rng, fmt):
    return 1 if fmt == "cf32" else 8 if fmt == "int8" else int(rng.choice([12, 16]))


def draw_taps(rng, M, P):
    return (rng.standard_normal(M * P) / M).astype(np.float32)


def host_input(rng, n, fmt, bw):
    if fmt == "cf32":
        return rng.standard_normal((n, 2)).astype(np.float32)
    return synth.pulsed_iq_numpy(n, bw, np.int8 if fmt == "int8" else np.int16, seed=int(rng.integers(1 << 30)))


def device_input(n, fmt, bw, seed):
    import torch
    if fmt == "cf32":
        g = torch.Generator(device="cuda")
        g.manual_seed(seed)
        return torch.randn((n, 2), dtype=torch.float32, device="cuda", generator=g)
    return synth.pulsed_iq_torch(n, bw, torch.int8 if fmt == "int8" else torch.int16, seed=seed, device="cuda")


def plan_handle(d, fmt, bw, h, kw, **extra):
    ch = Channelizer(d.M, taps=h, decimation=d.D, sample_format=fmt, bit_width=bw, **kw, **extra)
    ch.set_option(L.PFB_OPT_KERNEL, 2)   # the fused plan or an error, never the generic kernel
    ch.set_option(L.PFB_OPT_VARIANT, d.variant)
    return ch


def top_frames(c):
    """K: the longest call of the walk = the shortest rung of tests/test_gpu_plan_at_size.py's ladder."""
    return 4 * c + 3


def walk_lengths(D, K, hist_samples, both=None):
    """Call lengths in samples which, played in order from a reset handle, produce
    * every frame count 0 ... K,
    * every count 1 ... `both` (default (K - 1) // 2, which is 2 c + 1 for K = 4 c + 3) once from a frame boundary and
      once from a carried phase; the counts above alternate between the two,
    * a call that leaves phase D - 1 behind,
    * an empty call and calls of 1, D - 1, hist_samples - 1 and hist_samples samples.
    Pure arithmetic: frames = (phase + n) // D, phase = (phase + n) % D."""
    assert D >= 2 and K >= 1 and hist_samples > D
    both = (K - 1) // 2 if both is None else both
    lens, phase = [], 0

    def call(n):
        nonlocal phase
        lens.append(n)
        phase = (phase + n) % D

    call(0)
    call(1)                  # no frame; carries one sample
    call(D - 1)              # the frame that sample began
    call(hist_samples - 1)   # one sample short of replacing the whole history
    call(hist_samples)
    if phase:
        call(D - phase)      # back onto a frame boundary
    for F in range(1, K + 1):
        r = D - 1 if F == 1 else 1 + (7 * F) % (D - 1)   # 1 ... D - 1 samples over
        if F <= both:
            call(F * D + r)        # F frames from a boundary ...
            call(F * D - r)        # ... and F frames from phase r, back onto a boundary
        elif phase == 0:
            call(F * D + r)
        else:
            call(F * D - phase)
    return lens


def sweep_lengths(D, c, hist_samples):
    """The shorter walk of the schedule sweep: every count 0 ... 2 c + 1 in both phase classes, then one call of K."""
    lens = walk_lengths(D, 2 * c + 1, hist_samples, both=2 * c + 1)
    assert sum(lens) % D == 0   # it ends on a boundary
    return lens + [top_frames(c) * D + D // 2]
