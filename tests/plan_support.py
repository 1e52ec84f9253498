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
# every schedule pfb_set_option accepts but 9 (channel-major by slabs, a route).  A forced schedule, pair count or tile a
# plan lacks falls through inside select_fast (pfb_fast.hpp) -- in the end to the plan's sliding runs -- while the launch
# report keeps saying what was asked for: which kernel ran is the kernel entry's schedule and tag (last_entry, plan_entry)
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


# ---- kernel entries (pfb_kernel_entry, pfb_channelizer_dev.h) --------------------------------------------------------

def tag_parts(tag):
    """family, integer arguments and roles of a kernel tag (the grammar in pfb_channelizer_dev.h)"""
    head, *roles = tag.split("+")
    family, _, args = head.partition("<")
    return family, tuple(int(a) for a in args.rstrip(">").split(",")) if args else (), tuple(roles)


def entry_geometry(tag, d, frames_per_block):
    """(frames per workgroup, threads per workgroup) of the kernel `tag` names on table row d, from the kernels' own
    headers: what blocks and threads of an entry must be consistent with."""
    family, a, _ = tag_parts(tag)
    c, fpb = d.chunk_frames, frames_per_block
    return {"sliding": lambda: (fpb, d.threads), "overlap": lambda: (fpb, d.threads), "twin": lambda: (fpb, d.threads),
            "seg": lambda: (fpb, 64), "teams": lambda: (fpb, d.threads + 64 * c),
            "tile": lambda: (a[0] * c, 64 * a[0]), "tile_t": lambda: (a[0] * a[1] * c, 64 * a[0]),
            "shared": lambda: (a[0] * a[1], 64 * a[0]), "paired": lambda: (a[0] * a[1], 128 * a[0]),
            "pairs_sliding": lambda: (a[0] * fpb, 128 * a[0])}[family]()


CFG2, M64F32, M64I8, M64P16 = ("pfb_fast<M64,P12,D64,int16>", "pfb_fast<M64,P12,D64,cf32>", "pfb_fast<M64,P12,D64,int8>",
                               "pfb_fast<M64,P16,D64,int16>")
CFG5, CFG5F32, M56 = "pfb_fast<M128,P12,D64,int16>", "pfb_fast<M128,P12,D64,cf32>", "pfb_fast<M56,P12,D56,int16>"
M32, M1024, DUO = "pfb_fast<M32,P12,D32,int16>", "pfb_fast<M1024,P16,D1024,int16>", "pfb_fast<M1024,P16,D1024,int16,duo>"
M8F32, CFG3I8 = "pfb_fast<M8,P12,D8,cf32>", "pfb_fast<M256,P8,D256,int8>"

# (family of the GPU test, row, options, frames of the call, entry schedule, tag): literals read off the dispatch of the
# commit before select_fast existed (launch_fast in pfb_fast.hpp), not off what the library answers.  Options: schedule,
# frames_per_block, tile_waves, nontemporal, grid, experiment, magnitude, channel_major, out_aligned16.  The frames cover
# two whole workgroups of the entry and a partial third where the options fix the workgroup's frames; the policy's own
# run lengths (no frames_per_block) spread a call this short over more workgroups than that.
ENTRY_CASES = [
    # cfg2, schedule 4: key = tile_waves * 1000 + frames_per_block; the four keys of the sweep set, then the tuned
    # 8 x 64 shape in its three compiled-in roles
    ("cfg2", CFG2, dict(schedule=4, tile_waves=4, frames_per_block=64), 643, 4, "paired<4,64,4>"),
    ("cfg2", CFG2, dict(schedule=4, tile_waves=5, frames_per_block=64), 803, 4, "paired<5,64,5>"),
    ("cfg2", CFG2, dict(schedule=4, tile_waves=8, frames_per_block=48), 963, 4, "paired<8,48,4>"),
    ("cfg2", CFG2, dict(schedule=4, tile_waves=8, frames_per_block=128), 2563, 4, "paired<8,128,4>"),
    ("cfg2", CFG2, dict(schedule=4, tile_waves=8, frames_per_block=64), 1283, 4, "paired<8,64,4>+c64"),
    ("cfg2", CFG2, dict(schedule=4, nontemporal=True), 1283, 4, "paired<8,64,4>+c64+nt"),
    ("cfg2", CFG2, dict(schedule=4, magnitude=True), 1283, 4, "paired<8,64,4>+mag"),
    # tile_waves = 4 without a run length is key 4064 on cfg2 (the sweep set), 4 x 64 at 2 waves per SIMD elsewhere
    ("cfg2", CFG2, dict(schedule=4, tile_waves=4), 643, 4, "paired<4,64,4>"),
    ("cfg2", CFG2, dict(schedule=4, tile_waves=4, frames_per_block=48), 643, 4, "paired<4,64,2>"),
    ("m64", M64F32, dict(schedule=4, tile_waves=4), 643, 4, "paired<4,64,2>"),
    ("m64", M64I8, dict(schedule=4, tile_waves=4), 643, 4, "paired<4,64,2>"),
    ("m64", M64P16, dict(schedule=4, tile_waves=4), 643, 4, "paired<4,64,2>"),
    # a forced run length no key names: the report says 16-frame runs, the kernel runs 8 x 64
    ("cfg2", CFG2, dict(schedule=4, frames_per_block=16), 1283, 4, "paired<8,64,4>+c64"),
    ("cfg2", CFG2, dict(schedule=4, frames_per_block=40), 1283, 4, "paired<8,64,4>+c64"),
    # cfg2, schedule 3: the four keys every plan has, the three of the sweep set, and the tuned default for any other
    ("cfg2", CFG2, dict(schedule=3, tile_waves=8, frames_per_block=24), 483, 3, "shared<8,24>"),
    ("cfg2", CFG2, dict(schedule=3, tile_waves=8, frames_per_block=32), 643, 3, "shared<8,32>"),
    ("cfg2", CFG2, dict(schedule=3, tile_waves=8, frames_per_block=64), 1283, 3, "shared<8,64>"),
    ("cfg2", CFG2, dict(schedule=3, tile_waves=4, frames_per_block=64), 643, 3, "shared<4,64>"),
    ("cfg2", CFG2, dict(schedule=3, tile_waves=4, frames_per_block=32), 323, 3, "shared<4,32>"),
    ("cfg2", CFG2, dict(schedule=3, tile_waves=8, frames_per_block=48), 963, 3, "shared<8,48>"),
    ("cfg2", CFG2, dict(schedule=3, tile_waves=16, frames_per_block=24), 963, 3, "shared<16,24>"),
    ("cfg2", CFG2, dict(schedule=3, tile_waves=6, frames_per_block=40), 483, 3, "shared<8,24>"),
    # cfg2: the access-shape tiles, the defaults per output type and layout, the staged magnitudes and their fall-back
    ("cfg2", CFG2, dict(schedule=2, tile_waves=1), 23, 2, "tile<1>"),
    ("cfg2", CFG2, dict(schedule=2, tile_waves=4), 163, 2, "tile<8>"),
    ("cfg2", CFG2, dict(), 1283, 4, "paired<8,64,4>+c64"),
    ("cfg2", CFG2, dict(channel_major=True), 163, 8, "tile_t<4,2>"),
    ("cfg2", CFG2, dict(channel_major=True, schedule=2), 323, 2, "tile<8>+cm"),
    ("cfg2", CFG2, dict(channel_major=True, schedule=2, tile_waves=16), 323, 2, "tile<16>+cm"),
    ("cfg2", CFG2, dict(channel_major=True, schedule=0, frames_per_block=64), 163, 0, "sliding+cm"),
    ("cfg2", CFG2, dict(magnitude=True, frames_per_block=64), 163, 0, "sliding+ms"),
    ("cfg2", CFG2, dict(magnitude=True, frames_per_block=64, out_aligned16=False), 163, 0, "sliding+mag"),
    # M = 64 cf32: magnitudes stay on wave pairs
    ("m64", M64F32, dict(), 1283, 4, "paired<8,64,4>+c64"),
    ("m64", M64F32, dict(magnitude=True, frames_per_block=64), 1283, 7, "pairs_sliding<8,4>+mag"),
    # schedule 7: 4 pairs on request, 8 where the single-wave kernel runs 4 waves per SIMD and the LDS holds them, else 6
    ("m56", M56, dict(schedule=7, tile_waves=4, frames_per_block=64), 643, 7, "pairs_sliding<4,2>"),
    ("m56", M56, dict(schedule=7, tile_waves=6, frames_per_block=64), 963, 7, "pairs_sliding<6,3>+c64"),
    ("m56", M56, dict(schedule=7, tile_waves=8, frames_per_block=64), 1283, 7, "pairs_sliding<8,4>+c64"),
    ("m56", M56, dict(), 2603, 7, "pairs_sliding<8,4>+c64"),
    ("m128", CFG5, dict(schedule=7, tile_waves=4, frames_per_block=64), 643, 7, "pairs_sliding<4,2>"),
    ("m128", CFG5, dict(schedule=7, tile_waves=6, frames_per_block=64), 963, 7, "pairs_sliding<6,3>+c64"),
    ("m128", CFG5, dict(schedule=7, tile_waves=8, frames_per_block=64), 963, 7, "pairs_sliding<6,3>+c64"),
    ("m128", CFG5, dict(), 2603, 11, "overlap+c64"),
    ("m128", CFG5, dict(magnitude=True), 2603, 11, "overlap+mag"),
    ("m128", CFG5, dict(schedule=3), 483, 3, "shared<8,24>"),
    # 8-byte samples at M = 128: no 8-wave tile fits the LDS, every key takes the 4-wave tile of 64-frame runs
    ("m128", CFG5F32, dict(schedule=3), 643, 3, "shared<4,64>"),
    ("m128", CFG5F32, dict(schedule=3, tile_waves=8, frames_per_block=64), 643, 3, "shared<4,64>"),
    ("m128", CFG5F32, dict(), 2603, 0, "sliding+c64"),
    # channel-major defaults per band count: 2 waves x 4 chunks up to M = 32, 4 x 2 above
    ("m32", M32, dict(channel_major=True), 163, 8, "tile_t<2,4>"),
    ("m32", M32, dict(channel_major=True, schedule=8, tile_waves=4, frames_per_block=8), 83, 8, "tile_t<4,1>"),
    ("m32", M32, dict(channel_major=True, schedule=2), 163, 2, "tile<8>+cm"),   # forced: tile_waves, not the default's 16
    ("m32", M32, dict(channel_major=True, schedule=2, tile_waves=16), 323, 2, "tile<16>+cm"),
    # M = 1024: the teams by default (by slabs for a channel-major handle), the twin kernel with and without a grid cap
    ("m1024", M1024, dict(), 2603, 6, "teams+c64"),
    ("m1024", M1024, dict(magnitude=True), 2603, 6, "teams+mag"),
    ("m1024", M1024, dict(channel_major=True), 2603, 6, "teams+c64"),
    ("m1024", DUO, dict(), 2603, 13, "twin+c64"),
    ("m1024", DUO, dict(frames_per_block=64, grid=2), 163, 13, "twin+c64"),
    ("m1024", DUO, dict(magnitude=True, frames_per_block=64), 163, 13, "twin+mag"),
    # small banks: output type and layout compiled in
    ("m8", M8F32, dict(), 2603, 0, "seg+c64"),
    ("m8", M8F32, dict(magnitude=True), 2603, 0, "seg+mag"),
    ("m8", M8F32, dict(channel_major=True), 2603, 0, "seg+cm+c64"),
    ("m8", M8F32, dict(channel_major=True, magnitude=True), 2603, 0, "seg+cm+mag"),
    # a schedule the plan lacks: its sliding runs, at the run length the policy gives that schedule
    ("m256", CFG3I8, dict(schedule=4), 163, 0, "sliding+c64"),
    ("m256", CFG3I8, dict(schedule=3), 63, 0, "sliding+c64"),
    ("m256", CFG3I8, dict(schedule=6, frames_per_block=64), 163, 0, "sliding+c64"),
]
ENTRY_REQUEST_KEYS = ("schedule", "frames_per_block", "channel_major", "magnitude", "tile_waves", "nontemporal", "grid",
                      "experiment", "out_aligned16")


def plan_entry_for(row, frames, num_cus, opts):
    assert set(opts) <= set(ENTRY_REQUEST_KEYS), opts
    return L.plan_entry(row, frames, num_cus, **opts)
