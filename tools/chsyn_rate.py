"""Channel-synthesizer kernel rate on one MI355X: one JSON line per M x D x output x route.

Kernel ms = median of --reps device-event-timed calls (torch.cuda.Event around pfb_chsyn_process_async on the current
stream) after --warmup, on 2^--log2n channel values (F = 2^log2n / M frames: a record-sized matrix, far more than the
256 MiB Infinity Cache holds); algorithmic bytes = F * (8 M + out_bytes * D): every input value read once, every output
sample written once.  Both routes run at the fused shapes (P_g = 12), the generic route alone at M = 560 and 1024.
Next to each figure stands the byte-mix copy yardstick, pfb_measure_mix_copy at read 1 : write 2 with short-lived
waves over the same number of bytes.  The library has no copy kernel for the synthesizer's own, read-heavy mixes
(1 : 1 down to 4 : 1), so the yardstick says what the memory system gives a streaming kernel of this size, not a bound
for this mix.

    python tools/chsyn_rate.py [--log2n 27] [--reps 5] [--only fused|generic] [--out profiles/chsyn_rate.jsonl]
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sdr_channelizer_amd import ChannelSynthesizer, design_synthesis_taps  # noqa: E402
from sdr_channelizer_amd import _lib as L  # noqa: E402

PEAK = 8e12
OUT_BYTES = {"cf32": 8, "int16": 4}
FUSED_M = (56, 64, 128, 256)
GENERIC_ONLY_M = (560, 1024)
P_G = 12


def measure(s: ChannelSynthesizer, y: torch.Tensor, warmup: int, reps: int) -> float:
    stream = torch.cuda.current_stream()
    s.set_stream(stream.cuda_stream)
    times = []
    for i in range(warmup + reps):
        s.reset()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        out = s.process(y, sync=False)
        b.record(stream)
        b.synchronize()
        del out
        if i >= warmup:
            times.append(a.elapsed_time(b))
    return float(np.median(times))


def copy_yardstick(total_bytes: int, iters: int, cache: dict) -> float:
    """bytes per second of the 1 : 2 copy kernel (two rows per wave) moving total_bytes"""
    bytes_in = (total_bytes // 3) & ~0xfff
    if bytes_in not in cache:
        r = C.c_double()
        L.check(L.load().pfb_measure_mix_copy(0, bytes_in, 2, 2, iters, C.byref(r)), "pfb_measure_mix_copy")
        cache[bytes_in] = r.value
    return cache[bytes_in]


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2n", type=int, default=27)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--only", default="")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    sink = open(args.out, "a") if args.out else None
    yard: dict = {}
    for M in FUSED_M + GENERIC_ONLY_M:
        F = (1 << args.log2n) // M
        g = torch.Generator(device=dev).manual_seed(1)
        y = torch.view_as_complex(torch.randn((F, M, 2), dtype=torch.float32, device=dev, generator=g))
        for D in (M, M // 2):
            taps = design_synthesis_taps(M, D, P_G)
            for output in ("cf32", "int16"):
                algo = F * (8 * M + OUT_BYTES[output] * D)
                bound = copy_yardstick(algo, args.reps, yard)
                for route in (("fused", "generic") if M in FUSED_M else ("generic",)):
                    if args.only and route != args.only:
                        continue
                    with ChannelSynthesizer(M, taps, D, output=output, route=route) as s:
                        ms = measure(s, y, args.warmup, args.reps)
                        plan, kernel = s.plan, s.last_kernel
                    tbs = algo / (ms * 1e-3) / 1e12
                    line = json.dumps({
                        "route": route, "M": M, "D": D, "taps_per_channel": P_G, "q": plan.q, "output": output,
                        "tile_frames": plan.tile_frames, "kernel": kernel, "frames": F, "kernel_ms": round(ms, 4),
                        "msamples_per_s": round(F * D / ms / 1e3, 1), "algorithmic_bytes": algo,
                        "tb_per_s": round(tbs, 3), "fraction_of_8tbs": round(tbs * 1e12 / PEAK, 4),
                        "copy_1to2_tb_per_s": round(bound / 1e12, 3),
                        "fraction_of_copy_1to2": round(tbs * 1e12 / bound, 4)})
                    print(line, flush=True)
                    if sink:
                        sink.write(line + "\n")
                        sink.flush()
        del y
        torch.cuda.empty_cache()
    if sink:
        sink.close()


if __name__ == "__main__":
    main()
