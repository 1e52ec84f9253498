"""Epoch-folding rate on one MI355X: one JSON line per case.

Each case is one pfb_fold_process_async call on 2^--log2n float32 cells (exponential noise plus a train of period
2048) already on the device, over consecutive candidate periods around a centre: the median of --reps
device-event-timed runs (torch.cuda.Event on the handle's stream) after --warmup, the handle reset before each, with the
spread (min, max) beside it.  The reset is a memset of the profiles, a few MiB at most, and is inside the window.

Every candidate adds every cell once, so the work is cells x candidates additions, and -- each candidate re-reading the
buffer from the caches -- read_gbytes_per_s = 4 N NC / t is the equivalent read rate.  Every line carries the time
pfb_measure_stream_copy takes to move the same buffer (it reads one part and writes two: copy_ms = 3 * 4 N over its
rate) from the same process, for scale.  Nothing is gated: the figures go into DESIGN.md section 21.

    python tools/fold_rate.py [--log2n 24] [--reps 7] [--out profiles/fold_rate.jsonl]
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
from sdr_channelizer_amd import PriFold  # noqa: E402
from sdr_channelizer_amd import _lib as L  # noqa: E402

# (bin_cells, candidates, centre period)
CASES = ((4, 64, 2048), (4, 512, 2048), (4, 4096, 2048 + 1024), (16, 512, 32768), (1, 512, 2048),
         (8, 512, 8192), (32, 512, 65536), (64, 512, 131072))      # the last three: the other widths fold_tile takes


def timed(run, stream, warmup: int, reps: int) -> list:
    times = []
    for i in range(warmup + reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        run()
        b.record(stream)
        b.synchronize()
        if i >= warmup:
            times.append(a.elapsed_time(b))
    return times


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2n", type=int, default=24)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--cases", type=int, nargs="*", default=list(range(len(CASES))))
    ap.add_argument("--tier", type=int, default=0, help="pfb_fold_set_tier: 0 the library's choice, 1 direct, 2 tile")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    stream = torch.cuda.current_stream()
    lib = L.load()
    n = 1 << args.log2n
    g = torch.Generator(device=dev).manual_seed(1)
    x = -torch.log(torch.rand(n, dtype=torch.float32, device=dev, generator=g).clamp_min(1e-30))
    x[700::2048] += 4.0                               # the train: one cell in 2048 at five times the noise
    copy = C.c_double()
    L.check(lib.pfb_measure_stream_copy(-1, 4 * n, 10, C.byref(copy)), "pfb_measure_stream_copy")
    copy_ms = 3 * 4 * n / copy.value * 1e3
    sink = open(args.out, "a") if args.out else None
    for i in args.cases:
        bin_cells, nc, centre = CASES[i]
        periods = np.arange(centre - nc // 2, centre - nc // 2 + nc)
        with PriFold(periods, bin_cells) as fold:
            fold.set_stream(stream.cuda_stream)
            if args.tier:
                L.check(lib.pfb_fold_set_tier(fold._h, args.tier), "pfb_fold_set_tier")

            def run():
                fold.reset()
                fold.process_async(x)

            times = timed(run, stream, args.warmup, args.reps)
            kernel = fold.last_kernel
            assert fold.next_index == n
            rec = fold.scores()
            plan_bytes = int(fold.plan.profile_bytes)
        best = rec[int(np.argmax(rec["peak_mean"]))]
        ms = float(np.median(times))
        line = json.dumps({
            "bin_cells": bin_cells, "candidates": nc, "first_period": int(periods[0]), "last_period": int(periods[-1]),
            "cells": n, "profile_bytes": plan_bytes, "kernel": kernel,
            "ms": round(ms, 4), "ms_min": round(min(times), 4), "ms_max": round(max(times), 4), "reps": len(times),
            "gcell_candidates_per_s": round(n * nc / ms / 1e6, 2), "read_gbytes_per_s": round(4 * n * nc / ms / 1e6, 1),
            "copy_ms": round(copy_ms, 4), "copy_gbytes_per_s": round(copy.value / 1e9, 1),
            "highest_mean_period": int(best["period"]), "highest_mean_bin": int(best["peak_bin"])})
        print(line, flush=True)
        if sink:
            sink.write(line + "\n")
            sink.flush()
    if sink:
        sink.close()


if __name__ == "__main__":
    main()
