"""Fractional-period folding and regrid rates on one MI355X: one JSON line per case and tier.

Folder.  tools/fold_rate.py's cases -- one process_async call on 2^--log2n float32 cells already on the device, over
consecutive candidate periods around a centre -- run three ways in one process: pfb_fold_process_async on the integer
periods (the yardstick), pfb_qfold_process_async on the same periods as Q32 integers, and pfb_qfold_process_async with
a fraction (0.37) added to every period.  Both tiers are forced where both exist.  Each figure is the median of --reps
device-event-timed runs (torch.cuda.Event on the handle's stream) after --warmup, with min and max beside it.  Both
units are timed the same way: the handle's reset is issued before the first event (pfb_qfold_reset also uploads the
candidates' states and waits for the stream, so it cannot sit inside a device-timed window), and only the fold is in
the window.  tools/fold_rate.py keeps pfb_fold_reset's memset inside its window; its figures are that much larger.

Regrid.  One pfb_regrid_process_async call on 2^--log2n random elements at a period of 2048.37 with rows of 2048,
complex64 and float32.  Beside each, pfb_measure_stream_copy in the same process on the same number of bytes moved
(that copy reads one part and writes two, the regrid reads one and writes one: bytes_in = moved / 3), so that both work
on a working set of the same size; the line carries bytes moved per second for both.

Nothing is gated: the figures go into DESIGN.md section 27.

    python tools/qfold_rate.py [--log2n 24] [--reps 7] [--out profiles/qfold_rate.jsonl]
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
from sdr_channelizer_amd import FinePriFold, PriFold, Regrid  # noqa: E402
from sdr_channelizer_amd import _lib as L  # noqa: E402

# (bin_cells, candidates, centre period): tools/fold_rate.py's
CASES = ((4, 64, 2048), (4, 512, 2048), (4, 4096, 2048 + 1024), (16, 512, 32768), (1, 512, 2048),
         (8, 512, 8192), (32, 512, 65536), (64, 512, 131072))
FRACTION = int(round(0.37 * 2 ** 32))


def timed(prepare, run, stream, warmup: int, reps: int) -> list:
    times = []
    for i in range(warmup + reps):
        prepare()
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
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    stream = torch.cuda.current_stream()
    lib = L.load()
    n = 1 << args.log2n
    g = torch.Generator(device=dev).manual_seed(1)
    x = -torch.log(torch.rand(n, dtype=torch.float32, device=dev, generator=g).clamp_min(1e-30))
    x[700::2048] += 4.0
    sink = open(args.out, "a") if args.out else None

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if sink:
            sink.write(line + "\n")
            sink.flush()

    for i in args.cases:
        bin_cells, nc, centre = CASES[i]
        periods = np.arange(centre - nc // 2, centre - nc // 2 + nc)
        q = periods.astype(np.uint64) << np.uint64(32)
        tiers = (1, 2) if bin_cells in (8, 16, 32, 64) else (1,)
        for tier in tiers:
            base = None
            for what in ("fold", "qfold_int", "qfold_frac"):
                if what == "fold":
                    h = PriFold(periods, bin_cells)
                    L.check(lib.pfb_fold_set_tier(h._h, tier), "pfb_fold_set_tier")
                    prepare, run = h.reset, (lambda: h.process_async(x))
                else:
                    h = FinePriFold(q + np.uint64(FRACTION if what == "qfold_frac" else 0), bin_cells)
                    L.check(lib.pfb_qfold_set_tier(h._h, tier, 0), "pfb_qfold_set_tier")
                    prepare, run = h.reset, (lambda: h.process_async(x))
                with h:
                    h.set_stream(stream.cuda_stream)
                    times = timed(prepare, run, stream, args.warmup, args.reps)
                    kernel = h.last_kernel
                    assert h.next_index == n
                    rec = h.scores()
                ms = float(np.median(times))
                base = ms if what == "fold" else base
                best = rec[int(np.argmax(rec["peak_mean"]))]
                emit({"unit": what, "bin_cells": bin_cells, "candidates": nc, "first_period": int(periods[0]),
                      "last_period": int(periods[-1]), "fraction": 0.37 if what == "qfold_frac" else 0.0, "cells": n,
                      "kernel": kernel, "default": kernel == h.plan.kernel.decode(),
                      "ms": round(ms, 4), "ms_min": round(min(times), 4), "ms_max": round(max(times), 4), "reps": len(times),
                      "ratio_to_fold": round(ms / base, 3), "read_gbytes_per_s": round(4 * n * nc / ms / 1e6, 1),
                      "highest_mean_bin": int(best["peak_bin"])})
    for dtype, tdtype in ((np.complex64, torch.complex64), (np.float32, torch.float32)):
        elem = np.dtype(dtype).itemsize
        y = torch.randn(n, dtype=tdtype, device=dev, generator=g)
        with Regrid(2048.37, 2048, 0, dtype) as rg:
            rg.set_stream(stream.cuda_stream)
            m = rg.outputs_for(n)
            out = torch.empty(m, dtype=tdtype, device=dev)
            count = torch.zeros(1, dtype=torch.int64, device=dev)
            times = timed(rg.reset, lambda: rg.process_async(y, out, count), stream, args.warmup, args.reps)
            assert int(count.item()) == m
        moved = 2 * m * elem
        copy = C.c_double()
        L.check(lib.pfb_measure_stream_copy(-1, moved // 3, 10, C.byref(copy)), "pfb_measure_stream_copy")
        ms = float(np.median(times))
        emit({"unit": "regrid", "elem_bytes": elem, "period": 2048.37, "row_samples": 2048, "inputs": n, "outputs": m,
              "bytes_moved": moved, "ms": round(ms, 4), "ms_min": round(min(times), 4), "ms_max": round(max(times), 4),
              "reps": len(times), "moved_gbytes_per_s": round(moved / ms / 1e6, 1), "copy_bytes_moved": 3 * (moved // 3),
              "copy_gbytes_per_s": round(copy.value / 1e9, 1),
              "fraction_of_copy": round(moved / ms / 1e6 / (copy.value / 1e9), 3)})
    if sink:
        sink.close()


if __name__ == "__main__":
    main()
