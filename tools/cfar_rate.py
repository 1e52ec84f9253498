"""CFAR detector rate on one MI355X: one JSON line per element kind x block length x share of cells over.

Each case is one pfb_cfar_process_async call on 2^--log2n cells (float32 powers, or 8-byte bank cells) of exponential
noise, with about 1e-4 of the cells raised far over the threshold, or none: the median of --reps device-event-timed
runs (torch.cuda.Event on the current stream) after --warmup, the handle reset before each.  The detector reads the cells
twice (block sums, over bits), so gbytes_per_s = 2 * bytes_in / time.  Every line carries the rate of
pfb_measure_stream_copy at the same bytes_in from the same process: the 1:2 copy yardstick, whose figure is bytes moved
(read + written) per second.  The last line of each element kind repeats one case with the call's pointer one cell off
a 16-byte boundary (offset_cells = 1), where the kernels read single cells instead of 16-byte vectors.  Nothing is
gated: the figures go into DESIGN.md section 19.

    python tools/cfar_rate.py [--log2n 26] [--reps 7] [--out profiles/cfar_rate.jsonl]
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
from sdr_channelizer_amd import Cfar  # noqa: E402
from sdr_channelizer_amd import _lib as L  # noqa: E402

BLOCKS = (64, 1024)
SHARES = (1e-4, 0.0)
ALPHA = 30.0   # e^-30 of the noise cells cross it: none in 2^26


def timed(run, warmup: int, reps: int) -> float:
    stream = torch.cuda.current_stream()
    times = []
    for i in range(warmup + reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        run()
        b.record(stream)
        b.synchronize()
        if i >= warmup:
            times.append(a.elapsed_time(b))
    return float(np.median(times))


def make_cells(n: int, share: float, element: str, dev) -> torch.Tensor:
    g = torch.Generator(device=dev).manual_seed(1)
    p = torch.empty(n, dtype=torch.float32, device=dev).exponential_(1.0, generator=g)
    if share > 0:
        at = torch.randint(0, n, (int(n * share),), device=dev, generator=g)
        p[at] *= 1e4
    if element == "power":
        return p
    cells = torch.empty((n, 2), dtype=torch.float32, device=dev)
    cells[:, 0] = p
    cells[:, 1] = torch.randint(0, 64, (n,), dtype=torch.int32, device=dev, generator=g).view(torch.float32)
    return cells


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2n", type=int, default=26)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    stream = torch.cuda.current_stream()
    lib = L.load()
    n = 1 << args.log2n
    sink = open(args.out, "a") if args.out else None
    for element, eb in (("power", 4), ("cell", 8)):
        nbytes = n * eb
        copy = C.c_double()
        L.check(lib.pfb_measure_stream_copy(-1, nbytes, 10, C.byref(copy)), "pfb_measure_stream_copy")
        for share in SHARES:
            whole = make_cells(n + 4, share, element, dev)
            for block, offset in [(b, 0) for b in BLOCKS] + ([(BLOCKS[0], 1)] if share == 0.0 else []):
                x = whole[offset:offset + n]
                out = torch.zeros((1 << 15, 6), dtype=torch.int64, device=dev)
                count = torch.zeros(1, dtype=torch.int64, device=dev)
                with Cfar(block, 1, 8, ALPHA, element=element) as det:
                    det.set_stream(stream.cuda_stream)

                    def run():
                        det.reset()
                        det.process_async(x, out, count)

                    ms = timed(run, args.warmup, args.reps)
                    stats, kernel = det.stats, det.last_kernel
                gbs = 2 * nbytes / ms / 1e6
                line = json.dumps({
                    "element": element, "cells": n, "bytes_in": nbytes, "block_cells": block, "guard_blocks": 1,
                    "train_blocks": 8, "alpha": ALPHA, "share_raised": share, "offset_cells": offset,
                    "cells_over": stats["cells_over"],
                    "detections": int(count.item()), "dropped": stats["dropped"], "kernel": kernel, "ms": round(ms, 4),
                    "gcells_per_s": round(n / ms / 1e6, 2), "gbytes_per_s": round(gbs, 1),
                    "copy_gbytes_per_s": round(copy.value / 1e9, 1), "of_copy": round(gbs / (copy.value / 1e9), 3)})
                print(line, flush=True)
                if sink:
                    sink.write(line + "\n")
                    sink.flush()
            del x, whole
            torch.cuda.empty_cache()
    if sink:
        sink.close()


if __name__ == "__main__":
    main()
