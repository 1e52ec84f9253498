"""Range-Doppler CFAR detector rate on one MI355X: one JSON line per case.

Each case is one pfb_rdcfar_process_async call on maps of unit exponential noise with about 1e-4 of the cells raised far
over the threshold: median, min and max of --reps device-event-timed runs (torch.cuda.Event on the current stream)
after --warmup, the handle reset before each.  The detector reads every cell once from memory (the halo comes again
through the caches), so gbytes_per_s = bytes_in / time.  Every line carries the rate of pfb_measure_stream_copy at the
same bytes_in from the same process: the 1:2 copy yardstick, whose figure is bytes moved (read + written) per second.
Every line also carries the parent route for the same maps: their PFB_PD_BEST cells (made beforehand, not timed)
through the Cfar loop of detect_pulse_train -- reset, process, flush and the records' copy to the host per map.  That
route decides one cell per gate, this one every cell of the map.  Nothing is gated and no counters are collected: the
figures go into DESIGN.md section 22.

    python tools/rdcfar_rate.py [--reps 7] [--out profiles/rdcfar_rate.jsonl]
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
from sdr_channelizer_amd import Cfar, RangeDopplerCfar  # noqa: E402
from sdr_channelizer_amd import _lib as L  # noqa: E402

ALPHA = 30.0   # e^-30 of the noise cells cross it: none in 2^24
SHARE = 1e-4
# (name, maps, rows, gates, Wd, Gr, Tr, Pd)
CASES = (("nd64", 128, 64, 2048, 1, 4, 16, 1),
         ("nd1024", 8, 1024, 2048, 1, 4, 16, 1),
         ("one_row", 256, 1, 65536, 0, 4, 16, 0),
         ("nd64_replica_guard", 128, 64, 2048, 1, 104, 64, 1))


def timed(run, warmup: int, reps: int) -> list[float]:
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
    return times


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    stream = torch.cuda.current_stream()
    lib = L.load()
    arch = torch.cuda.get_device_properties(0).gcnArchName
    sink = open(args.out, "a") if args.out else None
    for name, n, ND, R, Wd, Gr, Tr, Pd in CASES:
        g = torch.Generator(device=dev).manual_seed(1)
        maps = torch.empty((n, ND, R), dtype=torch.float32, device=dev).exponential_(1.0, generator=g)
        flat = maps.view(-1)
        flat[torch.randint(0, flat.numel(), (int(flat.numel() * SHARE),), device=dev, generator=g)] *= 1e4
        nbytes = flat.numel() * 4
        copy = C.c_double()
        L.check(lib.pfb_measure_stream_copy(-1, nbytes, 10, C.byref(copy)), "pfb_measure_stream_copy")
        out = torch.zeros((1 << 16, 4), dtype=torch.int64, device=dev)
        count = torch.zeros(1, dtype=torch.int64, device=dev)
        with RangeDopplerCfar(ND, R, Wd, Gr, Tr, ALPHA, peak_half_width=Pd) as det:
            det.set_stream(stream.cuda_stream)

            def run():
                det.reset()
                det.process_async(maps, out, count)

            ms = timed(run, args.warmup, args.reps)
            stats, kernel, lds, band = det.stats, det.last_kernel, int(det.plan.lds_bytes), int(det.plan.tile_rows)
        # the parent route: the strongest row per gate through the 1-D block detector, one map at a time
        power, row = maps.max(dim=1)
        cells = torch.stack([power, (row.to(torch.int32) - ND // 2).view(torch.float32)], dim=2).contiguous()
        found = 0
        with Cfar(64, 1, 8, ALPHA, element="cell", merge_gap=Gr) as old:
            old.set_stream(stream.cuda_stream)

            def run_old():
                nonlocal found
                found = 0
                for m in cells:
                    old.reset()
                    found += len(old.process(m).cpu()) + len(old.flush(dev).cpu())

            ms_old = timed(run_old, args.warmup, args.reps)
        med = float(np.median(ms))
        gbs = nbytes / med / 1e6
        line = json.dumps({
            "case": name, "arch": arch, "maps": n, "rows": ND, "gates": R, "cells": flat.numel(), "bytes_in": nbytes,
            "doppler_half_width": Wd, "guard_gates": Gr, "train_gates": Tr, "peak_half_width": Pd, "alpha": ALPHA,
            "share_raised": SHARE, "cells_over": stats["cells_over"], "detections": int(count.item()),
            "dropped": stats["dropped"], "kernel": kernel, "tile_rows": band, "lds_bytes": lds,
            "ms_median": round(med, 4), "ms_min": round(min(ms), 4), "ms_max": round(max(ms), 4),
            "gcells_per_s": round(flat.numel() / med / 1e6, 2), "gbytes_per_s": round(gbs, 1),
            "copy_gbytes_per_s": round(copy.value / 1e9, 1), "of_copy": round(gbs / (copy.value / 1e9), 4),
            "best_route_cells": n * R, "best_route_records": found,
            "best_route_ms_median": round(float(np.median(ms_old)), 4), "best_route_ms_min": round(min(ms_old), 4),
            "best_route_ms_max": round(max(ms_old), 4), "reps": args.reps, "warmup": args.warmup, "counters": "none"})
        print(line, flush=True)
        if sink:
            sink.write(line + "\n")
            sink.flush()
        del maps, flat, cells
        torch.cuda.empty_cache()
    if sink:
        sink.close()


if __name__ == "__main__":
    main()
