"""Ordered-statistic CFAR detector rate on one MI355X: one JSON line per case.

Each case is one pfb_oscfar_process_async call on maps of unit exponential noise with about 1e-4 of the cells raised far
over the threshold, at rank 3 N / 4: median, min and max of --reps device-event-timed runs (torch.cuda.Event on the
current stream) after --warmup, the handle reset before each.  The cases are those of tools/rdcfar_rate.py.  The
yardstick is the cell-averaging detector of the same build: every line carries pfb_rdcfar_process_async (CA) timed in
the same process on the same maps, and os_over_ca, the ratio of the two medians.  Every line also carries the rate of
pfb_measure_stream_copy at the same bytes_in from the same process: the 1:2 copy yardstick, whose figure is bytes moved
(read + written) per second.  Nothing is gated and no counters are collected: the figures go into DESIGN.md section 23.

    python tools/oscfar_rate.py [--reps 7] [--out profiles/oscfar_rate.jsonl]
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
from sdr_channelizer_amd import OsCfar, RangeDopplerCfar  # noqa: E402
from sdr_channelizer_amd import _lib as L  # noqa: E402

ALPHA = 30.0   # of the noise cells next to none cross it, with the mean or with the upper quartile
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
        N = 2 * Tr * (2 * Wd + 1)
        rank = 3 * N // 4
        results = {}
        for label, make in (("os", lambda: OsCfar(ND, R, Wd, Gr, Tr, rank, ALPHA, peak_half_width=Pd)),
                            ("ca", lambda: RangeDopplerCfar(ND, R, Wd, Gr, Tr, ALPHA, peak_half_width=Pd))):
            with make() as det:
                det.set_stream(stream.cuda_stream)

                def run():
                    det.reset()
                    det.process_async(maps, out, count)

                ms = timed(run, args.warmup, args.reps)
                results[label] = dict(ms=ms, stats=det.stats, kernel=det.last_kernel, lds=int(det.plan.lds_bytes),
                                      band=int(det.plan.tile_rows), found=int(count.item()))
        o, c = results["os"], results["ca"]
        med, med_ca = float(np.median(o["ms"])), float(np.median(c["ms"]))
        gbs = nbytes / med / 1e6
        line = json.dumps({
            "case": name, "arch": arch, "maps": n, "rows": ND, "gates": R, "cells": flat.numel(), "bytes_in": nbytes,
            "doppler_half_width": Wd, "guard_gates": Gr, "train_gates": Tr, "peak_half_width": Pd, "alpha": ALPHA,
            "training_cells": N, "rank": rank, "share_raised": SHARE, "cells_over": o["stats"]["cells_over"],
            "detections": o["found"], "dropped": o["stats"]["dropped"], "kernel": o["kernel"], "tile_rows": o["band"],
            "lds_bytes": o["lds"], "ms_median": round(med, 4), "ms_min": round(min(o["ms"]), 4),
            "ms_max": round(max(o["ms"]), 4), "gcells_per_s": round(flat.numel() / med / 1e6, 2),
            "gbytes_per_s": round(gbs, 1), "copy_gbytes_per_s": round(copy.value / 1e9, 1),
            "of_copy": round(gbs / (copy.value / 1e9), 4),
            "ca_kernel": c["kernel"], "ca_cells_over": c["stats"]["cells_over"], "ca_detections": c["found"],
            "ca_ms_median": round(med_ca, 4), "ca_ms_min": round(min(c["ms"]), 4), "ca_ms_max": round(max(c["ms"]), 4),
            "os_over_ca": round(med / med_ca, 3), "reps": args.reps, "warmup": args.warmup, "counters": "none"})
        print(line, flush=True)
        if sink:
            sink.write(line + "\n")
            sink.flush()
        del maps, flat
        torch.cuda.empty_cache()
    if sink:
        sink.close()


if __name__ == "__main__":
    main()
