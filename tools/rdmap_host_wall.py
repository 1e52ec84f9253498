"""Host time per call of the two range-Doppler detectors on one MI355X: one JSON line per unit.

A repetition is the wall time (time.perf_counter) of --calls pfb_*_process_async calls of one 8 x 256 map of unit
exponential noise followed by one sync, on a handle that was reset and synced before the clock started; --reps of them
after --warmup.  The map is small so that the host side of a call -- the checks, the parameter block, four launches and
the count's copy -- is what the figure follows; the kernels are the same bytes on both sides of a comparison.  --tree
takes the package (and its built library) from another checkout, so that two commits are measured by alternating
processes in one session; compare the change's median with the spread of the parent's repetitions.  Nothing is gated
and no counters are collected: the figures go into profiles/rdmap_share_host_wall.txt.

    python tools/rdmap_host_wall.py [--tree DIR] [--reps 5] [--out FILE]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ND, R, WD, GR, TR, PD, ALPHA, RANK = 8, 256, 1, 2, 8, 1, 8.0, 36


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--label", default="")
    ap.add_argument("--calls", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.tree))
    from sdr_channelizer_amd import OsCfar, RangeDopplerCfar
    from sdr_channelizer_amd import _lib as L
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    arch = torch.cuda.get_device_properties(0).gcnArchName
    g = torch.Generator(device=dev).manual_seed(1)
    maps = torch.empty((1, ND, R), dtype=torch.float32, device=dev).exponential_(1.0, generator=g)
    out = torch.zeros((1024, 4), dtype=torch.int64, device=dev)
    count = torch.zeros(1, dtype=torch.int64, device=dev)
    sink = open(args.out, "a") if args.out else None
    units = (("rdcfar", lambda: RangeDopplerCfar(ND, R, WD, GR, TR, ALPHA, peak_half_width=PD)),
             ("oscfar", lambda: OsCfar(ND, R, WD, GR, TR, RANK, ALPHA, peak_half_width=PD)))
    for unit, make in units:
        with make() as det:
            ms = []
            for i in range(args.warmup + args.reps):
                det.reset()
                det.sync()
                t0 = time.perf_counter()
                for _ in range(args.calls):
                    det.process_async(maps, out, count)
                det.sync()
                if i >= args.warmup:
                    ms.append((time.perf_counter() - t0) * 1e3)
            assert det.next_map == args.calls
            line = json.dumps({
                "unit": unit, "label": args.label, "arch": arch, "library": os.path.relpath(L.LIB_PATH, args.tree),
                "rows": ND, "gates": R, "calls": args.calls, "detections_per_call": int(count.item()),
                "kernel": det.last_kernel, "ms": [round(v, 3) for v in ms], "ms_median": round(float(np.median(ms)), 3),
                "ms_min": round(min(ms), 3), "ms_max": round(max(ms), 3),
                "us_per_call_median": round(float(np.median(ms)) * 1e3 / args.calls, 3),
                "reps": args.reps, "warmup": args.warmup, "counters": "none"})
        print(line, flush=True)
        if sink:
            sink.write(line + "\n")
            sink.flush()
    if sink:
        sink.close()


if __name__ == "__main__":
    main()
