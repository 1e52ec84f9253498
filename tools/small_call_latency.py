#!/usr/bin/env python3
"""Per-call cost of pfb_process on device-resident dwell buffers of 2^k samples (the recorder-loop shape: one call per
dwell): synchronous calls, and asynchronous (queued) calls with one sync at the end.

Each figure is the median of --rounds timed loops of --reps calls; `spread` is max - min over the rounds.  With --json
one JSON line per size and mode, for an A/B script to collect.  --experiment sets PFB_OPT_EXPERIMENT (2 = the history
update as a launch of its own, the A side of the one-launch-per-call A/B); --root loads the package of another
checkout instead of this one."""
import argparse
import json
import os
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--log2", type=int, nargs="+", default=[12, 16, 20, 24])
ap.add_argument("--reps", type=int, default=200)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--experiment", type=int, default=0)
ap.add_argument("--json", action="store_true")
args = ap.parse_args()

sys.path.insert(0, args.root)
import torch  # noqa: E402
from sdr_channelizer_amd import Channelizer, design_prototype, synth  # noqa: E402
from sdr_channelizer_amd import _lib as L  # noqa: E402

M, P = 64, 12
ch = Channelizer(M, taps=design_prototype(M, P), bit_width=12)
if args.experiment:
    ch.set_option(L.PFB_OPT_EXPERIMENT, args.experiment)
for k in args.log2:
    n = 1 << k
    iq = synth.pulsed_iq_torch(n, 12, device="cuda")
    out = torch.empty((n // M + 1, M), dtype=torch.complex64, device="cuda")
    for sync in (True, False):
        for _ in range(20):
            ch(iq, out=out, sync=sync)
        torch.cuda.synchronize()
        us = []
        for _ in range(args.rounds):
            t0 = time.perf_counter()
            for _ in range(args.reps):
                ch(iq, out=out, sync=sync)
            ch.sync()
            torch.cuda.synchronize()
            us.append((time.perf_counter() - t0) / args.reps * 1e6)
        us.sort()
        med, spread = us[len(us) // 2], us[-1] - us[0]
        if args.json:
            print(json.dumps({"log2_samples": k, "mode": "sync" if sync else "queued", "us_per_call": round(med, 2),
                              "spread_us": round(spread, 2), "rounds": [round(u, 2) for u in us]}))
        else:
            print(f"2^{k:2d} samples per call, {'sync ' if sync else 'async'}: {med:8.1f} us per call (spread {spread:5.1f}) "
                  f"= {n / (med * 1e-6) / 1e6:9.1f} MS/s")
