"""Modulation-on-pulse rate on one MI355X: one JSON line per case.

A case is a list of P pulses of one length at random starts in a random series already on the device (the list and
the outputs on the device too), measured by one tier forced through pfb_mop_set_tier: 1 = mop_wave, 2 = mop_group,
3 = mop_split + mop_join.  pfb_mop_measure is synchronous, so a call is timed by the host clock around it.  The figure
is the median of --reps calls after --warmup, with the spread (min, max) beside it; pulses per second and the bytes of
the measured samples per second follow from it.  A case whose pulses hold more than --max-samples samples together is
left out, and so are mop_wave on pulses over 2^16 samples and mop_split on pulses under 2^12 (a single part).  The
tiers' records are compared byte for byte (int16) on every case.

Nothing is gated: the thresholds between the tiers (kGroupMin, kSplitMin in csrc/pfb_mop.hip) are read off these
lines, which go into DESIGN.md section 26.

    python tools/mop_rate.py [--formats int16 cf32] [--log2len 4 5 ... 20] [--log2pulses 0 4 6 8 10 16 22] [--out profiles/mop_rate.jsonl]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from sdr_channelizer_amd import PulseModulation  # noqa: E402
from sdr_channelizer_amd import _lib as L  # noqa: E402
from sdr_channelizer_amd.pulse_mod import pack_pulses  # noqa: E402

TIERS = {1: "mop_wave", 2: "mop_group", 3: "mop_split+mop_join"}


def timed(call, warmup: int, reps: int):
    times, out = [], None
    for i in range(warmup + reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = call()
        torch.cuda.synchronize()
        if i >= warmup:
            times.append((time.perf_counter() - t0) * 1e3)
    return times, out


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--formats", nargs="*", default=["int16", "cf32"])
    ap.add_argument("--log2len", type=int, nargs="*", default=list(range(4, 21)))
    ap.add_argument("--log2pulses", type=int, nargs="*", default=[0, 4, 6, 8, 10, 16, 22])
    ap.add_argument("--log2series", type=int, default=24)
    ap.add_argument("--max-samples", type=int, default=1 << 28)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    torch.cuda.set_device(0)
    lib = L.load()
    sink = open(args.out, "a") if args.out else None

    def emit(**row):
        line = json.dumps(row)
        print(line, flush=True)
        if sink:
            sink.write(line + "\n")
            sink.flush()

    rows = 1 << args.log2series
    rng = np.random.default_rng(1)
    for fmt in args.formats:
        if fmt == "cf32":
            x = torch.randn(rows, 2, device="cuda").view(torch.complex64).reshape(-1)
            bps = 8
        else:
            x = torch.randint(-2048, 2048, (rows, 2), device="cuda", dtype=torch.int16)
            bps = 4
        with PulseModulation(fmt, 12 if fmt != "cf32" else 0, 0, 8) as m:
            for log2len in args.log2len:
                n = 1 << log2len
                for log2p in args.log2pulses:
                    count = 1 << log2p
                    if count * n > args.max_samples:
                        continue
                    plist = pack_pulses(rng.integers(0, rows - n + 1, count), np.full(count, n))
                    d_list = torch.from_numpy(plist.view(np.uint8)).cuda()
                    first = None
                    for t, name in TIERS.items():
                        if (t == 1 and log2len > 16) or (t == 3 and log2len < 12):
                            continue
                        L.check(lib.pfb_mop_set_tier(m._h, t, 0, 0), "pfb_mop_set_tier")
                        times, out = timed(lambda: m.measure(x, d_list), args.warmup, args.reps)
                        assert m.last_kernel == name
                        got = out[0].cpu().numpy().tobytes()
                        same = None
                        if fmt != "cf32":
                            same = first is None or got == first
                            first = got if first is None else first
                        ms = float(np.median(times))
                        emit(fmt=fmt, samples=n, pulses=count, tier=t, kernels=name, ms=round(ms, 4),
                             ms_min=round(min(times), 4), ms_max=round(max(times), 4), reps=len(times),
                             mpulses_per_s=round(count / ms / 1e3, 4), gbytes_per_s=round(count * n * bps / ms / 1e6, 3),
                             same_bytes=same)
    if sink:
        sink.close()


if __name__ == "__main__":
    main()
