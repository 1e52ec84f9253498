"""Dwell analysis time per call on one MI355X: one JSON line per format and route.

A device-resident dwell of 2^--log2n samples of the benchmark pulse train (synth.pulsed_iq_torch: 100 us pulses every
millisecond at 0.5 full scale over Gaussian noise; complex64 = the same samples / 2048) goes through

    mean_skipfreq   analyze_dwell(statistic="mean", skip_freq=True)   the live loop: toa and snr only
    mean            analyze_dwell(statistic="mean")
    median          analyze_dwell(statistic="median")
    raw             extract_pdws_raw with both thresholds at --median-db  (what "median" is routed through)

call_ms = median over --reps of the time between two device events recorded around the call on the current stream;
the calls synchronise inside (noise floor and edge totals come back to the host), so this is the whole call as the
device sees it, host gaps included.  host_ms is the host clock around the same call.  --raw-only runs the last route
alone and needs nothing but extract_pdws_raw, so that --package-root can point at a checkout of an earlier commit.

    python tools/dwell_rate.py [--log2n 26] [--reps 20] [--only int16] [--raw-only] [--package-root DIR] [--label TEXT]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np
import torch


def measure(fn, warmup: int, reps: int):
    stream = torch.cuda.current_stream()
    for _ in range(warmup):
        out = fn()
    dev, host = [], []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t = time.perf_counter()
        a.record(stream)
        out = fn()
        b.record(stream)
        b.synchronize()
        host.append((time.perf_counter() - t) * 1e3)
        dev.append(a.elapsed_time(b))
    return float(np.median(dev)), float(np.median(host)), out


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2n", type=int, default=26)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--only", default="")
    ap.add_argument("--mean-db", type=float, default=5.7)     # mean |x| of the stream is 0.068: threshold 0.25
    ap.add_argument("--median-db", type=float, default=12.0)  # median |x| is 0.02: threshold 0.32 (tests/test_gpu_pdw.py)
    ap.add_argument("--raw-only", action="store_true")
    ap.add_argument("--label", default="", help="copied into every line (which checkout was measured)")
    ap.add_argument("--package-root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    args = ap.parse_args()
    sys.path.insert(0, args.package_root)
    from sdr_channelizer_amd import synth
    from sdr_channelizer_amd.pdw import extract_pdws_raw
    torch.cuda.set_device(0)
    n = 1 << args.log2n
    fs, fc = 56e6, 915e6
    for fmt in ("int16", "cf32"):
        if args.only and fmt not in args.only.split(","):
            continue
        iq = synth.pulsed_iq_torch(n, 12, device="cuda")
        if fmt == "cf32":
            iq = torch.view_as_complex((iq.to(torch.float32) / 2048.0).contiguous())
        routes = {"raw": lambda: extract_pdws_raw(iq, fs, fc, 0.0, snr_threshold_db=args.median_db,
                                                  trailing_threshold_db=args.median_db)}
        if not args.raw_only:
            from sdr_channelizer_amd import analyze_dwell
            routes = {
                "mean_skipfreq": lambda: analyze_dwell(iq, fs, fc, 0.0, snr_threshold_db=args.mean_db, skip_freq=True)[0],
                "mean": lambda: analyze_dwell(iq, fs, fc, 0.0, snr_threshold_db=args.mean_db)[0],
                "median": lambda: analyze_dwell(iq, fs, fc, 0.0, statistic="median", snr_threshold_db=args.median_db)[0],
                **routes,
            }
        for name, fn in routes.items():
            ms, host_ms, pdws = measure(fn, args.warmup, args.reps)
            print(json.dumps({"format": fmt, "route": name, "samples": n, "pulses": len(pdws), "call_ms": round(ms, 4),
                              "host_ms": round(host_ms, 4), "gsamples_per_s": round(n / ms / 1e6, 2),
                              "label": args.label}), flush=True)
        del iq
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
