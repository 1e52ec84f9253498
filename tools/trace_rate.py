"""Envelope and full-rate trace time on one MI355X: one JSON line per format and setting, appended to
profiles/trace_rate.jsonl.

A device buffer of 2^--log2n int16 samples (int8 and cf32: the same byte count) goes through

    envelope   Trace.envelope(sync=False) with bins of 64, 4096 and 2^19 samples: pfb_trace_envelope_async
    samples    pfb_trace_samples with both outputs (mag and phase_deg)

each timed between two device events on the stream the work runs on (median over --reps after --warmup).  Every line
carries the rate of pfb_measure_stream_copy at the same bytes_in from the same run: the 1:2 copy yardstick, whose
figure is bytes moved (read + written) per second.  The envelope reads bytes_in and writes 48 bytes per bin; `samples`
reads bytes_in and writes 8 bytes per sample.  Nothing is gated: the figures go into DESIGN.md section 14.

    python tools/trace_rate.py [--log2n 28] [--reps 5] [--only int16] [--out profiles/trace_rate.jsonl] [--label TEXT]
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def measure(fn, warmup: int, reps: int) -> float:
    stream = torch.cuda.current_stream()
    for _ in range(warmup):
        fn()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record(stream)
        fn()
        b.record(stream)
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms))


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2n", type=int, default=28, help="int16 samples; the other formats get the same bytes")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--only", default="")
    ap.add_argument("--label", default="")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "trace_rate.jsonl"))
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    from sdr_channelizer_amd import Trace
    from sdr_channelizer_amd import _lib as L
    torch.cuda.set_device(0)
    lib = L.load()
    nbytes = 4 << args.log2n
    copy = C.c_double()
    L.check(lib.pfb_measure_stream_copy(-1, nbytes, 10, C.byref(copy)), "pfb_measure_stream_copy")
    stream = torch.cuda.current_stream().cuda_stream
    for fmt, bw, dt, bps in (("int16", 12, torch.int16, 4), ("int8", 8, torch.int8, 2), ("cf32", 12, torch.float32, 8)):
        if args.only and fmt not in args.only.split(","):
            continue
        n = nbytes // bps
        iq = torch.empty((n, 2), dtype=dt, device="cuda")
        if dt == torch.float32:
            iq.uniform_(-1, 1)
        else:
            iq.random_(-(1 << (bw - 1)), 1 << (bw - 1))
        base = {"format": fmt, "bit_width": bw, "samples": n, "bytes_in": nbytes,
                "copy_gbytes_per_s": round(copy.value / 1e9, 1), "label": args.label}
        lines = []
        for B in (64, 4096, 1 << 19):
            with Trace(B, fmt, bw) as tr:
                tr.set_stream(stream)
                out = torch.empty((n // B, 48), dtype=torch.uint8, device="cuda")

                def run():
                    tr.reset()
                    tr.envelope(iq, out=out, sync=False)

                ms = measure(run, args.warmup, args.reps)
            lines.append(dict(base, setting=f"envelope_B{B}", bin_samples=B, ms=round(ms, 4), bytes_out=n // B * 48))
            del out
        with Trace(64, fmt, bw) as tr:
            tr.set_stream(stream)
            mag = torch.empty(n, dtype=torch.float32, device="cuda")
            ph = torch.empty(n, dtype=torch.float32, device="cuda")

            def run():
                L.check(lib.pfb_trace_samples(tr._h, C.c_void_p(iq.data_ptr()), n, C.c_void_p(mag.data_ptr()),
                                              C.c_void_p(ph.data_ptr()), L.PFB_MEM_DEVICE), "pfb_trace_samples")

            ms = measure(run, args.warmup, args.reps)   # synchronous: the event pair still brackets the kernel
        lines.append(dict(base, setting="samples_mag_phase", bin_samples=0, ms=round(ms, 4), bytes_out=8 * n))
        del mag, ph, iq
        torch.cuda.empty_cache()
        for line in lines:
            line["gsamples_per_s"] = round(n / line["ms"] / 1e6, 2)
            line["read_gbytes_per_s"] = round(nbytes / line["ms"] / 1e6, 1)
            line["moved_gbytes_per_s"] = round((nbytes + line["bytes_out"]) / line["ms"] / 1e6, 1)
            print(json.dumps(line), flush=True)
            with open(args.out, "a") as f:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
