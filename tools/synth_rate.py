"""Pulse-train generation time on one MI355X: one JSON line per format, appended to profiles/synth_rate.jsonl.

2^--log2n samples of the benchmark stream are made three ways into device memory, each timed between two device
events on the stream the work runs on (median over --reps after --warmup):

    native_ms   PulseTrain.generate(sync=False): one pfb_synth_generate_async kernel
    torch_ms    synth.pulsed_iq_torch: the same integers from elementwise torch kernels over int64 temporaries
    fill_ms     Tensor.fill_ of the same byte count: the write bound of the output alone

The first two outputs are compared once (torch.equal) before anything is timed.  The tool fails if the native
generator is slower than pulsed_iq_torch; the ratio to the fill is recorded, not gated.

    python tools/synth_rate.py [--log2n 28] [--reps 5] [--only int16] [--out profiles/synth_rate.jsonl] [--label TEXT]
"""
from __future__ import annotations

import argparse
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
    ap.add_argument("--log2n", type=int, default=28)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--only", default="")
    ap.add_argument("--label", default="")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "synth_rate.jsonl"))
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    from sdr_channelizer_amd import PulseTrain, synth
    torch.cuda.set_device(0)
    n = 1 << args.log2n
    slower = []
    for fmt, bw, dt in (("int16", 12, torch.int16), ("int8", 8, torch.int8)):
        if args.only and fmt not in args.only.split(","):
            continue
        with PulseTrain(sample_format=fmt, bit_width=bw) as pt:
            pt.set_stream(torch.cuda.current_stream().cuda_stream)
            out = torch.empty((n, 2), dtype=dt, device="cuda")
            pt.generate(n, out=out)
            want = synth.pulsed_iq_torch(n, bw, dtype=dt)
            assert torch.equal(out, want), f"{fmt}: the native stream is not pulsed_iq_torch's"
            del want
            native_ms = measure(lambda: pt.generate(n, out=out, sync=False), args.warmup, args.reps)
            fill_ms = measure(lambda: out.fill_(1), args.warmup, args.reps)
            torch_ms = measure(lambda: synth.pulsed_iq_torch(n, bw, dtype=dt), args.warmup, args.reps)
        nbytes = out.numel() * out.element_size()
        line = {"format": fmt, "bit_width": bw, "samples": n, "bytes": nbytes, "native_ms": round(native_ms, 4),
                "torch_ms": round(torch_ms, 4), "fill_ms": round(fill_ms, 4),
                "native_gsamples_per_s": round(n / native_ms / 1e6, 2), "native_gbytes_per_s": round(nbytes / native_ms / 1e6, 1),
                "fill_gbytes_per_s": round(nbytes / fill_ms / 1e6, 1), "native_over_fill": round(native_ms / fill_ms, 3),
                "torch_over_native": round(torch_ms / native_ms, 2), "label": args.label}
        print(json.dumps(line), flush=True)
        with open(args.out, "a") as f:
            f.write(json.dumps(line) + "\n")
        if native_ms > torch_ms:
            slower.append(fmt)
        del out
        torch.cuda.empty_cache()
    assert not slower, f"the native generator lost to pulsed_iq_torch for {slower}"


if __name__ == "__main__":
    main()
