"""Pulse-Doppler integration rate on one MI355X: one JSON line per Doppler length x output kind.

Each case is one pfb_pd_process_async call on 2^--log2n complex64 samples of noise cut into whole intervals of
K = ND pulses at pri = num_gates = --pri (every sample is a gate: the call reads each byte once, where it lies): the
median of --reps device-event-timed runs (torch.cuda.Event on the handle's stream) after --warmup, the handle reset
before each, with the spread (min, max) beside it.  bytes_moved = bytes read + bytes written; the input alone (1 GiB at
the default) is four times the 256 MB Infinity Cache.  Every line carries pfb_measure_stream_copy at the same
bytes_moved from the same process (its bytes_in = bytes_moved / 3: the yardstick reads one part and writes two), and
of_copy, the case's bytes per second over the yardstick's.  Nothing is gated: the figures go into DESIGN.md section 20.

    python tools/pd_rate.py [--log2n 27] [--pri 4096] [--reps 7] [--out profiles/pd_rate.jsonl]
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
from sdr_channelizer_amd import PulseDoppler  # noqa: E402
from sdr_channelizer_amd import _lib as L  # noqa: E402

LENGTHS = (8, 16, 32, 64, 128, 256, 512, 1024)
KINDS = ("complex", "power", "best", "noncoherent")


def timed(run, stream, warmup: int, reps: int) -> list:
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
    ap.add_argument("--log2n", type=int, default=27)
    ap.add_argument("--pri", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--lengths", type=int, nargs="*", default=list(LENGTHS))
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    stream = torch.cuda.current_stream()
    lib = L.load()
    n, pri = 1 << args.log2n, args.pri
    g = torch.Generator(device=dev).manual_seed(1)
    x = torch.randn((n, 2), dtype=torch.float32, device=dev, generator=g).view(torch.complex64).reshape(-1)
    count = torch.zeros(1, dtype=torch.int64, device=dev)
    sink = open(args.out, "a") if args.out else None
    for nd in args.lengths:
        cpis = n // (nd * pri)
        for kind in KINDS:
            with PulseDoppler(pri, nd, pri, 0, None, nd, kind) as pd:
                pd.set_stream(stream.cuda_stream)
                assert pd.cpis_for(n) == cpis
                per = int(pd.plan.cpi_outputs)
                out = torch.empty(cpis * per * (2 if kind == "best" else 1),
                                  dtype=torch.complex64 if kind == "complex" else torch.float32, device=dev)

                def run():
                    pd.reset()
                    pd.process_async(x, out, count)

                times = timed(run, stream, args.warmup, args.reps)
                kernel, tile = pd.last_kernel, int(pd.plan.tile_gates)
            assert int(count.item()) == cpis
            moved = cpis * nd * pri * 8 + out.numel() * out.element_size()
            copy = C.c_double()
            L.check(lib.pfb_measure_stream_copy(-1, moved // 3, 10, C.byref(copy)), "pfb_measure_stream_copy")
            ms = float(np.median(times))
            rate = moved / ms / 1e6
            line = json.dumps({
                "doppler_length": nd, "output": kind, "pri": pri, "num_gates": pri, "num_pulses": nd, "cpis": cpis,
                "samples": cpis * nd * pri, "bytes_moved": moved, "tile_gates": tile, "kernel": kernel,
                "ms": round(ms, 4), "ms_min": round(min(times), 4), "ms_max": round(max(times), 4), "reps": len(times),
                "gsamples_per_s": round(cpis * nd * pri / ms / 1e6, 2), "gbytes_per_s": round(rate, 1),
                "copy_gbytes_per_s": round(copy.value / 1e9, 1), "of_copy": round(rate / (copy.value / 1e9), 3)})
            print(line, flush=True)
            if sink:
                sink.write(line + "\n")
                sink.flush()
            del out
            torch.cuda.empty_cache()
    if sink:
        sink.close()


if __name__ == "__main__":
    main()
