"""Matched-filter kernel rate on one MI355X: one JSON line per format x K x NFFT x output x route.

Kernel ms = median of --reps device-event-timed calls (torch.cuda.Event around pfb_mf_process_async on the current
stream) after --warmup, on a stream of 2^--log2n samples -- far more than the 256 MiB Infinity Cache holds; algorithmic
bytes = N * bytes_in + (N - K + 1) * bytes_out (every input sample read once, every output written once).  Next to
each figure stands what pfb_measure_mix_copy reaches for the same byte mix with short-lived waves (read 1 : write 2 or
1 : 4; the other mixes have no copy kernel and print null): the bound a kernel with that traffic cannot beat.

    python tools/mf_rate.py [--log2n 27] [--reps 5] [--only fused|partitioned] [--out profiles/mf_rate.jsonl]
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
from sdr_channelizer_amd import MatchedFilter  # noqa: E402
from sdr_channelizer_amd import _lib as L  # noqa: E402

PEAK = 8e12
BYTES_IN = {"int8": 2, "int16": 4, "cf32": 8}
BIT_WIDTH = {"int8": 8, "int16": 12, "cf32": 1}
# route, format, output, K, fft lengths
CASES = [
    ("fused", "int16", "complex", 13, (1024, 2048, 4096)),
    ("fused", "int16", "complex", 104, (1024, 2048, 4096)),
    ("fused", "int16", "complex", 512, (1024, 2048, 4096)),
    ("fused", "int16", "complex", 1024, (2048, 4096)),
    ("fused", "int16", "complex", 2048, (4096,)),
    ("fused", "int16", "power", 13, (1024, 4096)),
    ("fused", "int16", "power", 1024, (2048, 4096)),
    ("fused", "int8", "complex", 13, (1024, 4096)),
    ("fused", "int8", "power", 13, (1024, 4096)),
    ("fused", "cf32", "complex", 13, (1024, 4096)),
    ("partitioned", "int16", "complex", 1024, (2048, 4096)),
    ("partitioned", "int16", "complex", 5600, (1024, 2048, 4096)),
    ("partitioned", "int16", "power", 56000, (2048, 4096)),
]


def make_input(fmt: str, n: int, dev) -> torch.Tensor:
    g = torch.Generator(device=dev).manual_seed(1)
    if fmt == "cf32":
        return torch.randn(2 * n, dtype=torch.float32, device=dev, generator=g)
    lim = 128 if fmt == "int8" else 2048
    return torch.randint(-lim, lim, (2 * n,), dtype=torch.int8 if fmt == "int8" else torch.int16, device=dev, generator=g)


def measure(mf: MatchedFilter, x: torch.Tensor, out: torch.Tensor, warmup: int, reps: int) -> float:
    stream = torch.cuda.current_stream()
    mf.set_stream(stream.cuda_stream)
    times = []
    for i in range(warmup + reps):
        mf.reset()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        mf.process(x, out=out, sync=False)
        b.record(stream)
        b.synchronize()
        if i >= warmup:
            times.append(a.elapsed_time(b))
    return float(np.median(times))


def copy_bound(bytes_in: int, ratio: float, iters: int, cache: dict):
    """bytes per second of the copy kernel with this read : write mix (pfb_measure_mix_copy, two rows per wave)"""
    if ratio not in (2.0, 4.0):
        return None
    key = (bytes_in, ratio)
    if key not in cache:
        r = C.c_double()
        L.check(L.load().pfb_measure_mix_copy(0, bytes_in, int(ratio), 2, iters, C.byref(r)), "pfb_measure_mix_copy")
        cache[key] = r.value
    return cache[key]


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2n", type=int, default=27)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--only", default="")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    n = 1 << args.log2n
    sink = open(args.out, "a") if args.out else None
    bounds: dict = {}
    rng = np.random.default_rng(5)
    for route, fmt, output, K, lengths in CASES:
        if args.only and route != args.only:
            continue
        x = make_input(fmt, n, dev)
        F = n - K + 1
        bytes_out = 8 if output == "complex" else 4
        out = torch.empty(F, dtype=torch.complex64 if output == "complex" else torch.float32, device=dev)
        algo = n * BYTES_IN[fmt] + F * bytes_out
        bound = copy_bound(n * BYTES_IN[fmt], bytes_out / BYTES_IN[fmt], args.reps, bounds)
        r = (rng.standard_normal(K) + 1j * rng.standard_normal(K)).astype(np.complex64)
        for nfft in lengths:
            with MatchedFilter(r, fmt, BIT_WIDTH[fmt], output, fft_length=nfft, route=route) as mf:
                ms = measure(mf, x, out, args.warmup, args.reps)
                plan, kernel = mf.plan, mf.last_kernel
            tbs = algo / (ms * 1e-3) / 1e12
            line = json.dumps({
                "route": route, "format": fmt, "output": output, "K": K, "nfft": nfft, "partitions": plan.partitions,
                "block_outputs": plan.block_outputs, "kernel": kernel, "samples": n, "kernel_ms": round(ms, 4),
                "msamples_per_s": round(n / ms / 1e3, 1), "algorithmic_bytes": algo, "tb_per_s": round(tbs, 3),
                "fraction_of_8tbs": round(tbs * 1e12 / PEAK, 4),
                "copy_bound_tb_per_s": None if bound is None else round(bound / 1e12, 3),
                "fraction_of_copy_bound": None if bound is None else round(tbs * 1e12 / bound, 4)})
            print(line, flush=True)
            if sink:
                sink.write(line + "\n")
                sink.flush()
        del x, out
        torch.cuda.empty_cache()
    if sink:
        sink.close()


if __name__ == "__main__":
    main()
