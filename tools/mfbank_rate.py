"""Matched-filter bank rate on one MI355X against the way the same question was answered before the bank: one JSON line
per NFFT x H.

The bank: one pfb_mfbank_process_async call (best output) on a stream of 2^--log2n int16 samples.  The yardstick, timed
in the same process on the same samples: H MatchedFilter power passes, hypothesis h with the replica modulated to bin
q_h, each writing its full-rate row, then torch.max over the H rows (power and index) -- every pass repeats the load and
the forward FFT.  Both are medians of --reps device-event-timed runs (torch.cuda.Event on the current stream) after
--warmup.  ms_per_hypothesis = bank_ms / H is what one more hypothesis costs the bank.

    python tools/mfbank_rate.py [--log2n 24] [--reps 5] [--K 507] [--out profiles/mfbank_rate.jsonl]
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sdr_channelizer_amd import MatchedFilter, MatchedFilterBank  # noqa: E402

LENGTHS = (1024, 2048, 4096)
HYPOTHESES = (1, 8, 64)


def make_input(n: int, dev) -> torch.Tensor:
    g = torch.Generator(device=dev).manual_seed(1)
    return torch.randint(-2048, 2048, (2 * n,), dtype=torch.int16, device=dev, generator=g)


def timed(run, warmup: int, reps: int) -> float:
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
    return float(np.median(times))


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2n", type=int, default=24)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--K", type=int, default=507)   # a Barker-13 pulse of 13 x 39 samples
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    stream = torch.cuda.current_stream()
    n, K = 1 << args.log2n, args.K
    F = n - K + 1
    x = make_input(n, dev)
    rng = np.random.default_rng(5)
    r = (rng.standard_normal(K) + 1j * rng.standard_normal(K)).astype(np.complex64)
    sink = open(args.out, "a") if args.out else None
    for nfft in LENGTHS:
        for H in HYPOTHESES:
            first_bin = -(H // 2)
            cells = torch.empty((F, 2), dtype=torch.float32, device=dev)
            with MatchedFilterBank(r, "int16", 12, first_bin=first_bin, num_hypotheses=H, fft_length=nfft) as bank:
                bank.set_stream(stream.cuda_stream)

                def run_bank():
                    bank.reset()
                    bank.process(x, out=cells, sync=False)

                bank_ms = timed(run_bank, args.warmup, args.reps)
                kernel, plan = bank.last_kernel, bank.plan
            del cells
            rows = torch.empty((H, F), dtype=torch.float32, device=dev)
            ramp = np.arange(K)
            filters = [MatchedFilter((r * np.exp(2j * np.pi * (first_bin + h) * ramp / nfft)).astype(np.complex64), "int16", 12,
                                     "power", fft_length=nfft, route="fused") for h in range(H)]
            for mf in filters:
                mf.set_stream(stream.cuda_stream)

            def run_yardstick():
                for h, mf in enumerate(filters):
                    mf.reset()
                    mf.process(x, out=rows[h], sync=False)
                return torch.max(rows, dim=0)

            yard_ms = timed(run_yardstick, args.warmup, args.reps)
            yard_kernel = filters[0].last_kernel
            for mf in filters:
                mf.release()
            del rows
            torch.cuda.empty_cache()
            line = json.dumps({
                "format": "int16", "K": K, "nfft": nfft, "hypotheses": H, "block_outputs": plan.block_outputs,
                "lds_bytes": plan.lds_bytes, "samples": n, "kernel": kernel, "bank_ms": round(bank_ms, 4),
                "ms_per_hypothesis": round(bank_ms / H, 4), "msamples_per_s": round(n / bank_ms / 1e3, 1),
                "hypothesis_msamples_per_s": round(n * H / bank_ms / 1e3, 1), "yardstick": f"{H} x {yard_kernel} + torch.max",
                "yardstick_ms": round(yard_ms, 4), "yardstick_over_bank": round(yard_ms / bank_ms, 3)})
            print(line, flush=True)
            if sink:
                sink.write(line + "\n")
                sink.flush()
    if sink:
        sink.close()


if __name__ == "__main__":
    main()
