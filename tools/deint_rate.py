"""Deinterleaver rate on one MI355X: one JSON line per case.

A case is a list of N synthetic arrival ticks already on the device -- 4 or 32 jittered trains with one pulse in ten
dropped and 2 % stray pulses -- and one of three calls on it: pfb_deint_run (the whole search), pfb_deint_histogram
(step 1 on the whole list) and pfb_deint_successors (steps 3 and 4 at the first train's period).  All three are
synchronous, so a call is timed by the host clock around it: it ends in a stream synchronise.  The figure is the median
of --reps calls after --warmup, with the spread (min, max) beside it.  The histogram is timed in both tiers
(pfb_deint_set_tier) on the same list, the run with both marking tiers.  Beside every figure stands the time the numpy
restatement (tests/deint_ref.py) takes for the same call on the same list, for scale only: one run, lists up to
--ref-max pulses.  Every device result is compared with the restatement's where that was computed.

Nothing is gated: the figures go into DESIGN.md section 25.

    python tools/deint_rate.py [--log2n 12 14 16 18 20] [--reps 5] [--out profiles/deint_rate.jsonl]
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
sys.path.insert(0, os.path.join(ROOT, "tests"))
import deint_ref as R  # noqa: E402
from sdr_channelizer_amd import Deinterleaver  # noqa: E402
from sdr_channelizer_amd import _lib as L  # noqa: E402
from sdr_channelizer_amd.deinterleave import records_to_numpy  # noqa: E402

PMIN, PMAX = 1000, 9000


def scene(n: int, trains: int, seed: int) -> np.ndarray:
    """n ticks: `trains` periods spread over 2000 .. 4000 ticks, jitter -1 .. 1, a tenth dropped, 2 % strays"""
    rng = np.random.default_rng(seed)
    periods = np.unique(np.linspace(2000, 4000, trains).astype(np.int64) | 1)
    rate = float(np.sum(0.9 / periods)) / 0.98
    span = int(n / rate * 1.05)
    parts = []
    for p in periods:
        k = np.arange((span - 1) // p)
        x = int(rng.integers(0, p)) + k * p + rng.integers(-1, 2, k.size)
        parts.append(x[rng.random(k.size) >= 0.1])
    parts.append(rng.integers(0, span, n // 50))
    t = np.sort(np.maximum(np.concatenate(parts), 0))
    assert len(t) >= n
    return t[:n].astype(np.uint64)


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
    ap.add_argument("--log2n", type=int, nargs="*", default=[12, 14, 16, 18, 20])
    ap.add_argument("--trains", type=int, nargs="*", default=[4, 32])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--ref-max", type=int, default=1 << 16, help="the longest list the numpy restatement is timed on")
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

    for log2n in args.log2n:
        for trains in args.trains:
            n = 1 << log2n
            t = scene(n, trains, 7 * log2n + trains)
            x = torch.from_numpy(t.view(np.int64)).cuda()
            # bin_ticks 1 gives 8001 bins, the LDS tier's size; the search itself is timed at 4 ticks a bin
            for what, W in (("histogram", 1), ("successors", 4), ("run", 4)):
                c = R.Cfg(pmin=PMIN, pmax=PMAX, W=W, Lv=16, detect=30, min_pulses=8, X=4, tol=5, fill=50, max_emitters=64)
                ref, ref_ms = None, None
                tau = 2001
                if n <= args.ref_max:
                    t0 = time.perf_counter()
                    ref = {"histogram": lambda: R.histogram(t, c), "successors": lambda: R.lengths(t, c, tau),
                           "run": lambda: R.run(t, c)}[what]()
                    ref_ms = round((time.perf_counter() - t0) * 1e3, 3)
                tiers = {"histogram": ((1, 0), (2, 0)), "successors": ((0, 0),), "run": ((0, 1), (0, 2))}[what]
                for hist_tier, mark_tier in tiers:
                    with Deinterleaver(c.pmin, c.pmax, c.W, **c.settings()) as d:
                        L.check(lib.pfb_deint_set_tier(d._h, hist_tier, mark_tier), "pfb_deint_set_tier")
                        call = {"histogram": lambda: d.histogram(x), "successors": lambda: d.successors(x, tau),
                                "run": lambda: d.run(x)}[what]
                        times, out = timed(call, args.warmup, args.reps)
                        kernel, stats = d.last_kernel, d.stats
                    same = None
                    if ref is not None:
                        if what == "histogram":
                            same = out.tobytes() == ref.tobytes()
                        elif what == "successors":
                            same = all(a.tobytes() == b.tobytes() for a, b in zip(out, ref))
                        else:
                            same = (records_to_numpy(out[0]).tobytes() == ref[0].tobytes()
                                    and out[1].cpu().numpy().tobytes() == ref[1].tobytes())
                    ms = float(np.median(times))
                    row = dict(call=what, pulses=n, trains=trains, bins=c.NB, kernels=kernel, ms=round(ms, 4),
                               ms_min=round(min(times), 4), ms_max=round(max(times), 4), reps=len(times),
                               mpulses_per_s=round(n / ms / 1e3, 3), numpy_ms=ref_ms, same_bytes=same)
                    if what == "run":
                        row.update(emitters=len(out[0]), **stats)
                    emit(**row)
    if sink:
        sink.close()


if __name__ == "__main__":
    main()
