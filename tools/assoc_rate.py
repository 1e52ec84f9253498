"""PDW association rate on one MI355X: one JSON line per case.

A case is a list of N synthetic items already on the device -- the rows of a channelized pulse table: pulses at a
steady rate, each a run of dwells through neighbouring cells with one-tick rows at its edges, `overlap` pulses in the
air at once in cells of their own -- and one of two calls on it: pfb_assoc_links (the edge search alone) and
pfb_assoc_run (the whole association).  The mean number of items that start inside an item's window is about 8 with 4
pulses in the air and about 64 with 48.  Both calls are synchronous, so a call is timed by the host clock around it: it
ends in a stream synchronise.  The figure is the median of --reps calls after --warmup, with the spread (min, max)
beside it.  Every case is timed in both tiers (pfb_assoc_set_tier) on the same list.  Beside every figure stands the
time the numpy restatement (tests/assoc_ref.py) takes for the same call on the same list, for scale only: one run.
Every device result is compared with the restatement's.

Nothing is gated: the figures go into DESIGN.md section 28.

    python tools/assoc_rate.py [--log2n 16 18 20] [--reps 5] [--out profiles/assoc_rate.jsonl]
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
import assoc_ref as R  # noqa: E402
from sdr_channelizer_amd import PulseAssociator  # noqa: E402
from sdr_channelizer_amd import _lib as L  # noqa: E402
from sdr_channelizer_amd.associate import groups_to_numpy  # noqa: E402

ROWS = 16          # rows of one pulse: 8 dwells, 4 one-tick rows at each edge
PULSE = 64         # ticks of one pulse


def scene(n: int, overlap: int, seed: int) -> np.ndarray:
    """n items: pulses of 64 ticks, `overlap` of them in the air at once, each in a band of 20 cells of its own"""
    rng = np.random.default_rng(seed)
    pulses = n // ROWS + 1
    first = (np.arange(pulses, dtype=np.int64) * PULSE) // overlap
    band = (np.arange(pulses) % max(overlap, 1)) * 20
    k = np.arange(8)
    start = np.concatenate([(first[:, None] + 8 * k[None, :]).ravel(), np.repeat(first, 4), np.repeat(first + PULSE - 1, 4)])
    length = np.concatenate([np.full(pulses * 8, 9), np.ones(pulses * 8, np.int64)])
    cell = np.concatenate([(band[:, None] + 4 + k[None, :]).ravel(), (band[:, None] + np.arange(4)[None, :]).ravel(),
                           (band[:, None] + 12 + np.arange(4)[None, :]).ravel()])
    weight = rng.random(start.size).astype(np.float32)
    order = np.argsort(start, kind="stable")[:n]
    return R.items(start[order].astype(np.uint64), length[order], cell[order], weight[order])


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
    ap.add_argument("--log2n", type=int, nargs="*", default=[16, 18, 20])
    ap.add_argument("--overlap", type=int, nargs="*", default=[4, 48], help="pulses in the air at once")
    ap.add_argument("--reps", type=int, default=5)
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

    for log2n in args.log2n:
        for overlap in args.overlap:
            n = 1 << log2n
            it = scene(n, overlap, 7 * log2n + overlap)
            c = R.Cfg(Rc=1, g=0, K=16 * overlap)
            x = torch.from_numpy(it.view(np.uint8).reshape(-1, 24).copy()).cuda()
            start, lim = it["start"], it["start"] + it["length"]
            window = float(np.mean(np.searchsorted(start, lim, side="right") - np.arange(n) - 1))
            for what in ("links", "run"):
                t0 = time.perf_counter()
                ref = R.links(it, c) if what == "links" else R.run(it, c)
                ref_ms = round((time.perf_counter() - t0) * 1e3, 3)
                for tier in (1, 2):
                    with PulseAssociator(**c.settings()) as a:
                        L.check(lib.pfb_assoc_set_tier(a._h, tier), "pfb_assoc_set_tier")
                        call = (lambda: a.links(x)) if what == "links" else (lambda: a.run(x))
                        times, out = timed(call, args.warmup, args.reps)
                        kernel, stats = a.last_kernel, a.stats
                    if what == "links":
                        same = all(g.tobytes() == r.tobytes() for g, r in zip(out, ref))
                    else:
                        same = (groups_to_numpy(out[0]).tobytes() == ref[0].tobytes()
                                and out[1].cpu().numpy().tobytes() == ref[1].tobytes()
                                and {k: stats[k] for k in R.STATS} == ref[2])
                    ms = float(np.median(times))
                    row = dict(call=what, items=n, overlap=overlap, window_items=c.K, mean_window=round(window, 2),
                               kernels=kernel, ms=round(ms, 4), ms_min=round(min(times), 4), ms_max=round(max(times), 4),
                               reps=len(times), mitems_per_s=round(n / ms / 1e3, 3), numpy_ms=ref_ms, same_bytes=same)
                    if what == "run":
                        row.update(**stats)
                    emit(**row)
    if sink:
        sink.close()


if __name__ == "__main__":
    main()
