"""PDW clustering rate on one MI355X: one JSON line per case.

A case is a list of N synthetic (u, v) items already on the device -- `clusters` blobs a few cells wide on a grid of
64 x 1, 1024 x 8 or 1024 x 1024 cells, a twentieth of the items strays -- and one call on it: pfb_cluster_histogram
(step 1), pfb_cluster_cell_roots (steps 1 to 4), pfb_cluster_run without and with the partition, and
pfb_cluster_gather of a tick list by the run's order.  The calls are synchronous (the gather is followed by a
synchronise), so a call is timed by the host clock around it.  The figure is the median of --reps calls after
--warmup, with the spread (min, max) beside it; a stage's time is the difference of two rows.  Where the grid allows it
the histogram is timed in both tiers (pfb_cluster_set_tier).  Every device result is compared with the numpy
restatement's (tests/cluster_ref.py), whose own time stands beside it for scale only: one run.

With --deint the deinterleaver's scene (tools/deint_rate.py: 32 trains, each given a frequency cell of its own with a
spread of a few cells) is timed whole (pfb_deint_run on the one list) and by cluster (deinterleave_clustered's device
work: the clustering, the gather and one pfb_deint_run per cluster), in the same session.

Nothing is gated: the figures go into DESIGN.md section 29.

    python tools/cluster_rate.py [--log2n 12 16 20] [--reps 5] [--deint 12 14] [--out profiles/cluster_rate.jsonl]
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
import cluster_cases as CC  # noqa: E402
import cluster_ref as R  # noqa: E402
from sdr_channelizer_amd import Deinterleaver, PulseClusterer  # noqa: E402
from sdr_channelizer_amd import _lib as L  # noqa: E402
from sdr_channelizer_amd.cluster import groups_to_numpy  # noqa: E402

GRIDS = ((64, 1), (1024, 8), (1024, 1024))


def scene(n: int, U: int, V: int, clusters: int, seed: int) -> np.ndarray:
    """n items: `clusters` blobs on a lattice that keeps them apart, a twentieth strays"""
    rng = np.random.default_rng(seed)
    k = np.arange(clusters)
    side_v = max(V // 2, 1) if V <= 8 else int(np.ceil(np.sqrt(clusters)))
    side_u = -(-clusters // side_v)
    cu, cv = ((k // side_v) * U) // side_u + U // (2 * side_u), ((k % side_v) * V) // side_v + V // (2 * side_v)
    who = rng.integers(0, clusters, n)
    # a spread of a cell where the lattice leaves room for it
    u = cu[who] + (np.rint(rng.normal(0, 1.0, n)).astype(np.int64) if U // side_u >= 8 else 0)
    v = cv[who] + (np.rint(rng.normal(0, 0.6, n)).astype(np.int64) if V // side_v >= 8 else 0)
    s = rng.random(n) < 0.05
    u[s], v[s] = rng.integers(0, U, int(s.sum())), rng.integers(0, V, int(s.sum()))
    return R.items_of(u, v)


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


def host(x):
    return x if isinstance(x, np.ndarray) else x.cpu().numpy()


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2n", type=int, nargs="*", default=[12, 16, 20])
    ap.add_argument("--clusters", type=int, nargs="*", default=[4, 1024])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--deint", type=int, nargs="*", default=[], help="log2 of the deinterleaver scenes to time")
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

    def stat(times):
        ms = float(np.median(times))
        return dict(ms=round(ms, 4), ms_min=round(min(times), 4), ms_max=round(max(times), 4), reps=len(times))

    for log2n in args.log2n:
        for U, V in GRIDS:
            for clusters in args.clusters:
                if clusters > U * V // 4:
                    continue                        # 1024 clusters do not fit 64 cells
                n = 1 << log2n
                it = scene(n, U, V, clusters, 7 * log2n + clusters)
                # a cell is dense well above what the strays alone put into it
                c = R.Cfg(U, V, 1, 1 if V > 1 else 0, minc=2 + n // (4 * U * V), minp=8, border=True)
                x = torch.from_numpy(it.view(np.int32).reshape(-1, 2).copy()).cuda()
                ticks = torch.arange(n, dtype=torch.int64, device="cuda")
                t0 = time.perf_counter()
                ref = R.run(it, c)
                ref_ms = round((time.perf_counter() - t0) * 1e3, 3)
                base = dict(items=n, grid="%dx%d" % (U, V), blobs=clusters, clusters=ref[5])
                tiers = (1, 2) if c.cells <= CC.LDS_CELLS else (2,)
                with PulseClusterer(**c.settings()) as a:
                    for tier in tiers:
                        L.check(lib.pfb_cluster_set_tier(a._h, tier), "pfb_cluster_set_tier")
                        times, out = timed(lambda: a.histogram(x), args.warmup, args.reps)
                        emit(call="histogram", **base, kernels=a.last_kernel, **stat(times),
                             same_bytes=out.tobytes() == R.histogram(it, c).tobytes())
                    L.check(lib.pfb_cluster_set_tier(a._h, 0), "pfb_cluster_set_tier")
                    times, out = timed(lambda: a.cell_roots(x), args.warmup, args.reps)
                    emit(call="cell_roots", **base, kernels=a.last_kernel, **stat(times),
                         same_bytes=out.tobytes() == R.cell_roots(R.histogram(it, c), c)[0].tobytes())
                    times, out = timed(lambda: a.run(x, want_order=False), args.warmup, args.reps)
                    emit(call="run_without_order", **base, kernels=a.last_kernel, **stat(times), **a.stats,
                         same_bytes=groups_to_numpy(out[0]).tobytes() == ref[0].tobytes() and host(out[1]).tobytes() == ref[1].tobytes())
                    times, out = timed(lambda: a.run(x), args.warmup, args.reps)
                    same = (groups_to_numpy(out[0]).tobytes() == ref[0].tobytes() and host(out[1]).tobytes() == ref[1].tobytes()
                            and host(out[2]).tobytes() == ref[2].tobytes() and host(out[3]).tobytes() == ref[3].tobytes()
                            and a.stats == ref[4])
                    emit(call="run", **base, kernels=a.last_kernel, **stat(times), numpy_ms=ref_ms,
                         mitems_per_s=round(n / float(np.median(times)) / 1e3, 3), same_bytes=same)
                    order = out[2]
                    times, out = timed(lambda: a.gather(ticks, order), args.warmup, args.reps)
                    emit(call="gather", **base, kernels=a.last_kernel, **stat(times),
                         same_bytes=host(out).tobytes() == ref[2].astype(np.int64).tobytes())

    for log2n in args.deint:
        n, trains = 1 << log2n, 32
        t, who, periods = CC.scene_with_trains(n, trains, 1)
        items = CC.scene_features(who)
        D, K = CC.SCENE_DEINT, CC.SCENE_CLUSTER
        x = torch.from_numpy(t.view(np.int64)).cuda()
        xi = torch.from_numpy(items.view(np.int32).reshape(-1, 2).copy()).cuda()
        with Deinterleaver(D.pmin, D.pmax, D.W, **D.settings()) as d, PulseClusterer(**K.settings()) as a:
            times, out = timed(lambda: d.run(x), args.warmup, args.reps)
            emit(call="deint_whole", pulses=n, trains=trains, emitters=len(out[0]), **d.stats, **stat(times))

            def by_cluster():
                rec, _, order, offsets = a.run(xi)
                cut = a.gather(x, order)
                off = offsets.cpu().numpy()
                found = tried = 0
                for k in range(len(off) - 2):
                    r, _ = d.run(cut[int(off[k]):int(off[k + 1])])
                    found, tried = found + len(r), tried + d.stats["candidates_tried"]
                return len(off) - 2, found, tried

            times, (G, found, tried) = timed(by_cluster, args.warmup, args.reps)
            emit(call="deint_by_cluster", pulses=n, trains=trains, clusters=G, emitters=found, candidates_tried=tried,
                 **stat(times))
    if sink:
        sink.close()


if __name__ == "__main__":
    main()
