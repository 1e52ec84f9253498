"""Waterfall time on one MI355X: one JSON line per element kind, layout, width and bin length, appended to
profiles/waterfall_rate.jsonl.

A device matrix of 2^--log2bytes bytes (1 GiB) goes through Waterfall.process(sync=False), pfb_wf_process_async, for

    element  complex (rows and columns), magnitude and power (rows)
    W        8, 56, 64, 560, 768, 1024
    B        16, 4096 and 2^19 / W rows

each timed between two device events on the stream the work runs on (median over --reps after --warmup).  Every line
carries the rate of pfb_measure_stream_copy at the same bytes_in from the same run: the 1:2 copy yardstick, whose
figure is bytes moved (read + written) per second.  The reduction reads bytes_in and writes 16 bytes per (bin, column).
Nothing is gated: the figures go into DESIGN.md section 16.

--file PATH [--bands M] also records once the wall time of waterfall_from_iq_file on that record against the way
without it: process_iq_file to the host, then numpy.

    python tools/waterfall_rate.py [--log2bytes 30] [--reps 5] [--only complex] [--out profiles/waterfall_rate.jsonl]
"""
from __future__ import annotations

import argparse
import ctypes as C
import importlib
import json
import os
import sys
import time

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


def emit(line: dict, out: str) -> None:
    print(json.dumps(line), flush=True)
    with open(out, "a") as f:
        f.write(json.dumps(line) + "\n")


def file_wall(W, path: str, bands: int, max_rows: int, out: str, label: str) -> None:
    """wall time of the record -> image route against process_iq_file to the host + numpy, second run of each"""
    from sdr_channelizer_amd import Channelizer
    for _ in range(2):
        t0 = time.perf_counter()
        img = W.waterfall_from_iq_file(path, bands, max_rows=max_rows, power=True)
        t_wf = time.perf_counter() - t0
    for _ in range(2):
        t0 = time.perf_counter()
        with Channelizer(bands, power=True) as ch:
            y, info = ch.process_iq_file(path)
        B = img.bin_rows
        full = y.shape[0] // B
        blk = y[:full * B].reshape(full, B, bands)
        ref = (blk.max(1), blk.mean(1, dtype=np.float64), blk.min(1), blk.argmax(1))
        t_np = time.perf_counter() - t0
    assert np.array_equal(ref[0], img.power_max[:full]) and np.array_equal(ref[3], img.peak_row[:full])
    emit({"setting": "record_to_image", "bands": bands, "samples": int(info.packet.numSamples), "bin_rows": B,
          "image_rows": int(img.power_max.shape[0]), "waterfall_from_iq_file_s": round(t_wf, 3),
          "process_iq_file_then_numpy_s": round(t_np, 3), "matrix_bytes": int(y.nbytes), "label": label}, out)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2bytes", type=int, default=30)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--only", default="")
    ap.add_argument("--label", default="")
    ap.add_argument("--file", default="")
    ap.add_argument("--bands", type=int, default=56)
    ap.add_argument("--max-rows", type=int, default=1024)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "waterfall_rate.jsonl"))
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    from sdr_channelizer_amd import _lib as L
    W = importlib.import_module("sdr_channelizer_amd.waterfall")
    torch.cuda.set_device(0)
    lib = L.load()
    if args.file:
        file_wall(W, args.file, args.bands, args.max_rows, args.out, args.label)
        return
    nbytes = 1 << args.log2bytes
    copy = C.c_double()
    L.check(lib.pfb_measure_stream_copy(-1, nbytes, 10, C.byref(copy)), "pfb_measure_stream_copy")
    stream = torch.cuda.current_stream().cuda_stream
    flat = torch.empty(nbytes // 4, dtype=torch.float32, device="cuda")
    flat.uniform_(0.01, 1)
    for element, layout in (("complex", "rows"), ("complex", "columns"), ("magnitude", "rows"), ("power", "rows")):
        if args.only and element not in args.only.split(","):
            continue
        elems = nbytes // (8 if element == "complex" else 4)
        x = torch.view_as_complex(flat.view(-1, 2)) if element == "complex" else flat
        for width in (8, 56, 64, 560, 768, 1024):
            rows = elems // width
            m = x[:rows * width].view(rows, width) if layout == "rows" else x[:rows * width].view(width, rows)
            for B in (16, 4096, (1 << 19) // width):
                with W.Waterfall(width, B, element, layout) as wf:
                    wf.set_stream(stream)
                    out = torch.empty((rows // B, width, 16), dtype=torch.uint8, device="cuda")

                    def run():
                        wf.reset()
                        wf.process(m, out=out, sync=False)

                    ms = measure(run, args.warmup, args.reps)
                bytes_in, bytes_out = rows * width * (elems and nbytes // elems), rows // B * width * 16
                emit({"element": element, "layout": layout, "width": width, "bin_rows": B, "rows": rows,
                      "bytes_in": bytes_in, "bytes_out": bytes_out, "ms": round(ms, 4),
                      "read_gbytes_per_s": round(bytes_in / ms / 1e6, 1),
                      "moved_gbytes_per_s": round((bytes_in + bytes_out) / ms / 1e6, 1),
                      "copy_gbytes_per_s": round(copy.value / 1e9, 1), "label": args.label}, args.out)
                del out


if __name__ == "__main__":
    main()
