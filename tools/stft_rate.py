"""STFT kernel rate on one MI355X: one JSON line per shape and kernel (fused, its loads and stores alone, forced generic).

Kernel ms = median of --reps device-event-timed launches (torch.cuda.Event around pfb_stft_process_async on the
current stream) after --warmup; algorithmic bytes = N * bytes_in + F * nfft * bytes_out (every input sample read once,
every output written once); fraction = (bytes / s) / 8 TB/s.  Kernel "loadstore" is the fused kernel with its loads and
stores only (pfb_stft_set_experiment, pfb_channelizer_dev.h): the memory part of the fused kernel's time.

    python tools/stft_rate.py [--log2n 30] [--reps 20] [--only headline] [--kernels fused,loadstore,generic]
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sdr_channelizer_amd import Stft  # noqa: E402
from sdr_channelizer_amd import _lib as L  # noqa: E402

PEAK = 8e12
# name, L, hop, nfft, format, bit width, output
SHAPES = [
    ("headline", 768, 768, 768, "int16", 12, "power"),   # spectrogram_my_iq.m: hamming(768), no overlap
    ("n1024_db", 1024, 1024, 1024, "int16", 12, "db"),   # generate_pulsed_iq.m:105 in dB
    ("n768_int8_complex", 768, 768, 768, "int8", 8, "complex"),
    ("n768_cf32_complex", 768, 768, 768, "cf32", 1, "complex"),
    ("n768_hop384", 768, 384, 768, "int16", 12, "power"),
    ("n768_hop192", 768, 192, 768, "int16", 12, "power"),
]
BYTES_IN = {"int8": 2, "int16": 4, "cf32": 8}


def make_input(fmt: str, n: int, dev) -> torch.Tensor:
    g = torch.Generator(device=dev).manual_seed(1)
    if fmt == "cf32":
        return torch.randn(2 * n, dtype=torch.float32, device=dev, generator=g)
    lim = 128 if fmt == "int8" else 2048
    dt = torch.int8 if fmt == "int8" else torch.int16
    return torch.randint(-lim, lim, (2 * n,), dtype=dt, device=dev, generator=g)


def measure(st: Stft, x: torch.Tensor, out: torch.Tensor, warmup: int, reps: int) -> float:
    stream = torch.cuda.current_stream()
    st.set_stream(stream.cuda_stream)
    for _ in range(warmup):
        st.reset()
        st(x, out=out, sync=False)
    times = []
    for _ in range(reps):
        st.reset()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        st(x, out=out, sync=False)
        b.record(stream)
        b.synchronize()
        times.append(a.elapsed_time(b))
    return float(np.median(times))


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2n", type=int, default=30)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--only", default="")
    ap.add_argument("--kernels", default="fused,loadstore,generic")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    n = 1 << args.log2n
    for name, Lw, H, nfft, fmt, bw, output in SHAPES:
        if args.only and name not in args.only.split(","):
            continue
        x = make_input(fmt, n, dev)
        F = (n - Lw) // H + 1
        odt = torch.complex64 if output == "complex" else torch.float32
        out = torch.empty((F, nfft), dtype=odt, device=dev)
        bytes_out = 8 if output == "complex" else 4
        algo = n * BYTES_IN[fmt] + F * nfft * bytes_out
        for kernel in args.kernels.split(","):
            with Stft(np.hamming(Lw), hop=H, fft_length=nfft, sample_format=fmt, bit_width=bw, output=output,
                      kernel="fused" if kernel == "loadstore" else kernel) as st:
                if kernel == "loadstore":
                    L.check(L.load().pfb_stft_set_experiment(st._h, 1), "pfb_stft_set_experiment")
                ms = measure(st, x, out, args.warmup, args.reps)
                name_k = st.last_kernel
            tbs = algo / (ms * 1e-3) / 1e12
            print(json.dumps({"shape": name, "L": Lw, "hop": H, "nfft": nfft, "format": fmt, "output": output,
                              "kernel": name_k, "samples": n, "frames": F, "kernel_ms": round(ms, 4),
                              "algorithmic_bytes": algo, "tb_per_s": round(tbs, 3),
                              "fraction_of_8tbs": round(tbs * 1e12 / PEAK, 4)}), flush=True)
        del x, out
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
