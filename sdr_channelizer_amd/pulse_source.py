"""The pulse-train source on the GPU, over the C ABI (pfb_synth_* in include/pfb_channelizer.h).

The reference makes its test signals in MATLAB:

    generate_pulsed_iq.m      pulses of PW every PRI, LFM sweep (LFM_EXTENT), Barker-13 chips (BARKER_13)
    generate_training_iq.m    the same train from a random start index, int16(x*2^15), a format-1 .iq record

``PulseTrain`` is that source as a handle: ``generate`` returns any stretch of the endless integer stream (the stream
position is an argument, so every shard or chunk can be made on its own and any cutting gives the same bits),
``write_iq`` writes a record without holding it in memory.  The keyword defaults are ``synth.py``'s benchmark stream:
``pulse_train(n)`` holds the integers of ``synth.pulsed_iq_torch(n)``.  Nothing here computes samples on the CPU.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib as L
from . import synth
from ._handle import _NP_DTYPE, Handle, is_torch

_FMT = {"int8": L.PFB_FMT_INT8_IQ, "int16": L.PFB_FMT_INT16_IQ, "cf32": L.PFB_FMT_CF32}


def _config(sample_format="int16", bit_width=12, seed=synth.SEED, fs=synth.FS, f0=None, pw_s=synth.PW_S,
            pri_s=synth.PRI_S, pw=None, pri=None, first_pulse=0, record_samples=0, lfm_extent_hz=0.0, barker13=False,
            barker_degrees=False, phase_from_zero=False, round_matlab=False, amplitude=synth.AMPLITUDE,
            noise_sigma=synth.NOISE_SIGMA, device=-1) -> L.PfbSynthConfig:
    """pw / pri in samples win over pw_s / pri_s in seconds, which are rounded as the scripts round them
    (generate_training_iq.m:37-38); f0=None is the carrier synth.py draws from the seed."""
    flags = ((L.PFB_SYNTH_BARKER13 if barker13 else 0) | (L.PFB_SYNTH_BARKER_DEGREES if barker_degrees else 0) |
             (L.PFB_SYNTH_PHASE_FROM_ZERO if phase_from_zero else 0) | (L.PFB_SYNTH_ROUND_MATLAB if round_matlab else 0))
    return L.PfbSynthConfig(
        C.sizeof(L.PfbSynthConfig), _FMT[sample_format], int(bit_width), flags,
        int(round(fs * pw_s)) if pw is None else int(pw), int(round(fs * pri_s)) if pri is None else int(pri),
        int(seed) & 0xFFFFFFFF, int(device), int(first_pulse), int(record_samples), float(fs),
        synth._carrier(seed, fs) if f0 is None else float(f0), float(lfm_extent_hz), float(amplitude),
        float(noise_sigma))


def synth_params(table: bool = False, **kw):
    """What the library derives from a configuration (pfb_synth_describe; host only, needs no device): a
    PfbSynthParams, and with table=True also the 65536-entry int64 cos table."""
    cfg = _config(**kw)
    out = L.PfbSynthParams()
    tab = np.empty(65536, np.int64) if table else None
    L.check(L.load().pfb_synth_describe(C.byref(cfg), C.byref(out),
                                        tab.ctypes.data_as(C.POINTER(C.c_int64)) if table else None),
            "pfb_synth_describe")
    return (out, tab) if table else out


class PulseTrain(Handle):
    """One configured pulse train on one GPU.  Keywords: see ``_config``."""

    _kind, _destroy, _get_device = "pulse train", "pfb_synth_destroy", "pfb_synth_get_device"

    def __init__(self, **kw):
        self._h = C.c_void_p()
        lib = L.load()
        self.config = _config(**kw)
        self.fmt = int(self.config.sample_format)
        L.check(lib.pfb_synth_create(C.byref(self.config), C.byref(self._h)), "pfb_synth_create")
        self._created(lib)
        self.params = L.PfbSynthParams()
        L.check(lib.pfb_synth_describe(C.byref(self.config), C.byref(self.params), None), "pfb_synth_describe")

    def set_stream(self, hip_stream: int) -> None:
        L.check(self._lib.pfb_synth_set_stream(self._h, C.c_void_p(hip_stream)), "pfb_synth_set_stream")

    def sync(self) -> None:
        L.check(self._lib.pfb_synth_sync(self._h), "pfb_synth_sync")

    def generate(self, n: int, start: int = 0, out=None, device: bool = True, sync: bool = True):
        """Samples start .. start + n - 1 as an (n, 2) array of I, Q: a torch tensor on the handle's GPU (device=True,
        or a CUDA tensor given as ``out``), else a numpy array filled through page-locked chunks.  sync=False only
        enqueues on the handle's stream (device output)."""
        n, start = int(n), int(start)
        if (device and out is None) or (is_torch(out) and out.is_cuda):
            import torch
            dt = {L.PFB_FMT_INT8_IQ: torch.int8, L.PFB_FMT_INT16_IQ: torch.int16, L.PFB_FMT_CF32: torch.float32}[self.fmt]
            if out is None:
                out = torch.empty((n, 2), dtype=dt, device=torch.device("cuda", self.device_index))
            elif self._device_samples(out) != n:
                raise ValueError(f"out holds {self._device_samples(out)} samples, {n} asked for")
            if sync:
                L.check(self._lib.pfb_synth_generate(self._h, start, n, C.c_void_p(out.data_ptr()), L.PFB_MEM_DEVICE),
                        "pfb_synth_generate")
            else:
                L.check(self._lib.pfb_synth_generate_async(self._h, start, n, C.c_void_p(out.data_ptr())),
                        "pfb_synth_generate_async")
            return out
        dt = np.dtype(_NP_DTYPE[self.fmt])
        if out is None:
            out = np.empty((n, 2), dtype=dt)
        elif not isinstance(out, np.ndarray) or out.dtype != dt or out.size != 2 * n or not out.flags.c_contiguous:
            raise ValueError(f"out must be a C-contiguous {dt} numpy array of {n} I,Q pairs")
        L.check(self._lib.pfb_synth_generate(self._h, start, n, C.c_void_p(out.ctypes.data), L.PFB_MEM_HOST),
                "pfb_synth_generate")
        return out

    def write_iq(self, path: str, n: int, start: int = 0, file_format: int = 1, header: L.PfbIqPacket | None = None) -> None:
        """One .iq record of samples start .. start + n - 1: format 1 (generate_training_iq.m:107-127) or 3 (the
        recorders').  header=None gives the script's "simulated" fields; a PfbIqPacket supplies the others (the
        library sets the marker, numSamples and bitWidth)."""
        L.check(self._lib.pfb_synth_write_iq_file(self._h, str(path).encode(), int(file_format), int(start), int(n),
                                                  C.byref(header) if header is not None else None),
                "pfb_synth_write_iq_file")


def pulse_train(n: int, start: int = 0, device: bool = True, **kw):
    """``PulseTrain(**kw).generate(n, start)`` in one call."""
    with PulseTrain(**kw) as pt:
        return pt.generate(n, start, device=device)
