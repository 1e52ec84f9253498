"""Pulse-Doppler integration over the C ABI (pfb_pd_* in include/pfb_channelizer.h, where the arithmetic is defined):
range-Doppler maps of a pulse train.

``PulseDoppler`` folds a complex stream -- the matched filter's complex output, or any cf32 stream -- at the pulse
repetition interval ``pri`` and transforms each coherent interval of ``num_pulses`` pulses down its columns: K pulses
add to 10 log10 K dB over one, and a phase step from pulse to pulse shows as a Doppler bin.  ``range_doppler`` is the
one-shot form, ``doppler_frequencies`` names the rows, ``detect_pulse_train`` runs matched filter, integration and CFAR
chunk by chunk on the device.  Nothing here computes on the CPU.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib as L
from ._handle import Handle, is_torch

_OUTPUT = {"complex": L.PFB_PD_COMPLEX, "power": L.PFB_PD_POWER, "best": L.PFB_PD_BEST,
           "noncoherent": L.PFB_PD_NONCOHERENT}
CELL_DTYPE = np.dtype([("power", "f4"), ("hypothesis", "i4")])
TRAIN_DET_DTYPE = np.dtype([("cpi", "u8"), ("gate", "u4"), ("first_gate", "u4"), ("last_gate", "u4"), ("doppler_bin", "i4"),
                            ("frequency", "f8"), ("peak_power", "f4"), ("noise", "f4")])


def _config(pri, num_pulses, num_gates, origin, window, doppler_length, output, centered, device):
    """(the config, the window array it points to: keep it alive as long as the config is used)"""
    w = None if window is None else np.ascontiguousarray(window, dtype=np.float32).reshape(-1)
    if w is not None and w.size != int(num_pulses):
        raise ValueError(f"the window has {w.size} values, num_pulses is {num_pulses}")
    ptr = None if w is None else w.ctypes.data_as(C.POINTER(C.c_float))
    cfg = L.PfbPdConfig(C.sizeof(L.PfbPdConfig), int(pri), int(origin), int(num_gates), int(num_pulses),
                        int(doppler_length), _OUTPUT[output], ptr, L.PFB_PD_CENTERED if centered else 0, int(device))
    return cfg, w


def describe_pulse_doppler(pri: int, num_pulses: int, num_gates: int, origin: int = 0, window=None,
                           doppler_length: int = 0, output: str = "power", centered: bool = False) -> L.PfbPdPlan:
    """The plan the library makes for these settings (pfb_pd_describe; host only, needs no device)."""
    cfg, _w = _config(pri, num_pulses, num_gates, origin, window, doppler_length, output, centered, -1)
    plan = L.PfbPdPlan()
    L.check(L.load().pfb_pd_describe(C.byref(cfg), C.byref(plan)), "pfb_pd_describe")
    return plan


def doppler_frequencies(pri: int, doppler_length: int, fs: float, centered: bool = False) -> np.ndarray:
    """d fs / (doppler_length pri) for the rows in the order they are written (pfb_pd_doppler_frequencies; host only).
    doppler_length = 0, "the smallest length that holds num_pulses", names no length here: ValueError; the plan's
    ``doppler_length`` or ``PulseDoppler.frequencies`` has the resolved one.  The array is sized by the library's plan."""
    if int(doppler_length) == 0:
        raise ValueError("doppler_length 0 depends on num_pulses: pass the resolved length (the plan's doppler_length)")
    cfg, _w = _config(pri, 1, 1, 0, None, doppler_length, "power", centered, -1)
    plan = L.PfbPdPlan()
    L.check(L.load().pfb_pd_describe(C.byref(cfg), C.byref(plan)), "pfb_pd_describe")
    out = np.empty(int(plan.doppler_length), np.float64)
    L.check(L.load().pfb_pd_doppler_frequencies(C.byref(cfg), float(fs), out.ctypes.data_as(C.POINTER(C.c_double))),
            "pfb_pd_doppler_frequencies")
    return out


class PulseDoppler(Handle):
    """Stateful pulse-Doppler integrator of a complex64 stream: gate r of pulse k of interval c is the stream sample
    origin + (c num_pulses + k) pri + r.  Each call returns the intervals its samples complete, shaped
    (intervals, doppler_length, num_gates) for "complex" and "power", (intervals, num_gates) for "noncoherent" and
    (intervals, num_gates, 2) float32 (power, hypothesis bits) for "best" from a tensor -- ``cells`` views them -- or a
    CELL_DTYPE array from numpy.  A stream may be cut into calls of any length and gives the same bits.  numpy in ->
    numpy out, CUDA tensor in -> CUDA tensor out."""

    _kind, _destroy, _get_device = "pulse-Doppler integrator", "pfb_pd_destroy", "pfb_pd_get_device"

    def __init__(self, pri: int, num_pulses: int, num_gates: int, origin: int = 0, window=None, doppler_length: int = 0,
                 output: str = "power", centered: bool = False, device: int = -1):
        self._h = C.c_void_p()
        lib = L.load()
        self.fmt = L.PFB_FMT_CF32
        self.output = output
        self.centered = bool(centered)
        self.pri = int(pri)
        cfg, _w = _config(pri, num_pulses, num_gates, origin, window, doppler_length, output, centered, device)
        L.check(lib.pfb_pd_create(C.byref(cfg), C.byref(self._h)), "pfb_pd_create")
        self._created(lib)
        self.plan = L.PfbPdPlan()
        L.check(lib.pfb_pd_describe(C.byref(cfg), C.byref(self.plan)), "pfb_pd_describe")
        self.doppler_length = int(self.plan.doppler_length)
        self.num_gates = int(num_gates)
        self._capacity = 1

    def reset(self) -> None:
        L.check(self._lib.pfb_pd_reset(self._h), "pfb_pd_reset")

    def set_stream(self, hip_stream: int) -> None:
        L.check(self._lib.pfb_pd_set_stream(self._h, C.c_void_p(hip_stream)), "pfb_pd_set_stream")

    def sync(self) -> None:
        L.check(self._lib.pfb_pd_sync(self._h), "pfb_pd_sync")

    @property
    def last_kernel(self) -> str:
        return self._lib.pfb_pd_last_kernel(self._h).decode()

    @property
    def next_index(self) -> int:
        """Stream index of the next sample to be taken."""
        m = C.c_uint64()
        L.check(self._lib.pfb_pd_next_index(self._h, C.byref(m)), "pfb_pd_next_index")
        return int(m.value)

    def set_index(self, next_sample: int) -> None:
        """Drop the open interval and make ``next_sample`` the stream index of the next sample."""
        L.check(self._lib.pfb_pd_set_index(self._h, int(next_sample)), "pfb_pd_set_index")

    def cpis_for(self, num_samples: int) -> int:
        f = C.c_uint64()
        L.check(self._lib.pfb_pd_cpis_for(self._h, int(num_samples), C.byref(f)), "pfb_pd_cpis_for")
        return int(f.value)

    def frequencies(self, fs: float) -> np.ndarray:
        """The pulse-to-pulse frequency each row stands for, in the order the rows are written."""
        return doppler_frequencies(self.pri, self.doppler_length, fs, self.centered)

    # -- output buffers ------------------------------------------------------------
    def _shape(self, n: int) -> tuple:
        if self.output in ("complex", "power"):
            return (n, self.doppler_length, self.num_gates)
        return (n, self.num_gates, 2) if self.output == "best" else (n, self.num_gates)

    def _buffer(self, n: int, device):
        """(buffer for n intervals, its pointer); a "best" buffer holds (power, hypothesis) as float32 pairs"""
        shape = self._shape(n)
        if device is None:
            buf = np.zeros(shape, np.complex64 if self.output == "complex" else np.float32)
            return buf, buf.ctypes.data
        import torch
        buf = torch.zeros(shape, dtype=torch.complex64 if self.output == "complex" else torch.float32, device=device)
        return buf, buf.data_ptr()

    def _call(self, fn, device):
        """Run fn(pointer, capacity, count) with an output buffer, grown and run again on PFB_ERR_CAPACITY."""
        count = C.c_uint64()
        while True:
            cap = self._capacity
            buf, ptr = self._buffer(cap, device)
            rc = fn(C.c_void_p(ptr), cap, C.byref(count))
            if rc != L.PFB_ERR_CAPACITY:
                break
            self._capacity = max(int(count.value), 2 * cap)  # the state is as before the call
        out = buf[: int(count.value)] if rc == L.PFB_OK else buf[:0]
        if device is None and self.output == "best":
            out = np.ascontiguousarray(out).view(CELL_DTYPE).reshape(out.shape[0], self.num_gates)
        return rc, out

    def process(self, y):
        """Take one buffer of the stream; returns the intervals it completes."""
        if is_torch(y) and y.is_cuda:
            n = self._device_samples(y)
            self._capacity = max(1, self.cpis_for(n))
            rc, out = self._call(lambda p, cap, cnt: self._lib.pfb_pd_process(
                self._h, C.c_void_p(y.data_ptr()), n, p, cap, cnt, L.PFB_MEM_DEVICE), y.device)
        else:
            a, n = self._host_samples(y)
            self._capacity = max(1, self.cpis_for(n))
            rc, out = self._call(lambda p, cap, cnt: self._lib.pfb_pd_process(
                self._h, C.c_void_p(a.ctypes.data), n, p, cap, cnt, L.PFB_MEM_HOST), None)
        L.check(rc, "pfb_pd_process")
        return out

    __call__ = process

    def process_async(self, y, out, count) -> None:
        """Queue one buffer of device samples on the handle's stream without a host sync (pfb_pd_process_async): the
        intervals it completes go to ``out``, a contiguous CUDA tensor of the output's dtype with room for whole
        intervals, their number to ``count``, an int64 CUDA tensor of one element.  PFB_ERR_CAPACITY queues nothing."""
        import torch
        n = self._device_samples(y)
        want = torch.complex64 if self.output == "complex" else torch.float32
        per = int(self.plan.cpi_outputs) * (2 if self.output == "best" else 1)
        if not (is_torch(out) and out.is_cuda and out.dtype == want and out.is_contiguous()
                and out.device.index == self.device_index and out.numel() % per == 0):
            raise ValueError(f"out must be a contiguous {want} tensor on cuda:{self.device_index} of whole intervals")
        if not (is_torch(count) and count.is_cuda and count.dtype == torch.int64 and count.numel() >= 1
                and count.is_contiguous() and count.device.index == self.device_index):
            raise ValueError(f"count must be an int64 tensor on cuda:{self.device_index}")
        L.check(self._lib.pfb_pd_process_async(self._h, C.c_void_p(y.data_ptr()), n, C.c_void_p(out.data_ptr()),
                                               out.numel() // per, C.c_void_p(count.data_ptr())), "pfb_pd_process_async")

    def flush(self, device=None):
        """Transform the open interval with its missing samples as zeros: one interval, or none when none is open.
        ``device``: a torch device for a tensor result."""
        mem = L.PFB_MEM_HOST if device is None else L.PFB_MEM_DEVICE
        rc, out = self._call(lambda p, cap, cnt: self._lib.pfb_pd_flush(self._h, p, cap, cnt, mem), device)
        L.check(rc, "pfb_pd_flush")
        return out


def cells(t) -> np.ndarray:
    """The "best" output of a ``PulseDoppler`` as a CELL_DTYPE array of shape (intervals, num_gates)."""
    if is_torch(t):
        t = t.cpu().numpy()
    a = np.ascontiguousarray(t)
    return a if a.dtype == CELL_DTYPE else a.view(CELL_DTYPE).reshape(a.shape[:-1])


def range_doppler(y, pri: int, num_pulses: int, num_gates: int | None = None, origin: int = 0, window=None,
                  doppler_length: int = 0, output: str = "power", centered: bool = False, flush: bool = False,
                  device: int = -1):
    """``PulseDoppler(...).process(y)`` in one call; num_gates=None takes every sample of the interval (pri gates).
    flush=True adds the interval the stream leaves open, its missing samples as zeros."""
    with PulseDoppler(pri, num_pulses, pri if num_gates is None else num_gates, origin, window, doppler_length, output,
                      centered, device) as pd:
        out = pd.process(y)
        if not flush:
            return out
        on_device = is_torch(y) and y.is_cuda
        tail = pd.flush(y.device if on_device else None)
        if on_device:
            import torch
            return torch.cat([out, tail])
        return np.concatenate([out, tail])


def detect_pulse_train(iq, replica, pri: int, num_pulses: int, *, pfa: float | None = None, alpha: float | None = None,
                       origin: int = 0, num_gates: int | None = None, window=None, doppler_length: int = 0,
                       block_cells: int = 64, guard_blocks: int | None = None, train_blocks: int = 8,
                       merge_gap: int | None = None, fs: float = 1.0, sample_format: str | None = None,
                       bit_width: int = 12, normalize: bool = False, chunk_samples: int = 1 << 22,
                       device: int = -1) -> np.ndarray:
    """The pulse trains of an I/Q stream that match ``replica`` and repeat every ``pri`` samples: a ``MatchedFilter``
    (complex output) feeds a ``PulseDoppler`` ("best" cells, centered), whose intervals go one by one through a ``Cfar``
    over the gates (bank cells) -- chunk by chunk on the device; neither the compressed stream nor the maps leave the
    GPU.  The detector is flushed and reset after every interval, so no training block spans two of them.  The interval
    the stream leaves open is taken too, its missing samples as zeros (the matched filter alone withholds the last
    K - 1 outputs of the last interval).

    The cells are the maxima over the Doppler rows.  ``pfa`` (default 1e-6) is a design figure per gate for
    ``doppler_length`` independent noise rows (a rectangular window over num_pulses = doppler_length pulses): the CA
    factor for pfa / doppler_length over the training cells, divided by the harmonic number H(doppler_length), the mean
    of such a maximum in units of one row's noise.  Give ``alpha`` for anything else.

    Returns TRAIN_DET_DTYPE records: the interval, the gate of the peak (the train's first sample is origin + gate,
    modulo pri), the run of gates over the threshold, the signed Doppler bin and its frequency bin * fs /
    (doppler_length * pri), the peak's power and the noise there."""
    import torch

    from .cfar import Cfar, cfar_alpha, records
    from .matched_filter import MatchedFilter, _format_of, _replica
    r = _replica(replica)
    K = r.size
    R = int(pri) if num_gates is None else int(num_gates)
    plan = describe_pulse_doppler(pri, num_pulses, R, origin, window, doppler_length, "best", True)
    ND = int(plan.doppler_length)
    if alpha is None:
        harmonic = float(np.sum(1.0 / np.arange(1, ND + 1)))
        alpha = cfar_alpha((1e-6 if pfa is None else pfa) / ND, 2 * int(train_blocks) * int(block_cells)) / harmonic
    elif pfa is not None:
        raise ValueError("give one of alpha and pfa")
    G = -(-K // block_cells) if guard_blocks is None else guard_blocks
    g = K if merge_gap is None else merge_gap
    fmt = sample_format or _format_of(iq)
    found = []
    with MatchedFilter(r, fmt, bit_width, "complex", normalize, device=device) as mf, \
            PulseDoppler(pri, num_pulses, R, origin, window, ND, "best", True, device=mf.device_index) as pd, \
            Cfar(block_cells, G, train_blocks, alpha, element="cell", merge_gap=g, device=mf.device_index) as det:
        dev = torch.device("cuda", mf.device_index)
        on_device = is_torch(iq) and iq.is_cuda
        x = iq if on_device else np.asarray(iq)
        if not on_device and np.iscomplexobj(x):
            x = np.ascontiguousarray(x, np.complex64).view(np.float32).reshape(-1, 2)
        x = x.reshape(-1, 2) if not (on_device and x.is_complex()) else x
        cpi = 0

        def take(maps):
            nonlocal cpi
            for m in maps:                       # (num_gates, 2) cells of one interval, on the device
                det.reset()
                recs = np.concatenate([records(det.process(m)), records(det.flush())])
                out = np.zeros(len(recs), TRAIN_DET_DTYPE)
                out["cpi"], out["gate"] = cpi, recs["peak_index"]
                out["first_gate"], out["last_gate"] = recs["first_index"], recs["last_index"]
                out["doppler_bin"] = recs["hypothesis"]
                out["frequency"] = recs["hypothesis"] * (float(fs) / (ND * int(pri)))
                out["peak_power"], out["noise"] = recs["peak_power"], recs["noise"]
                found.append(out)
                cpi += 1

        for s in range(0, x.shape[0], chunk_samples):
            part = x[s:s + chunk_samples]
            d = part if on_device else torch.from_numpy(np.array(part)).to(dev)
            take(pd.process(mf.process(d)))
        take(pd.flush(dev))
    return np.concatenate(found) if found else np.zeros(0, TRAIN_DET_DTYPE)
