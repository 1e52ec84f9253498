"""A 2-D CFAR detector over range-Doppler maps, over the C ABI (pfb_rdcfar_* in include/pfb_channelizer.h, where the
arithmetic is defined): one record per target from the power maps ``PulseDoppler`` leaves on the device.

``RangeDopplerCfar`` takes float32 maps of shape (maps, rows, gates) -- ``PulseDoppler(output="power")``, or the one-row
maps of ``output="noncoherent"`` as (maps, 1, gates) -- cut into calls of any number of maps, and returns one record per
cell that is over ``alpha`` times the noise around it and the largest of its neighbourhood.  ``detect_maps`` is the
one-shot form, ``detect_targets`` runs matched filter, integration and detector chunk by chunk on the device,
``detections_to_pdws`` turns records into what ``fit_event`` takes (the package exports it as ``targets_to_pdws``,
next to ``cfar.detections_to_pdws``).  Nothing here computes on the CPU.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib as L
from ._handle import Handle, is_torch
from .cfar import cfar_alpha
from .pdw import PDW_DTYPE

DET_DTYPE = np.dtype([("map", "u8"), ("row", "u4"), ("gate", "u4"), ("power", "f4"), ("noise", "f4"),
                      ("training_cells", "u4"), ("flags", "u4")])
TARGET_DTYPE = np.dtype([("cpi", "u8"), ("gate", "u4"), ("row", "u4"), ("doppler_bin", "i4"), ("frequency", "f8"),
                         ("power", "f4"), ("noise", "f4")])
_METHOD = {"ca": L.PFB_CFAR_CA, "go": L.PFB_CFAR_GO, "so": L.PFB_CFAR_SO}
_WORDS = DET_DTYPE.itemsize // 8  # a record as int64 words: how a tensor holds it


def _config(rows, gates, doppler_half_width, guard_gates, train_gates, peak_half_width, alpha, method, min_power, pitch,
            device) -> L.PfbRdcfarConfig:
    return L.PfbRdcfarConfig(C.sizeof(L.PfbRdcfarConfig), int(rows), int(gates), int(pitch), int(doppler_half_width),
                             int(guard_gates), int(train_gates), int(peak_half_width), _METHOD[method], float(alpha),
                             float(min_power), 0, int(device))


def describe_rdcfar(rows: int, gates: int, doppler_half_width: int, guard_gates: int, train_gates: int,
                    peak_half_width: int = 0, alpha: float = 1.0, method: str = "ca", min_power: float = 0.0,
                    pitch: int = 0) -> L.PfbRdcfarPlan:
    """The plan the library makes for these settings (pfb_rdcfar_describe; host only, needs no device)."""
    cfg = _config(rows, gates, doppler_half_width, guard_gates, train_gates, peak_half_width, alpha, method, min_power,
                  pitch, -1)
    plan = L.PfbRdcfarPlan()
    L.check(L.load().pfb_rdcfar_describe(C.byref(cfg), C.byref(plan)), "pfb_rdcfar_describe")
    return plan


def records(t) -> np.ndarray:
    """The records a ``RangeDopplerCfar`` returned as a tensor, as a structured numpy array."""
    if is_torch(t):
        t = t.cpu().numpy()
    return np.ascontiguousarray(t).view(DET_DTYPE).reshape(-1)


class RangeDopplerCfar(Handle):
    """CFAR detector of maps of ``rows`` Doppler rows by ``gates`` range gates: per cell, ``train_gates`` training gates
    on each side beyond ``guard_gates`` guard gates, over the 2 * ``doppler_half_width`` + 1 rows around its own (rows
    wrap, gates do not); a cell over its threshold is reported when no cell within ``peak_half_width`` rows and
    ``guard_gates`` gates beats it.  The factor is given as ``alpha`` or derived from ``pfa`` (the CA factor for
    2 * train_gates * (2 * doppler_half_width + 1) training cells).  Every map is decided on its own: maps may be cut
    into calls in any way.  numpy in -> structured numpy array out (DET_DTYPE); CUDA tensor in -> an (n, 4) int64
    tensor of the same records (``records`` views it).  ``pitch``: floats from row to row of the maps handed in, when
    they are a view of wider ones."""

    _kind, _destroy, _get_device = "range-Doppler CFAR detector", "pfb_rdcfar_destroy", "pfb_rdcfar_get_device"
    _abi = "pfb_rdcfar_"   # the entry points a subclass with the same calls (OsCfar) goes through instead

    def _run(self, name: str, *args) -> int:
        """Call the handle's entry point ``name`` (without the unit's prefix) and return its status."""
        return getattr(self._lib, self._abi + name)(self._h, *args)

    def __init__(self, rows: int, gates: int, doppler_half_width: int, guard_gates: int, train_gates: int,
                 alpha: float | None = None, *, pfa: float | None = None, peak_half_width: int = 0, method: str = "ca",
                 min_power: float = 0.0, pitch: int = 0, device: int = -1):
        if (alpha is None) == (pfa is None):
            raise ValueError("give one of alpha and pfa")
        if alpha is None:
            alpha = cfar_alpha(pfa, 2 * int(train_gates) * (2 * int(doppler_half_width) + 1))
        self._h = C.c_void_p()
        lib = L.load()
        self.rows, self.gates, self.pitch = int(rows), int(gates), int(pitch) or int(gates)
        self.alpha = float(np.float32(alpha))
        self._cfg = _config(rows, gates, doppler_half_width, guard_gates, train_gates, peak_half_width, alpha, method,
                            min_power, pitch, device)
        L.check(lib.pfb_rdcfar_create(C.byref(self._cfg), C.byref(self._h)), "pfb_rdcfar_create")
        self._created(lib)
        self.plan = L.PfbRdcfarPlan()
        L.check(lib.pfb_rdcfar_describe(C.byref(self._cfg), C.byref(self.plan)), "pfb_rdcfar_describe")
        self._capacity = 1024

    def reset(self) -> None:
        L.check(self._run("reset"), self._abi + "reset")

    def set_stream(self, hip_stream: int) -> None:
        L.check(self._run("set_stream", C.c_void_p(hip_stream)), self._abi + "set_stream")

    def sync(self) -> None:
        L.check(self._run("sync"), self._abi + "sync")

    @property
    def last_kernel(self) -> str:
        return getattr(self._lib, self._abi + "last_kernel")(self._h).decode()

    @property
    def next_map(self) -> int:
        """Index of the next map to be taken, counted since construction or reset."""
        m = C.c_uint64()
        L.check(self._run("next_map", C.byref(m)), self._abi + "next_map")
        return int(m.value)

    @property
    def stats(self) -> dict:
        s = L.PfbRdcfarStats()
        L.check(self._run("get_stats", C.byref(s)), self._abi + "get_stats")
        return {name: int(getattr(s, name)) for name, _ in L.PfbRdcfarStats._fields_}

    # -- maps ----------------------------------------------------------------------
    def _maps(self, shape, strides) -> int:
        """The number of maps of a (maps, rows, gates) buffer whose strides, in floats, are the handle's."""
        if len(shape) == 2:
            shape, strides = (1,) + tuple(shape), (self.rows * self.pitch,) + tuple(strides)
        if len(shape) != 3 or tuple(shape[1:]) != (self.rows, self.gates):
            raise ValueError(f"expected maps of shape (maps, {self.rows}, {self.gates}), got {tuple(shape)}")
        n = int(shape[0])
        want = (self.rows * self.pitch, self.pitch, 1)
        for k in range(3):
            if shape[k] > 1 and strides[k] != want[k] and n > 0:
                raise ValueError(f"the maps must lie {self.pitch} floats from row to row and {want[0]} from map to map")
        return n

    def _call(self, fn, device):
        """Run fn(pointer, capacity, count) with a record buffer, grown and run again on PFB_ERR_CAPACITY."""
        count = C.c_uint64()
        while True:
            cap = self._capacity
            if device is None:
                buf = np.zeros(cap, DET_DTYPE)
                ptr = buf.ctypes.data
            else:
                import torch
                buf = torch.zeros((cap, _WORDS), dtype=torch.int64, device=device)
                ptr = buf.data_ptr()
            rc = fn(C.c_void_p(ptr), cap, C.byref(count))
            if rc != L.PFB_ERR_CAPACITY:
                break
            self._capacity = max(int(count.value), 2 * cap)  # the state is as before the call
        return rc, buf[: int(count.value)] if rc == L.PFB_OK else buf[:0]

    def _device_maps(self, x) -> int:
        import torch
        if x.dtype != torch.float32:
            raise TypeError(f"expected torch.float32 maps for this {self._kind}, got {x.dtype}")
        if x.device.index != self.device_index:
            raise ValueError(f"maps are on cuda:{x.device.index}, the {self._kind} on cuda:{self.device_index}")
        return self._maps(tuple(x.shape), tuple(x.stride()))

    def process(self, x):
        """Take maps of shape (maps, rows, gates) -- or one (rows, gates) map; returns their detections."""
        if is_torch(x) and x.is_cuda:
            n = self._device_maps(x)
            rc, out = self._call(lambda p, cap, cnt: self._run(
                "process", C.c_void_p(x.data_ptr()), n, p, cap, cnt, L.PFB_MEM_DEVICE), x.device)
        else:
            a = np.asarray(x)
            if a.dtype != np.float32:
                raise TypeError(f"expected float32 maps for this {self._kind}, got {a.dtype}")
            n = self._maps(a.shape, tuple(s // 4 for s in a.strides))
            rc, out = self._call(lambda p, cap, cnt: self._run(
                "process", C.c_void_p(a.ctypes.data), n, p, cap, cnt, L.PFB_MEM_HOST), None)
        L.check(rc, self._abi + "process")
        return out

    __call__ = process

    def process_async(self, x, out, count) -> None:
        """Queue device maps on the handle's stream without a host sync (pfb_rdcfar_process_async): the records go to
        ``out``, a (capacity, 4) int64 CUDA tensor, their number to ``count``, an int64 CUDA tensor of one element.
        What does not fit is dropped and counted in ``stats["dropped"]``."""
        import torch
        n = self._device_maps(x)
        for t, what in ((out, "out"), (count, "count")):
            if not (is_torch(t) and t.is_cuda and t.dtype == torch.int64 and t.is_contiguous()
                    and t.device.index == self.device_index):
                raise ValueError(f"{what} must be a contiguous int64 tensor on cuda:{self.device_index}")
        if out.numel() % _WORDS or count.numel() < 1:
            raise ValueError(f"out holds records of {_WORDS} int64 words, count one element")
        L.check(self._run("process_async", C.c_void_p(x.data_ptr()), n, C.c_void_p(out.data_ptr()),
                          out.numel() // _WORDS, C.c_void_p(count.data_ptr())), self._abi + "process_async")


def detect_maps(maps, doppler_half_width: int, guard_gates: int, train_gates: int, alpha: float | None = None, *,
                pfa: float | None = None, peak_half_width: int = 0, method: str = "ca", min_power: float = 0.0,
                device: int = -1) -> np.ndarray:
    """``RangeDopplerCfar(...).process(maps)`` in one call: every detection of contiguous maps of shape (maps, rows,
    gates), or of one (rows, gates) map, as a structured array."""
    shape = tuple(maps.shape)
    if len(shape) not in (2, 3):
        raise ValueError(f"expected maps of shape (maps, rows, gates) or (rows, gates), got {shape}")
    with RangeDopplerCfar(shape[-2], shape[-1], doppler_half_width, guard_gates, train_gates, alpha, pfa=pfa,
                          peak_half_width=peak_half_width, method=method, min_power=min_power, device=device) as det:
        return records(det.process(maps))


def signed_bins(rows, num_rows: int, centered: bool) -> np.ndarray:
    """The signed Doppler bin of stored rows: row - num_rows // 2 when centered, else the FFT order's."""
    r = np.asarray(rows, np.int64)
    return r - num_rows // 2 if centered else np.where(r < (num_rows + 1) // 2, r, r - num_rows)


def detect_targets(iq, replica, pri: int, num_pulses: int, *, pfa: float | None = None, alpha: float | None = None,
                   origin: int = 0, num_gates: int | None = None, window=None, doppler_length: int = 0,
                   doppler_half_width: int = 1, guard_gates: int | None = None, train_gates: int = 64,
                   peak_half_width: int = 1, method: str = "ca", min_power: float = 0.0, fs: float = 1.0,
                   sample_format: str | None = None, bit_width: int = 12, normalize: bool = False,
                   chunk_samples: int = 1 << 22, device: int = -1, rank: int | None = None) -> np.ndarray:
    """The targets of an I/Q stream that match ``replica`` and repeat every ``pri`` samples: a ``MatchedFilter``
    (complex output) feeds a ``PulseDoppler`` (power maps, centered), whose intervals go, all those of a chunk in one
    call, through a ``RangeDopplerCfar`` -- chunk by chunk on the device; neither the compressed stream nor the maps
    leave the GPU.  The interval the stream leaves open is taken too, its missing samples as zeros.

    Defaults: guard_gates = len(replica) (the replica's range sidelobes), pfa = 1e-6 with the plain CA factor
    cfar_alpha(pfa, 2 * train_gates * (2 * doppler_half_width + 1)).  A cell trains on cells of its own rows, so no
    factor for the window is needed; but the compressed noise is correlated over a chip of the replica, and a taper
    correlates adjacent rows, so the training cells count for fewer than their number and the rate lies above ``pfa``
    (the header and DESIGN.md section 22).  Two trains in one gate on different Doppler rows give two records per
    interval.

    ``rank``: with an integer k the chain's detector is an ``OsCfar`` that takes the k-th smallest of the 2 *
    train_gates * (2 * doppler_half_width + 1) training cells as the noise (``method`` is then unused, and ``pfa`` means
    the ordered-statistic factor os_cfar_alpha(pfa, cells, k)): a second train in the first one's training window no
    longer hides the weaker one.  With None nothing changes.

    Returns TARGET_DTYPE records in ascending (cpi, row, gate): the interval, the gate (the train's first sample is
    origin + gate, modulo pri), the row as stored, the signed Doppler bin and its frequency bin * fs /
    (doppler_length * pri), the cell's power and the noise there."""
    import torch

    from .matched_filter import MatchedFilter, _format_of, _replica
    from .pulse_doppler import PulseDoppler
    r = _replica(replica)
    R = int(pri) if num_gates is None else int(num_gates)
    if alpha is None and pfa is None:
        pfa = 1e-6
    Gr = r.size if guard_gates is None else int(guard_gates)
    fmt = sample_format or _format_of(iq)
    found = []

    def detector(rows, dev_index):
        if rank is None:
            return RangeDopplerCfar(rows, R, doppler_half_width, Gr, train_gates, alpha, pfa=pfa,
                                    peak_half_width=peak_half_width, method=method, min_power=min_power, device=dev_index)
        from .os_cfar import OsCfar
        return OsCfar(rows, R, doppler_half_width, Gr, train_gates, int(rank), alpha, pfa=pfa,
                      peak_half_width=peak_half_width, min_power=min_power, device=dev_index)

    with MatchedFilter(r, fmt, bit_width, "complex", normalize, device=device) as mf, \
            PulseDoppler(pri, num_pulses, R, origin, window, doppler_length, "power", True, device=mf.device_index) as pd, \
            detector(pd.doppler_length, mf.device_index) as det:
        ND = pd.doppler_length
        dev = torch.device("cuda", mf.device_index)
        on_device = is_torch(iq) and iq.is_cuda
        x = iq if on_device else np.asarray(iq)
        if not on_device and np.iscomplexobj(x):
            x = np.ascontiguousarray(x, np.complex64).view(np.float32).reshape(-1, 2)
        x = x.reshape(-1, 2) if not (on_device and x.is_complex()) else x
        for s in range(0, x.shape[0], chunk_samples):
            part = x[s:s + chunk_samples]
            d = part if on_device else torch.from_numpy(np.array(part)).to(dev)
            found.append(records(det.process(pd.process(mf.process(d)))))
        found.append(records(det.process(pd.flush(dev))))
    recs = np.concatenate(found) if found else np.zeros(0, DET_DTYPE)
    out = np.zeros(len(recs), TARGET_DTYPE)
    out["cpi"], out["gate"], out["row"] = recs["map"], recs["gate"], recs["row"]
    out["doppler_bin"] = signed_bins(recs["row"], ND, True)
    out["frequency"] = out["doppler_bin"] * (float(fs) / (ND * int(pri)))
    out["power"], out["noise"] = recs["power"], recs["noise"]
    return out


def detections_to_pdws(dets, fs: float, fc: float, start: float, pri: int, num_pulses: int, rows: int, *,
                       origin: int = 0, centered: bool = True) -> np.ndarray:
    """Detections as pulse descriptor words (pfb_rdcfar_to_pdw; host only), what ``fit_event`` accepts: ``dets`` are
    DET_DTYPE records, or the TARGET_DTYPE records of ``detect_targets`` (centered rows).  toa of the interval's first
    pulse at that gate (1-based, as the extractors), freq = fc + signed bin * fs / (rows * pri), bin the signed bin,
    snr = 10 log10(power / noise), pw one sample."""
    a = np.asarray(dets)
    if a.dtype == TARGET_DTYPE:
        d = np.zeros(a.size, DET_DTYPE)
        d["map"], d["row"], d["gate"] = a["cpi"].reshape(-1), a["row"].reshape(-1), a["gate"].reshape(-1)
        d["power"], d["noise"] = a["power"].reshape(-1), a["noise"].reshape(-1)
    else:
        d = np.ascontiguousarray(a, dtype=DET_DTYPE).reshape(-1)
    out = np.zeros(d.size, PDW_DTYPE)
    L.check(L.load().pfb_rdcfar_to_pdw(C.c_void_p(d.ctypes.data), d.size, float(fs), float(fc), float(start), int(pri),
                                       int(num_pulses), int(origin), int(rows), int(bool(centered)),
                                       out.ctypes.data_as(C.POINTER(L.PfbPdw))), "pfb_rdcfar_to_pdw")
    return out
