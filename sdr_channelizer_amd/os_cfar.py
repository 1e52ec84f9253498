"""An ordered-statistic CFAR detector over range-Doppler maps, over the C ABI (pfb_oscfar_* in
include/pfb_channelizer.h, where the arithmetic is defined): the noise of a cell is the k-th smallest of its training
cells, not their mean, so a second target in the training window does not hide the weaker one.

``OsCfar`` is ``RangeDopplerCfar`` with a ``rank`` in place of a ``method``: the same maps in, the same records out
(``rd_cfar.DET_DTYPE``; ``targets_to_pdws`` takes them), the same calls.  ``detect_maps_os`` is the one-shot form,
``os_cfar_alpha`` the factor for a false-alarm rate, ``detect_targets(..., rank=k)`` the chain from I/Q.  Nothing here
computes on the CPU.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib as L
from .rd_cfar import RangeDopplerCfar, records


def os_cfar_alpha(pfa: float, training_cells: int, rank: int) -> float:
    """The factor that gives the false-alarm rate ``pfa`` on exponentially distributed cells when the noise is the
    ``rank``-th smallest of ``training_cells`` (pfb_oscfar_alpha; host only)."""
    a = C.c_double()
    L.check(L.load().pfb_oscfar_alpha(float(pfa), int(training_cells), int(rank), C.byref(a)), "pfb_oscfar_alpha")
    return float(a.value)


def _config(rows, gates, doppler_half_width, guard_gates, train_gates, peak_half_width, alpha, rank, min_power, pitch,
            device) -> L.PfbOscfarConfig:
    return L.PfbOscfarConfig(C.sizeof(L.PfbOscfarConfig), int(rows), int(gates), int(pitch), int(doppler_half_width),
                             int(guard_gates), int(train_gates), int(peak_half_width), int(rank), float(alpha),
                             float(min_power), 0, int(device))


def describe_oscfar(rows: int, gates: int, doppler_half_width: int, guard_gates: int, train_gates: int, rank: int,
                    peak_half_width: int = 0, alpha: float = 1.0, min_power: float = 0.0,
                    pitch: int = 0) -> L.PfbOscfarPlan:
    """The plan the library makes for these settings (pfb_oscfar_describe; host only, needs no device)."""
    cfg = _config(rows, gates, doppler_half_width, guard_gates, train_gates, peak_half_width, alpha, rank, min_power,
                  pitch, -1)
    plan = L.PfbOscfarPlan()
    L.check(L.load().pfb_oscfar_describe(C.byref(cfg), C.byref(plan)), "pfb_oscfar_describe")
    return plan


class OsCfar(RangeDopplerCfar):
    """Ordered-statistic CFAR detector of maps of ``rows`` Doppler rows by ``gates`` range gates: the geometry of
    ``RangeDopplerCfar`` (``train_gates`` per side beyond ``guard_gates``, over 2 * ``doppler_half_width`` + 1 rows), the
    noise of a cell the ``rank``-th smallest of its 2 * train_gates * (2 * doppler_half_width + 1) training cells
    (scaled to the cells there are at the gate edges).  The factor is given as ``alpha`` or derived from ``pfa``
    (os_cfar_alpha).  ``process``, ``process_async``, ``stats``, ``reset``, ``set_stream``, ``sync``, ``last_kernel`` and
    ``next_map`` are RangeDopplerCfar's, and so are the records."""

    _kind, _destroy, _get_device = "ordered-statistic CFAR detector", "pfb_oscfar_destroy", "pfb_oscfar_get_device"
    _abi = "pfb_oscfar_"

    def __init__(self, rows: int, gates: int, doppler_half_width: int, guard_gates: int, train_gates: int, rank: int,
                 alpha: float | None = None, *, pfa: float | None = None, peak_half_width: int = 0,
                 min_power: float = 0.0, pitch: int = 0, device: int = -1):
        if (alpha is None) == (pfa is None):
            raise ValueError("give one of alpha and pfa")
        if alpha is None:
            alpha = os_cfar_alpha(pfa, 2 * int(train_gates) * (2 * int(doppler_half_width) + 1), rank)
        self._h = C.c_void_p()
        lib = L.load()
        self.rows, self.gates, self.pitch = int(rows), int(gates), int(pitch) or int(gates)
        self.alpha, self.rank = float(np.float32(alpha)), int(rank)
        self._cfg = _config(rows, gates, doppler_half_width, guard_gates, train_gates, peak_half_width, alpha, rank,
                            min_power, pitch, device)
        L.check(lib.pfb_oscfar_create(C.byref(self._cfg), C.byref(self._h)), "pfb_oscfar_create")
        self._created(lib)
        self.plan = L.PfbOscfarPlan()
        L.check(lib.pfb_oscfar_describe(C.byref(self._cfg), C.byref(self.plan)), "pfb_oscfar_describe")
        self._capacity = 1024


def detect_maps_os(maps, doppler_half_width: int, guard_gates: int, train_gates: int, rank: int,
                   alpha: float | None = None, *, pfa: float | None = None, peak_half_width: int = 0,
                   min_power: float = 0.0, device: int = -1) -> np.ndarray:
    """``OsCfar(...).process(maps)`` in one call: every detection of contiguous maps of shape (maps, rows, gates), or of
    one (rows, gates) map, as a structured array."""
    shape = tuple(maps.shape)
    if len(shape) not in (2, 3):
        raise ValueError(f"expected maps of shape (maps, rows, gates) or (rows, gates), got {shape}")
    with OsCfar(shape[-2], shape[-1], doppler_half_width, guard_gates, train_gates, rank, alpha, pfa=pfa,
                peak_half_width=peak_half_width, min_power=min_power, device=device) as det:
        return records(det.process(maps))
