"""PRI search by epoch folding over the C ABI (pfb_fold_* in include/pfb_channelizer.h, where the arithmetic is
defined): where ``detect_pulse_train(pri=...)`` gets its number from.

``PriFold`` adds a float32 power stream -- what ``MatchedFilter(output="power")`` returns, or any float32 stream -- into
one profile of ``period // bin_cells`` phase bins per candidate period.  At the true period every pulse of a train lands
in the same bin and the bin stands out; one sample off, the train walks through the bins and averages away.  ``scores``
returns one record per candidate, ``fold_z`` turns records into a z-score, ``find_pri`` runs matched filter and folding
chunk by chunk on the device.  Only ``fold_z`` and the sort of ``find_pri`` compute on the CPU, on one record per
candidate.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib as L
from ._handle import Handle, is_torch

SCORE_DTYPE = np.dtype([("period", "u4"), ("num_bins", "u4"), ("bins_used", "u4"), ("peak_bin", "u4"),
                        ("peak_cells", "u4"), ("reserved", "u4"), ("peak_sum", "f4"), ("peak_mean", "f4"),
                        ("sum_means", "f8"), ("sum_sq_means", "f8"), ("cells", "u8")])
FOUND_DTYPE = np.dtype(SCORE_DTYPE.descr + [("z", "f8"), ("origin", "u4")])


def _config(periods, bin_cells, device):
    """(the config, the period array it points to: keep it alive as long as the config is used)"""
    p = np.asarray(periods)
    if p.size and (p.min() < 0 or p.max() > 0xffffffff):
        raise ValueError("periods are unsigned 32-bit sample counts")
    p = np.ascontiguousarray(p, dtype=np.uint32).reshape(-1)
    cfg = L.PfbFoldConfig(C.sizeof(L.PfbFoldConfig), int(bin_cells), p.size, p.ctypes.data_as(C.POINTER(C.c_uint32)), 0,
                          int(device))
    return cfg, p


def describe_fold(periods, bin_cells: int = 4) -> L.PfbFoldPlan:
    """The plan the library makes for these settings (pfb_fold_describe; host only, needs no device)."""
    cfg, _p = _config(periods, bin_cells, -1)
    plan = L.PfbFoldPlan()
    L.check(L.load().pfb_fold_describe(C.byref(cfg), C.byref(plan)), "pfb_fold_describe")
    return plan


def fold_counts(periods, bin_cells: int, candidate: int, num_cells: int) -> np.ndarray:
    """Cells per bin of one candidate after num_cells cells (pfb_fold_counts; host only): uint64, one per bin."""
    cfg, p = _config(periods, bin_cells, -1)
    if not 0 <= int(candidate) < p.size:
        raise IndexError(f"candidate {candidate} of {p.size}")
    out = np.zeros(max(int(p[int(candidate)]) // max(int(bin_cells), 1), 1), np.uint64)
    L.check(L.load().pfb_fold_counts(C.byref(cfg), int(candidate), int(num_cells),
                                     out.ctypes.data_as(C.POINTER(C.c_uint64))), "pfb_fold_counts")
    return out


def fold_z(scores) -> np.ndarray:
    """(peak_mean - mu) / sigma per record, mu and sigma the mean and deviation of the candidate's bin means:
    mu = sum_means / bins_used, sigma^2 = sum_sq_means / bins_used - mu^2.  0 where bins_used < 8 or the variance is
    not positive."""
    s = np.asarray(scores)
    used = s["bins_used"].astype(np.float64)
    z = np.zeros(s.shape, np.float64)
    with np.errstate(all="ignore"):
        mu = s["sum_means"] / used
        var = s["sum_sq_means"] / used - mu * mu
        ok = (s["bins_used"] >= 8) & (var > 0)
        z[ok] = (s["peak_mean"][ok].astype(np.float64) - mu[ok]) / np.sqrt(var[ok])
    return z


class PriFold(Handle):
    """Stateful epoch folder of a float32 stream over the candidate ``periods`` (samples; duplicates are separate
    candidates), ``bin_cells`` cells to a phase bin.  A stream may be cut into calls of any length and gives the same
    bits.  ``process`` takes numpy or a CUDA tensor; ``scores`` and ``profile`` may be read at any point mid-stream."""

    _kind, _destroy, _get_device = "PRI folder", "pfb_fold_destroy", "pfb_fold_get_device"

    def __init__(self, periods, bin_cells: int = 4, device: int = -1):
        self._h = C.c_void_p()
        lib = L.load()
        cfg, p = _config(periods, bin_cells, device)
        L.check(lib.pfb_fold_create(C.byref(cfg), C.byref(self._h)), "pfb_fold_create")
        self._created(lib)
        self.periods = p.copy()
        self.bin_cells = int(bin_cells)
        self.plan = L.PfbFoldPlan()
        L.check(lib.pfb_fold_describe(C.byref(cfg), C.byref(self.plan)), "pfb_fold_describe")

    def reset(self) -> None:
        L.check(self._lib.pfb_fold_reset(self._h), "pfb_fold_reset")

    def set_stream(self, hip_stream: int) -> None:
        L.check(self._lib.pfb_fold_set_stream(self._h, C.c_void_p(hip_stream)), "pfb_fold_set_stream")

    def sync(self) -> None:
        L.check(self._lib.pfb_fold_sync(self._h), "pfb_fold_sync")

    @property
    def last_kernel(self) -> str:
        return self._lib.pfb_fold_last_kernel(self._h).decode()

    @property
    def next_index(self) -> int:
        """Global index of the next cell to be taken: the number of cells folded so far."""
        m = C.c_uint64()
        L.check(self._lib.pfb_fold_next_index(self._h, C.byref(m)), "pfb_fold_next_index")
        return int(m.value)

    def _device_cells(self, x) -> int:
        import torch
        if not (is_torch(x) and x.is_cuda):
            raise TypeError(f"expected a CUDA tensor of cells for this {self._kind}")
        if x.dtype != torch.float32:
            raise TypeError(f"expected torch.float32 cells for this {self._kind}, got {x.dtype}")
        if x.device.index != self.device_index:
            raise ValueError(f"cells are on cuda:{x.device.index}, the {self._kind} on cuda:{self.device_index}")
        if not x.is_contiguous():
            raise ValueError("device cells must be contiguous")
        return x.numel()

    def process(self, x) -> None:
        """Fold one buffer of cells into every profile."""
        if is_torch(x) and x.is_cuda:
            n = self._device_cells(x)
            rc = self._lib.pfb_fold_process(self._h, C.c_void_p(x.data_ptr()), n, L.PFB_MEM_DEVICE)
        else:
            a = np.asarray(x.numpy() if is_torch(x) else x)
            if a.dtype != np.float32:
                raise TypeError(f"expected float32 cells for this {self._kind}, got {a.dtype}")
            a = np.ascontiguousarray(a).reshape(-1)
            rc = self._lib.pfb_fold_process(self._h, C.c_void_p(a.ctypes.data), a.size, L.PFB_MEM_HOST)
        L.check(rc, "pfb_fold_process")

    __call__ = process

    def process_async(self, x) -> None:
        """Queue one buffer of device cells on the handle's stream without a host sync (pfb_fold_process_async)."""
        n = self._device_cells(x)
        L.check(self._lib.pfb_fold_process_async(self._h, C.c_void_p(x.data_ptr()), n), "pfb_fold_process_async")

    def scores(self) -> np.ndarray:
        """One SCORE_DTYPE record per candidate, in list order, of the cells taken so far.  Changes no state."""
        out = np.zeros(self.periods.size, SCORE_DTYPE)
        L.check(self._lib.pfb_fold_scores(self._h, C.c_void_p(out.ctypes.data), out.size, L.PFB_MEM_HOST),
                "pfb_fold_scores")
        return out

    def profile(self, k: int) -> np.ndarray:
        """The float32 profile of candidate k: period // bin_cells sums."""
        if not 0 <= int(k) < self.periods.size:
            raise IndexError(f"candidate {k} of {self.periods.size}")
        out = np.zeros(int(self.periods[int(k)]) // self.bin_cells, np.float32)
        L.check(self._lib.pfb_fold_profile(self._h, int(k), C.c_void_p(out.ctypes.data), out.size, L.PFB_MEM_HOST),
                "pfb_fold_profile")
        return out

    def counts(self, k: int) -> np.ndarray:
        """Cells behind each bin of candidate k so far (uint64): profile(k) / counts(k) are the bin means."""
        return fold_counts(self.periods, self.bin_cells, k, self.next_index)


def find_pri(iq, replica, pri_min: int, pri_max: int, *, bin_cells: int = 4, extra_periods=(),
             sample_format: str | None = None, bit_width: int = 12, normalize: bool = False,
             chunk_samples: int = 1 << 22, device: int = -1) -> np.ndarray:
    """The repetition interval of the pulse train in an I/Q stream that matches ``replica``: a ``MatchedFilter`` (power
    output) feeds a ``PriFold`` chunk by chunk on the device; the compressed stream never leaves the GPU.  The
    candidates are every integer in [pri_min, pri_max] and then ``extra_periods``.

    Returns the score records sorted by z (``fold_z``) descending, ties to the smaller period, with the added fields
    ``z`` and ``origin`` = peak_bin * bin_cells: the train's compressed peak lies at origin .. origin + width - 1 modulo
    the period, width the peak bin's (bin_cells, more for the last bin).  ``found[0]["period"]`` is what goes into
    ``detect_pulse_train(pri=...)``.  Multiples of the true period score high too: list them only to rule them out."""
    import torch

    from .matched_filter import MatchedFilter, _format_of, _replica
    if int(pri_min) > int(pri_max):
        raise ValueError(f"pri_min = {pri_min} is above pri_max = {pri_max}")
    periods = np.concatenate([np.arange(int(pri_min), int(pri_max) + 1, dtype=np.int64),
                              np.asarray(list(extra_periods), dtype=np.int64)])
    r = _replica(replica)
    fmt = sample_format or _format_of(iq)
    with MatchedFilter(r, fmt, bit_width, "power", normalize, device=device) as mf, \
            PriFold(periods, bin_cells, device=mf.device_index) as fold:
        dev = torch.device("cuda", mf.device_index)
        on_device = is_torch(iq) and iq.is_cuda
        x = iq if on_device else np.asarray(iq)
        if not on_device and np.iscomplexobj(x):
            x = np.ascontiguousarray(x, np.complex64).view(np.float32).reshape(-1, 2)
        x = x.reshape(-1, 2) if not (on_device and x.is_complex()) else x
        for s in range(0, x.shape[0], chunk_samples):
            part = x[s:s + chunk_samples]
            d = part if on_device else torch.from_numpy(np.array(part)).to(dev)
            fold.process(mf.process(d))
        rec = fold.scores()
    return rank(rec, bin_cells)


def rank(scores, bin_cells: int) -> np.ndarray:
    """Score records as ``find_pri`` returns them: z and origin added, sorted by z descending, ties to the smaller
    period (and then to list order)."""
    rec = np.asarray(scores)
    found = np.zeros(rec.size, FOUND_DTYPE)
    for name in SCORE_DTYPE.names:
        found[name] = rec[name]
    found["z"] = fold_z(rec)
    found["origin"] = rec["peak_bin"] * np.uint32(bin_cells)
    order = np.lexsort((np.arange(rec.size), found["period"], -found["z"]))
    return found[order]
