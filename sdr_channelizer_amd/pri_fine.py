"""Fractional-PRI search and regridder over the C ABI (pfb_qfold_* and pfb_regrid_* in include/pfb_channelizer.h, where
the arithmetic is defined): from "PRI unknown and not a whole number of samples" to gate and Doppler bin.

A period is a uint64 holding samples times 2^32 (``period_q32`` / ``period_samples``).  ``FinePriFold`` is ``PriFold`` at
such periods, ``refine_pri`` and ``find_pri_fine`` search a grid of them, ``Regrid`` lays the windows of a train at such
a period onto an integer grid of ``row_samples`` a row, which ``PulseDoppler(pri=row_samples)`` and the detectors behind
it take as they are; ``detect_pulse_train_fine`` is that chain.  Only ``fold_z`` and the sort compute on the CPU, on one
record per candidate.
"""
from __future__ import annotations

import ctypes as C
from fractions import Fraction

import numpy as np

from . import _lib as L
from ._handle import Handle, is_torch
from .pri_search import PriFold, fold_z

QSCORE_DTYPE = np.dtype([("period_q32", "u8"), ("num_bins", "u4"), ("bins_used", "u4"), ("peak_bin", "u4"),
                         ("reserved", "u4"), ("peak_cells", "u8"), ("peak_sum", "f4"), ("peak_mean", "f4"),
                         ("sum_means", "f8"), ("sum_sq_means", "f8"), ("cells", "u8")])
QFOUND_DTYPE = np.dtype(QSCORE_DTYPE.descr + [("z", "f8"), ("origin", "u4"), ("period", "f8")])
MAX_CANDIDATES, MAX_PROFILE_BYTES = 4096, 64 << 20      # of one handle
MAX_SEARCH_SAMPLES = 1 << 27                            # find_pri_fine keeps 4 bytes a sample on the device


def period_q32(x) -> int:
    """A period in samples (float, Fraction or int) as the Q32 integer the library takes: exact for Fractions and ints
    whose value has 32 fractional bits or fewer, else rounded to nearest (ties to even) from the exact value given."""
    if isinstance(x, (bool, np.bool_)):
        raise TypeError("a period is a number of samples")
    f = Fraction(int(x)) if isinstance(x, (int, np.integer)) else Fraction(x)
    if f < 0:
        raise ValueError("periods are not negative")
    return int(round(f * (1 << 32)))


def period_samples(q) -> float:
    """The Q32 period q in samples, rounded to float64 once."""
    return float(Fraction(int(q), 1 << 32))


def _q32_list(periods) -> np.ndarray:
    """floats and Fractions are samples; Python and numpy ints are samples too; a uint64 array is Q32 already"""
    if isinstance(periods, np.ndarray) and periods.dtype == np.uint64:
        return np.ascontiguousarray(periods).reshape(-1)
    qs = [period_q32(p) for p in (periods.tolist() if isinstance(periods, np.ndarray) else list(periods))]
    if qs and max(qs) >= 1 << 64:
        raise ValueError("periods are below 2^32 samples")
    return np.array(qs, np.uint64).reshape(-1)


def _config(periods, bin_cells, device):
    """(the config, the Q32 array it points to: keep it alive as long as the config is used)"""
    q = _q32_list(periods)
    cfg = L.PfbQfoldConfig(C.sizeof(L.PfbQfoldConfig), int(bin_cells), q.size, 0,
                           q.ctypes.data_as(C.POINTER(C.c_uint64)), int(device), 0)
    return cfg, q


def describe_fine_fold(periods, bin_cells: int = 4) -> L.PfbQfoldPlan:
    """The plan the library makes for these settings (pfb_qfold_describe; host only, needs no device).  ``periods``:
    samples as floats, Fractions or ints, or a uint64 array of Q32 values."""
    cfg, _q = _config(periods, bin_cells, -1)
    plan = L.PfbQfoldPlan()
    L.check(L.load().pfb_qfold_describe(C.byref(cfg), C.byref(plan)), "pfb_qfold_describe")
    return plan


def fine_fold_counts(periods, bin_cells: int, candidate: int, num_cells: int, first_cell: int = 0) -> np.ndarray:
    """Cells first_cell <= i < num_cells per bin of one candidate (pfb_qfold_counts; host only): uint64, one per bin."""
    cfg, q = _config(periods, bin_cells, -1)
    if not 0 <= int(candidate) < q.size:
        raise IndexError(f"candidate {candidate} of {q.size}")
    out = np.zeros(max((int(q[int(candidate)]) >> 32) // max(int(bin_cells), 1), 1), np.uint64)
    L.check(L.load().pfb_qfold_counts(C.byref(cfg), int(candidate), int(first_cell), int(num_cells),
                                      out.ctypes.data_as(C.POINTER(C.c_uint64))), "pfb_qfold_counts")
    return out


class FinePriFold(PriFold):
    """``PriFold`` at periods given to 2^-32 of a sample: floats, Fractions or ints in samples, or a uint64 array of Q32
    values.  ``set_index`` clears the profiles and makes a cell index the next one, so that the head of a record can be
    skipped; ``scores`` returns QSCORE_DTYPE records, which ``fold_z`` takes as they are."""

    _kind, _destroy, _get_device = "fine PRI folder", "pfb_qfold_destroy", "pfb_qfold_get_device"

    def __init__(self, periods, bin_cells: int = 4, device: int = -1):
        self._h = C.c_void_p()
        lib = L.load()
        cfg, q = _config(periods, bin_cells, device)
        L.check(lib.pfb_qfold_create(C.byref(cfg), C.byref(self._h)), "pfb_qfold_create")
        self._created(lib)
        self.periods_q32 = q.copy()
        self.periods = np.array([period_samples(v) for v in q], np.float64)
        self.bin_cells = int(bin_cells)
        self.plan = L.PfbQfoldPlan()
        L.check(lib.pfb_qfold_describe(C.byref(cfg), C.byref(self.plan)), "pfb_qfold_describe")
        self._first = 0

    def reset(self) -> None:
        L.check(self._lib.pfb_qfold_reset(self._h), "pfb_qfold_reset")
        self._first = 0

    def set_index(self, next_cell: int) -> None:
        """Clear the profiles and make ``next_cell`` (<= 2^62) the index of the next cell taken."""
        L.check(self._lib.pfb_qfold_set_index(self._h, int(next_cell)), "pfb_qfold_set_index")
        self._first = int(next_cell)

    def set_stream(self, hip_stream: int) -> None:
        L.check(self._lib.pfb_qfold_set_stream(self._h, C.c_void_p(hip_stream)), "pfb_qfold_set_stream")

    def sync(self) -> None:
        L.check(self._lib.pfb_qfold_sync(self._h), "pfb_qfold_sync")

    @property
    def last_kernel(self) -> str:
        return self._lib.pfb_qfold_last_kernel(self._h).decode()

    @property
    def next_index(self) -> int:
        """Global index of the next cell to be taken."""
        m = C.c_uint64()
        L.check(self._lib.pfb_qfold_next_index(self._h, C.byref(m)), "pfb_qfold_next_index")
        return int(m.value)

    def process(self, x) -> None:
        """Fold one buffer of cells into every profile."""
        if is_torch(x) and x.is_cuda:
            n = self._device_cells(x)
            rc = self._lib.pfb_qfold_process(self._h, C.c_void_p(x.data_ptr()), n, L.PFB_MEM_DEVICE)
        else:
            a = np.asarray(x.numpy() if is_torch(x) else x)
            if a.dtype != np.float32:
                raise TypeError(f"expected float32 cells for this {self._kind}, got {a.dtype}")
            a = np.ascontiguousarray(a).reshape(-1)
            rc = self._lib.pfb_qfold_process(self._h, C.c_void_p(a.ctypes.data), a.size, L.PFB_MEM_HOST)
        L.check(rc, "pfb_qfold_process")

    __call__ = process

    def process_async(self, x) -> None:
        """Queue one buffer of device cells on the handle's stream without a host sync (pfb_qfold_process_async)."""
        n = self._device_cells(x)
        L.check(self._lib.pfb_qfold_process_async(self._h, C.c_void_p(x.data_ptr()), n), "pfb_qfold_process_async")

    def scores(self) -> np.ndarray:
        """One QSCORE_DTYPE record per candidate, in list order, of the cells taken so far.  Changes no state."""
        out = np.zeros(self.periods_q32.size, QSCORE_DTYPE)
        L.check(self._lib.pfb_qfold_scores(self._h, C.c_void_p(out.ctypes.data), out.size, L.PFB_MEM_HOST),
                "pfb_qfold_scores")
        return out

    def profile(self, k: int) -> np.ndarray:
        """The float32 profile of candidate k: floor(period) // bin_cells sums."""
        if not 0 <= int(k) < self.periods_q32.size:
            raise IndexError(f"candidate {k} of {self.periods_q32.size}")
        out = np.zeros((int(self.periods_q32[int(k)]) >> 32) // self.bin_cells, np.float32)
        L.check(self._lib.pfb_qfold_profile(self._h, int(k), C.c_void_p(out.ctypes.data), out.size, L.PFB_MEM_HOST),
                "pfb_qfold_profile")
        return out

    def counts(self, k: int) -> np.ndarray:
        """Cells behind each bin of candidate k since the start index (uint64)."""
        return fine_fold_counts(self.periods_q32, self.bin_cells, k, self.next_index, self._first)


def rank_fine(scores, bin_cells: int) -> np.ndarray:
    """Score records as ``refine_pri`` returns them: z, origin = peak_bin * bin_cells and period (samples) added, sorted
    by z descending, ties to the smaller period (and then to list order)."""
    rec = np.asarray(scores)
    found = np.zeros(rec.size, QFOUND_DTYPE)
    for name in QSCORE_DTYPE.names:
        found[name] = rec[name]
    found["z"] = fold_z(rec)
    found["origin"] = rec["peak_bin"] * np.uint32(bin_cells)
    found["period"] = [period_samples(q) for q in rec["period_q32"]]
    order = np.lexsort((np.arange(rec.size), found["period_q32"], -found["z"]))
    return found[order]


def grid_q32(lo, hi, step) -> np.ndarray:
    """The Q32 periods lo, lo + step, ... up to hi (samples; each rounded from its exact value), uint64."""
    lo, hi, step = Fraction(lo), Fraction(hi), Fraction(step)
    if step <= 0 or period_q32(step) == 0:
        raise ValueError("step must be at least 2^-33 of a sample")
    if lo > hi:
        raise ValueError(f"the grid's first period {float(lo)} is above its last {float(hi)}")
    n = int((hi - lo) / step + Fraction(1, 1 << 20))    # a last point that misses hi by rounding of the floats counts
    return np.array([period_q32(lo + k * step) for k in range(n + 1)], np.uint64)


def _loads(q, bin_cells):
    """the candidates cut into handle-loads of at most 4096 candidates and 64 MiB of profiles"""
    start, nbytes = 0, 0
    for k, v in enumerate(q):
        b = 4 * ((int(v) >> 32) // bin_cells)
        if k - start == MAX_CANDIDATES or (k > start and nbytes + b > MAX_PROFILE_BYTES):
            yield q[start:k]
            start, nbytes = k, 0
        nbytes += b
    if len(q) > start:
        yield q[start:]


def _search(power, q, bin_cells, device):
    """fold one float32 stream over every candidate of q, load by load; the records in list order"""
    import torch
    if is_torch(power) and power.is_cuda:
        p = power.reshape(-1)
        device = p.device.index
    else:
        a = np.asarray(power.numpy() if is_torch(power) else power)
        if a.dtype != np.float32:
            raise TypeError(f"expected float32 powers, got {a.dtype}")
        a = np.ascontiguousarray(a).reshape(-1)
        p = None
    rec = []
    for part in _loads(q, int(bin_cells)):
        with FinePriFold(part, bin_cells, device=device) as fold:
            if p is None:                           # once the device is known: the stream goes up once
                p = torch.from_numpy(a).to(torch.device("cuda", fold.device_index))
            fold.process(p)
            rec.append(fold.scores())
    return np.concatenate(rec) if rec else np.zeros(0, QSCORE_DTYPE)


def refine_pri(power, centre, half_span, step, bin_cells: int = 4, device: int = -1) -> np.ndarray:
    """The period of the train in a float32 power stream (device tensor or numpy), searched over centre - half_span ..
    centre + half_span in steps of ``step`` samples, in handle-loads of at most 4096 candidates and 64 MiB of profiles.
    Returns QFOUND_DTYPE records ranked as ``find_pri`` ranks: ``found[0]["period"]`` is the estimate, ``origin`` where
    the train's peak lies modulo the period (to one bin)."""
    c, h, s = Fraction(centre), Fraction(half_span), Fraction(step)
    if s <= 0:
        raise ValueError("step must be positive")
    n = int(h / s + Fraction(1, 1 << 20))
    q = np.array([period_q32(c + k * s) for k in range(-n, n + 1)], np.uint64)
    return rank_fine(_search(power, q, bin_cells, device), bin_cells)


def find_pri_fine(iq, replica, pri_min, pri_max, step, *, bin_cells: int = 4, sample_format: str | None = None,
                  bit_width: int = 12, normalize: bool = False, chunk_samples: int = 1 << 22,
                  device: int = -1) -> np.ndarray:
    """The repetition interval, to ``step`` samples, of the pulse train in an I/Q stream that matches ``replica``: a
    ``MatchedFilter`` (power output) runs once, its powers stay on the device (4 bytes a sample; more than 2^27
    samples is a ValueError: search a part of the record) and are folded over pri_min, pri_min + step, ... pri_max.
    Returns the ``refine_pri`` ranking."""
    import torch

    from .matched_filter import MatchedFilter, _format_of, _replica
    q = grid_q32(pri_min, pri_max, step)
    r = _replica(replica)
    fmt = sample_format or _format_of(iq)
    on_device = is_torch(iq) and iq.is_cuda
    x = iq if on_device else np.asarray(iq)
    if not on_device and np.iscomplexobj(x):
        x = np.ascontiguousarray(x, np.complex64).view(np.float32).reshape(-1, 2)
    x = x.reshape(-1, 2) if not (on_device and x.is_complex()) else x
    if x.shape[0] > MAX_SEARCH_SAMPLES:
        raise ValueError(f"{x.shape[0]} samples: find_pri_fine keeps the powers of at most {MAX_SEARCH_SAMPLES} on the device")
    with MatchedFilter(r, fmt, bit_width, "power", normalize, device=device) as mf:
        dev = torch.device("cuda", mf.device_index)
        parts = []
        for s in range(0, x.shape[0], chunk_samples):
            part = x[s:s + chunk_samples]
            d = part if on_device else torch.from_numpy(np.array(part)).to(dev)
            parts.append(mf.process(d).reshape(-1).clone())
        power = torch.cat(parts) if parts else torch.zeros(0, dtype=torch.float32, device=dev)
        return rank_fine(_search(power, q, bin_cells, mf.device_index), bin_cells)


def regrid_doppler_frequencies(period, doppler_length: int, fs: float, centered: bool = False) -> np.ndarray:
    """d fs / (doppler_length period) for the rows of maps made from a regridded stream: the true period, not the
    row length (pfb_regrid_doppler_frequencies; host only)."""
    out = np.empty(max(int(doppler_length), 1), np.float64)
    L.check(L.load().pfb_regrid_doppler_frequencies(_one_q32(period), int(doppler_length), int(bool(centered)), float(fs),
                                                    out.ctypes.data_as(C.POINTER(C.c_double))),
            "pfb_regrid_doppler_frequencies")
    return out


def _one_q32(period) -> int:
    q = int(period) if isinstance(period, np.uint64) else period_q32(period)
    if q >= 1 << 64:
        raise ValueError("periods are below 2^32 samples")
    return q


class Regrid(Handle):
    """Streaming gather of the windows of a train at ``period`` (samples as float, Fraction or int; np.uint64: Q32):
    output element k row_samples + r is input element origin + ceil(k period) + r, copied bit for bit.  A stream may be
    cut into calls of any length; each returns the elements whose source it holds.  numpy in -> numpy out, CUDA tensor
    in -> CUDA tensor out.  dtype: complex64 or float32."""

    _kind, _destroy, _get_device = "regridder", "pfb_regrid_destroy", "pfb_regrid_get_device"

    def __init__(self, period, row_samples: int, origin: int = 0, dtype=np.complex64, device: int = -1):
        self._h = C.c_void_p()
        lib = L.load()
        self.dtype = np.dtype(dtype)
        if self.dtype not in (np.dtype(np.complex64), np.dtype(np.float32)):
            raise TypeError(f"a regridder copies complex64 or float32 elements, not {self.dtype}")
        self.period_q32 = _one_q32(period)
        self.row_samples = int(row_samples)
        cfg = L.PfbRegridConfig(C.sizeof(L.PfbRegridConfig), self.row_samples, self.period_q32, int(origin),
                                self.dtype.itemsize, 0, int(device), 0)
        L.check(lib.pfb_regrid_create(C.byref(cfg), C.byref(self._h)), "pfb_regrid_create")
        self._created(lib)

    def reset(self) -> None:
        L.check(self._lib.pfb_regrid_reset(self._h), "pfb_regrid_reset")

    def set_index(self, next_input: int) -> None:
        """Make ``next_input`` the stream index of the next input element."""
        L.check(self._lib.pfb_regrid_set_index(self._h, int(next_input)), "pfb_regrid_set_index")

    def set_stream(self, hip_stream: int) -> None:
        L.check(self._lib.pfb_regrid_set_stream(self._h, C.c_void_p(hip_stream)), "pfb_regrid_set_stream")

    def sync(self) -> None:
        L.check(self._lib.pfb_regrid_sync(self._h), "pfb_regrid_sync")

    @property
    def next_index(self) -> int:
        m = C.c_uint64()
        L.check(self._lib.pfb_regrid_next_index(self._h, C.byref(m)), "pfb_regrid_next_index")
        return int(m.value)

    def outputs_for(self, num_inputs: int) -> int:
        """The output elements the next num_inputs input elements give."""
        m = C.c_uint64()
        L.check(self._lib.pfb_regrid_outputs_for(self._h, int(num_inputs), C.byref(m)), "pfb_regrid_outputs_for")
        return int(m.value)

    def _torch_dtype(self):
        import torch
        return torch.complex64 if self.dtype == np.complex64 else torch.float32

    def _device_elems(self, x) -> int:
        import torch
        if not (is_torch(x) and x.is_cuda):
            raise TypeError(f"expected a CUDA tensor for this {self._kind}")
        if x.device.index != self.device_index:
            raise ValueError(f"the tensor is on cuda:{x.device.index}, the {self._kind} on cuda:{self.device_index}")
        if not x.is_contiguous():
            raise ValueError("device elements must be contiguous")
        if x.dtype == self._torch_dtype():
            return x.numel()
        if self.dtype == np.complex64 and x.dtype == torch.float32 and x.numel() % 2 == 0:
            return x.numel() // 2                   # interleaved I, Q
        raise TypeError(f"expected {self._torch_dtype()} elements for this {self._kind}, got {x.dtype}")

    def process(self, x, capacity: int | None = None):
        """Take one buffer of the stream; returns the output elements whose source lies in it, flat.  ``capacity``: the
        room of the first attempt (default: what ``outputs_for`` says); the buffer is grown and the call made again on
        PFB_ERR_CAPACITY, which changes no state."""
        count = C.c_uint64()
        if is_torch(x) and x.is_cuda:
            import torch
            n = self._device_elems(x)
            make = lambda m: torch.zeros(m, dtype=self._torch_dtype(), device=x.device)  # noqa: E731
            src, mem, ptr = x.data_ptr(), L.PFB_MEM_DEVICE, (lambda b: b.data_ptr())
        else:
            a = np.asarray(x.numpy() if is_torch(x) else x)
            if self.dtype == np.complex64 and a.dtype == np.float32 and a.size % 2 == 0:
                a = np.ascontiguousarray(a).reshape(-1).view(np.complex64)
            if a.dtype != self.dtype:
                raise TypeError(f"expected {self.dtype} elements for this {self._kind}, got {a.dtype}")
            a = np.ascontiguousarray(a).reshape(-1)
            n = a.size
            make = lambda m: np.zeros(m, self.dtype)  # noqa: E731
            src, mem, ptr = a.ctypes.data, L.PFB_MEM_HOST, (lambda b: b.ctypes.data)
        cap = self.outputs_for(n) if capacity is None else int(capacity)
        while True:
            buf = make(max(cap, 1))
            rc = self._lib.pfb_regrid_process(self._h, C.c_void_p(src), n, C.c_void_p(ptr(buf)), cap, C.byref(count), mem)
            if rc != L.PFB_ERR_CAPACITY:
                break
            cap = int(count.value)
        L.check(rc, "pfb_regrid_process")
        return buf[: int(count.value)]

    __call__ = process

    def process_async(self, x, out, count) -> None:
        """Queue one buffer of device elements on the handle's stream without a host sync (pfb_regrid_process_async):
        the outputs go to ``out``, a contiguous CUDA tensor of the handle's dtype, their number to ``count``, an int64
        CUDA tensor of one element, in stream order.  PFB_ERR_CAPACITY queues nothing."""
        import torch
        n = self._device_elems(x)
        if not (is_torch(out) and out.is_cuda and out.dtype == self._torch_dtype() and out.is_contiguous()
                and out.device.index == self.device_index):
            raise ValueError(f"out must be a contiguous {self._torch_dtype()} tensor on cuda:{self.device_index}")
        if not (is_torch(count) and count.is_cuda and count.dtype == torch.int64 and count.numel() >= 1
                and count.is_contiguous() and count.device.index == self.device_index):
            raise ValueError(f"count must be an int64 tensor on cuda:{self.device_index}")
        L.check(self._lib.pfb_regrid_process_async(self._h, C.c_void_p(x.data_ptr()), n, C.c_void_p(out.data_ptr()),
                                                   out.numel(), C.c_void_p(count.data_ptr())), "pfb_regrid_process_async")


def regrid(y, period, row_samples: int, origin: int = 0, device: int = -1):
    """``Regrid(...).process(y)`` in one call; the element type is y's (complex64 or float32)."""
    if is_torch(y):
        dt = np.complex64 if y.is_complex() else np.float32
    else:
        dt = np.complex64 if np.iscomplexobj(y) else np.float32
    with Regrid(period, row_samples, origin, dt, device) as rg:
        return rg.process(y)


def detect_pulse_train_fine(iq, replica, period, num_pulses: int, num_gates: int | None = None, origin: int = 0, *,
                            pfa: float | None = None, alpha: float | None = None, window=None, doppler_length: int = 0,
                            block_cells: int = 64, guard_blocks: int | None = None, train_blocks: int = 8,
                            merge_gap: int | None = None, fs: float = 1.0, sample_format: str | None = None,
                            bit_width: int = 12, normalize: bool = False, chunk_samples: int = 1 << 22,
                            device: int = -1) -> np.ndarray:
    """``detect_pulse_train`` for a train whose repetition interval ``period`` is not a whole number of samples (a
    ``find_pri_fine`` record's ``period``, a deinterleaver's, or a uint64 Q32 value): ``MatchedFilter`` (complex) ->
    ``Regrid`` (rows of num_gates samples, default floor(period)) -> ``PulseDoppler(pri=num_gates)`` ("best" cells,
    centered) -> ``Cfar`` per interval, chunk by chunk on the device.  Returns the same TRAIN_DET_DTYPE records; the
    train's first sample is origin + gate, and ``frequency`` = doppler_bin fs / (doppler_length period) comes from the
    true period.  Each pulse is taken at the first whole sample at or after its true start."""
    import torch

    from .cfar import Cfar, cfar_alpha, records
    from .matched_filter import MatchedFilter, _format_of, _replica
    from .pulse_doppler import TRAIN_DET_DTYPE, PulseDoppler, describe_pulse_doppler
    r = _replica(replica)
    K = r.size
    q = _one_q32(period)
    R = (q >> 32) if num_gates is None else int(num_gates)
    plan = describe_pulse_doppler(R, num_pulses, R, 0, window, doppler_length, "best", True)
    ND = int(plan.doppler_length)
    if alpha is None:
        harmonic = float(np.sum(1.0 / np.arange(1, ND + 1)))
        alpha = cfar_alpha((1e-6 if pfa is None else pfa) / ND, 2 * int(train_blocks) * int(block_cells)) / harmonic
    elif pfa is not None:
        raise ValueError("give one of alpha and pfa")
    G = -(-K // block_cells) if guard_blocks is None else guard_blocks
    g = K if merge_gap is None else merge_gap
    fmt = sample_format or _format_of(iq)
    hz_per_bin = float(fs) / (ND * period_samples(q))
    found = []
    with MatchedFilter(r, fmt, bit_width, "complex", normalize, device=device) as mf, \
            Regrid(np.uint64(q), R, origin, np.complex64, device=mf.device_index) as rg, \
            PulseDoppler(R, num_pulses, R, 0, window, ND, "best", True, device=mf.device_index) as pd, \
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
                out["frequency"] = recs["hypothesis"] * hz_per_bin
                out["peak_power"], out["noise"] = recs["peak_power"], recs["noise"]
                found.append(out)
                cpi += 1

        for s in range(0, x.shape[0], chunk_samples):
            part = x[s:s + chunk_samples]
            d = part if on_device else torch.from_numpy(np.array(part)).to(dev)
            take(pd.process(rg.process(mf.process(d))))
        take(pd.flush(dev))
    return np.concatenate(found) if found else np.zeros(0, TRAIN_DET_DTYPE)
