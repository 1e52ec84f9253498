"""Time-binned waterfalls of channelizer and STFT output on the GPU, over the C ABI (pfb_wf_* in
include/pfb_channelizer.h).

The reference draws its two-dimensional pictures from the whole matrix:

    surf(abs(channelizer(x)))                  channelizer_example.m:56-71
    surf(f,t,abs(chan_iq))                     generate_channelized_training_iq.m:100-108
    mesh(..., abs(s).^2)                       spectrogram_my_iq.m:114-115

Nobody draws 1.4 million image rows.  ``Waterfall`` cuts the rows (frames) of such a matrix into bins of ``bin_rows`` --
one image row each -- and gives every (bin, column) pixel its largest, mean and smallest power and the row inside the
bin where the peak sits, without the matrix leaving the GPU; ``waterfall_from_iq_file`` goes from a record to the image
without the matrix ever existing in full.  Magnitude and dB are the caller's, one value per pixel; drawing stays with
the caller too.
"""
from __future__ import annotations

import ctypes as C
from typing import NamedTuple

import numpy as np

from . import _lib as L
from ._handle import Handle, is_torch

_ELEMENT = {"complex": L.PFB_WF_COMPLEX, "magnitude": L.PFB_WF_MAGNITUDE, "power": L.PFB_WF_POWER}
_LAYOUT = {"rows": L.PFB_WF_ROWS, "columns": L.PFB_WF_COLUMNS}

# the thresholds of csrc/pfb_waterfall.hip, for the tests to sit on
MAX_WIDTH = 65536            # kMaxWidth
MAX_BIN_ROWS = 1 << 24       # kMaxBin
TILE_ELEMS = 1 << 18         # kTileElems: "rows" cuts a bin every row_tile(width) rows; longer bins are folded from partials
MIN_TILE_ROWS, MAX_TILE_ROWS = 64, 4096
COLUMN_TILE = 4096           # kColTile: the same for "columns", in elements of one column
COLUMN_LANE_ELEMS = 16       # kLaneElems: "columns" gives a run of n elements pow2ceil(ceil(n / 16)) lanes, at most 256
VECTOR_BYTES = 16            # a slot of a row: 2 complex64 or 4 float32 columns
WAVE_SLOTS = 64              # rows of more slots take whole waves
GROUP_SLOTS = 256            # rows of more slots take several workgroups (column tiles)

# pfb_wf_cell
CELL_DTYPE = np.dtype([("power_max", "<f4"), ("power_mean", "<f4"), ("power_min", "<f4"), ("peak_row", "<u4")])


def row_tile(width: int, layout: str = "rows") -> int:
    """Rows per segment: a bin longer than this is reduced by several workgroups and folded."""
    if layout == "columns":
        return COLUMN_TILE
    return min(max(TILE_ELEMS // int(width), MIN_TILE_ROWS), MAX_TILE_ROWS)


def slot_columns(element: str) -> int:
    """Columns per 16-byte slot of a row."""
    return VECTOR_BYTES // (8 if element == "complex" else 4)


class WaterfallImage(NamedTuple):
    """What a picture of one pixel per (bin, column) needs; the four images are (bins, width)."""
    t: np.ndarray           # seconds of the first frame of each bin
    f: np.ndarray           # Hz of each column
    power_max: np.ndarray
    power_mean: np.ndarray
    power_min: np.ndarray
    peak_row: np.ndarray    # offset inside the bin of the first row holding power_max
    bin_rows: int
    rows_in_last: int       # rows of the last bin: bin_rows, fewer for a final partial bin
    info: L.PfbIqInfo | None = None


def choose_bin(rows: int, max_bins: int) -> int:
    """max(1, ceil(rows / max_bins)) (pfb_wf_choose_bin; host only)."""
    b = C.c_uint32()
    L.check(L.load().pfb_wf_choose_bin(int(rows), int(max_bins), C.byref(b)), "pfb_wf_choose_bin")
    return int(b.value)


def as_cells(cells, width: int | None = None) -> np.ndarray:
    """A structured numpy array (CELL_DTYPE) of what ``Waterfall.process`` returned: a view for a numpy result, a copy
    to the host for the (bins, width, 16) uint8 tensor of a CUDA call."""
    if is_torch(cells):
        cells = cells.cpu().numpy()
    if cells.dtype != CELL_DTYPE:
        cells = np.ascontiguousarray(cells).view(CELL_DTYPE)
        cells = cells.reshape(cells.shape[:-1])
    return cells if width is None else cells.reshape(-1, width)


class Waterfall(Handle):
    """Stateful reduction of a rows x width matrix that arrives in pieces: bin b covers rows [b B, (b+1) B) of
    everything fed since creation, ``reset()`` or ``flush()``; each call returns the cells of the bins it completes, and
    any cutting of the rows into calls gives the same cells (but for the last bit of power_mean)."""

    _kind, _destroy, _get_device = "waterfall", "pfb_wf_destroy", "pfb_wf_get_device"

    def __init__(self, width: int, bin_rows: int, element: str = "complex", layout: str = "rows", device: int = -1):
        self._h = C.c_void_p()
        lib = L.load()
        self.width, self.bin_rows = int(width), int(bin_rows)
        self.element, self.layout = element, layout
        if not (0 <= self.width < 2 ** 32 and 0 <= self.bin_rows < 2 ** 32):
            raise ValueError(f"width must be 1 .. 65536 and bin_rows 1 .. 2^24, got {width}, {bin_rows}")
        cfg = L.PfbWfConfig(C.sizeof(L.PfbWfConfig), self.width, self.bin_rows, _ELEMENT[element], _LAYOUT[layout], 0,
                            int(device))
        L.check(lib.pfb_wf_create(C.byref(cfg), C.byref(self._h)), "pfb_wf_create")
        self._created(lib)

    def reset(self) -> None:
        L.check(self._lib.pfb_wf_reset(self._h), "pfb_wf_reset")

    def set_stream(self, hip_stream: int) -> None:
        L.check(self._lib.pfb_wf_set_stream(self._h, C.c_void_p(hip_stream)), "pfb_wf_set_stream")

    def sync(self) -> None:
        L.check(self._lib.pfb_wf_sync(self._h), "pfb_wf_sync")

    def bins_for(self, rows: int) -> int:
        f = C.c_uint64()
        L.check(self._lib.pfb_wf_bins_for(self._h, int(rows), C.byref(f)), "pfb_wf_bins_for")
        return int(f.value)

    def _geometry(self, shape, ld: int, rows: int) -> tuple[int, int]:
        """(rows, pitch in elements) of a call.  A 2-D ``x`` is (rows, pitch) for "rows" and (width, pitch) for
        "columns", where ``rows`` may take the first rows of every column; a flat ``x`` needs ``rows`` and holds the
        matrix at pitch ``ld`` (0 = dense), its last row or column ending where the matrix ends."""
        W = self.width
        if len(shape) == 2:
            a, b = int(shape[0]), int(shape[1])
            if ld and ld != b:
                raise ValueError(f"ld = {ld}, the matrix has a pitch of {b}")
            if self.layout == "rows":
                if b < W:
                    raise ValueError(f"rows of {b} elements, the {self._kind} is {W} wide")
                return a, b
            if a != W or rows > b:
                raise ValueError(f"expected {W} columns of at least {max(rows, 0)} rows, got {a} of {b}")
            return (b if rows < 0 else int(rows)), b
        if len(shape) != 1 or rows < 0:
            raise ValueError("a flat buffer needs rows=, anything else must be 2-D")
        n = int(rows)
        dense = W if self.layout == "rows" else n
        pitch = int(ld) or dense
        need = 0 if n == 0 else ((n - 1) * pitch + W if self.layout == "rows" else (W - 1) * pitch + n)
        if pitch < dense or int(shape[0]) < need:
            raise ValueError(f"{n} rows at pitch {pitch} need {need} elements, the buffer holds {shape[0]}")
        return n, pitch

    def process(self, x, out=None, sync: bool = True, ld: int = 0, rows: int = -1):
        """The cells of the bins this matrix completes.  ``x``: (rows, pitch) for "rows", (width, pitch) for "columns"
        (``rows`` < pitch takes the first rows of every column), or a flat buffer with ``rows`` and ``ld``; complex64
        for "complex", float32 otherwise.  numpy in ("rows" only) -> a (bins, width) structured array (CELL_DTYPE); CUDA
        tensor in -> a (bins, width, 16) uint8 tensor on the same device (``as_cells`` views it).  ``out``: the same
        kind, with room for ``bins_for(rows)`` bins.  sync=False only enqueues on the handle's stream (CUDA input)."""
        f = C.c_uint64()
        W, cell = self.width, CELL_DTYPE.itemsize
        if is_torch(x) and x.is_cuda:
            import torch
            want = torch.complex64 if self.element == "complex" else torch.float32
            if x.dtype != want or not x.is_contiguous() or x.device.index != self.device_index:
                raise TypeError(f"expected a contiguous {want} matrix on cuda:{self.device_index} for this {self._kind}")
            n, pitch = self._geometry(tuple(x.shape), ld, rows)
            F = self.bins_for(n)
            if out is None:
                out = torch.empty((F, W, cell), dtype=torch.uint8, device=x.device)
            elif (not is_torch(out) or out.device != x.device or out.dtype != torch.uint8 or not out.is_contiguous()
                  or out.numel() < F * W * cell):
                raise ValueError(f"out must be a contiguous uint8 tensor on {x.device} with room for {F} bins")
            if sync:
                L.check(self._lib.pfb_wf_process(self._h, C.c_void_p(x.data_ptr()), n, pitch, C.c_void_p(out.data_ptr()),
                                                 F, C.byref(f), L.PFB_MEM_DEVICE), "pfb_wf_process")
            else:
                L.check(self._lib.pfb_wf_process_async(self._h, C.c_void_p(x.data_ptr()), n, pitch,
                                                       C.c_void_p(out.data_ptr()), F, C.byref(f)),
                        "pfb_wf_process_async")
            return out.reshape(-1)[:F * W * cell].reshape(F, W, cell)
        a = np.asarray(x)
        want = np.dtype(np.complex64 if self.element == "complex" else np.float32)
        if a.dtype != want or not a.flags.c_contiguous:
            raise TypeError(f"expected a C-contiguous {want} matrix for this {self._kind}, got {a.dtype}")
        n, pitch = self._geometry(a.shape, ld, rows)
        F = self.bins_for(n)
        if out is None:
            out = np.zeros((F, W), dtype=CELL_DTYPE)
        elif (not isinstance(out, np.ndarray) or out.dtype != CELL_DTYPE or out.size < F * W or not out.flags.c_contiguous):
            raise ValueError(f"out must be a C-contiguous CELL_DTYPE numpy array with room for {F} bins")
        L.check(self._lib.pfb_wf_process(self._h, C.c_void_p(a.ctypes.data), n, pitch,
                                         C.c_void_p(out.ctypes.data), F, C.byref(f), L.PFB_MEM_HOST), "pfb_wf_process")
        return out.reshape(-1)[:F * W].reshape(F, W)

    def flush(self) -> tuple[np.ndarray, int]:
        """(cells, rows): the open bin as a (1, width) structured array with the rows it holds, or (0, width) and 0; the
        next row starts a new bin."""
        cells = np.zeros((1, self.width), dtype=CELL_DTYPE)
        have = C.c_uint32()
        L.check(self._lib.pfb_wf_flush(self._h, C.c_void_p(cells.ctypes.data), C.byref(have)), "pfb_wf_flush")
        return cells[:1 if have.value else 0], int(have.value)


def _element_of(x) -> str:
    if is_torch(x):
        return "complex" if x.is_complex() else "power"
    return "complex" if np.iscomplexobj(x) else "power"


def waterfall(x, bin_rows: int | None = None, max_rows: int | None = None, *, element: str | None = None,
              layout: str = "rows", device: int = -1) -> tuple[np.ndarray, int]:
    """One matrix as at most ``max_rows`` image rows (or in bins of ``bin_rows``), the final partial bin included:
    (cells, rows_in_last) with cells a (bins, width) structured array.  ``x``: (rows, width) for "rows", (width, rows)
    for "columns"; complex64, or float32 taken as power unless ``element`` says "magnitude"; numpy ("rows" only) or a
    CUDA tensor."""
    if (bin_rows is None) == (max_rows is None):
        raise ValueError("give bin_rows or max_rows, not both")
    n, W = (x.shape[0], x.shape[1]) if layout == "rows" else (x.shape[1], x.shape[0])
    B = int(bin_rows) if bin_rows is not None else choose_bin(n, max_rows)
    with Waterfall(W, B, element or _element_of(x), layout, device) as wf:
        done = as_cells(wf.process(x), W)
        last, have = wf.flush()
    return np.concatenate([done, last]), (have or (B if done.size else 0))


def _image(cells: np.ndarray, t, f, B: int, rows_in_last: int, info) -> WaterfallImage:
    return WaterfallImage(t, f, cells["power_max"].copy(), cells["power_mean"].copy(), cells["power_min"].copy(),
                          cells["peak_row"].copy(), int(B), int(rows_in_last), info)


def waterfall_from_iq_file(path: str, num_bands: int | None = None, *, stft_window=None, max_rows: int = 1024,
                           chunk_samples: int = 0, device: int = -1, **kw) -> WaterfallImage:
    """One .iq record as an image of at most ``max_rows`` rows.  ``num_bands``: through a ``Channelizer`` of that many
    bands (``kw`` goes to it: taps, decimation, fftshift, magnitude, power, channel_major, ...); ``f`` is
    ``centerFrequencies`` in the handle's own column order and t[b] = b B D / fs.  ``stft_window``: through an ``Stft``
    with that window (``kw``: overlap_length, fft_length, output "power" or "complex", ...); both axes are
    ``stft_axes``, t that of the first frame of each bin.  The channel matrix never exists in full."""
    from . import iqfile
    from .channelizer import Channelizer
    from .stft import Stft
    if (num_bands is None) == (stft_window is None):
        raise ValueError("give num_bands or stft_window, not both")
    with open(path, "rb") as fh:
        head = iqfile.parse_header(fh.read(128))
    fmt = {L.PFB_FMT_INT8_IQ: "int8", L.PFB_FMT_INT16_IQ: "int16", L.PFB_FMT_CF32: "cf32"}[int(head.sample_format)]
    n, bw = int(head.packet.numSamples), int(head.packet.bitWidth)
    f_out, b_out, info = C.c_uint64(), C.c_uint32(), L.PfbIqInfo()
    if num_bands is not None:
        with Channelizer(num_bands, sample_format=fmt, bit_width=bw, device=device, **kw) as ch:
            frames, W = ch.frames_for(n), ch.num_bands
            B = choose_bin(frames, max_rows)
            cells = np.zeros((-(-frames // B), W), dtype=CELL_DTYPE)
            L.check(ch._lib.pfb_wf_from_channelizer_iq_file(
                ch._h, str(path).encode(), int(max_rows), int(chunk_samples), C.c_void_p(cells.ctypes.data),
                cells.shape[0], C.byref(f_out), C.byref(b_out), C.byref(info)), "pfb_wf_from_channelizer_iq_file")
            fs = float(info.packet.sampleRateSps)
            f = ch.centerFrequencies(fs)
            t = np.arange(cells.shape[0], dtype=np.float64) * (B * ch.decimation) / fs
    else:
        kw.setdefault("output", "power")
        with Stft(stft_window, sample_format=fmt, bit_width=bw, device=device, **kw) as st:
            frames, W = st.frames_for(n), st.fft_length
            B = choose_bin(frames, max_rows)
            cells = np.zeros((-(-frames // B), W), dtype=CELL_DTYPE)
            L.check(st._lib.pfb_wf_from_stft_iq_file(
                st._h, str(path).encode(), int(max_rows), int(chunk_samples), C.c_void_p(cells.ctypes.data),
                cells.shape[0], C.byref(f_out), C.byref(b_out), C.byref(info)), "pfb_wf_from_stft_iq_file")
            fs = float(info.packet.sampleRateSps)
            f, t_all = st.axes(fs, 0, frames)
            t = t_all[::B].copy()
    assert int(f_out.value) == cells.shape[0] and int(b_out.value) == B
    return _image(cells, t, f, B, frames - (cells.shape[0] - 1) * B if cells.shape[0] else 0, info)
