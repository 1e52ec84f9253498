"""The waterfall contract without a GPU: the numpy restatement (wf_ref) against the scripts' own lines, the cell layout,
the host-only entry point and every argument check that comes before the device."""
import ctypes as C
import importlib
import os
import re

import numpy as np
import pytest

import wf_ref as R
from abi_symbols import declared_symbols
from sdr_channelizer_amd import _lib as L
from sdr_channelizer_amd import build

# the package re-exports the function `waterfall`, which hides the module of that name from a plain import
waterfall = importlib.import_module("sdr_channelizer_amd.waterfall")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

WF_EXPORTS = {"pfb_wf_create", "pfb_wf_destroy", "pfb_wf_reset", "pfb_wf_set_stream", "pfb_wf_sync", "pfb_wf_get_device",
              "pfb_wf_bins_for", "pfb_wf_process", "pfb_wf_process_async", "pfb_wf_flush", "pfb_wf_choose_bin",
              "pfb_wf_from_channelizer_iq_file", "pfb_wf_from_stft_iq_file"}


@pytest.mark.parametrize("B", [1, 5, 64])
def test_restatement_is_the_scripts(B):
    """channelizer_example.m:56 and generate_channelized_training_iq.m:108 draw abs(x), spectrogram_my_iq.m:115
    abs(s).^2, of every element; a pixel of B rows is their max / min / mean over the bin.  abs() is np.hypot, within
    1 ulp of the magnitude; its square carries 2.5 * 2^-52 per term and the mean's sum (count - 1) * 2^-53, so
    (count + 3) * 2^-52 holds the script's float64 mean against the restatement's."""
    rows, W = 333, 7
    x = R.random_matrix("complex", rows, W, seed=B)
    x[10:13, 2] = 50.0                                      # the column's largest power three times: the first row wins
    mag = np.hypot(x.real.astype(np.float64), x.imag.astype(np.float64))
    got = R.waterfall(x, "complex", B)
    assert got.shape == (-(-rows // B), W) and got.dtype == R.CELL_DTYPE
    for b in range(got.shape[0]):
        m = mag[b * B:(b + 1) * B]
        p = m ** 2
        assert np.all(np.abs(np.sqrt(got["power_max"][b].astype(np.float64)) - m.max(0)) <= 2.0 ** -23 * m.max(0))
        assert np.all(np.abs(np.sqrt(got["power_min"][b].astype(np.float64)) - m.min(0)) <= 2.0 ** -23 * m.min(0))
        mean = p.mean(0)
        assert np.all(np.abs(got["power_mean"][b].astype(np.float64) - mean) <= (2.0 ** -24 + (len(m) + 3) * 2.0 ** -52) * mean)
        assert np.array_equal(got["peak_row"][b], R.powers(x[b * B:(b + 1) * B], "complex").argmax(0))
    if B == 5:
        assert got["peak_row"][2, 2] == 0                 # rows 10, 11, 12 of column 2 are equal: row 10 = bin 2, offset 0
    # the float32 kinds: |y| and |y|^2 as the channelizer stores them
    a = mag.astype(np.float32)
    assert R.same_selections(R.waterfall(a, "magnitude", B), R.cells_of(a.astype(np.float64) ** 2, B))
    pw = (a * a).astype(np.float32)
    assert R.same_selections(R.waterfall(pw, "power", B), R.cells_of(pw.astype(np.float64), B))


@pytest.mark.parametrize("element", R.ELEMENTS)
def test_restatement_does_not_depend_on_the_cutting(element):
    """fold the figures of the pieces of a bin, cut anywhere: the selections are the same bits, the mean within 1 ulp"""
    B, W = 40, 5
    x = R.random_matrix(element, 3 * B, W, seed=9)
    x[50:70, 1] = x[45, 1]        # the largest power may sit on both sides of a cut
    p = R.powers(x, element)
    whole = R.cells_of(p, B)
    for cut in (0, 1, 39, 40, 41, 45, 46, 50, 60, 70, 119, 120):
        folded = np.zeros_like(whole)
        for b in range(3):
            pieces = [q for q in (p[b * B:max(b * B, min(cut, (b + 1) * B))], p[max(b * B, min(cut, (b + 1) * B)):(b + 1) * B])
                      if q.shape[0]]
            first = b * B
            best, low, total, at = None, None, 0.0, None
            for q in pieces:
                off = first - b * B
                mx, am = q.max(0), q.argmax(0) + off
                take = (mx > best) if best is not None else np.ones(W, bool)   # a later piece wins only with more power
                best = np.where(take, mx, best) if best is not None else mx
                at = np.where(take, am, at) if at is not None else am
                low = np.minimum(low, q.min(0)) if low is not None else q.min(0)
                total = total + q.sum(0)
                first += q.shape[0]
            folded["power_max"][b], folded["power_min"][b] = best.astype(np.float32), low.astype(np.float32)
            folded["power_mean"][b], folded["peak_row"][b] = (total / B).astype(np.float32), at
        R.check_cells(folded, whole, f"cut {cut}")


def test_cell_layout():
    assert C.sizeof(L.PfbWfCell) == 16 == R.CELL_DTYPE.itemsize == waterfall.CELL_DTYPE.itemsize
    assert R.CELL_DTYPE == waterfall.CELL_DTYPE
    for name, _ in L.PfbWfCell._fields_:
        assert getattr(L.PfbWfCell, name).offset == R.CELL_DTYPE.fields[name][1], name
        assert getattr(L.PfbWfCell, name).size == R.CELL_DTYPE.fields[name][0].itemsize, name
    assert [n for n, _ in L.PfbWfCell._fields_] == list(R.CELL_DTYPE.names)
    assert C.sizeof(L.PfbWfConfig) == 28
    assert L.load().pfb_abi_version() == 2
    assert waterfall.row_tile(8) == 4096 and waterfall.row_tile(1024) == 256 and waterfall.row_tile(65536) == 64
    assert waterfall.row_tile(8, "columns") == waterfall.COLUMN_TILE
    assert waterfall.slot_columns("complex") == 2 and waterfall.slot_columns("power") == 4


def test_choose_bin():
    lib = L.load()
    b = C.c_uint32(77)
    for max_bins in (1, 7, 1024, 2 ** 32 - 1):
        for n in (0, 1, max_bins, max_bins + 1, 2 ** 24, 2 ** 32 + 5):
            want = max(1, -(-n // max_bins))
            if want > 2 ** 24:
                assert lib.pfb_wf_choose_bin(n, max_bins, C.byref(b)) == L.PFB_ERR_BAD_ARG, (n, max_bins)
                continue
            assert lib.pfb_wf_choose_bin(n, max_bins, C.byref(b)) == L.PFB_OK and b.value == want, (n, max_bins)
            assert waterfall.choose_bin(n, max_bins) == want
    assert lib.pfb_wf_choose_bin(2 ** 24, 1, C.byref(b)) == L.PFB_OK and b.value == 2 ** 24
    assert lib.pfb_wf_choose_bin(2 ** 24 + 1, 1, C.byref(b)) == L.PFB_ERR_BAD_ARG
    assert lib.pfb_wf_choose_bin(100, 0, C.byref(b)) == L.PFB_ERR_BAD_ARG
    assert lib.pfb_wf_choose_bin(100, 10, None) == L.PFB_ERR_BAD_ARG


def config(W=8, B=4, element=0, layout=0, flags=0, size=None, device=-1):
    return L.PfbWfConfig(C.sizeof(L.PfbWfConfig) if size is None else size, W, B, element, layout, flags, device)


def test_arguments_are_checked_before_the_device():
    lib = L.load()
    h = C.c_void_p()

    def create(**kw):
        cfg = config(**kw)
        return lib.pfb_wf_create(C.byref(cfg), C.byref(h))

    assert lib.pfb_wf_create(None, C.byref(h)) == L.PFB_ERR_BAD_ARG
    cfg = config()
    assert lib.pfb_wf_create(C.byref(cfg), None) == L.PFB_ERR_BAD_ARG
    assert create(size=24) == L.PFB_ERR_BAD_ARG
    assert create(W=0) == L.PFB_ERR_BAD_ARG and create(W=65537) == L.PFB_ERR_BAD_ARG
    assert create(B=0) == L.PFB_ERR_BAD_ARG and create(B=2 ** 24 + 1) == L.PFB_ERR_BAD_ARG
    assert create(element=3) == L.PFB_ERR_BAD_ARG and create(layout=2) == L.PFB_ERR_BAD_ARG
    for bit in (1, 2, 1 << 31):
        assert create(flags=bit) == L.PFB_ERR_BAD_ARG
    assert not h.value
    # null handles and pointers
    u, b, w = C.c_uint64(), C.c_uint32(), C.c_uint32()
    buf = np.zeros(64, np.float32)
    p = C.c_void_p(buf.ctypes.data)
    assert lib.pfb_wf_destroy(None) == lib.pfb_wf_reset(None) == lib.pfb_wf_sync(None) == L.PFB_ERR_BAD_ARG
    assert lib.pfb_wf_set_stream(None, None) == lib.pfb_wf_get_device(None, None) == L.PFB_ERR_BAD_ARG
    assert lib.pfb_wf_bins_for(None, 5, C.byref(u)) == L.PFB_ERR_BAD_ARG
    for mem in (L.PFB_MEM_HOST, L.PFB_MEM_DEVICE, 2):
        assert lib.pfb_wf_process(None, p, 4, 0, p, 1, C.byref(u), mem) == L.PFB_ERR_BAD_ARG
    assert lib.pfb_wf_process_async(None, p, 4, 0, p, 1, C.byref(u)) == L.PFB_ERR_BAD_ARG
    assert lib.pfb_wf_flush(None, p, C.byref(w)) == L.PFB_ERR_BAD_ARG
    info = L.PfbIqInfo()
    fake = C.c_void_p(16)   # never dereferenced: the other arguments fail first
    for call in (lib.pfb_wf_from_channelizer_iq_file, lib.pfb_wf_from_stft_iq_file):
        assert call(None, b"x.iq", 16, 0, p, 1, C.byref(u), C.byref(b), C.byref(info)) == L.PFB_ERR_BAD_ARG
        assert call(fake, None, 16, 0, p, 1, C.byref(u), C.byref(b), C.byref(info)) == L.PFB_ERR_BAD_ARG
        assert call(fake, b"x.iq", 0, 0, p, 1, C.byref(u), C.byref(b), C.byref(info)) == L.PFB_ERR_BAD_ARG
        assert call(fake, b"x.iq", 16, 0, None, 1, C.byref(u), C.byref(b), C.byref(info)) == L.PFB_ERR_BAD_ARG
        assert call(fake, b"x.iq", 16, 0, p, 1, None, C.byref(b), C.byref(info)) == L.PFB_ERR_BAD_ARG
        assert call(fake, b"x.iq", 16, 0, p, 1, C.byref(u), None, C.byref(info)) == L.PFB_ERR_BAD_ARG
        assert call(fake, b"x.iq", 16, 0, C.c_void_p(buf.ctypes.data + 8), 1, C.byref(u), C.byref(b), None) \
            == L.PFB_ERR_BAD_ARG
    with pytest.raises(ValueError):
        waterfall.waterfall(np.zeros((4, 4), np.float32))                    # neither bin_rows nor max_rows
    with pytest.raises(ValueError):
        waterfall.waterfall_from_iq_file("x.iq")                             # neither route


def test_a_valid_config_needs_a_device():
    lib = L.load()
    if lib.pfb_device_count() > 0:
        pytest.skip("a GPU is present")
    h = C.c_void_p()
    for W in (1, 65536):
        for B in (1, 2 ** 24):
            for element in range(3):
                for layout in range(2):
                    cfg = config(W=W, B=B, element=element, layout=layout)
                    assert lib.pfb_wf_create(C.byref(cfg), C.byref(h)) == L.PFB_ERR_NO_DEVICE and not h.value
    with pytest.raises(L.PfbError) as e:
        waterfall.Waterfall(8, 4)
    assert e.value.status == L.PFB_ERR_NO_DEVICE


def test_exports_header_and_guard():
    declared = {n for n in declared_symbols() if n.startswith("pfb_wf_")} - {"pfb_wf_cell", "pfb_wf_config", "pfb_wf_handle"}
    assert declared == WF_EXPORTS == {n for n in L.EXPORTS if n.startswith("pfb_wf_")}
    lib = L.load()
    for name in WF_EXPORTS:
        assert hasattr(lib, name) and getattr(lib, name).argtypes is not None, name
    import sdr_channelizer_amd as pkg
    for name in ("Waterfall", "WaterfallImage", "waterfall", "waterfall_from_iq_file"):
        assert name in pkg.__all__ and getattr(pkg, name) is getattr(waterfall, name)
    src = open(os.path.join(ROOT, "sdr_channelizer_amd", "csrc", "pfb_waterfall.hip")).read()
    found = {}
    for m in re.finditer(r'^extern "C" int (\w+)\(', src, re.M):
        rest = src[m.start():]
        found[m.group(1)] = rest[: rest.index("\n}\n")]
    assert set(found) == WF_EXPORTS
    for name, body in found.items():
        assert "abi_guard" in body.split("{", 1)[1][:80], name
    assert src.count('extern "C"') == len(found)
    assert "atomic" not in src.replace("No atomics", "").replace("floating-point atomics", "")
    assert "sqrt" not in src and "log10" not in src
    assert "pfb_waterfall.hip" in build.SOURCES
    hdr = open(os.path.join(ROOT, "include", "pfb_channelizer.h")).read()
    assert "#define PFB_ABI_VERSION 2" in hdr
