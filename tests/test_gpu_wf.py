"""The waterfall unit (pfb_wf_*) on the GPU against its numpy restatement (wf_ref).  Pass condition everywhere
(wf_ref.check_cells): power_max, power_min and peak_row bit for bit, power_mean within 1 float32 ulp -- a bound that is
derived, not measured: a double sum of at most 2^24 non-negative terms in any order is within 2^-29 relative of the exact
sum, 1/32 of a float32 ulp, so two roundings of it differ only across a rounding boundary.  Every cell is compared.
No call is larger than 2^20 elements: where 5 B + 3 rows would be more, the longest k B + 3 that fits is taken."""
import ctypes as C
import importlib
import os

import numpy as np
import pytest

import wf_ref as R
from gpu_support import cuda_torch
from sdr_channelizer_amd import Channelizer, PulseTrain, Stft, center_frequencies, pinned_empty, stft_axes
from sdr_channelizer_amd import _lib as L

W = importlib.import_module("sdr_channelizer_amd.waterfall")   # the package's `waterfall` is the function

pytestmark = pytest.mark.gpu

MAX_ELEMS = 1 << 20
WIDTHS = [1, 2, 3, 7, 8, 56, 63, 64, 65, 130, 560, 768, 1024, 4096]
ROUTES = [("complex", "rows"), ("magnitude", "rows"), ("power", "rows"), ("complex", "columns"), ("power", "columns")]
BIG = {"complex": np.complex64(2.0 ** 30), "magnitude": np.float32(2.0 ** 30), "power": np.float32(2.0 ** 60)}


@pytest.fixture(scope="module")
def torch():
    return cuda_torch()


def device_piece(torch, piece, layout):
    """rows a..b of the matrix as the call's tensor: (n, W), or the call's own (W, n) columns"""
    return torch.from_numpy(np.ascontiguousarray(piece if layout == "rows" else piece.T)).cuda()


def run_cuts(torch, wf, x, cuts, flush=True):
    """feed rows cuts[i] .. cuts[i+1] of x call by call; the cells of every call, then the flushed bin"""
    outs = []
    for a, b in zip(cuts[:-1], cuts[1:]):
        outs.append(W.as_cells(wf.process(device_piece(torch, x[a:b], wf.layout)), wf.width))
    have = 0
    if flush:
        last, have = wf.flush()
        outs.append(last)
    return np.concatenate(outs), have


def bins_to_try(width, layout):
    T = W.row_tile(width, layout)
    cap = max(1, MAX_ELEMS // width)
    return [B for B in (1, 2, 3, 63, 64, 65, T - 1, T, T + 1, 3 * T + 5) if B + 1 <= cap]


def call_lengths(B, width):
    cap = max(1, MAX_ELEMS // width)
    k = max(1, min(5, (cap - 3) // B))
    return [0, 1, B - 1, B, B + 1, k * B + 3]


@pytest.mark.parametrize("width", WIDTHS)
def test_shapes(torch, width):
    """every width of the list x every bin length (1, 2, 3, 63, 64, 65, the row tile - 1 / + 0 / + 1 and a bin several
    tiles long) x the row counts 0, 1, B-1, B, B+1, 5B+3 -- each as a first call, then all one after the other, so that
    every later call meets an open bin -- and a flush; all three kinds by rows, complex and power by columns"""
    for element, layout in ROUTES:
        Bs = bins_to_try(width, layout)
        assert len(Bs) >= 6
        x = R.random_matrix(element, max(sum(call_lengths(B, width)) for B in Bs), width, seed=width)
        p = R.powers(x, element)
        for B in Bs:
            ns = call_lengths(B, width)
            with W.Waterfall(width, B, element, layout) as wf:
                for n in ns:                                        # as first calls
                    wf.reset()
                    got, have = run_cuts(torch, wf, x, [0, n])
                    assert have == n % B and wf.bins_for(0) == 0
                    R.check_cells(got, R.cells_of(p[:n], B), (element, layout, B, n))
                wf.reset()
                cuts = np.concatenate([[0], np.cumsum(ns)]).tolist()
                got, have = run_cuts(torch, wf, x, cuts)
                assert have == cuts[-1] % B
                R.check_cells(got, R.cells_of(p[:cuts[-1]], B), (element, layout, B, "sequence"))


@pytest.mark.parametrize("element,slots", [("complex", 2), ("power", 4), ("magnitude", 4)])
def test_width_thresholds(torch, element, slots):
    """the widths at which a row's slots fill a wave and a workgroup, - 1 / + 0 / + 1, with 16-byte slots (a dense
    matrix) and with one-element slots (an odd pitch)"""
    assert W.slot_columns(element) == slots
    for limit in (W.WAVE_SLOTS, W.GROUP_SLOTS):
        for per_slot in (slots, 1):
            for width in (limit * per_slot - 1, limit * per_slot, limit * per_slot + 1):
                if per_slot > 1:
                    pitch = -(-width // slots) * slots            # rows 16 bytes apart: 16-byte slots
                else:
                    pitch = width + (0 if width % slots else 1)   # no multiple of 16 bytes: one-element slots
                for B in (3, W.row_tile(width) + 1):
                    n = 2 * B + 2
                    x = R.random_matrix(element, n, pitch, seed=width + B)
                    with W.Waterfall(width, B, element) as wf:
                        got = W.as_cells(wf.process(torch.from_numpy(x).cuda()), width)
                        last, have = wf.flush()
                    want = R.waterfall(x[:, :width], element, B)
                    R.check_cells(np.concatenate([got, last]), want, (element, width, pitch, B))
                    assert have == 2


@pytest.mark.parametrize("width", [1, 3, 8, 65])
def test_edges(torch, width):
    """every row count 0 .. 20, a 16-byte-aligned pointer and one an element past it, a dense pitch and one 3 longer,
    elements of 2^60 power in the pitch's gap and on both sides of the call (they would win every max), and 0xA5 guard
    bytes around `out`, which must be intact"""
    for element, layout in ROUTES:
        dt = R.NP_DTYPE[element]
        x = R.random_matrix(element, 20, width, seed=width)
        p = R.powers(x, element)
        for B in (1, 4, 7):
            with W.Waterfall(width, B, element, layout) as wf:
                for n in range(21):
                    for gap in (0, 3):
                        for off in (16, 17):
                            dense = width if layout == "rows" else n
                            pitch = dense + gap
                            outer, inner = (n, width) if layout == "rows" else (width, n)
                            need = (outer - 1) * pitch + inner if outer and inner else 0
                            flat = np.full(off + need + 16, BIG[element], dtype=dt)
                            m = x[:n] if layout == "rows" else x[:n].T
                            for i in range(outer if inner else 0):
                                flat[off + i * pitch: off + i * pitch + inner] = m[i]
                            d = torch.from_numpy(flat).cuda()
                            F = n // B
                            guard = torch.full((64 + F * width * 16 + 64,), 0xA5, dtype=torch.uint8, device="cuda")
                            wf.reset()
                            got = wf.process(d[off:off + need], out=guard[64:64 + F * width * 16], rows=n,
                                             ld=pitch if gap or layout == "rows" else 0)
                            last, have = wf.flush()
                            where = (element, layout, B, n, gap, off)
                            assert torch.all(guard[:64] == 0xA5) and torch.all(guard[64 + F * width * 16:] == 0xA5), where
                            R.check_cells(np.concatenate([W.as_cells(got, width), last]), R.cells_of(p[:n], B), where)
                            assert have == n % B


def planted(element, rows, width, pairs, value, seed):
    """a matrix of powers in (1e-4, 1) whose column c holds `value` in both rows of pairs[c % len(pairs)]"""
    x = R.random_matrix(element, rows, width, seed)
    x = (x / np.abs(x).max() * np.float32(0.9)).astype(R.NP_DTYPE[element])
    x[np.abs(x) < 0.02] = 0.02
    for c in range(width):
        r1, r2 = pairs[c % len(pairs)]
        x[r1, c] = x[r2, c] = value
    return x


@pytest.mark.parametrize("width", [3, 64, 130])
def test_ties(torch, width):
    """the same maximum twice per column, the two rows on either side of a lane group, a wave, a tile, a partial's
    lane in the fold and a call: the first row wins in every one; the same minimum twice gives that minimum"""
    for element, layout in ROUTES:
        T = W.row_tile(width, layout)
        B = 11 * T + 5
        if 2 * B * width > 4 * MAX_ELEMS:
            B = 3 * T + 5
        rows, cut = 2 * B, B + T + 7
        step = max(1, 256 // max(1, width // W.slot_columns(element)))     # about the rows one pass of a workgroup takes
        pairs = [(B + 0, B + 1), (B + 1, B + 1 + step), (B + 5, B + 5 + 64), (B + T - 1, B + T), (B + 3, B + 2 * T + 3),
                 (cut - 1, cut), (B + 2, 2 * B - 1)]
        if 11 * T + 5 == B:
            pairs.append((B + T + 1, B + 9 * T + 1))                       # partials 1 and 9: one fold lane, two rounds
        for value, field in ((3.0, "power_max"), (0.001, "power_min")):
            x = planted(element, rows, width, pairs, value, seed=width)
            want = R.waterfall(x, element, B)
            if field == "power_max":
                for c in range(width):
                    assert want["peak_row"][1, c] == pairs[c % len(pairs)][0] - B
            for cuts in ([0, rows], [0, cut, rows], [0, B - 1, cut - 1, cut, rows]):
                chunk = max(1, MAX_ELEMS // width)
                fine = sorted(set(cuts) | set(range(0, rows, chunk)))
                with W.Waterfall(width, B, element, layout) as wf:
                    got, _ = run_cuts(torch, wf, x, fine)
                R.check_cells(got, want, (element, layout, field, cuts))


@pytest.mark.parametrize("width,B", [(56, 700), (560, 500), (8, 5000)])
def test_cuttings(torch, width, B):
    """random cuttings of one matrix into 1 .. 40 calls: the selections are those of one call bit for bit, the mean is
    within 1 ulp; the same cutting twice gives the same bytes"""
    rng = np.random.default_rng(width)
    rows = min(5 * B + B // 3, MAX_ELEMS // width)
    for element, layout in ROUTES:
        x = R.random_matrix(element, rows, width, seed=B)
        want = R.waterfall(x, element, B)
        with W.Waterfall(width, B, element, layout) as wf:
            one, _ = run_cuts(torch, wf, x, [0, rows])
            R.check_cells(one, want, (element, layout, "one call"))
            for calls in (2, 7, 40):
                cuts = [0] + sorted(rng.integers(0, rows + 1, calls - 1).tolist()) + [rows]
                wf.reset()
                a, _ = run_cuts(torch, wf, x, cuts)
                wf.reset()
                b, _ = run_cuts(torch, wf, x, cuts)
                assert a.tobytes() == b.tobytes(), (element, layout, calls)
                assert R.same_selections(a, one), (element, layout, calls)
                R.check_cells(a, want, (element, layout, calls))


@pytest.mark.parametrize("width,B", [(7, 40), (130, 100), (1024, 300)])
def test_non_finite(torch, width, B):
    """one NaN and one inf in known (bin, column) cells: every other cell is exact and nothing faults.  The only test
    that leaves cells out: exactly the two planted ones."""
    rows = 3 * B + 5
    for element, layout in ROUTES:
        x = R.random_matrix(element, rows, width, seed=B)
        good = R.waterfall(x, element, B)
        x[B + 3, width // 2] = np.nan
        x[2 * B + 1, width - 1] = np.inf
        with W.Waterfall(width, B, element, layout) as wf:
            got, have = run_cuts(torch, wf, x, [0, B + 3, B + 4, rows])
        keep = np.ones(good.shape, bool)
        keep[1, width // 2] = keep[2, width - 1] = False
        assert have == 5 and got.shape == good.shape
        for k in ("power_max", "power_min", "peak_row"):
            assert np.array_equal(got[k][keep].view(np.uint32), good[k][keep].view(np.uint32)), (element, layout, k)
        assert R.ulps32(got["power_mean"][keep], good["power_mean"][keep]).max() <= 1


def test_host_pointers_and_argument_checks(torch):
    """host matrices, pageable and page-locked, dense and with a pitch, give the device's cells; what a call checks of
    its arguments once there is a handle; PFB_ERR_CAPACITY changes no state"""
    lib = L.load()
    for element in R.ELEMENTS:
        for width, B in ((56, 9), (130, 300)):
            rows = 4 * B + 7
            x = R.random_matrix(element, rows, width + 3, seed=B)
            dense = np.ascontiguousarray(x[:, :width])
            pinned = pinned_empty(dense.shape, dense.dtype)
            pinned[...] = dense
            want = R.waterfall(dense, element, B)
            with W.Waterfall(width, B, element) as wf:
                for src in (dense, pinned, x):
                    wf.reset()
                    got = wf.process(src[:2 * B + 1])
                    got = np.concatenate([got, wf.process(src[2 * B + 1:]), wf.flush()[0]])
                    R.check_cells(got, want, (element, width, src is x))
    with W.Waterfall(8, 4, "power") as wf, W.Waterfall(8, 4, "power", "columns") as wc:
        x = torch.from_numpy(R.random_matrix("power", 16, 8, seed=1)).cuda()
        out = torch.zeros(4 * 8 * 16 + 16, dtype=torch.uint8, device="cuda")
        u = C.c_uint64()
        px, po = x.data_ptr(), out.data_ptr()
        call = lambda h, *a: lib.pfb_wf_process(h._h, *a)                    # noqa: E731
        assert call(wf, px, 16, 7, po, 4, C.byref(u), L.PFB_MEM_DEVICE) == L.PFB_ERR_BAD_ARG      # ld < W
        assert call(wc, px, 2, 1, po, 4, C.byref(u), L.PFB_MEM_DEVICE) == L.PFB_ERR_BAD_ARG       # ld < rows
        assert call(wf, px, 16, 0, po, 4, C.byref(u), 2) == L.PFB_ERR_BAD_ARG                     # mem
        assert call(wf, px + 2, 15, 0, po, 4, C.byref(u), L.PFB_MEM_DEVICE) == L.PFB_ERR_BAD_ARG  # x off its element
        assert call(wf, px, 16, 0, po + 8, 4, C.byref(u), L.PFB_MEM_DEVICE) == L.PFB_ERR_BAD_ARG  # out off 16 bytes
        assert call(wf, None, 16, 0, po, 4, C.byref(u), L.PFB_MEM_DEVICE) == L.PFB_ERR_BAD_ARG
        assert call(wf, px, 16, 0, None, 4, C.byref(u), L.PFB_MEM_DEVICE) == L.PFB_ERR_BAD_ARG
        host = np.zeros((8, 16), np.float32)
        cells = np.zeros((4, 8), W.CELL_DTYPE)
        assert call(wc, host.ctypes.data, 16, 0, cells.ctypes.data, 4, C.byref(u), L.PFB_MEM_HOST) == L.PFB_ERR_BAD_ARG
        assert lib.pfb_wf_process_async(wf._h, px, 16, 7, po, 4, C.byref(u)) == L.PFB_ERR_BAD_ARG
        assert wf.bins_for(3) == 0 and wf.bins_for(4) == 1                   # none of them moved the handle
        # capacity: the number needed, and no state change
        wf.process(x[:3])
        assert call(wf, x[3:].data_ptr(), 13, 0, po, 2, C.byref(u), L.PFB_MEM_DEVICE) == L.PFB_ERR_CAPACITY and u.value == 4
        assert lib.pfb_wf_process_async(wf._h, x[3:].data_ptr(), 13, 0, po, 3, C.byref(u)) == L.PFB_ERR_CAPACITY and u.value == 4
        assert wf.bins_for(1) == 1 and wf.bins_for(0) == 0
        got = W.as_cells(wf.process(x[3:]), 8)
        R.check_cells(got, R.waterfall(x.cpu().numpy(), "power", 4), "after PFB_ERR_CAPACITY")
        assert wf.flush()[1] == 0


@pytest.mark.parametrize("layout", ["rows", "columns"])
def test_async_calls_with_a_stream_switch_and_a_growing_scratch(torch, layout):
    """calls enqueued without a sync between them, each longer than the last (the partials' scratch grows under calls
    still in flight), with the handle moved to another stream half way"""
    width, element = 130, "complex"
    B = 3 * W.row_tile(width, layout) + 11
    ns = [7, B // 2, B, 2 * B + 3, 3 * B + 1]
    ns = [min(n, MAX_ELEMS // width) for n in ns]
    x = R.random_matrix(element, sum(ns), width, seed=3)
    cuts = np.concatenate([[0], np.cumsum(ns)]).tolist()
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    with W.Waterfall(width, B, element, layout) as wf:
        pieces = [device_piece(torch, x[a:b], layout) for a, b in zip(cuts[:-1], cuts[1:])]
        torch.cuda.synchronize()
        outs = []
        wf.set_stream(streams[0].cuda_stream)
        for i, t in enumerate(pieces):
            if i == 3:
                wf.set_stream(streams[1].cuda_stream)
            outs.append(wf.process(t, sync=False))
        wf.sync()
        torch.cuda.synchronize()
        last, have = wf.flush()
        got = np.concatenate([W.as_cells(o, width) for o in outs] + [last])
        wf.set_stream(0)
    assert have == cuts[-1] % B
    R.check_cells(got, R.waterfall(x, element, B), layout)


# ---- records -------------------------------------------------------------------------------------------------

N_RECORD, PW, PRI, FIRST, F0 = 200003, 400, 50000, 12345, 7e6
MAX_ROWS, CHUNK = 40, 4101


@pytest.fixture(scope="module")
def record(torch, tmp_path_factory):
    path = os.path.join(tmp_path_factory.mktemp("wf"), "pulses.iq")
    with PulseTrain(pw=PW, pri=PRI, first_pulse=FIRST, f0=F0) as pt:
        pt.write_iq(path, N_RECORD, 0, file_format=3)
        fs = float(pt.config.fs)
    return path, fs


def check_pulse(img, column, frame_lo, frame_hi):
    """the first pulse shows in power_max at its (bin, column), and peak_row points at a frame inside it"""
    B = img.bin_rows
    bins = sorted({frame_lo // B, frame_hi // B})
    b = max(bins, key=lambda k: img.power_max[k, column])
    floor = np.median(img.power_max[:, column])
    assert img.power_max[b, column] > 50 * floor, (img.power_max[b, column], floor)
    assert frame_lo <= b * B + int(img.peak_row[b, column]) <= frame_hi
    assert int(np.argmax(img.power_max[b])) == column


@pytest.mark.parametrize("M", [8, 56])
def test_channelizer_records(torch, record, M):
    """the file route against Waterfall over the matrix process_iq_file returns: complex, magnitude and power output,
    with and without fftshift, frame-major and channel-major; selections exact (the channelizer gives the same bits
    under any cutting), the mean within 1 ulp; bin_rows, rows_in_last and both axes"""
    path, fs = record
    for kw in (dict(), dict(magnitude=True), dict(power=True), dict(fftshift=True), dict(power=True, fftshift=True)):
        for channel_major in (False, True):
            img = W.waterfall_from_iq_file(path, M, max_rows=MAX_ROWS, chunk_samples=CHUNK, channel_major=channel_major, **kw)
            with Channelizer(M, channel_major=channel_major, **kw) as ch:
                y, info = ch.process_iq_file(path)
                D = ch.decimation
            element = "power" if kw.get("power") else "magnitude" if kw.get("magnitude") else "complex"
            frames = y.shape[1] if channel_major else y.shape[0]
            B = W.choose_bin(frames, MAX_ROWS)
            cells, last = W.waterfall(torch.from_numpy(y).cuda(), B, element=element,
                                      layout="columns" if channel_major else "rows")
            where = (M, kw, channel_major)
            assert img.bin_rows == B and img.rows_in_last == last == (frames % B or B), where
            got = np.zeros(cells.shape, W.CELL_DTYPE)
            for k in W.CELL_DTYPE.names:
                got[k] = getattr(img, k)
            R.check_cells(got, cells, where)
            R.check_cells(got, R.waterfall(y.T if channel_major else y, element, B), where)
            order = "centered" if kw.get("fftshift") else "fft"
            assert np.array_equal(img.f, center_frequencies(M, fs, order))
            assert np.array_equal(img.t, np.arange(cells.shape[0]) * (B * D) / fs)
            assert int(info.packet.numSamples) == N_RECORD == int(img.info.packet.numSamples)
            column = int(np.argmin(np.abs(img.f - F0)))
            check_pulse(img, column, FIRST // D, (FIRST + PW + M * 12) // D + 1)


@pytest.mark.parametrize("output", ["power", "complex"])
def test_stft_records(torch, record, output):
    path, fs = record
    nfft = 768
    img = W.waterfall_from_iq_file(path, stft_window=np.hamming(nfft), max_rows=MAX_ROWS, chunk_samples=CHUNK, output=output)
    with Stft(np.hamming(nfft), sample_format="int16", bit_width=12, output=output) as st:
        y, _ = st.process_iq_file(path)
    frames = y.shape[0]
    B = W.choose_bin(frames, MAX_ROWS)
    cells, last = W.waterfall(torch.from_numpy(y).cuda(), B)
    assert img.bin_rows == B and img.rows_in_last == last == (frames % B or B) and frames == N_RECORD // nfft
    got = np.zeros(cells.shape, W.CELL_DTYPE)
    for k in W.CELL_DTYPE.names:
        got[k] = getattr(img, k)
    R.check_cells(got, cells, output)
    R.check_cells(got, R.waterfall(y, "complex" if output == "complex" else "power", B), output)
    f, t = stft_axes(nfft, nfft, nfft, fs, "centered", 0, frames)
    assert np.array_equal(img.f, f) and np.array_equal(img.t, t[::B])
    column = int(np.argmin(np.abs(f - F0)))
    check_pulse(img, column, FIRST // nfft, (FIRST + PW) // nfft)
    with Stft(np.hamming(nfft), sample_format="int16", bit_width=12, output="db") as st:
        u, b = C.c_uint64(), C.c_uint32()
        out = np.zeros((MAX_ROWS, nfft), W.CELL_DTYPE)
        assert L.load().pfb_wf_from_stft_iq_file(st._h, path.encode(), MAX_ROWS, 0, out.ctypes.data, MAX_ROWS, C.byref(u),
                                                 C.byref(b), None) == L.PFB_ERR_BAD_ARG
