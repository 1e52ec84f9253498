"""The pulse-train source on the MI355X, bit for bit against the numpy yardstick (synth_ref): no tolerances anywhere.
The yardstick gets its cos table from pfb_synth_describe, so that a libm difference cannot pass for a kernel fault (the
table itself is pinned by test_synth_cpu.py)."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import synth_ref as R
from gpu_support import cuda_torch
from sdr_channelizer_amd import _lib as L
from sdr_channelizer_amd import iqfile, pulse_source, synth
from sdr_channelizer_amd import Channelizer, PulseTrain, design_prototype

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FORMATS = [("int16", 12), ("int8", 8), ("int16", 16)]
STARTS = (0, 123457, 2 ** 32 - 1000, 2 ** 40 + 7)   # 2^32 - 1000: the hash's high word changes inside the call
EDGE = dict(pw=13, pri=37, first_pulse=5)            # period wraps and pulse edges inside single lanes' vectors


@pytest.fixture(scope="module")
def torch():
    return cuda_torch()


def reference(kw, start, n):
    """Samples start .. start + n - 1 of the stream PulseTrain(**kw) makes, by the yardstick."""
    cfg = pulse_source._config(**kw)
    d = R.derive(cfg.pulse_samples, cfg.period_samples, cfg.fs, cfg.f0, cfg.bit_width, cfg.flags, cfg.lfm_extent_hz,
                 cfg.amplitude, cfg.noise_sigma)
    _, tab = pulse_source.synth_params(table=True, **kw)
    return R.stream(start, n, d, tab, cfg.seed, cfg.bit_width, kw.get("sample_format", "int16"), cfg.first_pulse,
                    cfg.record_samples, cfg.flags)


@pytest.mark.parametrize("fmt,bw", FORMATS)
def test_default_stream(torch, fmt, bw):
    n = 200000
    with PulseTrain(sample_format=fmt, bit_width=bw) as pt:
        for start in STARTS:
            got = pt.generate(n, start).cpu().numpy()
            assert np.array_equal(got, reference(dict(sample_format=fmt, bit_width=bw), start, n)), start
            assert np.array_equal(got, synth.pulsed_iq_counter_numpy(n, bw, got.dtype, start=start)), start


@pytest.mark.parametrize("fmt,bw", [("int16", 12), ("int8", 8), ("cf32", 12)])
def test_vector_edges(torch, fmt, bw):
    """Every n from 0 to 70 at every start from 0 to 9, into a 16-byte aligned pointer and into one a sample past it:
    the scalar head and tail, and nothing written outside [out, out + n)."""
    kw = dict(sample_format=fmt, bit_width=bw, **EDGE)
    want = reference(kw, 0, 80)
    row = 80                                  # samples per row: 160, 320 or 640 bytes, every row base 16-byte aligned
    cases = [(n, start, off) for n in range(71) for start in range(10) for off in (0, 1)]
    guard = 77 if fmt != "cf32" else 77.0
    with PulseTrain(**kw) as pt:
        buf = pt.generate(len(cases) * row, 0)  # the right dtype and device
        assert buf.data_ptr() % 16 == 0
        buf.fill_(guard)
        rows = buf.view(len(cases), row, 2)
        for r, (n, start, off) in enumerate(cases):
            pt.generate(n, start, out=rows[r, off:off + n], sync=False)
        pt.sync()
        got = rows.cpu().numpy()
    for r, (n, start, off) in enumerate(cases):
        assert np.array_equal(got[r, off:off + n], want[start:start + n]), (n, start, off)
        assert np.all(got[r, :off] == guard) and np.all(got[r, off + n:] == guard), (n, start, off)


def pulses(iq, pri, first=0):
    """pulses in a noise-free record: its samples are zero exactly where the train is off"""
    on = np.any(iq != 0, axis=1)
    starts = on[first::pri]
    assert on.sum() % max(int(starts.sum()), 1) == 0
    return int(starts.sum())


@pytest.mark.parametrize("pw,pri,record,count", [(13, 37, 3 * 37 + 14, 3), (13, 37, 3 * 37 + 15, 4),
                                                 (5600, 56000, 560000, 10)])
def test_record_rule(torch, pw, pri, record, count):
    """Only pulses that fit the record: (idx + numSamplesForPw) < length(mag) with the script's 1-based idx."""
    kw = dict(pw=pw, pri=pri, record_samples=record, noise_sigma=0.0)
    got = pulse_source.pulse_train(record, **kw).cpu().numpy()
    assert np.array_equal(got, reference(kw, 0, record))
    assert pulses(got, pri) == count


SWITCHES = {
    "lfm_up": dict(lfm_extent_hz=5e6),
    "lfm_down_from_zero": dict(lfm_extent_hz=-3e6, phase_from_zero=True),
    "barker_quirk": dict(barker13=True),
    "barker_degrees_lfm": dict(barker13=True, barker_degrees=True, lfm_extent_hz=5e6),
    "cf32": dict(sample_format="cf32"),
    "cf32_barker_lfm_16": dict(sample_format="cf32", bit_width=16, barker13=True, lfm_extent_hz=-3e6),
    "full_scale_16": dict(bit_width=16, amplitude=1.0),
    "full_scale_8": dict(sample_format="int8", bit_width=8, amplitude=1.0, lfm_extent_hz=5e6),
    "noise_free": dict(noise_sigma=0.0, barker13=True),
    "matlab_rounding_first_record": dict(round_matlab=True, first_pulse=60001, record_samples=150000, seed=7, f0=-13.37e6),
    "int8_narrow": dict(sample_format="int8", bit_width=2, amplitude=2.0, noise_sigma=1.0),
}


@pytest.mark.parametrize("name", SWITCHES)
def test_switches(torch, name):
    kw, start, n = SWITCHES[name], 50001, 130003   # the pulses at 56000, 112000 and 168000, odd start and length
    got = pulse_source.pulse_train(n, start, **kw).cpu().numpy()
    want = reference(kw, start, n)
    assert got.dtype == want.dtype and np.array_equal(got, want)
    if name.startswith("barker") or name == "noise_free":
        assert pulse_source.synth_params(**kw).pulse_samples == 5603   # 5600 -> 13 chips of 431
    if name == "full_scale_16":
        assert got.max() == 32767 and got.min() == -32768
    if name == "full_scale_8":
        assert got.max() == 127 and got.min() == -128
    if name == "noise_free":
        assert pulses(got[56000 - start:], 56000) == 3 and np.count_nonzero(np.any(got != 0, axis=1)) == 3 * 5603


def test_rounding(torch):
    """I alternates between the exact ties +100.5 and -100.5: half up gives +101 / -100, MATLAB's int16() +101 / -101."""
    kw = dict(bit_width=12, amplitude=100.5 / 2048, f0=synth.FS / 2, phase_from_zero=True, noise_sigma=0.0, pw=13, pri=37)
    up = pulse_source.pulse_train(74, **kw).cpu().numpy()
    away = pulse_source.pulse_train(74, round_matlab=True, **kw).cpu().numpy()
    assert np.array_equal(up, reference(kw, 0, 74)) and np.array_equal(away, reference(dict(round_matlab=True, **kw), 0, 74))
    tie = np.array([101, -100] * 6 + [101])
    assert np.array_equal(up[:13, 0], tie) and np.array_equal(up[37:50, 0], tie) and not up[13:37].any()
    assert np.array_equal(away[:13, 0], np.where(tie < 0, -101, tie)) and not away[:, 1].any()
    assert not np.array_equal(up, away)


def test_grid_stride(torch):
    """One call in which every workgroup of the capped grid (8 per CU) takes more than one step."""
    with PulseTrain(sample_format="int8", bit_width=8) as pt:
        cus = torch.cuda.get_device_properties(pt.device_index).multi_processor_count
        n = min(2 * (8 * cus * 256 * 8) + (1 << 20) + 3, (1 << 24) + 3)   # two whole steps of 8-sample vectors and a bit
        got = pt.generate(n, 2 ** 32 - 12345).cpu().numpy()
    assert np.array_equal(got, reference(dict(sample_format="int8", bit_width=8), 2 ** 32 - 12345, n))


def test_any_cutting_gives_the_same_bits(torch):
    kw = dict(pw=1000, pri=4321, first_pulse=777, record_samples=250000, lfm_extent_hz=5e6, barker13=True, seed=99,
              f0=7.25e6)
    a, b = 2 ** 32 - 150000, 2 ** 32 + 150001
    kw["first_pulse"] += a - 100000
    kw["record_samples"] += a
    want = reference(kw, a, b - a)
    with PulseTrain(**kw) as pt:
        whole = pt.generate(b - a, a)
        assert np.array_equal(whole.cpu().numpy(), want)
        pieces = torch.empty_like(whole)
        at, sizes, i = a, (1, 7, 4099, 33, 65537, 2, 12345), 0
        while at < b:
            m = min(sizes[i % len(sizes)], b - at)
            pt.generate(m, at, out=pieces[at - a:at - a + m], sync=False)
            at, i = at + m, i + 1
        pt.sync()
        assert torch.equal(pieces, whole)
        # the host route (page-locked chunks), and the async route on a side stream
        assert np.array_equal(pt.generate(b - a, a, device=False), want)
        side = torch.cuda.Stream()
        pt.set_stream(side.cuda_stream)
        out = torch.zeros_like(whole)
        pt.generate(b - a, a, out=out, sync=False)
        pt.sync()
        assert torch.equal(out, whole)
        pt.set_stream(0)
    # a host call longer than one chunk of 2^22 samples: the double buffering turns over
    with PulseTrain() as pt:
        n = (1 << 23) + 4097
        got = pt.generate(n, 5, device=False)
        assert np.array_equal(got, pt.generate(n, 5).cpu().numpy())
        assert np.array_equal(got[-300000:], reference({}, 5 + n - 300000, 300000))


def test_generate_validates_arguments(torch):
    lib = L.load()
    with PulseTrain() as pt, PulseTrain(sample_format="cf32") as pf, PulseTrain(sample_format="int8", bit_width=8) as p8:
        buf = torch.zeros((16, 2), dtype=torch.int16, device="cuda")
        ptr = C.c_void_p(buf.data_ptr())
        assert lib.pfb_synth_generate(pt._h, 2 ** 64 - 4, 8, ptr, L.PFB_MEM_DEVICE) == L.PFB_ERR_BAD_ARG   # start + n overflows
        assert lib.pfb_synth_generate_async(pt._h, 2 ** 64 - 4, 8, ptr) == L.PFB_ERR_BAD_ARG
        assert lib.pfb_synth_generate(pt._h, 0, 8, None, L.PFB_MEM_DEVICE) == L.PFB_ERR_BAD_ARG
        assert lib.pfb_synth_generate(pt._h, 0, 8, ptr, 2) == L.PFB_ERR_BAD_ARG
        assert lib.pfb_synth_generate(pt._h, 0, 8, C.c_void_p(buf.data_ptr() + 2), L.PFB_MEM_DEVICE) == L.PFB_ERR_BAD_ARG
        assert lib.pfb_synth_generate(pt._h, 2 ** 64 - 9, 8, ptr, L.PFB_MEM_DEVICE) == L.PFB_OK   # the last samples one can ask for
        assert not buf[8:].any()
        assert lib.pfb_synth_write_iq_file(pf._h, b"never.iq", 3, 0, 8, None) == L.PFB_ERR_BAD_FORMAT   # cf32 has no record
        assert lib.pfb_synth_write_iq_file(p8._h, b"never.iq", 1, 0, 8, None) == L.PFB_ERR_BAD_FORMAT   # the script writes 16-bit
        assert lib.pfb_synth_write_iq_file(pt._h, b"never.iq", 2, 0, 8, None) == L.PFB_ERR_BAD_ARG
        assert lib.pfb_synth_write_iq_file(pt._h, None, 1, 0, 8, None) == L.PFB_ERR_BAD_ARG
        assert not os.path.exists("never.iq")


def test_records(torch, tmp_path):
    n, start = 300001, 4242
    one, three, eight = (os.path.join(tmp_path, f) for f in ("one.iq", "three.iq", "eight.iq"))
    # format 1, as generate_training_iq.m writes it: 16 bits, phase from zero, int16() rounding
    kw = dict(bit_width=16, amplitude=1.0, noise_sigma=0.0, phase_from_zero=True, round_matlab=True, pw=3000, pri=20000,
              first_pulse=1234, record_samples=start + n)
    want = reference(kw, start, n)
    with PulseTrain(**kw) as pt:
        pt.write_iq(one, n, start)
        dev = pt.generate(n, start)
    rec = iqfile.read_iq(one)
    assert np.array_equal(rec.iq, want)
    assert (rec.fileFormat, rec.fs, rec.bw, rec.fc, rec.gain, rec.bitWidth, rec.linkSpeed, rec.boardName, rec.sampleStartTime) \
        == (1, 56e6, 56e6, 0.0, 0.0, 16, 1, "simulated", 0.0)
    by_python = os.path.join(tmp_path, "one_py.iq")
    iqfile.write_iq_fmt1(by_python, want, 56e6)
    assert open(one, "rb").read() == open(by_python, "rb").read()
    # format 3 with the caller's header fields, 12 bits
    pk = L.PfbIqPacket()
    L.load().pfb_iq_fill_packet(C.byref(pk), 0, 915000000, 40000000, 56000000, 31.5, 0, 0, b"bladeRF", b"f00d", 1.7e9)
    with PulseTrain() as pt:
        pt.write_iq(three, n, start, file_format=3, header=pk)
    rec = iqfile.read_iq(three)
    assert np.array_equal(rec.iq, reference({}, start, n))
    assert (rec.fileFormat, rec.fs, rec.bw, rec.fc, rec.bitWidth, rec.boardName, rec.serialNo, rec.sampleStartTime) \
        == (3, 56e6, 40e6, 915e6, 12, "bladeRF", "f00d", 1.7e9) and abs(rec.gain - 31.5) == 0
    # format 3 from an int8 handle, default fields = iqfile.write_iq's
    kw8 = dict(sample_format="int8", bit_width=8)
    with PulseTrain(**kw8) as pt:
        pt.write_iq(eight, 70001, start, file_format=3)
    by_python = os.path.join(tmp_path, "eight_py.iq")
    iqfile.write_iq(by_python, reference(kw8, start, 70001), 56e6, 0.0, 8)
    assert open(eight, "rb").read() == open(by_python, "rb").read()
    # the generated tensor is the recorders' buffer: an existing channelizer takes it as it takes the reference array
    taps = design_prototype(64, 12)
    with Channelizer(64, taps=taps, sample_format="int16", bit_width=16) as ch:
        y_dev = ch(dev).cpu().numpy()
    with Channelizer(64, taps=taps, sample_format="int16", bit_width=16) as ch:
        y_ref = ch(torch.from_numpy(want).cuda()).cpu().numpy()
    assert y_dev.shape[0] == n // 64 and np.array_equal(y_dev, y_ref)


def test_cpp_host_makes_records_without_python(torch, tmp_path):
    """examples/synth_record.cpp built with g++ and run as its own process: its records parse, and their payloads are
    the yardstick's for the parameters it reports."""
    from sdr_channelizer_amd import LIB_PATH
    cxx = shutil.which("g++") or shutil.which("hipcc")
    if cxx is None:
        pytest.skip("no C++ compiler on this box")
    exe = os.path.join(tmp_path, "synth_record")
    libdir = os.path.dirname(LIB_PATH)
    subprocess.run([cxx, "-std=c++17", "-O1", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "synth_record.cpp"),
                    "-o", exe, "-L" + libdir, "-lpfb_channelizer", "-Wl,-rpath," + libdir], check=True)
    out = subprocess.run([exe, "12345", str(tmp_path), "0.02"], check=True, capture_output=True, text=True, timeout=120).stdout
    seen = 0
    for line in out.splitlines():
        m = re.match(r"(training|pulsed) (\S+) (.*)", line)
        if not m:
            continue
        f = {k: (int(v) if re.fullmatch(r"-?\d+", v) else float(v) if k in ("f0", "lfm") else v)
             for k, v in (t.split("=") for t in m.group(3).split())}
        assert f["board"] == "simulated" and f["format"] == (1 if m.group(1) == "training" else 3)
        kw = dict(bit_width=16, amplitude=1.0, noise_sigma=0.0, f0=f["f0"], pw=f["pw"], pri=f["pri"], first_pulse=f["first"],
                  record_samples=f["n"], lfm_extent_hz=f["lfm"], barker13=bool(f["barker"]),
                  phase_from_zero=m.group(1) == "training", round_matlab=True)
        rec = iqfile.read_iq(m.group(2))
        assert rec.fileFormat == (1 if m.group(1) == "training" else 3) and rec.bitWidth == 16 and rec.fs == 56e6
        assert rec.iq.shape[0] == f["n"] == f["read_back"] and np.array_equal(rec.iq, reference(kw, 0, f["n"]))
        assert pulses(rec.iq, f["pri"], f["first"]) == f["pulses"] > 0
        seen += 1
    assert seen == 2, out
