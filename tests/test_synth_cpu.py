"""The pulse-train source without a GPU: the numpy yardstick (synth_ref) against the streams and phases synth.py already
defines, what pfb_synth_describe derives against the yardstick, argument validation, and the record header writer."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import synth_ref as R
from sdr_channelizer_amd import _lib as L
from sdr_channelizer_amd import iqfile, pulse_source, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STARTS = (0, 123457, 2 ** 32 - 1000, 2 ** 40 + 7)
PW, PRI = 5600, 56000


def default_derive(bit_width, **kw):
    return R.derive(PW, PRI, synth.FS, synth._carrier(synth.SEED, synth.FS), bit_width, **kw)


@pytest.mark.parametrize("fmt,bw", [("int16", 12), ("int8", 8), ("int16", 16)])
@pytest.mark.parametrize("start", STARTS)
def test_ref_default_is_the_counter_stream(fmt, bw, start):
    n = 200000
    got = R.stream(start, n, default_derive(bw), R.cos_table(bw), synth.SEED, bw, fmt)
    want = synth.pulsed_iq_counter_numpy(n, bw, np.int8 if fmt == "int8" else np.int16, start=start)
    assert got.dtype == want.dtype and np.array_equal(got, want)


@pytest.mark.parametrize("lfm,flags", [(5e6, 0), (-3e6, 0), (0.0, R.BARKER13), (0.0, R.BARKER13 | R.BARKER_DEGREES),
                                       (5e6, R.BARKER13)])
def test_ref_phase_agrees_with_pulse_phase(lfm, flags):
    fs, f0 = synth.FS, synth._carrier(synth.SEED, synth.FS)
    d = R.derive(PW, PRI, fs, f0, 12, flags, lfm_extent_hz=lfm)
    on, ph, k = R.on_and_phase(0, 2 * PRI, d, flags=flags)
    assert on.sum() == 2 * d["pw"]
    want = synth.pulse_phase(k[on].astype(np.int64), f0, fs, d["pw"], lfm, bool(flags & R.BARKER13),
                             matlab_quirks=not flags & R.BARKER_DEGREES)
    diff = ph[on].astype(np.float64) * (2.0 * np.pi / 2.0 ** 32) - want
    diff = np.abs((diff + np.pi) % (2.0 * np.pi) - np.pi)
    assert diff.max() < 1e-5, diff.max()


CASES = {
    "default": dict(),
    "negative_f0": dict(f0=-13.37e6),
    "negative_lfm": dict(lfm_extent_hz=-3e6),
    "barker": dict(barker13=True),
    "barker_degrees_lfm": dict(barker13=True, barker_degrees=True, lfm_extent_hz=5e6),
    "pw1": dict(pw=1, pri=7, lfm_extent_hz=5e6),
}


@pytest.mark.parametrize("name", CASES)
def test_describe_matches_the_yardstick(name):
    kw = dict(CASES[name])
    got = pulse_source.synth_params(**kw)
    flags = (R.BARKER13 if kw.get("barker13") else 0) | (R.BARKER_DEGREES if kw.get("barker_degrees") else 0)
    f0 = kw.get("f0", synth._carrier(synth.SEED, synth.FS))
    d = R.derive(kw.get("pw", PW), kw.get("pri", PRI), synth.FS, f0, 12, flags, lfm_extent_hz=kw.get("lfm_extent_hz", 0.0))
    assert (got.pulse_samples, got.chip_samples, got.fcw, got.dcw, got.noise_gain, got.barker_offset) == \
        (d["pw"], d["chip"], d["fcw"], d["dcw"], d["gain"], d["off"])
    if name == "barker":
        assert got.pulse_samples == 5603 and got.chip_samples == 431
    if name == "pw1":
        assert got.dcw == 0
    if name == "negative_lfm":
        assert got.dcw > 2 ** 63   # two's complement


@pytest.mark.parametrize("bw", [8, 12, 16])
def test_describe_table_is_the_cos_table(bw):
    _, tab = pulse_source.synth_params(table=True, bit_width=bw, sample_format="int16")
    assert np.array_equal(tab, synth._cos_table(bw)) and np.array_equal(tab, R.cos_table(bw))


def test_arguments_are_validated_before_the_device():
    lib = L.load()
    out, h = L.PfbSynthParams(), C.c_void_p()

    def both(want, **kw):
        cfg = pulse_source._config(**{"pw": PW, "pri": PRI, **kw})   # in samples: nothing to derive from a bad fs
        assert lib.pfb_synth_describe(C.byref(cfg), C.byref(out), None) == want, kw
        assert lib.pfb_synth_create(C.byref(cfg), C.byref(h)) == want and not h, kw

    assert lib.pfb_synth_describe(None, C.byref(out), None) == L.PFB_ERR_BAD_ARG
    assert lib.pfb_synth_describe(C.byref(pulse_source._config()), None, None) == L.PFB_ERR_BAD_ARG
    assert lib.pfb_synth_create(None, C.byref(h)) == L.PFB_ERR_BAD_ARG
    assert lib.pfb_synth_create(C.byref(pulse_source._config()), None) == L.PFB_ERR_BAD_ARG
    cfg = pulse_source._config()
    cfg.struct_size = 8
    assert lib.pfb_synth_describe(C.byref(cfg), C.byref(out), None) == L.PFB_ERR_BAD_ARG
    assert lib.pfb_synth_create(C.byref(cfg), C.byref(h)) == L.PFB_ERR_BAD_ARG
    for kw in (dict(pw=0), dict(pw=8, pri=7), dict(pw=5, pri=2 ** 31), dict(amplitude=2.5), dict(amplitude=-0.1),
               dict(noise_sigma=1.5), dict(noise_sigma=-1e-3), dict(fs=float("nan")), dict(fs=0.0),
               dict(f0=float("inf")), dict(lfm_extent_hz=float("nan")), dict(amplitude=float("nan")),
               dict(noise_sigma=float("inf")), dict(barker_degrees=True), dict(lfm_extent_hz=0.6 * synth.FS * (PW - 1)),
               dict(pw=60, pri=64, barker13=True)):   # 60 -> 65 chips' worth of samples, past the period
        both(L.PFB_ERR_BAD_ARG, **kw)
    cfg = pulse_source._config()
    cfg.flags = 16
    assert lib.pfb_synth_describe(C.byref(cfg), C.byref(out), None) == L.PFB_ERR_BAD_ARG
    for kw in (dict(sample_format="int8", bit_width=9), dict(sample_format="int8", bit_width=1), dict(bit_width=17),
               dict(bit_width=1), dict(sample_format="cf32", bit_width=17), dict(sample_format="cf32", bit_width=0)):
        both(L.PFB_ERR_BAD_FORMAT, **kw)
    cfg = pulse_source._config()
    cfg.sample_format = 7
    assert lib.pfb_synth_describe(C.byref(cfg), C.byref(out), None) == L.PFB_ERR_BAD_FORMAT
    # every other entry point refuses a null handle
    dev = C.c_int()
    assert lib.pfb_synth_destroy(None) == lib.pfb_synth_set_stream(None, None) == lib.pfb_synth_sync(None) == L.PFB_ERR_BAD_ARG
    assert lib.pfb_synth_generate(None, 0, 0, None, 0) == lib.pfb_synth_generate_async(None, 0, 0, None) == L.PFB_ERR_BAD_ARG
    assert lib.pfb_synth_get_device(None, C.byref(dev)) == L.PFB_ERR_BAD_ARG
    assert lib.pfb_synth_write_iq_file(None, b"x.iq", 1, 0, 0, None) == L.PFB_ERR_BAD_ARG
    # a valid configuration: a handle where there is a device, PFB_ERR_NO_DEVICE (never a CPU fallback) where there is none
    rc = lib.pfb_synth_create(C.byref(pulse_source._config()), C.byref(h))
    if lib.pfb_device_count() > 0:
        assert rc == L.PFB_OK and lib.pfb_synth_destroy(h) == L.PFB_OK
    else:
        assert rc == L.PFB_ERR_NO_DEVICE and not h
        with pytest.raises(L.PfbError) as e:
            pulse_source.PulseTrain()
        assert e.value.status == L.PFB_ERR_NO_DEVICE


def serialize(pk, fmt, capacity=128):
    buf = C.create_string_buffer(capacity)
    n = C.c_size_t()
    rc = L.load().pfb_iq_serialize_header(C.byref(pk), fmt, buf, capacity, C.byref(n))
    return rc, buf.raw[: n.value]


def test_serialize_header(tmp_path):
    lib = L.load()
    iq = np.arange(20, dtype=np.int16).reshape(-1, 2)
    # format 1: what generate_training_iq.m writes by hand = iqfile.write_iq_fmt1's header
    path = os.path.join(tmp_path, "one.iq")
    iqfile.write_iq_fmt1(path, iq, 56e6, start_time=1.5e9)
    want = open(path, "rb").read()[:104]
    pk = L.PfbIqPacket()
    lib.pfb_iq_fill_packet(C.byref(pk), 0x03030303, 0, 56000000, 56000000, 0.0, 10, 16, b"simulated", None, 1.5e9)
    pk.linkSpeed = 1
    rc, got = serialize(pk, 1)
    assert rc == L.PFB_OK and got == want
    info = iqfile.parse_header(got)
    assert (info.file_format, info.header_bytes, info.packet.numSamples, info.packet.bitWidth) == (1, 104, 10, 16)
    assert info.packet.sampleStartTime == 1.5e9 and info.packet.boardName == b"simulated" and info.packet.linkSpeed == 1
    # format 3: the struct as the recorders write it
    lib.pfb_iq_fill_packet(C.byref(pk), 0x03030303, 915000000, 56000000, 56000000, 31.5, 10, 12, b"bladeRF", b"abc", 2.25)
    rc, got = serialize(pk, 3)
    assert rc == L.PFB_OK and got == bytes(pk)
    info = iqfile.parse_header(got)
    assert bytes(info.packet) == bytes(pk) and info.file_format == 3
    # format 2 stores the gain as the integer the reader takes it for
    pk.rxGainDb = 31.0
    rc, got = serialize(pk, 2)
    info = iqfile.parse_header(got)
    assert rc == L.PFB_OK and len(got) == 112 and info.file_format == 2 and info.rx_gain_as_read == 31.0
    assert info.packet.frequencyHz == 915000000
    # short buffers, unknown formats, values the narrower words cannot hold
    for fmt, cap in ((1, 103), (3, 111), (0, 128), (4, 128)):
        assert serialize(pk, fmt, cap)[0] == L.PFB_ERR_BAD_ARG
    buf = C.create_string_buffer(128)
    assert lib.pfb_iq_serialize_header(None, 3, buf, 128, None) == L.PFB_ERR_BAD_ARG
    assert lib.pfb_iq_serialize_header(C.byref(pk), 3, None, 128, None) == L.PFB_ERR_BAD_ARG
    assert lib.pfb_iq_serialize_header(C.byref(pk), 3, buf, 128, None) == L.PFB_OK   # `written` is optional
    pk.frequencyHz = 2 ** 32
    assert serialize(pk, 1)[0] == L.PFB_ERR_BAD_ARG and serialize(pk, 2)[0] == L.PFB_OK
    pk.frequencyHz, pk.rxGainDb = 0, -1.0
    assert serialize(pk, 1)[0] == L.PFB_ERR_BAD_ARG and serialize(pk, 3)[0] == L.PFB_OK


def test_synth_entry_points_sit_under_the_abi_guard():
    """As test_nothing_thrown_crosses_the_c_abi does for pfb_pdw.hip: every extern "C" definition of the unit."""
    src = open(os.path.join(ROOT, "sdr_channelizer_amd", "csrc", "pfb_synth.hip")).read()
    found = {}
    for m in re.finditer(r'^extern "C" int (\w+)\(', src, re.M):
        rest = src[m.start():]
        found[m.group(1)] = rest[: rest.index("\n}\n")]
    assert set(found) == {n for n in L.EXPORTS if n.startswith("pfb_synth_")} and len(found) == 9
    for name, body in found.items():
        assert "abi_guard" in body.split("{", 1)[1][:80], name
    assert src.count('extern "C"') == len(found)
