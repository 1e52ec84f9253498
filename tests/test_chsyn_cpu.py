"""The channel synthesizer without a GPU: the numpy restatement against the definition written out, its index
arithmetic against the channelizer's own options, the reconstruction facts the header quotes, and the host side of the
C ABI (argument checks in their documented order, plans, struct sizes, exports)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import chsyn_ref as R
from abi_symbols import declared_symbols
from oracle.pfb_oracle import OracleConfig, channelize_numpy
from sdr_channelizer_amd import _lib as L
from sdr_channelizer_amd import synthesizer as sy

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHSYN_EXPORTS = {"pfb_chsyn_describe", "pfb_chsyn_create", "pfb_chsyn_destroy", "pfb_chsyn_reset",
                 "pfb_chsyn_set_stream", "pfb_chsyn_sync", "pfb_chsyn_get_device", "pfb_chsyn_set_frame_index",
                 "pfb_chsyn_get_frame_index", "pfb_chsyn_samples_for", "pfb_chsyn_set_weights", "pfb_chsyn_process",
                 "pfb_chsyn_process_async", "pfb_chsyn_last_kernel"}
FUSED_M = (56, 64, 128, 256)
MIB64 = 64 << 20


def crandn(rng, *shape):
    return rng.standard_normal(shape) + 1j * rng.standard_normal(shape)


# -- the restatement ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("M", [2, 3, 8, 12])
def test_restatement_equals_the_literal_double_sum(M):
    rng = np.random.default_rng(M)
    for D in ([M] if M % 2 else [M, M // 2]):
        for flags in (0, R.FFTSHIFT, R.DEROTATE, R.FFTSHIFT | R.DEROTATE):
            for weights in (None, rng.standard_normal(M)):
                y, g = crandn(rng, 7, M), rng.standard_normal(3 * M)
                for frame0 in (0, 5):
                    a = R.synthesize(y, g, M, D, flags=flags, weights=weights, frame0=frame0)
                    b = R.synthesize_literal(y, g, M, D, flags=flags, weights=weights, frame0=frame0)
                    assert a.shape == (7 * D,) and np.abs(a - b).max() < 1e-12 * np.abs(b).max()
                    f32 = R.synthesize_f32(y, g, M, D, flags=flags, weights=weights, frame0=frame0)
                    assert f32.dtype == np.complex64 and np.abs(f32 - b).max() < 1e-5 * np.abs(b).max()


def test_restatement_streams():
    """history in, history out: any cutting of the frames gives the same samples"""
    rng = np.random.default_rng(1)
    M, D = 8, 4
    y, g = crandn(rng, 20, M), rng.standard_normal(3 * M)
    whole = R.synthesize(y, g, M, D)
    hist, parts = None, []
    for a, b in ((0, 1), (1, 1), (1, 3), (3, 12), (12, 20)):
        x, hist = R.synthesize(y[a:b], g, M, D, history=hist, return_history=True)
        parts.append(x)
    assert np.array_equal(np.concatenate(parts), whole)


@pytest.mark.parametrize("M,D", [(8, 8), (8, 4), (12, 6), (5, 5), (56, 28)])
def test_flags_undo_the_channelizers_options(oracle, M, D):
    """Synthesizing shifted or derotated analysis output with the flag set equals synthesizing the plain output."""
    rng = np.random.default_rng(M + D)
    h = oracle.design_prototype(M, 4)
    g = rng.standard_normal(2 * M)
    x = crandn(rng, D * 40)
    plain = R.synthesize(channelize_numpy(x, h, OracleConfig(M, 4, D)), g, M, D)
    for fftshift in (False, True):
        for derotate in (False, True):
            y = channelize_numpy(x, h, OracleConfig(M, 4, D, fftshift=fftshift, derotate=derotate))
            flags = (R.FFTSHIFT if fftshift else 0) | (R.DEROTATE if derotate else 0)
            got = R.synthesize(y, g, M, D, flags=flags)
            assert np.abs(got - plain).max() < 1e-12 * np.abs(plain).max(), (fftshift, derotate)
            if flags and not (D == M and flags == R.DEROTATE):  # without the flag it is another signal
                assert np.abs(R.synthesize(y, g, M, D) - plain).max() > 1e-3 * np.abs(plain).max()
    # a stream that starts at frame 7: the derotation index is the absolute one
    y = channelize_numpy(x, h, OracleConfig(M, 4, D, derotate=True))
    tail = R.synthesize(y[7:], g, M, D, flags=R.DEROTATE, frame0=7,
                        history=R.frame_rows(y[:7], M, R.DEROTATE, D=D)[7 - (g.size // D - 1):])
    assert np.abs(tail - plain[7 * D:]).max() < 1e-12 * np.abs(plain).max()


@pytest.mark.parametrize("M", [16, 56, 64])
def test_oversampled_bank_reconstructs(oracle, M):
    """D = M/2, analysis design(M, 12), synthesis design(D, 24), scale D: the input comes back delayed by
    L_h/2 + L_g/2 - (D-1), to 1e-4, at gain 1 +- 1e-5."""
    D = M // 2
    h, g = oracle.design_prototype(M, 12), oracle.design_prototype(D, 24)
    assert g.size == 12 * M
    rng = np.random.default_rng(M)
    N = D * 400
    x = crandn(rng, N)
    cfg = OracleConfig(M, 12, D)
    xr = R.synthesize(channelize_numpy(x, h, cfg), g, M, D)
    delay = R.synthesis_delay(h.size, g.size, cfg.offset)
    assert delay == sy.synthesis_delay(h.size, g.size, cfg.offset) == h.size // 2 + g.size // 2 - (D - 1)
    settle = h.size + g.size
    ref, got = x[settle:N - delay], xr[delay + settle:]
    rel = np.linalg.norm(got - ref) / np.linalg.norm(ref)
    gain = np.vdot(ref, got).real / np.vdot(ref, ref).real
    print(f"M={M}: rel={rel:.3e} gain-1={gain - 1:.2e}")
    assert rel <= 1e-4 and abs(gain - 1) <= 1e-5
    # the delay formula is exact: one sample either way is off by orders of magnitude
    for wrong in (delay - 1, delay + 1):
        off = xr[wrong + settle:wrong + settle + ref.size - 1]
        assert np.linalg.norm(off - ref[:-1]) / np.linalg.norm(ref) > 0.1


def test_critically_sampled_bank_does_not(oracle):
    """D = M with g = h reconstructs only to some 20 %: the documentation says so, and why"""
    M = 16
    h = oracle.design_prototype(M, 12)
    x = crandn(np.random.default_rng(0), M * 300)
    cfg = OracleConfig(M, 12, M)
    xr = R.synthesize(channelize_numpy(x, h, cfg), h, M, M)
    delay = R.synthesis_delay(h.size, h.size, cfg.offset)
    ref, got = x[2 * h.size:x.size - delay], xr[delay + 2 * h.size:]
    rel = np.linalg.norm(got - ref) / np.linalg.norm(ref)
    assert 0.05 < rel < 0.4, rel
    hdr = open(os.path.join(ROOT, "include", "pfb_channelizer.h")).read()
    assert "root-Nyquist" in hdr and "root-Nyquist" in sy.__doc__


def test_a_mask_keeps_its_band_and_drops_the_rest(oracle):
    M, D = 64, 32
    h, g = oracle.design_prototype(M, 12), oracle.design_prototype(D, 24)
    n = np.arange(D * 300)
    kept, dropped = 9, 12  # channel centres: k / M cycles per sample
    tone = lambda k: np.exp(2j * np.pi * k * n / M)  # noqa: E731
    cfg = OracleConfig(M, 12, D)
    delay = R.synthesis_delay(h.size, g.size, cfg.offset)
    settle = h.size + g.size
    mask = np.zeros(M)
    mask[kept - 1:kept + 2] = 1.0  # a band of three columns: its centre tone passes whole
    def level(k):  # noqa: E306
        xr = R.synthesize(channelize_numpy(tone(k), h, cfg), g, M, D, weights=mask)
        return np.sqrt(np.mean(np.abs(xr[delay + settle:]) ** 2)), xr
    lk, xk = level(kept)
    ld, _ = level(dropped)
    assert abs(lk - 1) < 1e-3
    assert np.abs(xk[delay + settle:] - tone(kept)[settle:n.size - delay]).max() < 1e-3
    drop_db = 20 * np.log10(ld / lk)
    print(f"a tone three columns from the kept one drops by {drop_db:.1f} dB")
    # measured in this restatement (float64): -104.6 dB, what the 80 dB Kaiser prototypes leave of a tone whose nearest
    # kept column is two away; asserted with a 6 dB margin
    assert drop_db < -104.6 + 6.0


def test_quantizer_rounds_halves_away_and_saturates():
    x = np.array([0.5, -0.5, 1.5, -1.5, 2.49, 2047.0, 2047.5, 5000.0, -2048.0, -2048.5, -1e9, np.nan, np.inf, -np.inf]) / 2048
    z = np.empty(x.size, np.complex128)
    z.real, z.imag = x, x[::-1]
    with np.errstate(invalid="ignore"):
        q = R.quantize_int16(z, 12)
    assert q[:, 0].tolist() == [1, -1, 2, -2, 2, 2047, 2047, 2047, -2048, -2048, -2048, 0, 2047, -2048]
    assert q[:, 1].tolist() == q[::-1, 0].tolist()


# -- the C ABI, host side ----------------------------------------------------------------------------------

def make_cfg(M=64, P=12, D=0, taps=None, scale=0.0, out=L.PFB_FMT_CF32, bw=12, layout=0, flags=0, route=0, size=None,
             keep=[]):
    t = np.ones(min(M, 8192) * min(P, 64), np.float32) if taps is None else np.asarray(taps, np.float32)
    keep.append(t)
    return L.PfbChsynConfig(C.sizeof(L.PfbChsynConfig) if size is None else size, M, P, D,
                            t.ctypes.data_as(C.POINTER(C.c_float)), scale, out, bw, layout, flags, route, -1)


def both(**kw):
    """(describe, create) statuses of one configuration"""
    lib = L.load()
    cfg, plan, h = make_cfg(**kw), L.PfbChsynPlan(), C.c_void_p()
    rd = lib.pfb_chsyn_describe(C.byref(cfg), C.byref(plan))
    rc = lib.pfb_chsyn_create(C.byref(cfg), C.byref(h))
    if rc == L.PFB_OK:
        lib.pfb_chsyn_destroy(h)
    return rd, rc


def test_argument_checks_come_in_the_documented_order():
    lib = L.load()
    BAD, FMT, UNS = L.PFB_ERR_BAD_ARG, L.PFB_ERR_BAD_FORMAT, L.PFB_ERR_UNSUPPORTED
    plan, h = L.PfbChsynPlan(), C.c_void_p()
    assert lib.pfb_chsyn_describe(None, C.byref(plan)) == lib.pfb_chsyn_create(None, C.byref(h)) == BAD
    cfg = make_cfg()
    assert lib.pfb_chsyn_describe(C.byref(cfg), None) == lib.pfb_chsyn_create(C.byref(cfg), None) == BAD
    cfg.taps = None
    assert lib.pfb_chsyn_describe(C.byref(cfg), C.byref(plan)) == BAD
    nan = np.ones(64 * 12, np.float32)
    nan[700] = np.nan
    for kw in (dict(size=8), dict(M=1), dict(M=0), dict(P=0), dict(D=3), dict(M=9, P=1, D=4), dict(D=65), dict(D=16),
               dict(taps=nan), dict(scale=float("inf")), dict(scale=float("nan")), dict(scale=1e300), dict(flags=4),
               dict(route=3), dict(layout=2)):
        assert both(**kw) == (BAD, BAD), kw
    # BAD_ARG wins over BAD_FORMAT, BAD_FORMAT over UNSUPPORTED
    assert both(flags=8, out=7) == (BAD, BAD)
    for kw in (dict(out=L.PFB_FMT_INT8_IQ), dict(out=7), dict(out=L.PFB_FMT_INT16_IQ, bw=1),
               dict(out=L.PFB_FMT_INT16_IQ, bw=17), dict(out=7, M=5000), dict(out=7, layout=1)):
        assert both(**kw) == (FMT, FMT), kw
    for kw in (dict(M=4097, P=1), dict(M=5000, P=1), dict(P=25), dict(layout=L.PFB_LAYOUT_CHANNEL_MAJOR),
               dict(M=60, route=L.PFB_CHSYN_ROUTE_FUSED), dict(M=256, P=24, D=128, route=L.PFB_CHSYN_ROUTE_FUSED),
               dict(M=4096, P=1, route=L.PFB_CHSYN_ROUTE_FUSED)):
        assert both(**kw) == (UNS, UNS), kw
    # null handles
    u = C.c_uint64()
    buf = np.zeros(256, np.complex64)
    p = C.c_void_p(buf.ctypes.data)
    assert lib.pfb_chsyn_destroy(None) == lib.pfb_chsyn_reset(None) == lib.pfb_chsyn_sync(None) == BAD
    assert lib.pfb_chsyn_set_stream(None, None) == lib.pfb_chsyn_get_device(None, None) == BAD
    assert lib.pfb_chsyn_set_frame_index(None, 0) == lib.pfb_chsyn_get_frame_index(None, C.byref(u)) == BAD
    assert lib.pfb_chsyn_samples_for(None, 5, C.byref(u)) == lib.pfb_chsyn_set_weights(None, None) == BAD
    assert lib.pfb_chsyn_process(None, p, 1, 0, p, 64, C.byref(u), L.PFB_MEM_HOST) == BAD
    assert lib.pfb_chsyn_process(None, p, 1, 0, p, 64, C.byref(u), 2) == BAD
    assert lib.pfb_chsyn_process_async(None, p, 1, 0, p, 64, C.byref(u)) == BAD
    assert lib.pfb_chsyn_last_kernel(None) == b""


def test_a_valid_config_needs_a_device():
    lib = L.load()
    if lib.pfb_device_count() > 0:
        pytest.skip("a GPU is present")
    for kw in (dict(), dict(M=2, P=1), dict(M=4096, P=24, D=2048), dict(M=3, P=24), dict(bw=99),
               dict(out=L.PFB_FMT_INT16_IQ, bw=2), dict(out=L.PFB_FMT_INT16_IQ, bw=16), dict(M=64, D=64), dict(M=64, D=32),
               dict(M=256, P=12, D=128, route=L.PFB_CHSYN_ROUTE_FUSED), dict(route=L.PFB_CHSYN_ROUTE_GENERIC),
               dict(flags=3, scale=-2.5)):
        assert both(**kw) == (L.PFB_OK, L.PFB_ERR_NO_DEVICE), kw


def test_no_cpu_fallback():
    if L.load().pfb_device_count() > 0:
        pytest.skip("a GPU is present")
    with pytest.raises(L.PfbError) as e:
        sy.ChannelSynthesizer(64, decimation=32)
    assert e.value.status == L.PFB_ERR_NO_DEVICE
    with pytest.raises(L.PfbError) as e:
        sy.synthesize(np.zeros((4, 8), np.complex64), np.ones(8, np.float32))
    assert e.value.status == L.PFB_ERR_NO_DEVICE
    with pytest.raises(L.PfbError) as e:
        sy.isolate_band(np.zeros((1000, 2), np.int16), 64, [3])
    assert e.value.status == L.PFB_ERR_NO_DEVICE
    with pytest.raises(ValueError):
        sy.isolate_band(np.zeros((1000, 2), np.int16), 7, [3])


@pytest.mark.parametrize("M", [2, 3, 8, 12, 25, 56, 64, 128, 130, 256, 560, 1024, 4096])
def test_describe_plans(M):
    for D in ([M] if M % 2 else [M, M // 2]):
        for P in (1, 2, 12, 24):
            taps = np.ones(M * P, np.float32)
            Q = M * P // D
            plans = {}
            for route in ("auto", "fused", "generic"):
                for output in ("cf32", "int16"):
                    try:
                        plan = sy.describe(M, taps, D, route=route, output=output)
                    except L.PfbError as e:
                        assert e.status == L.PFB_ERR_UNSUPPORTED and route == "fused"
                        plans[route] = None
                        continue
                    plans[route] = plan
                    assert plan.decimation == D and plan.q == Q and plan.carried_bytes == (Q - 1) * M * 8
                    if plan.route == L.PFB_CHSYN_ROUTE_FUSED:
                        assert M in FUSED_M and route != "generic" and plan.workspace_bytes == 0
                        T = plan.tile_frames
                        row = M + 2 * {56: 7, 64: 8, 128: 8, 256: 16}[M]   # a row and its padding, in values
                        assert T >= 1 and (T + Q - 1) * row * 8 <= 65536    # a workgroup's LDS
                        # the re-read (Q-1)/T is at most a quarter wherever 64 KiB allow
                        assert 4 * (Q - 1) <= T or (T + 1 + Q - 1) * row * 8 > 65536
                    else:
                        assert plan.route == L.PFB_CHSYN_ROUTE_GENERIC and route != "fused"
                        assert 0 < plan.workspace_bytes <= MIB64 and plan.workspace_bytes % (8 * M) == 0
                        assert plan.workspace_bytes + 8 * M > MIB64
                        assert 1 <= plan.tile_frames and 2 * plan.tile_frames * M * 8 <= 65536
            # auto is fused exactly where fused exists
            assert (plans["auto"].route == L.PFB_CHSYN_ROUTE_FUSED) == (plans["fused"] is not None)
            assert (plans["fused"] is not None) <= (M in FUSED_M)
            if M in (56, 64) or (M == 128 and Q <= 24):
                assert plans["fused"] is not None, (M, D, P)


def test_describe_does_not_depend_on_the_other_settings():
    taps = np.ones(128 * 12, np.float32)
    base = sy.describe(128, taps, 64)
    for kw in (dict(scale=3.0), dict(fftshift=True), dict(derotate=True), dict(bit_width=16)):
        assert bytes(sy.describe(128, taps, 64, **kw)) == bytes(base), kw
    assert base.q == 24 and base.route == L.PFB_CHSYN_ROUTE_FUSED and base.decimation == 64
    assert sy.describe(128, taps, 0).decimation == sy.describe(128, taps, 128).decimation == 128


def test_exports():
    lib = L.load()
    declared = {n for n in declared_symbols() if n.startswith("pfb_chsyn_")}
    assert declared == CHSYN_EXPORTS == {n for n in L.EXPORTS if n.startswith("pfb_chsyn_")}
    for name in CHSYN_EXPORTS:
        assert hasattr(lib, name), name
    assert C.sizeof(L.PfbChsynConfig) == 56 and C.sizeof(L.PfbChsynPlan) == 32
    assert (L.PFB_CHSYN_FFTSHIFT, L.PFB_CHSYN_DEROTATE) == (1, 2)
    assert (L.PFB_CHSYN_ROUTE_AUTO, L.PFB_CHSYN_ROUTE_FUSED, L.PFB_CHSYN_ROUTE_GENERIC) == (0, 1, 2)
    hdr = open(os.path.join(ROOT, "include", "pfb_channelizer.h")).read()
    for word in ("PFB_CHSYN_FFTSHIFT = 1u << 0, PFB_CHSYN_DEROTATE = 1u << 1",
                 "PFB_CHSYN_ROUTE_AUTO = 0, PFB_CHSYN_ROUTE_FUSED = 1, PFB_CHSYN_ROUTE_GENERIC = 2",
                 "delta = L_h/2 + L_g/2 - input_offset", "#define PFB_ABI_VERSION 2"):
        assert word in hdr, word
    assert hdr.index("pfb_chsyn_describe") > hdr.index("pfb_wf_from_stft_iq_file")   # its own section, after the waterfalls
    import sdr_channelizer_amd as pkg
    for name in ("ChannelSynthesizer", "synthesize", "design_synthesis_taps", "synthesis_delay", "isolate_band"):
        assert name in pkg.__all__ and getattr(pkg, name) is getattr(sy, name)


def test_the_struct_sizes_are_the_compilers(tmp_path):
    import shutil
    import subprocess
    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.skip("no gcc")
    src = tmp_path / "sizes.c"
    src.write_text('#include "pfb_channelizer.h"\n#include <stdio.h>\n#include <stddef.h>\nint main(void) {\n'
                   '  printf("%zu %zu %zu %zu\\n", sizeof(pfb_chsyn_config), sizeof(pfb_chsyn_plan),\n'
                   '         offsetof(pfb_chsyn_config, scale), offsetof(pfb_chsyn_config, device_id));\n  return 0;\n}\n')
    exe = tmp_path / "sizes"
    subprocess.run([gcc, "-std=c99", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)],
                   check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert r.stdout.split() == [str(C.sizeof(L.PfbChsynConfig)), str(C.sizeof(L.PfbChsynPlan)),
                                str(L.PfbChsynConfig.scale.offset), str(L.PfbChsynConfig.device_id.offset)]


def test_chsyn_entry_points_sit_under_the_abi_guard():
    src = open(os.path.join(ROOT, "sdr_channelizer_amd", "csrc", "pfb_chsyn.hip")).read()
    found = {}
    for m in re.finditer(r'^extern "C" int (\w+)\(', src, re.M):
        rest = src[m.start():]
        found[m.group(1)] = rest[: rest.index("\n}\n")]
    assert set(found) == CHSYN_EXPORTS - {"pfb_chsyn_last_kernel"}
    for name, body in found.items():
        assert "abi_guard" in body.split("{", 1)[1][:80], name
    rest = [ln for ln in src.splitlines() if ln.startswith('extern "C"') and not ln.startswith('extern "C" int ')]
    assert rest == ['extern "C" const char* pfb_chsyn_last_kernel(const pfb_chsyn_handle* h) '
                    '{ return h ? h->last_kernel : ""; }']
    from sdr_channelizer_amd import build
    assert "pfb_chsyn.hip" in build.SOURCES
    # the device is resolved after every argument check: NO_DEVICE comes last
    create = src[src.index("int create_chsyn("):]
    assert create.index("chsyn_check(cfg") < create.index("resolve_device") < create.index("hipMalloc")


def test_design_helpers(oracle):
    assert np.array_equal(sy.design_synthesis_taps(64, 32), oracle.design_prototype(32, 24).astype(np.float32))
    assert np.array_equal(sy.design_synthesis_taps(56), oracle.design_prototype(56, 12).astype(np.float32))
    assert sy.design_synthesis_taps(64, 32, 6).size == 64 * 6
    with pytest.raises(ValueError):
        sy.design_synthesis_taps(9, 4, 1)
    assert sy.synthesis_delay(768, 768, 31) == 737
