"""Modulation on pulse without a GPU: the numpy restatement (mop_ref) against the literal per-sample loops, the 2^62
bound and the limb sums at full scale, the cf32 bound against exact rational arithmetic, every argument check that
comes before the device and their order, the struct layouts, the exports, pfb_mop_figures, pfb_mop_pulses_from_pdw,
phase_code, and -- on the restatement alone -- the accuracy table that test_gpu_mop.py takes its tolerances from."""
import ctypes as C
import importlib
import math
import os
import re
import shutil
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import mop_cases as MC
import mop_ref as R
import synth_ref as S
from abi_symbols import declared_symbols
from sdr_channelizer_amd import _lib as L
from sdr_channelizer_amd.pdw import PDW_DTYPE

pm = importlib.import_module("sdr_channelizer_amd.pulse_mod")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MOP_EXPORTS = {"pfb_mop_describe", "pfb_mop_create", "pfb_mop_destroy", "pfb_mop_set_stream", "pfb_mop_sync",
               "pfb_mop_get_device", "pfb_mop_measure", "pfb_mop_measure_async", "pfb_mop_last_kernel", "pfb_mop_figures",
               "pfb_mop_pulses_from_pdw"}


# -- the definition ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ["int8", "int16"])
def test_restatement_is_the_literal_loops(fmt):
    x = MC.random_series(fmt, 400, 3)
    x[:6] = np.iinfo(x.dtype).min                      # full scale, and an exact tie of the peak
    for n in list(range(0, 12)) + [63, 64, 65, 130, 257]:
        for start in (0, 400 - n):
            rec, negs, _ = R.measure(x, R.pulses([start], [n]), max_negatives=16)
            lit = R.literal(x[start:start + n, 0], x[start:start + n, 1])
            r = rec[0]
            assert (r["n"], r["neg_count"]) == (n, len(lit["negs"]))
            for name in R.SUMS:
                assert r[name] == float(lit[name]), (n, name)          # every sum here is under 2^53
            assert negs[0].tolist() == (lit["negs"] + [R.NONE] * 16)[:16]
            assert (r["first_neg"], r["last_neg"]) == ((lit["negs"][0], lit["negs"][-1]) if lit["negs"] else (R.NONE, R.NONE))
            assert r["peak_index"] == lit["peak_index"] and r["peak_power"] == lit["peak_power"]
            assert r["flags"] == (R.SHORT if n < 3 else 0) | (R.NEGS_CLIPPED if len(lit["negs"]) > 16 else 0)
            assert r["negs_listed"] == min(len(lit["negs"]), 16)


@pytest.mark.parametrize("fmt,maxneg", [("int8", 4), ("int16", 2), ("int16", 0)])
def test_the_long_list_form_is_the_restatement(fmt, maxneg):
    x = MC.random_series(fmt, 512, 9)
    x[100:140] = np.iinfo(x.dtype).min
    rng = np.random.default_rng(4)
    lengths = rng.integers(3, 10, 300)
    plist = R.pulses([int(rng.integers(0, 512 - n + 1)) for n in lengths], lengths)
    rec, negs, _ = R.measure(x, plist, max_negatives=maxneg)
    many = R.measure_many(x, plist, maxneg)
    assert many[0].tobytes() == rec.tobytes() and many[1].tobytes() == negs.tobytes()


def test_the_bound_and_the_limb_sums_at_full_scale():
    n = 1 << 20
    x = np.full((n, 2), -32768, np.int16)
    I, Q = R.components(x, 0, n)
    t = R.terms(I, Q)
    assert int(t["a"].max()) == 1 << 31 and int(t["s2re"].max()) == 1 << 62 and t["s2re"].dtype == np.int64   # 63-bit terms
    exact = (1 << 62) * (n - 1 - (n - 1) // 2)
    assert exact.bit_length() == 82                                          # what one int64 could not hold
    reported, total = R.limb_sum(t["s2re"])
    assert total == exact and reported == float(exact)
    assert int((t["s2re"] >> 32).sum()) < 1 << 52 and int((t["s2re"] & 0xFFFFFFFF).sum()) < 1 << 52   # the limbs stay exact
    assert int(t["p"].sum()) == n << 31 < 1 << 53 and int(t["a"].sum()) == (n - 1) << 31 < 1 << 53
    # mixed signs at full scale: the limb sum is the float64 nearest the exact sum
    rng = np.random.default_rng(5)
    y = rng.choice(np.array([-32768, 32767], np.int16), (4097, 2))
    t = R.terms(*R.components(y, 0, 4097))
    for name in ("s2re", "s2im"):
        reported, total = R.limb_sum(t[name])
        assert total == sum(int(v) for v in t[name]) and reported == float(total)
        assert abs(int(np.abs(t[name]).max())) <= 1 << 62


def test_the_cf32_bound_holds_against_exact_arithmetic():
    """a sequential float64 twin of the sums against rational arithmetic: within (n + 4) 2^-53 sum m_i"""
    rng = np.random.default_rng(7)
    for n in (3, 8, 65, 300):
        for scale in (1.0, 1e-3, 1e6):
            z = ((rng.standard_normal(n) + 1j * rng.standard_normal(n)) * scale).astype(np.complex64)
            I, Q = R.components(z, 0, n)
            t = R.terms(I, Q)
            _, _, bound = R.one(I, Q, 8)
            fi, fq = [Fraction(float(v)) for v in I], [Fraction(float(v)) for v in Q]
            a = [fi[i + 1] * fi[i] + fq[i + 1] * fq[i] for i in range(n - 1)]
            b = [fq[i + 1] * fi[i] - fi[i + 1] * fq[i] for i in range(n - 1)]
            Lg = (n - 1) // 2
            exact = {"energy": sum(fi[i] * fi[i] + fq[i] * fq[i] for i in range(n)), "s1_re": sum(a), "s1_im": sum(b),
                     "s2_re": sum(a[i + Lg] * a[i] + b[i + Lg] * b[i] for i in range(n - 1 - Lg)),
                     "s2_im": sum(b[i + Lg] * a[i] - a[i + Lg] * b[i] for i in range(n - 1 - Lg))}
            for name, v in (("energy", t["p"]), ("s1_re", t["a"]), ("s1_im", t["b"]), ("s2_re", t["s2re"]), ("s2_im", t["s2im"])):
                for order in (v, v[::-1]):
                    twin = 0.0
                    for term in order:
                        twin += float(term)
                    assert abs(Fraction(twin) - exact[name]) <= Fraction(bound[name]), (n, scale, name)


# -- the arguments -----------------------------------------------------------------------------------------------------
GOOD = dict(sample_format=L.PFB_FMT_INT16_IQ, bit_width=12, trim_samples=0, max_negatives=32, device_id=-1)


def config(size=None, **kw):
    return L.PfbMopConfig(C.sizeof(L.PfbMopConfig) if size is None else size, **{**GOOD, **kw})


def both(**kw):
    lib = L.load()
    cfg = config(**kw)
    plan, h = L.PfbMopPlan(), C.c_void_p()
    C.memset(C.byref(plan), 0x5a, C.sizeof(plan))
    d = lib.pfb_mop_describe(C.byref(cfg), C.byref(plan))
    c = lib.pfb_mop_create(C.byref(cfg), C.byref(h))
    assert d == L.PFB_OK or bytes(plan) == b"\x5a" * C.sizeof(plan)
    assert not h.value or c == L.PFB_OK
    if h.value:
        lib.pfb_mop_destroy(h)
    return d, c


def test_arguments_are_checked_before_the_device_and_in_order():
    lib = L.load()
    BAD, FMT = L.PFB_ERR_BAD_ARG, L.PFB_ERR_BAD_FORMAT
    plan, h = L.PfbMopPlan(), C.c_void_p()
    cfg = config()
    assert lib.pfb_mop_describe(None, C.byref(plan)) == lib.pfb_mop_describe(C.byref(cfg), None) == BAD
    assert lib.pfb_mop_create(None, C.byref(h)) == lib.pfb_mop_create(C.byref(cfg), None) == BAD
    bad = [(dict(size=20), BAD), (dict(size=28), BAD), (dict(max_negatives=129), BAD), (dict(trim_samples=(1 << 19) + 1), BAD),
           (dict(sample_format=3), FMT), (dict(bit_width=0), FMT), (dict(bit_width=17), FMT),
           (dict(sample_format=L.PFB_FMT_INT8_IQ, bit_width=9), FMT)]
    for kw, status in bad:
        assert both(**kw) == (status, status), kw
        assert both(**{"device_id": 1 << 20, **kw}) == (status, status), kw     # before the device is looked at
    # an earlier refusal wins over a later one
    assert both(size=20, sample_format=3) == (BAD, BAD)
    assert both(max_negatives=129, sample_format=3) == (BAD, BAD) and both(trim_samples=1 << 20, bit_width=0) == (BAD, BAD)
    assert both(max_negatives=129, trim_samples=1 << 20) == (BAD, BAD)
    for kw in (dict(max_negatives=128), dict(max_negatives=0), dict(trim_samples=1 << 19), dict(bit_width=16), dict(bit_width=1),
               dict(sample_format=L.PFB_FMT_CF32, bit_width=0), dict(sample_format=L.PFB_FMT_INT8_IQ, bit_width=8)):
        assert lib.pfb_mop_describe(C.byref(config(**kw)), C.byref(plan)) == L.PFB_OK, kw
    # null handles
    buf = np.zeros(64, np.uint64)
    p = C.c_void_p(buf.ctypes.data)
    assert lib.pfb_mop_destroy(None) == lib.pfb_mop_sync(None) == lib.pfb_mop_set_stream(None, None) == BAD
    assert lib.pfb_mop_get_device(None, None) == BAD and lib.pfb_mop_set_tier(None, 0, 0, 0) == BAD
    for mem in (L.PFB_MEM_HOST, L.PFB_MEM_DEVICE, 2):
        assert lib.pfb_mop_measure(None, p, 8, 1, 0, mem, p, 1, mem, p, p) == BAD
    assert lib.pfb_mop_measure_async(None, p, 8, 1, 0, p, 1, p, p) == BAD
    assert lib.pfb_mop_last_kernel(None) == b"" and not buf.any()
    with pytest.raises(ValueError):
        pm.describe_modulation(max_negatives=-1)
    with pytest.raises(L.PfbError):
        pm.describe_modulation(max_negatives=129)


def test_a_valid_config_needs_a_device():
    if L.load().pfb_device_count() > 0:
        pytest.skip("a GPU is present")
    assert both() == (L.PFB_OK, L.PFB_ERR_NO_DEVICE)
    with pytest.raises(L.PfbError) as e:
        pm.PulseModulation()
    assert e.value.status == L.PFB_ERR_NO_DEVICE
    with pytest.raises(L.PfbError) as e:
        pm.measure_pulses(MC.random_series("int16", 64, 1), [0], [64])
    assert e.value.status == L.PFB_ERR_NO_DEVICE


def test_describe():
    for fmt in ("int8", "int16", "cf32"):
        plan = pm.describe_modulation(fmt, 8)
        assert (plan.group_min, plan.split_min, plan.part_samples, plan.grid_cap, plan.slice_pulses, plan.split_slots) \
            == (MC.GROUP_MIN, MC.SPLIT_MIN, MC.PART, MC.GRID_CAP, MC.SLICE, MC.SLOTS)
        assert plan.threads == 256 and plan.stage_bytes == 32 << 20
        assert 64 <= plan.group_min < plan.part_samples and 2 * plan.part_samples <= plan.split_min <= 1 << 20
        assert (plan.wave_kernel, plan.group_kernel, plan.split_kernel, plan.join_kernel) \
            == (b"mop_wave", b"mop_group", b"mop_split", b"mop_join")
    # the work of a slice, the partial slots, and a host list's slice with its records; the lists scale with max_negatives
    small, big = pm.describe_modulation(max_negatives=0).scratch_bytes, pm.describe_modulation(max_negatives=128).scratch_bytes
    assert 9 << 20 <= small <= 11 << 20 and big - small == ((1 << 16) + 256 * 64) * 128 * 4
    assert (small, big) == (10223872, 52166912)     # to the byte: the sizes before the scratch was carved through the shared carver


def test_exports():
    lib = L.load()
    declared = {n for n in declared_symbols() if n.startswith("pfb_mop_")}
    assert declared == MOP_EXPORTS == {n for n in L.EXPORTS if n.startswith("pfb_mop_")}
    assert L.EXPORTS[-len(MOP_EXPORTS):][0] == "pfb_mop_describe" and L.EXPORTS[-len(MOP_EXPORTS) - 1].startswith("pfb_deint_")
    assert "pfb_mop_set_tier" in L.DEV_EXPORTS
    for name in MOP_EXPORTS:
        assert hasattr(lib, name), name
    assert (C.sizeof(L.PfbMopConfig), C.sizeof(L.PfbMopPulse), C.sizeof(L.PfbMopRecord), C.sizeof(L.PfbMopPlan),
            C.sizeof(L.PfbMopFigure)) == (24, 16, 96, 168, 48)
    assert pm.MOP_DTYPE == R.MOP and pm.MOP_DTYPE.itemsize == 96 and pm.PULSE_DTYPE == R.PULSE
    for dt, cls in ((pm.MOP_DTYPE, L.PfbMopRecord), (pm.PULSE_DTYPE, L.PfbMopPulse), (pm.FIGURE_DTYPE, L.PfbMopFigure)):
        for (name, _), (cname, _) in zip(dt.descr, cls._fields_):
            assert name == cname and dt.fields[name][1] == getattr(cls, cname).offset
    assert (L.PFB_MOP_OUTSIDE, L.PFB_MOP_SHORT, L.PFB_MOP_TRUNCATED, L.PFB_MOP_NEGS_CLIPPED) \
        == (R.OUTSIDE, R.SHORT, R.TRUNCATED, R.NEGS_CLIPPED)
    hdr = open(os.path.join(ROOT, "include", "pfb_channelizer.h")).read()
    assert "#define PFB_ABI_VERSION 2" in hdr and lib.pfb_abi_version() == 2
    assert hdr.index("pfb_mop_describe(") > hdr.index("pfb_deint_ticks_from_toa(")     # its own section, at the end
    assert "EVERY EXPRESSION BELOW IS EVALUATED AS WRITTEN" in hdr
    import sdr_channelizer_amd as pkg
    names = ["MOP_DTYPE", "PulseModulation", "measure_pulses", "measure_pdws", "modulation_figures", "phase_code",
             "replica_from_measurement", "modulation_from_iq_file"]
    at = pkg.__all__.index("Deinterleaver")
    assert pkg.__all__[at - len(names):at] == names
    for name in names:
        assert getattr(pkg, name) is getattr(pm, name)


def test_the_struct_layouts_are_the_compilers(tmp_path):
    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.skip("no gcc")
    lines, want = [], []
    for cname, cls in (("pfb_mop_config", L.PfbMopConfig), ("pfb_mop_pulse", L.PfbMopPulse), ("pfb_mop_record", L.PfbMopRecord),
                       ("pfb_mop_plan", L.PfbMopPlan), ("pfb_mop_figure", L.PfbMopFigure)):
        lines.append(f'  printf("%zu\\n", sizeof({cname}));')
        want.append(C.sizeof(cls))
        for name, _ in cls._fields_:
            lines.append(f'  printf("%zu\\n", offsetof({cname}, {name}));')
            want.append(getattr(cls, name).offset)
    src = tmp_path / "sizes.c"
    src.write_text('#include "pfb_channelizer.h"\n#include <stdio.h>\n#include <stddef.h>\nint main(void) {\n'
                   + "\n".join(lines) + "\n  return 0;\n}\n")
    exe = tmp_path / "sizes"
    subprocess.run([gcc, "-std=c99", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)],
                   check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert [int(v) for v in r.stdout.split()] == want


def test_mop_entry_points_sit_under_the_abi_guard():
    src = open(os.path.join(ROOT, "sdr_channelizer_amd", "csrc", "pfb_mop.hip")).read()
    found = {}
    for m in re.finditer(r'^extern "C" int (\w+)\(', src, re.M):
        rest = src[m.start():]
        found[m.group(1)] = rest[: rest.index("\n}\n")]
    assert set(found) == (MOP_EXPORTS - {"pfb_mop_last_kernel"}) | {"pfb_mop_set_tier"}
    for name, body in found.items():
        assert "abi_guard" in body.split("{", 1)[1][:80], name
    from sdr_channelizer_amd import build
    assert "pfb_mop.hip" in build.SOURCES
    code = re.sub(r"//.*", "", src)
    assert "#pragma clang fp contract(off)" in code and "asm" not in code
    for line in code.splitlines():                                            # integer atomics only
        if "atomic" in line:
            assert "atomicAdd(&p.ctl[" in line, line


# -- the host helpers --------------------------------------------------------------------------------------------------
def test_figures_follow_the_formulas():
    rng = np.random.default_rng(11)
    rec = np.zeros(40, R.MOP)
    rec["n"] = rng.integers(0, 3000, 40)
    rec["n"][:4] = [0, 1, 2, 3]
    for name in R.SUMS:
        rec[name] = rng.standard_normal(40) * 1e9
    rec["energy"] = np.abs(rec["energy"])
    rec["neg_count"] = rng.integers(0, 30, 40)
    rec["neg_count"][4:8] = [0, 1, 2, 3]
    rec["flags"][8] = R.OUTSIDE
    for fs in (56e6, 1.0, 2.4e9):
        got = pm.modulation_figures(rec, fs)
        for g, w in zip(got, R.figures(rec, fs)):
            for name, v in zip(("freq_hz", "rate_hz_per_s", "extent_hz", "mean_power", "flips"), w):
                assert abs(g[name] - v) <= 1e-12 * abs(v), (name, g[name], v)
            assert g["kind"] == w[5] and g["reserved"] == 0
    assert got["kind"][:4].tolist() == [4, 4, 4, got["kind"][3]] and got["kind"][3] != 4 and got["kind"][8] == 4
    lib = L.load()
    out = np.zeros(2, pm.FIGURE_DTYPE)
    for fs in (0.0, -1.0, math.inf, math.nan):
        assert lib.pfb_mop_figures(C.c_void_p(rec.ctypes.data), 2, fs, C.c_void_p(out.ctypes.data)) == L.PFB_ERR_BAD_ARG
    assert lib.pfb_mop_figures(None, 2, 1.0, C.c_void_p(out.ctypes.data)) == L.PFB_ERR_BAD_ARG
    assert lib.pfb_mop_figures(None, 0, 1.0, None) == L.PFB_OK and not out.view(np.uint8).any()
    # the sweep test is one Rayleigh bin of the pulse, the code test two negatives
    r = np.zeros(3, R.MOP)
    r["n"], r["s1_re"] = 1001, 1.0
    Lg = 500
    for k, extent in enumerate((0.999, 1.001, -1.001)):                       # in bins of fs / n
        ang = 2 * math.pi * Lg * extent / (1001 * 1000)
        r["s2_re"][k], r["s2_im"][k] = math.cos(ang), math.sin(ang)
    r["neg_count"] = [1, 2, 0]
    assert pm.modulation_figures(r, 56e6)["kind"].tolist() == [0, 3, 1]


def oracle_pulses(oracle, x, t0=1000.0):
    pd, _ = oracle.extract_pdws_raw(x[:, 0] / 2048.0 + 1j * (x[:, 1] / 2048.0), MC.FS, 1e9, t0, snr_db=MC.CHAIN_SNR_DB)
    pdws = np.zeros(len(pd), PDW_DTYPE)
    for name in ("toa", "freq", "pw", "snr", "bin", "mag"):
        pdws[name] = [p[name] for p in pd]
    return pdws, pm.pulses_from_pdws(pdws, MC.FS, t0)


def test_pulses_from_pdws_the_oracle_extracts(oracle):
    x, d, first = MC.chain_stream("lfm")
    pdws, pulses = oracle_pulses(oracle, x)
    assert len(pulses) == 6
    for k, p in enumerate(pulses):                       # the scripts' toa is 1-based: start is the 0-based sample
        assert abs(int(p["start"]) - (first + 4000 * k)) <= 2 and abs(int(p["length"]) - 1000) <= 3 and p["column"] == 0
        assert int(p["start"]) == round((pdws["toa"][k] - 1000.0) * MC.FS) - 1
        assert int(p["length"]) == round(pdws["pw"][k] * MC.FS)
    # the refusals: nothing is written
    lib = L.load()
    out = np.full(4, 77, pm.PULSE_DTYPE)
    ok = np.zeros(4, PDW_DTYPE)
    ok["toa"], ok["pw"] = [1e-6, 2e-6, 3e-6, 4e-6], 1e-6

    def call(p, rate=1e6, t0=0.0, n=None):
        return lib.pfb_mop_pulses_from_pdw(C.c_void_p(p.ctypes.data), len(p) if n is None else n, rate, t0,
                                           C.c_void_p(out.ctypes.data))
    BAD = L.PFB_ERR_BAD_ARG
    assert call(ok, rate=0.0) == call(ok, rate=math.nan) == call(ok, t0=math.inf) == call(ok, n=(1 << 31) + 1) == BAD
    assert lib.pfb_mop_pulses_from_pdw(None, 4, 1e6, 0.0, C.c_void_p(out.ctypes.data)) == BAD
    for field, v in (("toa", math.nan), ("toa", 0.0), ("toa", 1e30), ("pw", -1e-6), ("pw", math.inf), ("pw", 5000.0), ("bin", -1)):
        p = ok.copy()
        p[field][2] = v
        assert call(p) == BAD, (field, v)
    assert (out["start"] == 77).all()
    assert call(ok) == L.PFB_OK and out["start"].tolist() == [0, 1, 2, 3] and out["length"].tolist() == [1] * 4


def test_phase_code():
    chip, signs = pm.phase_code(MC.BARKER_NEGS, 1001)
    assert chip == 77.0 and (signs * signs[0]).tolist() == list(S.BARKER_13)
    # unused entries, a single negative of noise, and the order do not matter
    noisy = np.array([R.NONE, 100] + MC.BARKER_NEGS[::-1] + [R.NONE], np.uint32)
    assert pm.phase_code(noisy, 1001)[1].tolist() == signs.tolist()
    # a pulse cut by a few samples at each end (trim, or the extractor's edges) keeps the code
    chip, cut = pm.phase_code(np.array(MC.BARKER_NEGS) - 5, 1001 - 9)
    assert abs(chip - 77.0) < 1e-9 and cut.tolist() == signs.tolist()
    # gaps of 2 and 4 chips only: the chip is half the smallest gap
    assert pm.phase_code([198, 199, 598, 599], 1000)[0] == 400.0       # nothing says 200: the spacing the gaps show
    chip, s = pm.phase_code([198, 199, 398, 399, 698, 699], 1000)
    assert chip == 100.0 and s.tolist() == [1, 1, -1, -1, 1, 1, 1, -1, -1, -1]
    assert pm.phase_code([], 500) == (500.0, pytest.approx(np.ones(1)))
    assert pm.phase_code([R.NONE] * 8, 500)[1].tolist() == [1]


# -- the accuracy table, on the restatement alone ----------------------------------------------------------------------
def test_the_accuracy_table():
    print("\n| input | sigma | mid frequency error, MHz | extent error, MHz | negatives |")
    worst = {}
    for name, kw in MC.TABLE.items():
        want_f = 3e6 + kw.get("extent", 0.0) / 2
        for sigma in MC.SIGMAS:
            ef, ee, negs = [], [], []
            for seed in MC.SEEDS:
                x, n = MC.synth_pulse(seed=seed, sigma=sigma, **kw)
                rec, _, _ = R.measure(x, R.pulses([0], [n]))
                f = R.figures(rec, MC.FS)[0]
                ef.append(f[0] - want_f)
                ee.append(f[2] - kw.get("extent", 0.0))
                negs.append(int(rec[0]["neg_count"]))
            worst[name, sigma] = (max(map(abs, ef)), max(map(abs, ee)), min(negs), max(negs))
            print("| %s | %g | %.4f | %.4f | %d..%d |" % (name, sigma, worst[name, sigma][0] / 1e6, worst[name, sigma][1] / 1e6,
                                                          min(negs), max(negs)))
    # every printed figure is the documented one (mop_cases.MEASURED): a change of S1's or S2's
    # accuracy, at any noise, shows here
    for name in MC.TABLE:
        for k, sigma in enumerate(MC.SIGMAS):
            freq, extent, least, most = MC.MEASURED[name][k]
            got = worst[name, sigma]
            assert abs(got[0] / 1e6 - freq) <= MC.TABLE_SLACK and abs(got[1] / 1e6 - extent) <= MC.TABLE_SLACK, (name, sigma, got)
            assert got[2:] == (least, most), (name, sigma, got)
    assert worst["LFM 40 MHz, pw 1000", MC.CHAIN_SIGMA][1] <= MC.EXTENT_TOL_LFM40 / MC.MARGIN + 1e6 * MC.TABLE_SLACK
    assert worst["LFM 40 MHz, pw 1000", MC.CHAIN_SIGMA][0] <= MC.FREQ_TOL_LFM40 / MC.MARGIN + 1e6 * MC.TABLE_SLACK
    # lag 1 instead of the half-length lag drowns in the noise: the 5 MHz chirp at sigma 2^-6, over the same seeds
    off = []
    for seed in MC.SEEDS:
        x, n = MC.synth_pulse(pw=1000, extent=5e6, seed=seed, sigma=2.0 ** -6)
        t = R.terms(*R.components(x, 0, n))
        a, b = t["a"].astype(np.float64), t["b"].astype(np.float64)
        lag1 = math.atan2(float((b[1:] * a[:-1] - a[1:] * b[:-1]).sum()), float((a[1:] * a[:-1] + b[1:] * b[:-1]).sum()))
        off.append(lag1 / (2 * math.pi) * MC.FS * (n - 1) - 5e6)
    print("lag 1 reads %.3f .. %.3f MHz for the 5 MHz chirp" % ((5e6 + min(off)) / 1e6, (5e6 + max(off)) / 1e6))
    assert max(map(abs, off)) > 10 * worst["LFM 5 MHz, pw 1000", 2.0 ** -6][1]


def test_the_chain_on_the_restatement(oracle):
    """what test_gpu_mop.py asks of the device chain, first on oracle PDWs and the restatement: the figures and the code
    at trim 8, and at trim 0 the replica made from the measurement, through the float64 matched filter (mf_ref)"""
    for kind in ("lfm", "barker"):
        x, d, first = MC.chain_stream(kind)
        _, pulses = oracle_pulses(oracle, x)
        rec, negs, _ = R.measure(x, pulses, trim=8, max_negatives=32)
        fig = R.figures(rec, MC.FS)
        assert len(rec) == 6
        for r, f, q in zip(rec, fig, negs):
            print(kind, "n %d, mid %.4f MHz, extent %.4f MHz, %d negatives, kind %d" % (r["n"], f[0] / 1e6, f[2] / 1e6,
                                                                                       r["neg_count"], f[5]))
            if kind == "lfm":
                # the measured part is n of the 1000 samples: its share of the 40 MHz, around the same mid frequency
                assert abs(f[2] - 40e6 * (r["n"] - 1) / 999) <= MC.EXTENT_TOL_LFM40 and f[5] == 1
                assert abs(f[0] - 23e6) <= MC.FREQ_TOL_LFM40
            else:
                assert f[4] == 6.0 and f[5] == 2
                chip, signs = pm.phase_code(q, int(r["n"]))
                assert abs(chip - 77.0) <= 0.5 and (signs * signs[0]).tolist() == list(S.BARKER_13)
        # the replica: the whole pulses, as the extractor found them
        rec0, negs0, _ = R.measure(x, pulses, trim=0, max_negatives=32)
        replica = pm.replica_from_measurement(rec0, negs0, MC.FS, 12)
        assert replica.dtype == np.complex64 and len(replica) == d["pw"] and abs(abs(replica[0]) - 0.5) < 0.01
        offsets = MC.replica_peak_offsets(x, replica, first)
        print(kind, "matched-filter peaks at", offsets, "samples from the pulses' first samples")
        assert offsets == [0] * 6           # the exact sample, for both trains: what the device chain is held to


def test_a_replica_without_a_list_of_negatives_has_no_code(oracle):
    x, d, first = MC.chain_stream("barker")
    _, pulses = oracle_pulses(oracle, x)
    rec, negs, _ = R.measure(x, pulses, max_negatives=32)
    coded = pm.replica_from_measurement(rec, negs, MC.FS, 12)
    none, empty = (pm.replica_from_measurement(rec, q, MC.FS, 12) for q in (None, R.measure(x, pulses, max_negatives=0)[1]))
    assert none.tobytes() == empty.tobytes() and len(none) == len(coded) == 1001
    signs = np.sign((coded / none).real)
    assert (signs[:5 * 77] == 1).all() and (signs[5 * 77 + 1:7 * 77 - 1] == -1).all() and np.allclose(np.abs(coded), np.abs(none))
