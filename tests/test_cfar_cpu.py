"""The CFAR detector's contract without a GPU: the numpy restatement (cfar_ref) against a literal per-cell loop, the
closing rule walked cell by cell, the design false-alarm rate, pfb_cfar_alpha, the plan, every argument check that
comes before the device, the struct layouts, the exports and the ABI guard, and pfb_cfar_to_pdw into pfb_event_fit."""
import ctypes as C
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import cfar_ref as R
from abi_symbols import declared_symbols
from sdr_channelizer_amd import _lib as L
from sdr_channelizer_amd import cfar

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFAR_EXPORTS = {"pfb_cfar_describe", "pfb_cfar_alpha", "pfb_cfar_create", "pfb_cfar_destroy", "pfb_cfar_reset",
                "pfb_cfar_set_stream", "pfb_cfar_sync", "pfb_cfar_get_device", "pfb_cfar_next_index", "pfb_cfar_get_stats",
                "pfb_cfar_process", "pfb_cfar_flush", "pfb_cfar_process_async", "pfb_cfar_to_pdw", "pfb_cfar_last_kernel"}


# -- the definition, cell by cell ---------------------------------------------------
def tree(v):
    if len(v) == 1:
        return np.float32(v[0])
    with np.errstate(all="ignore"):
        return np.float32(tree(v[: len(v) // 2]) + tree(v[len(v) // 2:]))


def literal(p, n, flushed, C, G, T, method, alpha, min_power, g, hyp=None):
    """The header text as a loop over cells: every cell works its block's noise out from scratch."""
    p = [np.float32(v) for v in p[:n]]
    nbc = n // C
    S = [tree(p[b * C:(b + 1) * C]) for b in range(nbc)]
    decided = n if flushed else max(0, nbc - G - T) * C
    out, run, without, n_over = [], None, 0, 0
    f64 = np.float64

    def close():
        out.append((run["first"], run["last"], run["pk"], run["pp"], run["noise"], run["hyp"], run["n"], run["flags"], 0))

    with np.errstate(all="ignore"):
        for i in range(decided):
            b = i // C
            lead = [j for j in range(b - G - T, b - G) if j >= 0]
            lag = [j for j in range(b + G + 1, b + G + T + 1) if j < nbc]
            sl = sr = f64(0.0)
            for j in lead:
                sl = sl + f64(S[j])
            for j in lag:
                sr = sr + f64(S[j])
            nl, nr = len(lead), len(lag)
            if nl + nr == 0:
                noise = None
                without += 1
            elif method == R.CA:
                noise = np.float32((sl + sr) / f64((nl + nr) * C))
            else:
                sides = ([sl / f64(nl * C)] if nl else []) + ([sr / f64(nr * C)] if nr else [])
                if any(math.isnan(s) for s in sides):
                    noise = np.float32(np.nan)
                else:
                    noise = np.float32(max(sides) if method == R.GO else min(sides))
            over = noise is not None and bool(p[i] > np.float32(alpha) * noise) and bool(p[i] > np.float32(min_power))
            if over:
                n_over += 1
                if run is None:
                    run = {"first": i, "n": 0, "pp": None}
                run["last"] = i
                run["n"] += 1
                if run["pp"] is None or p[i] > run["pp"]:
                    run.update(pk=i, pp=p[i], noise=noise, hyp=-1 if hyp is None else int(hyp[i]),
                               flags=R.ONE_SIDED if nl + nr < 2 * T else 0)
            elif run is not None and i - run["last"] == g + 1:  # the (g+1)-th decided cell after the run's last
                close()
                run = None
        if run is not None and flushed:
            close()
            run = None
    stats = {"cells_in": n, "cells_decided": decided, "cells_over": n_over, "cells_without_noise": without,
             "detections": len(out), "dropped": 0, "open_run": int(run is not None)}
    return np.array(out, R.DET) if out else np.zeros(0, R.DET), stats


def spiky(n, seed, spikes=8, level=200.0):
    rng = np.random.default_rng(seed)
    p = rng.exponential(1.0, n).astype(np.float32)
    at = rng.integers(0, max(n, 1), spikes)
    p[at[: n and spikes]] *= np.float32(level)
    return p


@pytest.mark.parametrize("method", [R.CA, R.GO, R.SO])
@pytest.mark.parametrize("G,T,g", [(0, 1, 0), (1, 2, 1), (2, 3, 5), (0, 2, 40)])
def test_restatement_is_the_definition(method, G, T, g):
    C = 4
    for seed, n in enumerate((0, 3, 4, 37, 120, 200)):
        p = spiky(n, seed)
        if n > 60:
            p[50:53] = p[50:53].max() * 50        # a run of three, two equal maxima: the lower index is the peak
            p[58] = np.inf
            p[20] = np.nan
        hyp = np.arange(n, dtype=np.int32) * 7 - 100
        for flushed in (False, True):
            for cut in sorted({n, n // 2, max(n - 5, 0)}):
                want, wstats = literal(p, cut, flushed, C, G, T, method, 3.0, 0.5, g, hyp)
                got, gstats = R.detect(p, cut, flushed, C, G, T, method, 3.0, 0.5, g, hyp)
                assert got.tobytes() == want.tobytes(), (n, cut, flushed)
                assert gstats == wstats, (n, cut, flushed)


def test_tree_sum_is_not_the_sequential_sum():
    """the restatement would pass with any summation order if the data never told them apart: these do"""
    p = np.array([1e8, 1.0, -1e8, 1.0] * 16, np.float32)
    S = R.block_sums(p, 64)
    assert S[0] == tree(list(p)) and S[0] != np.float32(np.cumsum(p, dtype=np.float32)[-1])


def test_emission_order_and_the_closing_rule():
    C, G, T, g = 4, 1, 2, 6
    n = 200
    p = np.ones(n, np.float32)
    for at in (41, 43, 50, 70, 71, 120, 127, 135, 160):   # gaps 1, 6 (one run), 19, 0, 48, 6, 7 (a new run), 24
        p[at] = 1000.0
    final, _ = R.detect(p, n, True, C, G, T, R.CA, 4.0, 0.0, g)
    assert [(int(d["first_index"]), int(d["last_index"])) for d in final] == [(41, 50), (70, 71), (120, 127), (135, 135),
                                                                              (160, 160)]
    seen = 0
    for cells in range(n + 1):
        got, stats = R.detect(p, cells, False, C, G, T, R.CA, 4.0, 0.0, g)
        decided = max(0, cells // C - G - T) * C
        closed = [d for d in final if decided >= int(d["last_index"]) + g + 2]   # g+1 decided cells follow the last
        assert len(got) == len(closed) >= seen and got.tobytes() == final[: len(got)].tobytes(), cells
        assert stats["cells_decided"] == decided
        seen = len(got)
    assert seen == 5   # 160 + 6 + 2 <= the 188 cells decided without a flush


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_design_false_alarm_rate(seed):
    """unit exponential noise against alpha = cfar_alpha(1e-3, 1024): the over count among fully trained blocks lies
    within 5 sqrt(n Pfa) of n Pfa"""
    n, C, G, T, pfa = 1 << 22, 64, 1, 8, 1e-3
    rng = np.random.default_rng(seed)
    z = (rng.standard_normal(n) + 1j * rng.standard_normal(n)) / np.sqrt(2.0)
    p = (z.real ** 2 + z.imag ** 2).astype(np.float32)
    alpha = cfar.cfar_alpha(pfa, 2 * T * C)
    over, _noise, trained = R.decide(p, n, False, C, G, T, R.CA, alpha, 0.0)
    full = np.repeat(trained == 2 * T, C)[: len(over)]
    cells = int(full.sum())
    count = int(over[full].sum())
    print(f"seed {seed}: {count} over of {cells} fully trained cells, expected {cells * pfa:.0f} +- {5 * math.sqrt(cells * pfa):.0f}")
    assert cells > n - (2 * (G + T) + 1) * C
    assert abs(count - cells * pfa) <= 5 * math.sqrt(cells * pfa)


def test_alpha():
    lib = L.load()
    a = C.c_double(-1.0)
    for pfa, N in ((1e-3, 1024), (1e-7, 1024), (0.5, 1), (1e-12, 8), (0.999, 65536)):
        assert lib.pfb_cfar_alpha(pfa, N, C.byref(a)) == L.PFB_OK
        assert abs(a.value - R.alpha_ca(pfa, N)) <= 1e-12 * R.alpha_ca(pfa, N) and cfar.cfar_alpha(pfa, N) == a.value
    assert abs(cfar.cfar_alpha(1e-3, 1) - 999.0) < 1e-9   # one training cell: 1/pfa - 1
    assert abs(cfar.cfar_alpha(1e-3, 1 << 40) - math.log(1e3)) < 1e-3  # many: -ln(pfa)
    a.value = -1.0
    for pfa, N in ((0.0, 8), (1.0, 8), (-0.1, 8), (1.5, 8), (np.nan, 8), (np.inf, 8), (1e-3, 0)):
        assert lib.pfb_cfar_alpha(pfa, N, C.byref(a)) == L.PFB_ERR_BAD_ARG and a.value == -1.0
    assert lib.pfb_cfar_alpha(1e-3, 8, None) == L.PFB_ERR_BAD_ARG


def config(element=0, method=0, C_=64, G=1, T=8, g=0, alpha=5.0, min_power=0.0, flags=0, size=None, device=-1):
    return L.PfbCfarConfig(C.sizeof(L.PfbCfarConfig) if size is None else size, element, method, C_, G, T, g, alpha,
                           min_power, flags, device)


def both(**kw):
    """the status of pfb_cfar_describe and of pfb_cfar_create for one config, their outputs untouched on failure"""
    lib = L.load()
    cfg = config(**kw)
    plan, h = L.PfbCfarPlan(), C.c_void_p()
    C.memset(C.byref(plan), 0x5a, C.sizeof(plan))
    d = lib.pfb_cfar_describe(C.byref(cfg), C.byref(plan))
    c = lib.pfb_cfar_create(C.byref(cfg), C.byref(h))
    assert d == L.PFB_OK or bytes(plan) == b"\x5a" * C.sizeof(plan)
    assert not h.value or c == L.PFB_OK
    if h.value:
        lib.pfb_cfar_destroy(h)
    return d, c


def test_arguments_are_checked_before_the_device_and_in_order():
    lib = L.load()
    BAD = L.PFB_ERR_BAD_ARG
    plan, h = L.PfbCfarPlan(), C.c_void_p()
    cfg = config()
    assert lib.pfb_cfar_describe(None, C.byref(plan)) == lib.pfb_cfar_describe(C.byref(cfg), None) == BAD
    assert lib.pfb_cfar_create(None, C.byref(h)) == lib.pfb_cfar_create(C.byref(cfg), None) == BAD
    bad = [dict(size=40), dict(size=48), dict(element=2), dict(method=3)]
    bad += [dict(C_=c) for c in (0, 1, 2, 3, 5, 48, 96, 1023, 1025, 2048, 1 << 31)]
    bad += [dict(G=65), dict(G=1 << 31), dict(T=0), dict(T=33), dict(g=(1 << 20) + 1)]
    bad += [dict(alpha=a) for a in (0.0, -1.0, np.nan, np.inf, -np.inf)]
    bad += [dict(min_power=m) for m in (-1.0, np.nan, -np.inf)]
    bad += [dict(flags=f) for f in (1, 2, 1 << 31)]
    for kw in bad:
        assert both(**kw) == (BAD, BAD), kw
        assert both(device=1 << 20, **kw) == (BAD, BAD), kw   # before the device is looked at
    assert not h.value
    # null handles and pointers
    u, st = C.c_uint64(7), L.PfbCfarStats()
    buf = np.zeros(64, np.float32)
    p = C.c_void_p(buf.ctypes.data)
    assert lib.pfb_cfar_destroy(None) == lib.pfb_cfar_reset(None) == lib.pfb_cfar_sync(None) == BAD
    assert lib.pfb_cfar_set_stream(None, None) == lib.pfb_cfar_get_device(None, None) == BAD
    assert lib.pfb_cfar_next_index(None, C.byref(u)) == lib.pfb_cfar_get_stats(None, C.byref(st)) == BAD
    assert lib.pfb_cfar_process(None, p, 16, p, 1, C.byref(u), L.PFB_MEM_HOST) == BAD
    assert lib.pfb_cfar_process(None, p, 16, p, 1, C.byref(u), 2) == BAD
    assert lib.pfb_cfar_flush(None, p, 1, C.byref(u), L.PFB_MEM_HOST) == BAD
    assert lib.pfb_cfar_process_async(None, p, 16, p, 1, p) == BAD
    assert u.value == 7 and lib.pfb_cfar_last_kernel(None) == b""


def test_a_valid_config_needs_a_device():
    if L.load().pfb_device_count() > 0:
        pytest.skip("a GPU is present")
    for kw in (dict(), dict(C_=4, G=0, T=1), dict(C_=1024, G=64, T=32, g=1 << 20), dict(element=1, method=2),
               dict(min_power=np.inf), dict(alpha=1e-30)):
        assert both(**kw) == (L.PFB_OK, L.PFB_ERR_NO_DEVICE), kw
    with pytest.raises(L.PfbError) as e:
        cfar.Cfar(64, 1, 8, pfa=1e-6)
    assert e.value.status == L.PFB_ERR_NO_DEVICE
    with pytest.raises(L.PfbError) as e:
        cfar.detect(np.ones(1000, np.float32), 64, 1, 8, 5.0)
    assert e.value.status == L.PFB_ERR_NO_DEVICE


def test_describe():
    for element, eb in (("power", 4), ("cell", 8)):
        for C_, tier in ((4, "lanes"), (16, "lanes"), (64, "lanes"), (128, "lanes"), (256, "wave"), (512, "subsums"),
                         (1024, "subsums")):
            for G, T in ((0, 1), (1, 2), (3, 32), (64, 32)):
                plan = cfar.describe_cfar(C_, G, T, element=element)
                assert plan.latency_cells == (G + T + 1) * C_ and plan.training_cells == 2 * T * C_
                assert plan.carry_bytes == (G + T + 1) * C_ * eb + (2 * (G + T) + 2) * 4
                assert plan.sum_kernel.decode() == f"pfb_cfar_sum<{tier},{element}>"
    base = bytes(cfar.describe_cfar(64, 1, 8))
    for kw in (dict(alpha=9.0), dict(method="go"), dict(method="so"), dict(merge_gap=77), dict(min_power=3.0)):
        assert bytes(cfar.describe_cfar(64, 1, 8, **kw)) == base, kw
    with pytest.raises(ValueError):
        cfar.Cfar(64, 1, 8)
    with pytest.raises(ValueError):
        cfar.Cfar(64, 1, 8, 5.0, pfa=1e-3)


def test_exports():
    lib = L.load()
    declared = {n for n in declared_symbols() if n.startswith("pfb_cfar_")}
    assert declared == CFAR_EXPORTS == {n for n in L.EXPORTS if n.startswith("pfb_cfar_")}
    for name in CFAR_EXPORTS:
        assert hasattr(lib, name), name
    assert (C.sizeof(L.PfbCfarConfig), C.sizeof(L.PfbCfarPlan), C.sizeof(L.PfbCfarDet), C.sizeof(L.PfbCfarStats)) \
        == (44, 56, 48, 56)
    assert cfar.DET_DTYPE.itemsize == R.DET.itemsize == 48 and cfar.DET_DTYPE == R.DET
    assert [cfar.DET_DTYPE.fields[n][1] for n, _ in L.PfbCfarDet._fields_] == [getattr(L.PfbCfarDet, n).offset
                                                                              for n, _ in L.PfbCfarDet._fields_]
    assert (L.PFB_CFAR_POWER, L.PFB_CFAR_BANK_CELL, L.PFB_CFAR_CA, L.PFB_CFAR_GO, L.PFB_CFAR_SO) == (0, 1, 0, 1, 2)
    hdr = open(os.path.join(ROOT, "include", "pfb_channelizer.h")).read()
    assert "PFB_CFAR_POWER = 0, PFB_CFAR_BANK_CELL = 1" in hdr and "PFB_CFAR_CA = 0, PFB_CFAR_GO = 1, PFB_CFAR_SO = 2" in hdr
    assert "#define PFB_ABI_VERSION 2" in hdr and lib.pfb_abi_version() == 2
    assert hdr.index("pfb_cfar_describe(") > hdr.index("pfb_mfbank_last_kernel(")   # its own section, after the bank's
    import sdr_channelizer_amd as pkg
    names = ["Cfar", "cfar_alpha", "detect", "detect_pulses", "pulse_detections_from_iq_file", "detections_to_pdws"]
    at = pkg.__all__.index("MatchedFilterBank")
    assert pkg.__all__[at - len(names):at] == names
    for name in names:
        assert getattr(pkg, name) is getattr(cfar, name)


def test_the_struct_layouts_are_the_compilers(tmp_path):
    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.skip("no gcc")
    fields = [("pfb_cfar_config", L.PfbCfarConfig), ("pfb_cfar_plan", L.PfbCfarPlan), ("pfb_cfar_det", L.PfbCfarDet),
              ("pfb_cfar_stats", L.PfbCfarStats)]
    lines, want = [], []
    for cname, cls in fields:
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


def test_cfar_entry_points_sit_under_the_abi_guard():
    src = open(os.path.join(ROOT, "sdr_channelizer_amd", "csrc", "pfb_cfar.hip")).read()
    found = {}
    for m in re.finditer(r'^extern "C" int (\w+)\(', src, re.M):
        rest = src[m.start():]
        found[m.group(1)] = rest[: rest.index("\n}\n")]
    assert set(found) == CFAR_EXPORTS - {"pfb_cfar_last_kernel"}
    for name, body in found.items():
        assert "abi_guard" in body.split("{", 1)[1][:80], name
    assert src.count('extern "C"') == len(found) + 1
    from sdr_channelizer_amd import build
    assert "pfb_cfar.hip" in build.SOURCES
    create = src[src.index("int create_cfar("):]
    create = create[: create.index("\n}\n")]
    assert create.index("cfar_check(cfg") < create.index("resolve_device") < create.index("allocate_cfar(")


def test_to_pdw_and_event_fit():
    lib = L.load()
    fs, fc, t0 = 2.0e6, 915e6, 100.0
    n = 9
    d = np.zeros(n, R.DET)
    d["first_index"] = 1000 * np.arange(n) + 10
    d["last_index"] = d["first_index"] + 4
    d["peak_index"] = d["first_index"] + 2
    snr_db = 20.0 - 0.5 * (np.arange(n) - 4.0) ** 2            # a parabola with its top at pulse 4
    d["noise"] = 2.0
    d["peak_power"] = (2.0 * 10.0 ** (snr_db / 10.0)).astype(np.float32)
    d["hypothesis"] = -1
    pd = cfar.detections_to_pdws(d, fs, fc, t0)
    assert pd.dtype == cfar.PDW_DTYPE and len(pd) == n
    assert np.array_equal(pd["toa"], (d["peak_index"] + 1) / fs + t0) and np.array_equal(pd["pw"], np.full(n, 5 / fs))
    want_snr = 10 * np.log10(d["peak_power"].astype(np.float64) / 2.0)
    assert np.abs(pd["snr"] - want_snr).max() < 1e-12 and np.abs(pd["mag"] - np.sqrt(d["peak_power"].astype(np.float64))).max() < 1e-12
    assert not pd["sat"].any() and (pd["bin"] == -1).all() and (pd["freq"] == fc).all()
    from sdr_channelizer_amd import fit_event
    t_peak, snr_peak, coef = fit_event(pd)
    assert abs(t_peak - pd["toa"][4]) < 1e-6 and abs(snr_peak - 20.0) < 1e-3 and coef[2] < 0
    # bank detections: the bin of the hypothesis
    d["hypothesis"] = np.arange(n)
    pb = cfar.detections_to_pdws(d, fs, fc, t0, bin_hz=fs / 4096, first_bin=-4, bin_step=2)
    assert np.allclose(pb["freq"], fc + (np.arange(n) - 4) * 2 * fs / 4096, rtol=0, atol=1e-6) and (pb["bin"] == np.arange(n)).all()
    assert len(cfar.detections_to_pdws(d[:0], fs, fc, t0)) == 0
    out = np.zeros(n, cfar.PDW_DTYPE)
    po = out.ctypes.data_as(C.POINTER(L.PfbPdw))
    for bad_fs in (0.0, -1.0, np.nan, np.inf):
        assert lib.pfb_cfar_to_pdw(C.c_void_p(d.ctypes.data), n, bad_fs, fc, t0, 0.0, 0, 1, po) == L.PFB_ERR_BAD_ARG
    assert lib.pfb_cfar_to_pdw(None, n, fs, fc, t0, 0.0, 0, 1, po) == L.PFB_ERR_BAD_ARG
    assert lib.pfb_cfar_to_pdw(C.c_void_p(d.ctypes.data), n, fs, fc, t0, 0.0, 0, 1, None) == L.PFB_ERR_BAD_ARG
    assert not out.view(np.uint8).any()
