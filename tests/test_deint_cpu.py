"""The deinterleaver without a GPU: the numpy restatement (deint_ref) against the literal triple loop and the literal
walk, the candidate rule bin by bin on a designed histogram, every argument check that comes before the device and
their order, the struct layouts, the exports, pfb_deint_ticks_from_toa, merge_emitters, and -- on the restatement
alone -- the designed scene with its two companions that test_gpu_deint.py relies on."""
import ctypes as C
import importlib
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import deint_cases as DC
import deint_ref as R
from abi_symbols import declared_symbols
from sdr_channelizer_amd import _lib as L
from sdr_channelizer_amd.pdw import PDW_DTYPE

# the module, not the function of the same name that the package exports
di = importlib.import_module("sdr_channelizer_amd.deinterleave")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEINT_EXPORTS = {"pfb_deint_describe", "pfb_deint_create", "pfb_deint_destroy", "pfb_deint_set_stream", "pfb_deint_sync",
                 "pfb_deint_get_device", "pfb_deint_run", "pfb_deint_histogram", "pfb_deint_successors",
                 "pfb_deint_last_kernel", "pfb_deint_get_stats", "pfb_deint_ticks_from_toa"}


# -- the definition, sentence by sentence ------------------------------------------------------------------------------
def small_lists():
    rng = np.random.default_rng(1)
    lists = [np.zeros(0, np.uint64), np.array([7], np.uint64), DC.train(100, 9, 3), np.repeat(DC.train(100, 5), 3)]
    for n in (2, 17, 60):
        lists.append(np.sort(rng.integers(0, 40 * n, n)).astype(np.uint64))
        lists.append(np.sort(np.concatenate([DC.train(97, n, 5), rng.integers(0, 97 * n, n // 2)])).astype(np.uint64))
    return lists


@pytest.mark.parametrize("c", [R.Cfg(50, 400, 1, 4, X=1, tol=2), R.Cfg(90, 130, 7, 1, X=0, tol=3), R.Cfg(20, 999, 13, 256, X=2, tol=2),
                               R.Cfg(100, 100, 1, 3, X=8, tol=5)])
def test_restatement_is_the_literal_loops(c):
    for a in small_lists() + DC.window_lists(c, 100) + [DC.edge_list(c)]:
        assert R.histogram(a, c).tobytes() == R.literal_histogram(a, c).tobytes()
        for tau in (c.pmin, 100, c.pmax):
            if c.e * (2 * c.X + 3) >= tau:
                continue
            succ, step = R.successors(a, c, tau)
            lit = R.literal_successors(a, c, tau)
            assert succ.tobytes() == lit[0].tobytes() and step.tobytes() == lit[1].tobytes(), (a, tau)
            ln, per, end = R.chains(succ, step)
            for i in range(len(a)):
                assert (ln[i], per[i], end[i]) == R.literal_chain(succ, step, i)[:3]


def test_the_windows_and_the_ties():
    c = R.Cfg(50, 400, 1, 4, X=2, tol=2)
    got = [R.successors(a, c, 100) for a in DC.window_lists(c, 100)]
    firsts = [(int(s[0]), int(st[0])) for s, st in got]
    # per step m + 1: one tick under the window, its lower edge, its upper edge, one tick over
    assert firsts[:12] == [(-1, 0), (1, 1), (1, 1), (-1, 0), (-1, 0), (1, 2), (1, 2), (-1, 0), (-1, 0), (1, 3), (1, 3), (-1, 0)]
    assert firsts[12:] == [(1, 1), (1, 1), (2, 1), (1, 1)]
    assert got[14][0].tolist() == [2, 2, 4, 4, -1, -1, -1]      # a duplicate as the successor: the lowest of them
    assert got[15][0].tolist() == [1, 3, 4, -1, -1]             # 99 beats 102; from 99, 198 (1 off) beats 201 (2 off)


def test_the_candidate_rule_bin_by_bin():
    c = R.Cfg(pmin=100, pmax=111, W=1, detect=50, min_pulses=4)
    #     k    0  1  2  3  4  5  6  7  8  9 10 11
    C_ = [9, 9, 2, 5, 5, 5, 1, 3, 0, 4, 6, 6]
    span = 1000           # floor(1000 / tau) = 10 .. 9 pairs: half of them is 5
    want = {0: True,      # no left neighbour: 9 > 0, 9 >= 9, S = 18
            1: False,     # not above its left neighbour (a plateau is taken at its first bin)
            2: False, 3: True,   # 5 > 2, 5 >= 5, S = 12
            4: False, 5: False,  # the rest of the plateau
            6: False,
            7: False,     # a peak, but S = 4 < 5
            8: False,
            9: False,     # 4 > 0 but 4 < 6
            10: True,     # 6 > 4, 6 >= 6, S = 16
            11: False}    # no right neighbour, but not above the left one
    for k, yes in want.items():
        assert R.is_candidate(C_, c, span, k) == yes, k
    assert [k for k, _, _ in R.candidates(C_, c, span)] == [0, 3, 10]
    assert R.candidates(C_, c, span)[1] == (3, 103, 12)
    # the last bin with no right neighbour, the only bin with neither
    assert R.is_candidate([0, 0, 7], R.Cfg(100, 102, detect=1, min_pulses=4), 50, 2)
    one = R.Cfg(100, 100, detect=1, min_pulses=4)
    assert R.is_candidate([3], one, 50, 0) and not R.is_candidate([2], one, 50, 0)      # min_pulses - 1
    # the span's share: 30 % of floor(10^6 / 102) = 9803 pairs is 2941 (rounded up from 2940.9)
    share = R.Cfg(100, 104, W=5, detect=30, min_pulses=4)
    assert share.tau(0) == 102 and R.needed(share, 10 ** 6, 0) == 2941
    assert R.is_candidate([2941], share, 10 ** 6, 0) and not R.is_candidate([2940], share, 10 ** 6, 0)
    assert R.needed(share, (1 << 62) - 1, 0) == -(-(((1 << 62) - 1) // 102) * 30 // 100)           # no 64-bit wrap


# -- the arguments -----------------------------------------------------------------------------------------------------
GOOD = dict(min_period=400, max_period=8000, bin_ticks=4, max_level=16, detect_percent=30, min_pulses=8, max_missing=4,
            tolerance=5, fill_percent=50, max_emitters=64, flags=0, device_id=-1)


def config(size=None, **kw):
    return L.PfbDeintConfig(C.sizeof(L.PfbDeintConfig) if size is None else size, **{**GOOD, **kw})


def both(n=0, **kw):
    """the status of pfb_deint_describe and of pfb_deint_create for one config, their outputs untouched on failure"""
    lib = L.load()
    cfg = config(**kw)
    plan, h = L.PfbDeintPlan(), C.c_void_p()
    C.memset(C.byref(plan), 0x5a, C.sizeof(plan))
    d = lib.pfb_deint_describe(C.byref(cfg), n, C.byref(plan))
    c = lib.pfb_deint_create(C.byref(cfg), C.byref(h))
    assert d == L.PFB_OK or bytes(plan) == b"\x5a" * C.sizeof(plan)
    assert not h.value or c == L.PFB_OK
    if h.value:
        lib.pfb_deint_destroy(h)
    return d, c


def test_arguments_are_checked_before_the_device_and_in_order():
    lib = L.load()
    BAD = L.PFB_ERR_BAD_ARG
    plan, h = L.PfbDeintPlan(), C.c_void_p()
    cfg = config()
    assert lib.pfb_deint_describe(None, 0, C.byref(plan)) == lib.pfb_deint_describe(C.byref(cfg), 0, None) == BAD
    assert lib.pfb_deint_create(None, C.byref(h)) == lib.pfb_deint_create(C.byref(cfg), None) == BAD
    # one case per refusal, in the header's order
    bad = [dict(size=48), dict(size=56),
           dict(min_period=0), dict(max_period=399), dict(max_period=(1 << 31) + 1), dict(bin_ticks=0),
           dict(min_period=1000, max_period=1000 + 65536, bin_ticks=1),                       # 65537 bins
           dict(max_level=0), dict(max_level=257), dict(detect_percent=0), dict(detect_percent=101),
           dict(min_pulses=2), dict(min_pulses=(1 << 20) + 1), dict(max_missing=9),
           dict(tolerance=37), dict(tolerance=0, bin_ticks=37), dict(min_period=55, max_missing=4, tolerance=5),  # e (2X + 3) >= pmin
           dict(fill_percent=0), dict(fill_percent=101), dict(max_emitters=0), dict(max_emitters=1025),
           dict(flags=1), dict(flags=1 << 31)]
    for kw in bad:
        assert both(**kw) == (BAD, BAD), kw
        assert both(**{"device_id": 1 << 20, **kw}) == (BAD, BAD), kw    # before the device is looked at
    # each earlier refusal wins over a later one: the order is observable only through both being refused, so walk
    # the list pairwise and see that no later mistake rescues an earlier one
    for first, second in zip(bad[2:-1], bad[3:]):
        if not set(first) & set(second):
            assert both(**first, **second) == (BAD, BAD)
    # the limits themselves pass describe
    for kw in (dict(min_period=1000, max_period=1000 + 65535, bin_ticks=1), dict(max_period=1 << 31, bin_ticks=1 << 15),
               dict(max_level=256), dict(max_level=1), dict(min_pulses=3), dict(min_pulses=1 << 20), dict(max_missing=8, tolerance=21),
               dict(max_missing=0), dict(tolerance=36), dict(min_period=56, max_missing=4, tolerance=5), dict(fill_percent=1),
               dict(fill_percent=100), dict(max_emitters=1), dict(max_emitters=1024), dict(min_period=4, max_period=4, bin_ticks=1, max_missing=0, tolerance=1)):
        assert lib.pfb_deint_describe(C.byref(config(**kw)), 1 << 20, C.byref(plan)) == L.PFB_OK, kw
    assert lib.pfb_deint_describe(C.byref(cfg), (1 << 20) + 1, C.byref(plan)) == BAD
    # null handles and pointers
    buf = np.zeros(64, np.uint64)
    p = C.c_void_p(buf.ctypes.data)
    u = C.c_uint64(7)
    st = L.PfbDeintStats()
    assert lib.pfb_deint_destroy(None) == lib.pfb_deint_sync(None) == lib.pfb_deint_set_stream(None, None) == BAD
    assert lib.pfb_deint_get_device(None, None) == lib.pfb_deint_get_stats(None, C.byref(st)) == BAD
    for mem in (L.PFB_MEM_HOST, L.PFB_MEM_DEVICE, 2):
        assert lib.pfb_deint_run(None, p, 8, mem, p, 1, C.byref(u), p) == BAD and u.value == 7
        assert lib.pfb_deint_histogram(None, p, 8, mem, p, 64) == lib.pfb_deint_successors(None, p, 8, mem, 100, p, p, p) == BAD
    assert lib.pfb_deint_last_kernel(None) == b"" and lib.pfb_deint_set_tier(None, 0, 0) == BAD
    assert not buf.any()
    with pytest.raises(ValueError):
        di.describe_deinterleaver(-1, 100)
    with pytest.raises(ValueError):
        di.describe_deinterleaver(100, 1 << 32)


def test_a_valid_config_needs_a_device():
    if L.load().pfb_device_count() > 0:
        pytest.skip("a GPU is present")
    assert both() == (L.PFB_OK, L.PFB_ERR_NO_DEVICE)
    with pytest.raises(L.PfbError) as e:
        di.Deinterleaver(400, 8000, 4)
    assert e.value.status == L.PFB_ERR_NO_DEVICE
    with pytest.raises(L.PfbError) as e:
        di.deinterleave(DC.train(100, 20), 50, 400)
    assert e.value.status == L.PFB_ERR_NO_DEVICE


def test_describe():
    for nb, name in ((1, "lds"), (DC.LDS_BINS, "lds"), (DC.LDS_BINS + 1, "global"), (65536, "global")):
        plan = di.describe_deinterleaver(1000, 1000 + nb - 1, 1, num_pulses=5000, tolerance=5)
        assert (plan.num_bins, plan.lds_bins, plan.tile_pulses, plan.successor_threads) == (nb, DC.LDS_BINS, DC.TILE, DC.GROUP)
        assert plan.histogram_kernel.decode() == "pfb_deint_hist_" + name
        assert plan.successor_kernel == b"pfb_deint_succ" and plan.marking_kernel == b"pfb_deint_mark_tables"
        assert plan.lds_bytes == (DC.TILE + 256) * 8 + (DC.LDS_BINS * 4 if name == "lds" else 4) <= 64 << 10
    small, big = (di.describe_deinterleaver(400, 8000, 4, num_pulses=n).scratch_bytes for n in (1, 1 << 20))
    # 68 bytes a pulse, the histogram and the counts, and 20 kept jump tables of 4 bytes a pulse for the marking pass
    assert small < 1 << 20 and 148 << 20 <= big <= 150 << 20
    assert di.describe_deinterleaver(400, 8000, 4, num_pulses=1024).scratch_bytes == small
    # the carving, to the byte: the sizes before the scratch was carved through the shared carver
    c = DC.SMALL
    got = tuple(di.describe_deinterleaver(c.pmin, c.pmax, c.W, num_pulses=n, **c.settings()).scratch_bytes
                for n in (0, 1, 1024, 1025, 1 << 20))
    assert got == (157440, 157440, 157440, 308992, 155195136), got


def test_exports():
    lib = L.load()
    declared = {n for n in declared_symbols() if n.startswith("pfb_deint_")}
    assert declared == DEINT_EXPORTS == {n for n in L.EXPORTS if n.startswith("pfb_deint_")}
    for name in DEINT_EXPORTS:
        assert hasattr(lib, name), name
    assert (C.sizeof(L.PfbDeintConfig), C.sizeof(L.PfbDeintPlan), C.sizeof(L.PfbDeintEmitter), C.sizeof(L.PfbDeintStats)) \
        == (52, 128, 48, 32)
    assert di.EMITTER_DTYPE == R.EMITTER and di.EMITTER_DTYPE.itemsize == 48
    for (name, _), (cname, _) in zip(di.EMITTER_DTYPE.descr, L.PfbDeintEmitter._fields_):
        assert name == cname and di.EMITTER_DTYPE.fields[name][1] == getattr(L.PfbDeintEmitter, cname).offset
    hdr = open(os.path.join(ROOT, "include", "pfb_channelizer.h")).read()
    assert "#define PFB_ABI_VERSION 2" in hdr and lib.pfb_abi_version() == 2
    assert hdr.index("pfb_deint_describe(") > hdr.index("pfb_oscfar_last_kernel(")   # its own section, at the end
    assert "THE SAME CALL TWICE, AND HOST AND DEVICE INPUT, GIVE THE SAME BYTES" in hdr
    import sdr_channelizer_amd as pkg
    names = ["Deinterleaver", "deinterleave", "deinterleave_pdws", "deinterleave_detections", "merge_emitters",
             "describe_deinterleaver", "ticks_from_toa", "EMITTER_DTYPE"]
    at = pkg.__all__.index("OsCfar")
    assert pkg.__all__[at - len(names):at] == names
    for name in names:
        assert getattr(pkg, name) is getattr(di, name)


def test_the_struct_layouts_are_the_compilers(tmp_path):
    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.skip("no gcc")
    lines, want = [], []
    for cname, cls in (("pfb_deint_config", L.PfbDeintConfig), ("pfb_deint_plan", L.PfbDeintPlan),
                       ("pfb_deint_emitter", L.PfbDeintEmitter), ("pfb_deint_stats", L.PfbDeintStats)):
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


def test_deint_entry_points_sit_under_the_abi_guard():
    src = open(os.path.join(ROOT, "sdr_channelizer_amd", "csrc", "pfb_deint.hip")).read()
    found = {}
    for m in re.finditer(r'^extern "C" int (\w+)\(', src, re.M):
        rest = src[m.start():]
        found[m.group(1)] = rest[: rest.index("\n}\n")]
    assert set(found) == (DEINT_EXPORTS - {"pfb_deint_last_kernel"}) | {"pfb_deint_set_tier"}   # the dev header's switch
    for name, body in found.items():
        assert "abi_guard" in body.split("{", 1)[1][:80], name
    from sdr_channelizer_amd import build
    assert "pfb_deint.hip" in build.SOURCES
    code = re.sub(r"//.*", "", src)
    assert "atomicAdd(" in code and "float" not in code.replace("std::isfinite", "")     # integer atomics only


# -- pfb_deint_ticks_from_toa ------------------------------------------------------------------------------------------
def test_ticks_from_toa():
    lib = L.load()
    # to nearest, ties to even; a stable sort: equal ticks keep the caller's order
    toa = np.array([10.5, 3.49, 2.5, 3.5, 0.0, 3.51, 1.5, 2.49], np.float64)
    ticks, order = di.ticks_from_toa(toa, 1.0)
    assert ticks.tolist() == [0, 2, 2, 2, 3, 4, 4, 10] and order.tolist() == [4, 2, 6, 7, 1, 3, 5, 0]
    want = R.ticks_from_toa(toa, 0.0, 1.0)
    assert ticks.tobytes() == want[0].tobytes() and order.tobytes() == want[1].tobytes()
    rng = np.random.default_rng(2)
    toa = 1e-3 + rng.random(5000) * 0.05
    for rate, t0 in ((56e6, 1e-3), (1e9, 0.0), (1.0, 0.0), (3.3e7, -2.0)):
        got, want = di.ticks_from_toa(toa, rate, t0), R.ticks_from_toa(toa, t0, rate)
        assert got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes()
        assert (np.diff(got[0].astype(np.int64)) >= 0).all() and sorted(got[1].tolist()) == list(range(5000))
    # the stride walks a pfb_pdw array's toa field in place
    pdws = np.zeros(300, PDW_DTYPE)
    pdws["toa"] = rng.permutation(300) * 1e-5
    pdws["freq"] = 1e9
    got, want = di.ticks_from_toa(pdws, 1e6), R.ticks_from_toa(pdws["toa"], 0.0, 1e6)
    assert got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes()
    assert got[0].tolist() == [10 * k for k in range(300)]
    # the refusals: nothing is written
    BAD = L.PFB_ERR_BAD_ARG
    t, o = np.full(4, 77, np.uint64), np.full(4, 77, np.uint32)
    tp, op = C.c_void_p(t.ctypes.data), C.c_void_p(o.ctypes.data)

    def call(values, stride=8, t0=0.0, rate=1.0, n=None, tp=tp, op=op):
        a = np.array(values, np.float64)
        return lib.pfb_deint_ticks_from_toa(C.c_void_p(a.ctypes.data), stride, len(a) if n is None else n, t0, rate, tp, op)

    ok = [1.0, 2.0, 3.0, 4.0]
    assert call(ok, tp=None) == call(ok, op=None) == call(ok, stride=7) == call(ok, stride=0) == BAD
    assert lib.pfb_deint_ticks_from_toa(None, 8, 4, 0.0, 1.0, tp, op) == BAD and call(ok, n=(1 << 31) + 1) == BAD
    for rate in (0.0, -1.0, np.inf, np.nan):
        assert call(ok, rate=rate) == BAD
    assert call(ok, t0=np.nan) == call(ok, t0=np.inf) == BAD
    for v in (np.nan, np.inf, -np.inf, -0.51, float(1 << 62), 1e30):
        assert call([1.0, 2.0, v, 4.0]) == BAD, v
    assert (t == 77).all() and (o == 77).all()
    assert call([1.0, -0.5, 0.4, float((1 << 62) - 1024)]) == L.PFB_OK       # -0.5 rounds to 0
    assert t.tolist() == [0, 0, 1, (1 << 62) - 1024] and o.tolist() == [1, 2, 0, 3]
    assert lib.pfb_deint_ticks_from_toa(None, 8, 0, 0.0, 1.0, None, None) == L.PFB_OK


# -- merge_emitters ----------------------------------------------------------------------------------------------------
def emitter(first, period, pulses, periods=None, first_pulse=0):
    periods = pulses - 1 if periods is None else periods
    r = np.zeros((), di.EMITTER_DTYPE)
    r["first_tick"], r["last_tick"] = first, first + round(period * periods)
    r["period"] = (int(r["last_tick"]) - first) / periods
    r["pulses"], r["periods"], r["first_pulse"] = pulses, periods, first_pulse
    return r


def test_merge_emitters():
    rec = np.array([emitter(1000, 2048, 50, first_pulse=3),          # 0: a train ...
                    emitter(77, 3000, 40, first_pulse=0),            # 1
                    emitter(1000 + 2048 * 49 + 2048 * 7 + 3, 2048, 30, first_pulse=200),   # 2: ... that went on after 7 periods
                    emitter(500, 2048, 60, first_pulse=1),           # 3: the same period, but overlapping 0 in time
                    emitter(90, 6000, 12, first_pulse=2),            # 4: twice the period of 1: a remainder
                    emitter(1000 + 2048 * 200 + 1024, 2048, 20, first_pulse=400)])   # 5: half a period out of step
    labels = np.array([0, 1, 3, 0, 2, 2, -1, 4, 5, 1, 3], np.int32)
    out, lab, rem = di.merge_emitters(rec, labels, rel_tol=1e-3, tolerance=1.0)
    assert len(out) == 5 and lab.tolist() == [0, 1, 2, 0, 0, 0, -1, 3, 4, 1, 2]
    m = out[0]
    assert (m["first_tick"], m["last_tick"], m["first_pulse"]) == (1000, rec[2]["last_tick"], 3)
    assert (m["pulses"], m["periods"]) == (80, 49 + 29 + 7) and m["period"] == (int(m["last_tick"]) - 1000) / 85
    assert [bytes(out[k]) for k in (1, 2, 3, 4)] == [bytes(rec[k]) for k in (1, 3, 4, 5)]
    assert rem.tolist() == [-1, -1, -1, 1, -1]
    # 3 ticks late after 7 periods passes at one tick a period; it does not at a third of one
    assert len(di.merge_emitters(rec, labels, 1e-3, 0.3)[0]) == 6
    # periods that differ by more than rel_tol are two emitters
    far = np.array([emitter(0, 2048, 50), emitter(2048 * 60, 2052, 50)])
    assert len(di.merge_emitters(far, np.zeros(0, np.int32), 1e-3)[0]) == 2
    assert len(di.merge_emitters(far, np.zeros(0, np.int32), 3e-3, 250.0)[0]) == 1
    empty = di.merge_emitters(np.zeros(0, di.EMITTER_DTYPE), np.array([-1, -1], np.int32))
    assert len(empty[0]) == 0 and empty[1].tolist() == [-1, -1] and len(empty[2]) == 0


# -- the designed scene, on the restatement alone ----------------------------------------------------------------------
def test_the_designed_scene():
    """four trains, four records: what test_gpu_deint.py compares the device against is first shown to be a clean
    separation, with room under every condition"""
    t, who = DC.scene()
    assert 2900 <= len(t) <= 3300 and (np.diff(t.astype(np.int64)) >= 0).all()
    rec, labels, stats = DC.expected("scene")
    rows, strays = DC.quality(who, rec, labels)
    for e, (top, purity, share) in enumerate(rows):
        print("record %d: candidate %d, period %.3f, %d pulses, train %d, purity %.4f, recovered %.4f"
              % (e, rec[e]["candidate_period"], rec[e]["period"], rec[e]["pulses"], top, purity, share))
    print("strays assigned: %d of %d; %s" % (strays, DC.SCENE_STRAYS, stats))
    assert len(rec) == 4 and sorted(top for top, _, _ in rows) == [0, 1, 2, 3]
    assert all(purity >= 0.98 for _, purity, _ in rows) and all(share >= 0.90 for _, _, share in rows)
    assert strays <= 0.05 * DC.SCENE_STRAYS
    assert min(purity for _, purity, _ in rows) >= 0.99 and min(share for _, _, share in rows) >= 0.95   # the room
    for (top, _, _), r in zip(rows, rec):
        assert abs(r["period"] - DC.SCENE_TRAINS[top][0]) < 0.01
    assert stats["pulses_assigned"] == int((labels >= 0).sum()) == int(rec["pulses"].sum())
    assert stats["candidates_tried"] - stats["candidates_refused"] == 4 and stats["rounds"] == 5


def test_without_the_fill_rule_a_sub_period_is_extracted():
    """fill_percent = 1 is no rule to speak of: 1200 ticks, two fifths of the 3000-tick period, strings that train's
    pulses together through the miss windows, five periods a hit, record after record"""
    t, who = DC.scene()
    rec, labels, _ = DC.expected("scene_no_fill")
    assert len(rec) > 4
    sub = rec[np.abs(rec["period"] - 1200) < 2]
    assert len(sub) >= 1 and rec[0]["candidate_period"] == 1202
    assert (100 * (sub["pulses"].astype(np.int64) - 1) < 50 * sub["periods"]).all()      # what 50 % refuses
    mine = who[labels == 0]
    assert (mine == 1).mean() >= 0.8                                                    # pulses of the 3000-tick train
    # the same candidate is tried and refused with the rule
    assert DC.expected("scene")[2]["candidates_refused"] >= 1 and not (np.abs(DC.expected("scene")[0]["period"] - 1200) < 2).any()


def test_twice_the_period_is_a_candidate_but_the_period_comes_first():
    t, _ = DC.scene()
    c = DC.SCENE
    C_ = R.histogram(t, c)
    span = int(t[-1]) - int(t[0])
    ks = [k for k, _, _ in R.candidates(C_, c, span)]
    k1, k2 = (2048 - c.pmin) // c.W, (4096 - c.pmin) // c.W
    assert k1 in ks and k2 in ks and ks.index(k1) < ks.index(k2)
    rec = DC.expected("scene")[0]
    assert rec[0]["bin"] == k1 and not (np.abs(rec["period"] - 4096) < 8).any()
