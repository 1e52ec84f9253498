"""The PDW association without a GPU: the numpy restatement (assoc_ref) against the literal double loop with a
union-find, the designed inputs of assoc_cases proven on the restatement alone, every argument check that comes before
the device and their order, the struct layouts, the exports, pfb_assoc_items_from_pdws, and -- with the float64 oracle --
the scene that the unit is for: a channelized chirp and edge tone, many rows a pulse, one group a pulse."""
import ctypes as C
import importlib
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import assoc_cases as AC
import assoc_ref as R
from abi_symbols import declared_symbols
from sdr_channelizer_amd import _lib as L
from sdr_channelizer_amd.pdw import PDW_DTYPE

# the module, not the function of the same name that the package exports
am = importlib.import_module("sdr_channelizer_amd.associate")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ASSOC_EXPORTS = {"pfb_assoc_describe", "pfb_assoc_create", "pfb_assoc_destroy", "pfb_assoc_set_stream", "pfb_assoc_sync",
                 "pfb_assoc_get_device", "pfb_assoc_run", "pfb_assoc_links", "pfb_assoc_last_kernel", "pfb_assoc_get_stats",
                 "pfb_assoc_items_from_pdws"}


# -- the definition ----------------------------------------------------------------------------------------------------
def same_as_literal(it, c):
    rec, labels, stats = R.run(it, c)
    lit_rec, lit_labels, lit_stats = R.literal_run(it, c)
    assert labels.tobytes() == lit_labels.tobytes() and stats == lit_stats, (it, c)
    assert len(rec) == len(lit_rec)
    for got, want in zip(rec, lit_rec):
        assert {k: int(got[k]) for k in R.GROUP.names} == want
    pairs, clipped = R.literal_edges(it, c)
    a, b, cl = R.edges(it, c)
    assert list(zip(a.tolist(), b.tolist())) == pairs and cl.tolist() == clipped
    first, count = R.links(it, c)
    for i in range(len(it)):
        mine = [j for k, j in pairs if k == i]
        assert (first[i], count[i]) == (min(mine, default=-1), len(mine))


@pytest.mark.parametrize("seed", range(6))
def test_restatement_is_the_literal_loops_on_random_lists(seed):
    for n, K, Rc, g, span in ((0, 3, 1, 0, 1), (1, 3, 1, 0, 1), (2, 1, 0, 0, 1), (40, 1, 1, 0, 2), (90, 5, 0, 3, 3),
                              (120, 200, 2, 1, 1), (150, 7, 1, 0, 8), (60, 4, 64, 50, 4)):
        same_as_literal(*AC.random_list(100 * seed + n, n, K=K, Rc=Rc, g=g, span=span))


@pytest.mark.parametrize("name", [n for n in sorted(AC.CASES) if "window" not in n])
def test_the_designed_lists_on_the_literal_loops(name):
    it, c = AC.inputs(name)
    assert R.acceptable(it, c)
    if len(it) <= 3 * AC.TILE + 1:
        same_as_literal(it, c)


def test_what_each_designed_list_is_there_for():
    E = AC.expected
    assert [E(n)[2]["groups"] for n in ("n_0", "n_1", "n_2", "n_2_apart")] == [0, 1, 1, 2]
    # a link at distance exactly K, none at K + 1, where the window and not the time ended the search
    for at, over, K in (("k1_at_1", "k1_at_2", 1), ("k7_at_7", "k7_at_8", 7),
                        ("lds_window_at_k", "lds_window_at_k_plus_1", AC.LDS_WINDOW),
                        ("global_window_at_k", "global_window_at_k_plus_1", AC.LDS_WINDOW + 1)):
        rec, labels, stats, (first, count) = E(at)
        assert (first[0], count[0], labels[K], stats["edges"], rec[0]["members"]) == (K, 1, 0, 1, 2) and len(labels) == K + 1
        rec, labels, stats, (first, count) = E(over)
        assert (first[0], count[0], labels[K + 1], stats["edges"], stats["largest_group"]) == (-1, 0, K + 1, 0, 1)
        assert stats["clipped"] >= 1 and R.edges(*AC.inputs(over))[2][0]
    assert AC.inputs("window_4096")[1].K == 4096 and E("window_4096")[2]["edges"] == 1
    for g in ("0", "large"):
        assert E("slack_%s_at" % g)[2]["groups"] == 1 and E("slack_%s_over" % g)[2]["groups"] == 2
    assert E("cells_at_reach")[2]["groups"] == 3 and E("cells_over_reach")[2]["groups"] == 6
    assert E("cells_extreme")[2]["groups"] == 3 and E("cells_extreme")[1].tolist() == [0, 1, 0, 2]
    assert E("reach_0_split_pulse")[1].tolist() == [0, 0, 1, 2]
    n = 3 * AC.TILE + 1
    rec, labels, stats, (first, count) = E("staircase")
    assert stats == dict(groups=1, edges=n - 1, clipped=0, largest_group=n, linked_items=n)
    assert first.tolist() == list(range(1, n)) + [-1] and count.tolist() == [1] * (n - 1) + [0]
    rec, labels, stats, (first, count) = E("star")
    assert stats["groups"] == 1 and stats["edges"] == 300 == count[0] and not count[1:].any() and rec[0]["best_item"] == 0
    assert (rec[0]["cell_lo"], rec[0]["cell_hi"], rec[0]["best_cell"]) == (-64, 64, 0)
    rec, labels, stats, _ = E("duplicates")
    assert rec["members"].tolist() == [5, 3, 4] and rec["best_item"].tolist() == [0, 5, 8] and stats["edges"] == 10 + 3 + 6
    rec, labels, stats, _ = E("full_range")
    assert rec["members"].tolist() == [2, 3, 5] and rec[2]["length_sum"] == 4 * ((1 << 32) - 1) > 1 << 33
    assert rec[2]["end_tick"] == (1 << 62) - (1 << 33) - 1 + (1 << 32) - 1 and rec[1]["first_tick"] == 1 << 61
    for name in ("tile_less_1", "tile", "tile_plus_1", "tiles_3_plus_1", "random_dense", "random_sparse"):
        assert 1 < E(name)[2]["groups"] < len(AC.inputs(name)[0]) and E(name)[2]["linked_items"] > 0


def test_the_weights_follow_the_key_order():
    it, c = AC.inputs("weights")
    keys = R.weight_key(it["weight"]).tolist()
    bits = it["weight"].view(np.uint32)
    assert bits[13] == 0xffc00000 or bits[13] == 0xffffffff or (bits[13] >> 31 == 1 and np.isnan(it["weight"][13]))   # -NaN kept its sign
    ordered = np.array([-np.inf, -3e38, -1.0, -1e-45, -0.0, 0.0, 1e-45, 1.0, 3e38, np.inf], np.float32)
    k = R.weight_key(ordered).astype(np.int64)
    assert (np.diff(k) > 0).all()
    assert R.weight_key(np.array([np.nan], np.float32))[0] > k[-1] and keys[13] < k[0]
    rec = AC.expected("weights")[0]
    # ties to the lowest index; -0 under +0; +NaN over +Inf; -NaN under -Inf; a denormal over 0
    assert rec["members"].tolist() == [3, 2, 2, 2, 2, 2, 2, 3, 3, 2]
    assert (rec["best_item"] - rec["first_item"]).tolist() == [0, 1, 0, 1, 1, 0, 1, 0, 1, 0]


def test_the_backward_pulls_need_three_synchronous_rounds():
    it, c = AC.inputs("backward")
    a, b, _ = R.edges(it, c)
    m = 40
    assert len(a) == 2 * (m - 1) and (b >= m).all() and (a < b).all()          # no edge among the first m items
    lab, rounds = R.components(len(it), a, b)
    assert not lab.any() and rounds >= 3
    # after the first round the later odd cells still hold their own labels: the minimum has not gone backwards yet
    one = np.arange(len(it))
    np.minimum.at(one, np.maximum(one[a], one[b]), np.minimum(one[a], one[b]))
    assert one[:m].tolist() == list(range(m)) and one[m:].tolist() == list(range(m - 1))


def test_the_scene_is_one_group_a_pulse():
    it, who = AC.scene(40 * 25)
    assert len(it) == 1000 and R.acceptable(it, AC.SCENE)
    for c in (AC.SCENE, R.Cfg(1, 1, 8), R.Cfg(2, 0, 8), R.Cfg(2, 1, 16)):
        rec, labels, stats = R.run(it, c)
        assert labels.tolist() == who.tolist() and rec["members"].tolist() == [AC.CHIRP_ROWS, AC.TONE_ROWS] * 40
        assert ((rec["end_tick"] - rec["first_tick"]) == AC.PULSE).all() and (rec["first_tick"] == np.arange(80) * AC.PRI).all()
        assert rec["best_cell"][0::2].tolist() == [33] * 40 and rec["best_cell"][1::2].tolist() == [20, 21] * 20
    assert R.run(it, R.Cfg(0, 0, 8))[2]["groups"] == 1000
    assert R.run(it, AC.SCENE)[2]["clipped"] > 0          # the tone's full rows reach past 8 items


# -- the arguments -----------------------------------------------------------------------------------------------------
GOOD = dict(cell_reach=1, slack_ticks=0, window_items=64, flags=0, device_id=-1)


def config(size=None, **kw):
    return L.PfbAssocConfig(C.sizeof(L.PfbAssocConfig) if size is None else size, **{**GOOD, **kw})


def both(n=0, **kw):
    """the status of pfb_assoc_describe and of pfb_assoc_create for one config, their outputs untouched on failure"""
    lib = L.load()
    cfg = config(**kw)
    plan, h = L.PfbAssocPlan(), C.c_void_p()
    C.memset(C.byref(plan), 0x5a, C.sizeof(plan))
    d = lib.pfb_assoc_describe(C.byref(cfg), n, C.byref(plan))
    c = lib.pfb_assoc_create(C.byref(cfg), C.byref(h))
    assert d == L.PFB_OK or bytes(plan) == b"\x5a" * C.sizeof(plan)
    assert not h.value or c == L.PFB_OK
    if h.value:
        lib.pfb_assoc_destroy(h)
    return d, c


def test_arguments_are_checked_before_the_device_and_in_order():
    lib = L.load()
    BAD = L.PFB_ERR_BAD_ARG
    plan, h = L.PfbAssocPlan(), C.c_void_p()
    cfg = config()
    assert lib.pfb_assoc_describe(None, 0, C.byref(plan)) == lib.pfb_assoc_describe(C.byref(cfg), 0, None) == BAD
    assert lib.pfb_assoc_create(None, C.byref(h)) == lib.pfb_assoc_create(C.byref(cfg), None) == BAD
    # one case per refusal, in the header's order
    bad = [dict(size=20), dict(size=28), dict(cell_reach=65), dict(cell_reach=1 << 31), dict(slack_ticks=1 << 31),
           dict(window_items=0), dict(window_items=4097), dict(flags=1), dict(flags=1 << 31)]
    for kw in bad:
        assert both(**kw) == (BAD, BAD), kw
        assert both(**{"device_id": 1 << 20, **kw}) == (BAD, BAD), kw    # before the device is looked at
    for first, second in zip(bad[2:-1], bad[3:]):
        if not set(first) & set(second):
            assert both(**first, **second) == (BAD, BAD)
    for kw in (dict(cell_reach=0), dict(cell_reach=64), dict(slack_ticks=(1 << 31) - 1), dict(window_items=1),
               dict(window_items=4096)):
        assert lib.pfb_assoc_describe(C.byref(config(**kw)), 1 << 20, C.byref(plan)) == L.PFB_OK, kw
    assert lib.pfb_assoc_describe(C.byref(cfg), (1 << 20) + 1, C.byref(plan)) == BAD
    # null handles and pointers
    buf = np.zeros(64, np.uint64)
    p = C.c_void_p(buf.ctypes.data)
    u = C.c_uint64(7)
    st = L.PfbAssocStats()
    assert lib.pfb_assoc_destroy(None) == lib.pfb_assoc_sync(None) == lib.pfb_assoc_set_stream(None, None) == BAD
    assert lib.pfb_assoc_get_device(None, None) == lib.pfb_assoc_get_stats(None, C.byref(st)) == BAD
    for mem in (L.PFB_MEM_HOST, L.PFB_MEM_DEVICE, 2):
        assert lib.pfb_assoc_run(None, p, 8, mem, p, 1, C.byref(u), p) == BAD and u.value == 7
        assert lib.pfb_assoc_links(None, p, 8, mem, p, p) == BAD
    assert lib.pfb_assoc_last_kernel(None) == b"" and lib.pfb_assoc_set_tier(None, 0) == BAD
    assert not buf.any()
    with pytest.raises(ValueError):
        am.describe_associator(-1)
    with pytest.raises(ValueError):
        am.describe_associator(1, 1 << 32)


def test_a_valid_config_needs_a_device():
    if L.load().pfb_device_count() > 0:
        pytest.skip("a GPU is present")
    assert both() == (L.PFB_OK, L.PFB_ERR_NO_DEVICE)
    with pytest.raises(L.PfbError) as e:
        am.PulseAssociator()
    assert e.value.status == L.PFB_ERR_NO_DEVICE
    with pytest.raises(L.PfbError) as e:
        am.associate(AC.scene(50)[0])
    assert e.value.status == L.PFB_ERR_NO_DEVICE


def test_describe():
    for K, name in ((1, "lds"), (AC.LDS_WINDOW, "lds"), (AC.LDS_WINDOW + 1, "global"), (4096, "global")):
        plan = am.describe_associator(1, 0, K, num_items=5000)
        assert (plan.tile_items, plan.lds_window) == (AC.TILE, AC.LDS_WINDOW)
        assert plan.link_kernel.decode() == "pfb_assoc_link_" + name
        assert plan.component_kernel == b"pfb_assoc_hook" and plan.record_kernel == b"pfb_assoc_gather"
        # start and cell of the tile and the K + 1 behind it at the tier's bound (in whole 16 bytes), end + g of the tile
        assert plan.lds_bytes == ((AC.TILE + AC.LDS_WINDOW + 4) * 12 + AC.TILE * 8 if name == "lds" else 0) <= 64 << 10
    small, big = (am.describe_associator(num_items=n).scratch_bytes for n in (1, 1 << 20))
    assert small < 1 << 20 and 156 << 20 <= big <= 157 << 20         # 156 bytes an item
    assert am.describe_associator(num_items=1024).scratch_bytes == small
    # the carving, to the byte: the sizes before the scratch was carved through the shared carver
    got = tuple(am.describe_associator(num_items=n).scratch_bytes for n in (0, 1, 1024, 1025, 1 << 20))
    assert got == (164352, 164352, 164352, 324096, 163582464), got


def test_exports():
    lib = L.load()
    declared = {n for n in declared_symbols() if n.startswith("pfb_assoc_")}
    assert declared == ASSOC_EXPORTS == {n for n in L.EXPORTS if n.startswith("pfb_assoc_")}
    assert "pfb_assoc_set_tier" in L.DEV_EXPORTS and "pfb_assoc_set_tier" in declared_symbols(("pfb_channelizer_dev.h",))
    for name in ASSOC_EXPORTS | {"pfb_assoc_set_tier"}:
        assert hasattr(lib, name), name
    at = L.EXPORTS.index("pfb_assoc_describe")
    assert L.EXPORTS[at - 1].startswith("pfb_regrid_") and L.EXPORTS[at + len(ASSOC_EXPORTS)] == "pfb_rdcfar_describe"
    assert (C.sizeof(L.PfbAssocItem), C.sizeof(L.PfbAssocConfig), C.sizeof(L.PfbAssocPlan), C.sizeof(L.PfbAssocGroup),
            C.sizeof(L.PfbAssocStats)) == (24, 24, 120, 48, 48)
    for dtype, ref, cls in ((am.ASSOC_ITEM_DTYPE, R.ITEM, L.PfbAssocItem), (am.GROUP_DTYPE, R.GROUP, L.PfbAssocGroup)):
        assert dtype == ref and dtype.itemsize == C.sizeof(cls)
        for (name, _), (cname, _) in zip(dtype.descr, cls._fields_):
            assert name == cname and dtype.fields[name][1] == getattr(cls, cname).offset
    assert am.STATS_FIELDS == R.STATS + ("rounds",) == tuple(n for n, _ in L.PfbAssocStats._fields_)
    hdr = open(os.path.join(ROOT, "include", "pfb_channelizer.h")).read()
    assert "#define PFB_ABI_VERSION 2" in hdr and lib.pfb_abi_version() == 2
    assert hdr.index("pfb_assoc_describe(") > hdr.index("pfb_regrid_doppler_frequencies(")   # its own section, at the end
    import sdr_channelizer_amd as pkg
    names = ["PulseAssociator", "associate", "associate_pdws", "fuse_pdws", "describe_associator", "ASSOC_ITEM_DTYPE",
             "GROUP_DTYPE"]
    at = pkg.__all__.index("ChannelSynthesizer")
    assert pkg.__all__[at - len(names):at] == names
    for name in names:
        assert getattr(pkg, name) is getattr(am, name)


def test_the_struct_layouts_are_the_compilers(tmp_path):
    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.skip("no gcc")
    lines, want = [], []
    for cname, cls in (("pfb_assoc_item", L.PfbAssocItem), ("pfb_assoc_config", L.PfbAssocConfig),
                       ("pfb_assoc_plan", L.PfbAssocPlan), ("pfb_assoc_group", L.PfbAssocGroup),
                       ("pfb_assoc_stats", L.PfbAssocStats)):
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


def test_assoc_entry_points_sit_under_the_abi_guard():
    src = open(os.path.join(ROOT, "sdr_channelizer_amd", "csrc", "pfb_assoc.hip")).read()
    found = {}
    for m in re.finditer(r'^extern "C" int (\w+)\(', src, re.M):
        rest = src[m.start():]
        found[m.group(1)] = rest[: rest.index("\n}\n")]
    assert set(found) == (ASSOC_EXPORTS - {"pfb_assoc_last_kernel"}) | {"pfb_assoc_set_tier"}   # the dev header's switch
    for name, body in found.items():
        assert "abi_guard" in body.split("{", 1)[1][:80], name
    from sdr_channelizer_amd import build
    assert "pfb_assoc.hip" in build.SOURCES
    code = re.sub(r"//.*", "", src)
    assert "atomicMin(" in code and "atomicAdd(" in code
    for call in re.findall(r"atomic\w+\(&a\.(?:ctl->)?(\w+)", code):            # integer atomics only
        assert call in ("bad", "edges", "clipped", "largest", "linked", "label", "acc_end", "acc_sum", "acc_best",
                        "acc_members", "acc_lo", "acc_hi"), call
    assert len(re.findall(r"\bfloat\b", code)) == 1                           # the item's weight, when a PDW becomes one


# -- pfb_assoc_items_from_pdws -----------------------------------------------------------------------------------------
def test_items_from_pdws():
    lib = L.load()
    rng = np.random.default_rng(5)
    pdws = np.zeros(400, PDW_DTYPE)
    pdws["toa"] = 2.0 + rng.integers(0, 100, 400) * 1e-6 + rng.random(400) * 1e-7
    pdws["pw"] = rng.integers(0, 50, 400) * 0.5e-6             # halves of a tick: ties to even
    pdws["bin"] = rng.integers(-3, 56, 400)
    pdws["mag"] = rng.random(400) * 10 - 1
    pdws["freq"], pdws["snr"], pdws["sat"] = 1e9, 20.0, 1
    for rate, t0 in ((1e6, 2.0), (56e6, 1.0), (1.0, 0.0)):
        got, want = am.items_from_pdws(pdws, rate, t0), R.items_from_pdws(pdws, t0, rate)
        assert got[0].dtype == am.ASSOC_ITEM_DTYPE and got[0].tobytes() == want[0].tobytes()
        assert got[1].tobytes() == want[1].tobytes() and sorted(got[1].tolist()) == list(range(400))
        assert (np.diff(got[0]["start"].astype(np.int64)) >= 0).all() and not got[0]["reserved"].any()
    it, order = am.items_from_pdws(pdws, 1e6, 2.0)
    assert (it["cell"] == pdws["bin"][order]).all() and (it["weight"] == pdws["mag"][order].astype(np.float32)).all()
    assert len(set(it["start"].tolist())) < 400                # equal starts: the sort's stability was exercised
    # the refusals: nothing is written
    BAD = L.PFB_ERR_BAD_ARG
    items, o = np.full(4 * 24, 0x5a, np.uint8), np.full(4, 77, np.uint32)
    ip, op = C.c_void_p(items.ctypes.data), C.c_void_p(o.ctypes.data)

    def call(toa=(1.0, 2.0, 3.0, 4.0), pw=(1.0, 1.0, 1.0, 1.0), t0=0.0, rate=1.0, n=None, ip=ip, op=op):
        p = np.zeros(4, PDW_DTYPE)
        p["toa"], p["pw"] = toa, pw
        return lib.pfb_assoc_items_from_pdws(C.c_void_p(p.ctypes.data), 4 if n is None else n, t0, rate, ip, op)

    assert call(ip=None) == call(op=None) == call(n=(1 << 31) + 1) == BAD
    assert lib.pfb_assoc_items_from_pdws(None, 4, 0.0, 1.0, ip, op) == BAD
    for rate in (0.0, -1.0, np.inf, np.nan):
        assert call(rate=rate) == BAD
    assert call(t0=np.nan) == call(t0=np.inf) == BAD
    for v in (np.nan, np.inf, -np.inf, -0.51, float(1 << 62), 1e30):
        assert call(toa=(1.0, 2.0, v, 4.0)) == BAD, v
    for v in (np.nan, np.inf, -0.51, float(1 << 32), 1e30):
        assert call(pw=(1.0, 2.0, v, 4.0)) == BAD, v
    assert (items == 0x5a).all() and (o == 77).all()
    assert call(toa=(1.0, -0.5, 0.4, float((1 << 62) - 1024)), pw=(0.5, 1.5, 2.5, float((1 << 32) - 1))) == L.PFB_OK
    got = items.view(am.ASSOC_ITEM_DTYPE)
    assert got["start"].tolist() == [0, 0, 1, (1 << 62) - 1024] and o.tolist() == [1, 2, 0, 3]
    assert got["length"].tolist() == [2, 2, 0, (1 << 32) - 1]
    assert lib.pfb_assoc_items_from_pdws(None, 0, 0.0, 1.0, None, None) == L.PFB_OK


# -- what the unit is for, measured with the oracle --------------------------------------------------------------------
def motivating_scene(oracle):
    """15 pulses of 2240 samples, PRI 22 400, through the float64 oracle's 56-channel bank and extractor: the even
    pulses sweep 5 MHz around +3 MHz, the odd ones are a tone at -7.5 MHz, the edge of two channels"""
    from oracle.pfb_oracle import OracleConfig
    M, P, fs, pulses, pw, pri = 56, 12, 56e6, 15, 2240, 22400
    rng = np.random.default_rng(7)
    n = pulses * pri + pri // 2
    x = 0.003 * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
    t = np.arange(pw) / fs
    first = [pri // 4 + k * pri for k in range(pulses)]
    for k, at in enumerate(first):
        if k % 2 == 0:
            f0, rate = 3e6 - 2.5e6, 5e6 / (pw / fs)
            x[at:at + pw] += 0.3 * np.exp(2j * np.pi * (f0 * t + 0.5 * rate * t * t))
        else:
            x[at:at + pw] += 0.3 * np.exp(2j * np.pi * -7.5e6 * t)
    h = oracle.design_prototype(M, P)
    y = oracle.channelize(x, h, OracleConfig(M, P, M, fftshift=True), "polyphase")
    found = oracle.extract_pdws(y, fs, 0.0, 0.0, snr_db=15.0, matlab_quirks=False)
    pdws = np.zeros(len(found), PDW_DTYPE)
    for name in PDW_DTYPE.names:
        pdws[name] = [f[name] for f in found]
    return pdws, np.array(first) / M, pw / M, fs / M


def test_the_motivating_scene_with_the_oracle(oracle):
    pdws, first_frame, frames, rate = motivating_scene(oracle)
    print("%d PDWs for %d pulses" % (len(pdws), len(first_frame)))
    assert len(pdws) > 5 * len(first_frame)                    # the extractor's table is several rows a pulse
    it, order = R.items_from_pdws(pdws, 0.0, rate)
    for c in (R.Cfg(1, 0, 64), R.Cfg(1, 1, 64), R.Cfg(2, 0, 64)):
        rec, labels, stats = R.run(it, c)
        print(c, stats, rec["members"].tolist(), rec["best_cell"].tolist())
        assert len(rec) == len(first_frame) and stats["clipped"] == 0
        # each group spans its pulse: within the bank's rise and fall, P frames at either end
        assert (np.abs(rec["first_tick"].astype(np.int64) - first_frame) <= 12).all()
        assert (np.abs(rec["end_tick"].astype(np.int64) - (first_frame + frames)) <= 12).all()
        assert (rec["members"] >= 2).all()
        assert len(set(rec["best_cell"][1::2].tolist()) - {20, 21}) == 0      # -7.5 MHz: the edge of columns 20 and 21
        assert (np.abs(rec["best_cell"][0::2].astype(int) - 31) <= 3).all()   # +3 MHz is column 31
    assert R.run(it, R.Cfg(0, 0, 64))[2]["edges"] == 0 and R.run(it, R.Cfg(0, 0, 64))[2]["groups"] == len(pdws)
