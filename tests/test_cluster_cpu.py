"""The PDW clustering without a GPU: the numpy restatement (cluster_ref) against the literal loops over cells with a
union-find, the designed inputs of cluster_cases proven on the restatement alone, every argument check that comes before
the device and their order, the struct layouts, the exports, pfb_cluster_items_from_pdws, and -- on the restatements of
this unit and of the deinterleaver -- the scene that the unit is for: 32 trains in one list, one cluster a train, one
candidate a cluster."""
import ctypes as C
import os
import re
import shutil
import subprocess
import sys
import time

import numpy as np
import pytest

import cluster_cases as CC
import cluster_ref as R
import deint_ref as DR
from abi_symbols import declared_symbols
from sdr_channelizer_amd import _lib as L
from sdr_channelizer_amd import cluster as cm
from sdr_channelizer_amd.pdw import PDW_DTYPE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLUSTER_EXPORTS = {"pfb_cluster_" + n for n in (
    "describe", "create", "destroy", "set_stream", "sync", "get_device", "run", "histogram", "cell_roots", "gather",
    "last_kernel", "get_stats", "items_from_pdws")}


# -- the definition ----------------------------------------------------------------------------------------------------
def same_as_literal(it, c):
    rec, labels, order, offsets, stats, G = R.run(it, c)
    lit_rec, lit_labels, lit_stats, lit_root = R.literal_run(it, c)
    H = R.histogram(it, c)
    assert labels.tobytes() == lit_labels.tobytes(), (it, c)
    assert R.cell_roots(H, c)[0].tobytes() == lit_root.tobytes()
    assert stats.pop("hook_rounds") == R.literal_rounds(H.tolist(), c)
    assert stats == lit_stats and G == len(lit_rec) == len(rec)
    for got, want in zip(rec, lit_rec):
        assert {k: int(got[k]) for k in R.GROUP.names} == want
    # the stable order
    key = np.where(labels < 0, G, labels)
    assert order.tobytes() == np.argsort(key, kind="stable").astype(np.uint32).tobytes()
    assert sorted(order.tolist()) == list(range(len(it))) and offsets[G + 1] == len(it) and offsets[0] == 0
    for k in range(G + 1):
        mine = order[offsets[k]:offsets[k + 1]]
        assert (np.diff(mine.astype(np.int64)) > 0).all() and (key[mine] == k).all()


@pytest.mark.parametrize("seed", range(6))
def test_restatement_is_the_literal_loops_on_random_grids(seed):
    for n, c in ((0, R.Cfg(3, 3)), (1, R.Cfg(1, 1, 0, 0)), (60, R.Cfg(9, 7, 1, 1, minc=2)), (200, R.Cfg(12, 5, 2, 1, minc=3, minp=9, border=True)),
                 (150, R.Cfg(30, 1, 3, 0, minc=2, border=True)), (120, R.Cfg(1, 25, 0, 2, minp=4)), (300, R.Cfg(10, 10, 8, 8, minc=4, border=True)),
                 (250, R.Cfg(16, 16, 0, 0, minc=2, minp=3, border=True)), (90, R.Cfg(20, 4, 1, 0, minc=1, minp=5))):
        same_as_literal(CC.random_list(100 * seed + n, n, c, blobs=5, stray=0.3), c)


@pytest.mark.parametrize("name", sorted(CC.CASES))
def test_the_designed_lists_on_the_literal_loops(name):
    it, c = CC.inputs(name)
    if c.cells <= 1600 and len(it) <= 2400:
        same_as_literal(it, c)


def test_what_each_designed_list_is_there_for():
    E = CC.expected
    assert [E(n)[5] for n in ("n_0", "n_1", "n_2")] == [0, 1, 2]
    assert E("n_0")[3].tolist() == [0, 0] and E("n_0")[4] == dict.fromkeys(R.STATS, 0)
    assert E("grid_1x1")[1].tolist() == [0, 0, -1, -1, -1] and E("grid_1x1")[4]["outside"] == 3
    # item counts around the tiles, every list with items outside the grid
    for name, tile in (("hist", CC.HIST_TILE), ("label", CC.LABEL_TILE), ("part", CC.PART_TILE)):
        assert [len(CC.inputs("%s_tile_%s" % (name, t))[0]) for t in ("less_1", "at", "plus_1", "two_plus_1")] == \
            [tile - 1, tile, tile + 1, 2 * tile + 1]
    for name in CC.CASES:
        if "_tile_" in name:
            assert E(name)[5] >= 1 and E(name)[4]["outside"] > 0
    # the grids at the tier's bound
    assert CC.inputs("grid_lds_bound")[1].cells == CC.inputs("grid_lds_bound_1d")[1].cells == CC.LDS_CELLS
    assert CC.inputs("grid_over_lds_bound")[1].cells == CC.LDS_CELLS + 1
    assert CC.inputs("grid_17_wide")[1].V == 17                     # one over the widest block of the component kernels
    # reach: joined at the reach, apart one over it, in u, in v and diagonally
    for axis in ("u", "v", "diag"):
        assert E("reach_%s_at" % axis)[5] < E("reach_%s_over" % axis)[5]
    assert (E("reach_u_at")[5], E("reach_u_over")[5], E("reach_v_at")[5], E("reach_v_over")[5]) == (1, 2, 1, 2)
    assert E("reach_diag_at")[0]["cells"].tolist() == [3] and E("reach_diag_over")[5] == 4
    assert E("reach_0")[5] == 4 and E("reach_0")[0]["cells"].tolist() == [1, 1, 1, 1]
    # the widest reach, down and to either side: (0,0)-(8,8)-(16,0) and (31,31)-(39,39); (25,0) is 9 rows under (16,0)
    rec = E("reach_8")[0]
    assert rec["cells"].tolist() == [3, 1, 1, 2]
    assert (rec["root_u"].tolist(), rec["root_v"].tolist()) == ([0, 16, 25, 31], [0, 17, 0, 31])
    # min_cell_count at c - 1 and c
    rec, labels, _, _, stats, G = E("min_cell_count")
    assert G == 1 and stats["dense_cells"] == 1 and stats["unassigned"] == 4 and rec["pulses"].tolist() == [5]
    # min_pulses at p - 1 and p, the numbering closes the gap: five components with 10, 9, 10, 2 and 2 pulses
    rec, labels, _, offsets, stats, G = E("min_pulses")
    assert stats["components"] == 5 and G == 2 and rec["pulses"].tolist() == [10, 10] and stats["unassigned"] == 13
    assert rec["root_u"].tolist() == [1, 15] and offsets.tolist() == [0, 10, 20, 33]
    # the border cell between two components joins the lower root, which is not its lowest dense neighbour; it bridges nothing
    it, c = CC.inputs("border_lowest_root")
    rec, labels, _, _, stats, G = E("border_lowest_root")
    roots = R.cell_roots(R.histogram(it, c), c)[0].reshape(c.U, c.V)
    assert G == stats["components"] == 2 and stats["border_cells"] == 1 and roots[2, 4] == 5 == roots[2, 5] and roots[2, 3] == 19
    assert rec["pulses"].tolist() == [12, 5] and rec["cells"].tolist() == [4, 1] and rec["v_min"].tolist() == [4, 3]
    assert stats["unassigned"] == 1                                   # the lone item at (6, 1): no dense cell in reach
    rec, labels, _, _, stats, G = E("border_off")
    assert G == 2 and stats["border_cells"] == 0 and stats["unassigned"] == 3 and rec["pulses"].tolist() == [10, 5]
    # outside on every side, and the int32 limits
    rec, labels, _, offsets, stats, G = E("outside")
    assert stats["outside"] == 12 and G == 2 and labels[4:].tolist() == [-1] * 12 and offsets.tolist() == [0, 2, 4, 16]
    # one cell: the wave-combining path
    rec = E("one_cell")[0]
    assert rec["peak_count"].tolist() == [5000] == rec["pulses"].tolist() and rec["cells"].tolist() == [1]
    assert int(E("sum_past_2_32")[0]["sum_u"][0]) == 5000 * ((1 << 20) - 1) > 1 << 32
    # the components that need many rounds
    for name, rounds in (("serpentine", 6), ("comb", 7)):
        rec, _, _, _, stats, G = E(name)
        assert G == 1 == stats["components"] and stats["hook_rounds"] == rounds > 3 and CC.inputs(name)[1].cells == 64 * 64
        assert rec["pulses"][0] == len(CC.inputs(name)[0]) == stats["dense_cells"]
    # the radix passes: one for G + 1 <= 256
    for G, passes in ((254, 1), (255, 1), (256, 2), (257, 2), (65535, 2)):
        got = E("isolated_%d" % G)
        assert got[5] == G and (1 if G + 1 <= 256 else 2) == passes and got[4]["unassigned"] == 0 and got[4]["outside"] == 2
        assert got[3][G:].tolist() == [G, G + 2]
    assert E("isolated_65536")[5] == 65536 and E("isolated_65536")[0] is None
    assert R.run(*CC.inputs("isolated_257"), capacity=256)[:2] == (None, None)
    # the alternating labels
    it, c = CC.inputs("alternating")
    rec, labels, order, offsets, stats, G = E("alternating")
    assert labels[:8].tolist() == [0, 1, 2, -1, 0, 1, 2, -1] and len(it) > 2 * CC.PART_TILE and G == 3
    assert order[:3].tolist() == [0, 4, 8] and order[offsets[3]:offsets[3] + 2].tolist() == [3, 7]
    rec = E("duplicates")[0]
    assert rec["pulses"].tolist() == [160, 120] and rec["first_item"].tolist() == [0, 2]


def test_the_big_list_is_what_it_is_for():
    it, c = CC.big()
    assert len(it) == 1 << 20 and (c.U, c.V) == (1024, 1024)


# -- the arguments -----------------------------------------------------------------------------------------------------
GOOD = dict(cells_u=64, cells_v=4, reach_u=1, reach_v=0, min_cell_count=1, min_pulses=1, flags=0, device_id=-1)


def config(size=None, **kw):
    return L.PfbClusterConfig(C.sizeof(L.PfbClusterConfig) if size is None else size, **{**GOOD, **kw})


def both(n=0, **kw):
    """the status of pfb_cluster_describe and of pfb_cluster_create for one config, their outputs untouched on failure"""
    lib = L.load()
    cfg = config(**kw)
    plan, h = L.PfbClusterPlan(), C.c_void_p()
    C.memset(C.byref(plan), 0x5a, C.sizeof(plan))
    d = lib.pfb_cluster_describe(C.byref(cfg), n, C.byref(plan))
    c = lib.pfb_cluster_create(C.byref(cfg), C.byref(h))
    assert d == L.PFB_OK or bytes(plan) == b"\x5a" * C.sizeof(plan)
    assert not h.value or c == L.PFB_OK
    if h.value:
        lib.pfb_cluster_destroy(h)
    return d, c


def test_arguments_are_checked_before_the_device_and_in_order():
    lib = L.load()
    BAD = L.PFB_ERR_BAD_ARG
    plan, h = L.PfbClusterPlan(), C.c_void_p()
    cfg = config()
    assert lib.pfb_cluster_describe(None, 0, C.byref(plan)) == lib.pfb_cluster_describe(C.byref(cfg), 0, None) == BAD
    assert lib.pfb_cluster_create(None, C.byref(h)) == lib.pfb_cluster_create(C.byref(cfg), None) == BAD
    # one case per refusal, in the header's order
    bad = [dict(size=32), dict(size=40), dict(cells_u=0), dict(cells_v=0), dict(cells_u=1 << 11, cells_v=(1 << 9) + 1),
           dict(cells_u=1 << 31, cells_v=1 << 31), dict(reach_u=9), dict(reach_v=9), dict(min_cell_count=0),
           dict(min_cell_count=(1 << 20) + 1), dict(min_pulses=0), dict(min_pulses=(1 << 20) + 1), dict(flags=2),
           dict(flags=3), dict(flags=1 << 31)]
    for kw in bad:
        assert both(**kw) == (BAD, BAD), kw
        assert both(**{"device_id": 1 << 20, **kw}) == (BAD, BAD), kw    # before the device is looked at
    for first, second in zip(bad[2:-1], bad[3:]):
        if not set(first) & set(second):
            assert both(**first, **second) == (BAD, BAD)
    for kw in (dict(cells_u=1, cells_v=1), dict(cells_u=1 << 20, cells_v=1), dict(cells_u=1, cells_v=1 << 20),
               dict(cells_u=1024, cells_v=1024), dict(reach_u=0), dict(reach_u=8, reach_v=8), dict(min_cell_count=1 << 20),
               dict(min_pulses=1 << 20), dict(flags=1)):
        assert lib.pfb_cluster_describe(C.byref(config(**kw)), 1 << 20, C.byref(plan)) == L.PFB_OK, kw
    assert lib.pfb_cluster_describe(C.byref(cfg), (1 << 20) + 1, C.byref(plan)) == BAD
    # null handles and pointers
    buf = np.zeros(64, np.uint64)
    p = C.c_void_p(buf.ctypes.data)
    u = C.c_uint64(7)
    st = L.PfbClusterStats()
    assert lib.pfb_cluster_destroy(None) == lib.pfb_cluster_sync(None) == lib.pfb_cluster_set_stream(None, None) == BAD
    assert lib.pfb_cluster_get_device(None, None) == lib.pfb_cluster_get_stats(None, C.byref(st)) == BAD
    for mem in (L.PFB_MEM_HOST, L.PFB_MEM_DEVICE, 2):
        assert lib.pfb_cluster_run(None, p, 8, mem, p, 1, C.byref(u), p, p, p) == BAD and u.value == 7
        assert lib.pfb_cluster_histogram(None, p, 8, mem, p, 1 << 20) == BAD
        assert lib.pfb_cluster_cell_roots(None, p, 8, mem, p, 1 << 20) == BAD
    assert lib.pfb_cluster_gather(None, p, 8, p, 8, p) == BAD
    assert lib.pfb_cluster_last_kernel(None) == b"" and lib.pfb_cluster_set_tier(None, 0) == BAD
    assert not buf.any()
    with pytest.raises(ValueError):
        cm.describe_clusterer(-1)
    with pytest.raises(ValueError):
        cm.describe_clusterer(4, 1 << 32)


def test_a_valid_config_needs_a_device():
    if L.load().pfb_device_count() > 0:
        pytest.skip("a GPU is present")
    assert both() == (L.PFB_OK, L.PFB_ERR_NO_DEVICE)
    with pytest.raises(L.PfbError) as e:
        cm.PulseClusterer(8)
    assert e.value.status == L.PFB_ERR_NO_DEVICE
    with pytest.raises(L.PfbError) as e:
        cm.cluster_pulses(np.arange(5))
    assert e.value.status == L.PFB_ERR_NO_DEVICE


def test_describe():
    for (U, V), name, block in (((1, 1), "lds", (256, 1)), ((CC.LDS_CELLS, 1), "lds", (256, 1)), ((128, 64), "lds", (16, 16)),
                                ((CC.LDS_CELLS + 1, 1), "global", (256, 1)), ((1024, 1024), "global", (16, 16)),
                                ((100, 2), "lds", (128, 2)), ((100, 3), "lds", (64, 4)), ((50, 17), "lds", (16, 16)),
                                ((5, 8), "lds", (32, 8))):
        plan = cm.describe_clusterer(U, V, num_items=5000)
        assert (plan.hist_tile, plan.label_tile, plan.part_tile, plan.lds_cells) == (CC.HIST_TILE, CC.LABEL_TILE, CC.PART_TILE, CC.LDS_CELLS)
        assert plan.cells == U * V and plan.max_clusters == 65535 and (plan.block_u, plan.block_v) == block
        assert plan.histogram_kernel.decode() == "pfb_cluster_hist_" + name
        assert plan.component_kernel == b"pfb_cluster_hook" and plan.partition_kernel == b"pfb_cluster_part1"
        assert plan.lds_bytes == (CC.LDS_CELLS * 4 if name == "lds" else 0) <= 64 << 10
        # the halo the component kernel stages fits its static array for every reach
        assert (plan.block_u + 16) * (plan.block_v + 16) <= 4624
    small, big = (cm.describe_clusterer(1024, 1024, num_items=n).scratch_bytes for n in (1, 1 << 20))
    assert big - small == ((1 << 20) - 1024) * (8 + 4 + 4 + 4 + 1) and 56 << 20 < small < 70 << 20   # 52 bytes a cell and the slots
    assert cm.describe_clusterer(1024, 1024, num_items=1024).scratch_bytes == small
    # the carving, to the byte: the sizes before the scratch was carved through the shared carver
    for (U, V), want in (((64, 1), (308992, 308992, 308992, 330496, 22307584)),
                         ((1024, 8), (1435392, 1435392, 1435392, 1456896, 23433984)),
                         ((1024, 1024), (60581632, 60581632, 60581632, 60603136, 82580224))):
        got = tuple(cm.describe_clusterer(U, V, num_items=n).scratch_bytes for n in (0, 1, 1024, 1025, 1 << 20))
        assert got == want, (U, V, got)


def test_exports():
    lib = L.load()
    declared = {n for n in declared_symbols() if n.startswith("pfb_cluster_")}
    assert declared == CLUSTER_EXPORTS == {n for n in L.EXPORTS if n.startswith("pfb_cluster_")}
    assert "pfb_cluster_set_tier" in L.DEV_EXPORTS and "pfb_cluster_set_tier" in declared_symbols(("pfb_channelizer_dev.h",))
    for name in CLUSTER_EXPORTS | {"pfb_cluster_set_tier"}:
        assert hasattr(lib, name), name
    assert (C.sizeof(L.PfbClusterItem), C.sizeof(L.PfbClusterConfig), C.sizeof(L.PfbClusterPlan), C.sizeof(L.PfbClusterGroup),
            C.sizeof(L.PfbClusterStats)) == (8, 36, 144, 64, 48)
    for dtype, ref, cls in ((cm.CLUSTER_ITEM_DTYPE, R.ITEM, L.PfbClusterItem), (cm.CLUSTER_GROUP_DTYPE, R.GROUP, L.PfbClusterGroup)):
        assert dtype == ref and dtype.itemsize == C.sizeof(cls)
        for (name, _), (cname, _) in zip(dtype.descr, cls._fields_):
            assert name == cname and dtype.fields[name][1] == getattr(cls, cname).offset
    assert cm.STATS_FIELDS == R.STATS == tuple(n for n, _ in L.PfbClusterStats._fields_)
    hdr = open(os.path.join(ROOT, "include", "pfb_channelizer.h")).read()
    assert "#define PFB_ABI_VERSION 2" in hdr and lib.pfb_abi_version() == 2
    assert hdr.index("pfb_cluster_describe(") > hdr.index("pfb_assoc_items_from_pdws(")     # its own section, at the end
    assert "#define PFB_CLUSTER_BORDER 1u" in hdr and cm.BORDER == 1
    assert "pfb_cluster_* splits the list first" in hdr and "(that is pfb_cluster_*)" in hdr  # the two "Not built" lines
    import sdr_channelizer_amd as pkg
    names = ["PulseClusterer", "cluster_pulses", "cluster_pdws", "cluster_items_from_pdws", "describe_clusterer",
             "deinterleave_clustered", "deinterleave_clustered_figures", "CLUSTER_ITEM_DTYPE", "CLUSTER_GROUP_DTYPE"]
    at = pkg.__all__.index("PulseAssociator")
    assert pkg.__all__[at - len(names):at] == names
    for name in names:
        assert getattr(pkg, name) is getattr(cm, name.replace("cluster_items_from_pdws", "items_from_pdws"))


def test_the_struct_layouts_are_the_compilers(tmp_path):
    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.skip("no gcc")
    lines, want = [], []
    for cname, cls in (("pfb_cluster_item", L.PfbClusterItem), ("pfb_cluster_config", L.PfbClusterConfig),
                       ("pfb_cluster_plan", L.PfbClusterPlan), ("pfb_cluster_group", L.PfbClusterGroup),
                       ("pfb_cluster_stats", L.PfbClusterStats)):
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


def test_cluster_entry_points_sit_under_the_abi_guard():
    src = open(os.path.join(ROOT, "sdr_channelizer_amd", "csrc", "pfb_cluster.hip")).read()
    found = {}
    for m in re.finditer(r'^extern "C" int (\w+)\(', src, re.M):
        rest = src[m.start():]
        found[m.group(1)] = rest[: rest.index("\n}\n")]
    assert set(found) == (CLUSTER_EXPORTS - {"pfb_cluster_last_kernel"}) | {"pfb_cluster_set_tier"}   # the dev header's switch
    for name, body in found.items():
        assert "abi_guard" in body.split("{", 1)[1][:80], name
    from sdr_channelizer_amd import build
    assert "pfb_cluster.hip" in build.SOURCES
    code = re.sub(r"//.*", "", src)
    device = re.sub(r"//.*", "", src[:src.index("// host:")])
    assert "__global__" in device and "__global__" not in re.sub(r"//.*", "", src[src.index("// host:"):])
    assert "atomicMin(" in device and "atomicAdd(" in device and "__ballot(" in device
    assert not re.search(r"\b(float|double)\b", device)                       # no float on the device
    assert "rocprim" not in code.lower() and "hipcub" not in code.lower()
    # the same of the device part of the core it includes: the workgroup scan and the scan of the workgroups' counts
    core = open(os.path.join(ROOT, "sdr_channelizer_amd", "csrc", "pfb_list.hpp")).read()
    assert '#include "pfb_list.hpp"' in src
    core_device = re.sub(r"//.*", "", core[:core.index("// host:")])
    assert "block_scan(" in core_device and "void __launch_bounds__(kThreads) list_scan(" in core_device
    assert "__global__" not in re.sub(r"//.*", "", core[core.index("// host:"):])
    assert not re.search(r"\b(float|double)\b", core_device)
    assert "rocprim" not in core.lower() and "hipcub" not in core.lower()
    # the partition ranks with ballots and LDS counts: the only atomic of its three kernels is the tile's digit count
    part = device[device.index("void __launch_bounds__(kThreads) part_scan"):device.index("template <class T>")]
    assert "atomic" not in part


# -- pfb_cluster_items_from_pdws ---------------------------------------------------------------------------------------
def test_items_from_pdws():
    lib = L.load()
    rng = np.random.default_rng(5)
    pdws = np.zeros(400, PDW_DTYPE)
    pdws["freq"] = 1e9 + rng.integers(-40, 400, 400) * 0.25e6 + rng.random(400) * 1e3
    pdws["pw"] = rng.integers(0, 50, 400) * 0.5e-6
    pdws["toa"], pdws["snr"], pdws["sat"], pdws["mag"] = 1.0, 20.0, 1, 2.0
    for f0, fs, ps in ((1e9, 1e6, 0.0), (1e9, 0.25e6, 1e-6), (0.0, 1.0, 0.5e-6), (1.00001e9, 3e5, 7e-7)):
        got, want = cm.items_from_pdws(pdws, fs, ps, f0), R.items_from_pdws(pdws, f0, fs, ps)
        assert got.dtype == cm.CLUSTER_ITEM_DTYPE and got.tobytes() == want.tobytes(), (f0, fs, ps)
        assert (got["v"] == 0).all() == (ps == 0.0)
    assert (cm.items_from_pdws(pdws, 1e6, 0.0, 1e9)["u"] < 0).any()             # floor, not truncation
    # figures that are not finite or do not fit: INT32_MIN, outside every grid
    odd = np.zeros(12, PDW_DTYPE)
    odd["freq"] = [np.nan, np.inf, -np.inf, 2147483647.0, 2147483648.0, -2147483648.0, -2147483649.0, 5.5, -0.5, 7.0, 7.0, 1e300]
    odd["pw"] = [1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, np.nan, np.inf, 2147483648.0, 2147483647.5, 1.0]
    got = cm.items_from_pdws(odd, 1.0, 1.0, 0.0)
    m = CC.I32_MIN
    assert got["u"].tolist() == [m, m, m, CC.I32_MAX, m, m, m, m, m, m, 7, m]
    assert got["v"].tolist() == [0, 0, 0, 1, 0, 1, 0, 0, 0, 0, CC.I32_MAX, 0]
    assert got.tobytes() == R.items_from_pdws(odd, 0.0, 1.0, 1.0).tobytes()
    assert (R.cell_of(got[got["u"] == m], R.Cfg(1 << 20, 1)) == -1).all()
    # a stride: every second PDW of a table
    wide = np.zeros(10, np.dtype([("a", PDW_DTYPE), ("b", PDW_DTYPE)]))
    wide["a"]["freq"], wide["b"]["freq"] = np.arange(10) * 3.0, -1.0
    items = np.zeros(10, cm.CLUSTER_ITEM_DTYPE)
    args = (0.0, 1.0, 0.0, C.c_void_p(items.ctypes.data))
    assert lib.pfb_cluster_items_from_pdws(C.c_void_p(wide.ctypes.data), 10, 2 * PDW_DTYPE.itemsize, *args) == L.PFB_OK
    assert items["u"].tolist() == list(range(0, 30, 3))
    # the refusals: nothing is written
    BAD = L.PFB_ERR_BAD_ARG
    out = np.full(4 * 8, 0x5a, np.uint8)
    four = np.zeros(4, PDW_DTYPE)

    def call(p=four.ctypes.data, n=4, stride=PDW_DTYPE.itemsize, f0=0.0, fs=1.0, ps=0.0, o=out.ctypes.data):
        return lib.pfb_cluster_items_from_pdws(C.c_void_p(p), n, stride, f0, fs, ps, C.c_void_p(o))

    assert call(p=None) == call(o=None) == call(n=(1 << 31) + 1) == BAD
    assert call(stride=PDW_DTYPE.itemsize - 8) == call(stride=PDW_DTYPE.itemsize + 4) == call(stride=0) == BAD
    for v in (np.nan, np.inf, -np.inf):
        assert call(f0=v) == call(fs=v) == call(ps=v) == BAD
    assert call(fs=0.0) == call(fs=-1.0) == call(ps=-1e-9) == BAD
    assert (out == 0x5a).all()
    assert call() == L.PFB_OK and not out.any()
    assert lib.pfb_cluster_items_from_pdws(None, 0, PDW_DTYPE.itemsize, 0.0, 1.0, 0.0, None) == L.PFB_OK


# -- what the unit is for, on the restatements alone -------------------------------------------------------------------
def test_the_motivating_scene_on_the_references():
    """tools/deint_rate.py's 32-train scene at 2^12 pulses.  Measured here: the whole list at W = 4 makes 39 records
    from 2453 candidates (2414 refused); split by cluster, 32 records from 32 candidates, none refused."""
    n, trains = 1 << 12, 32
    ticks, who, periods = CC.scene_with_trains(n, trains, 1)
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import deint_rate
        assert deint_rate.scene(n, trains, 1).tobytes() == ticks.tobytes()     # the meter's scene, tick for tick
    finally:
        sys.path.remove(os.path.join(ROOT, "tools"))
    assert len(periods) == trains and (who >= 0).sum() > 0.97 * n
    items = CC.scene_features(who)
    spread = items["u"][who >= 0] - (CC.SCENE_FIRST + CC.SCENE_PITCH * who[who >= 0])
    assert spread.min() <= -3 and spread.max() >= 3 and len(set(items["u"][who < 0].tolist())) > 60   # a few cells; anywhere
    rec, labels, order, offsets, stats, G = R.run(items, CC.SCENE_CLUSTER)
    # one cluster per train: every train's pulses in one cluster, no cluster with two trains
    assert G == trains
    for k in range(trains):
        mine = labels[who == k]
        assert (mine[mine >= 0] == k).all() and (mine >= 0).mean() > 0.98
    D = CC.SCENE_DEINT
    tried = refused = assigned = 0
    for k in range(G):
        mine = order[offsets[k]:offsets[k + 1]]
        r, sub, st = DR.run(ticks[mine], D)
        assert len(r) == 1 and abs(r[0]["period"] - periods[k]) < 0.05, (k, r, periods[k])   # exactly one emitter, the train's
        assert (who[mine][sub == 0] == k).mean() > 0.97
        tried, refused, assigned = tried + st["candidates_tried"], refused + st["candidates_refused"], assigned + st["pulses_assigned"]
    t0 = time.perf_counter()
    whole_rec, _, whole = DR.run(ticks, D)
    print("whole list: %d records, %d tried, %d refused, %d assigned, %.1f s; by cluster: %d records, %d tried, %d refused, "
          "%d assigned" % (len(whole_rec), whole["candidates_tried"], whole["candidates_refused"], whole["pulses_assigned"],
                           time.perf_counter() - t0, G, tried, refused, assigned))
    assert 10 * tried < whole["candidates_tried"]
    assert (tried, refused) == (trains, 0) and assigned > 0.97 * (who >= 0).sum()


def test_the_chain_case_on_the_references():
    pdws, who, periods = CC.chain_table()
    K = CC.CHAIN_CLUSTER
    cluster = R.Cfg(48, 1, K["reach_u"], K["reach_v"], K["min_cell_count"], K["cluster_min_pulses"], K["border"])
    emitters, labels, clusters, stats = CC.reference_chain(pdws, CC.CHAIN_DEINT, CC.CHAIN_RATE, CC.CHAIN_STEP_HZ,
                                                           CC.CHAIN_FREQ0, 48, cluster)
    assert len(clusters) == len(emitters) == 8 and stats["candidates_tried"] == 8
    assert [k for k, _ in emitters] == list(range(8)) and all(abs(e["period"] - p) < 0.1 for (_, e), p in zip(emitters, periods))
    assert 50 <= min((who == k).sum() for k in range(8)) and max((who == k).sum() for k in range(8)) <= 70
