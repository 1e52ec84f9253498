"""The PDW clustering on the device: labels, records, order, offsets, count, stats, histogram and cell roots against the
numpy restatement (cluster_ref), byte for byte -- over the designed lists of cluster_cases that sit on one sentence of
the definition each, at the tile and tier boundaries, through both histogram tiers, from host and device memory,
between guard bytes, across a stream switch, on one list of 2^20 items, and along the chain the unit is for: a PDW table
clustered by frequency, cut by cluster on the device and deinterleaved one cluster at a time."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import cluster_cases as CC  # noqa: E402
import cluster_ref as R  # noqa: E402
from gpu_support import cuda_torch  # noqa: E402
from sdr_channelizer_amd import PulseClusterer, cluster_pulses, deinterleave_clustered  # noqa: E402
from sdr_channelizer_amd import _lib as L  # noqa: E402
from sdr_channelizer_amd import cluster as cm  # noqa: E402

GUARD = 0x5A
LDS, GLOBAL = "pfb_cluster_hist_lds", "pfb_cluster_hist_global"


@pytest.fixture(scope="module")
def torch():
    return cuda_torch()


def make(c: R.Cfg) -> PulseClusterer:
    return PulseClusterer(**c.settings())


def on_device(torch, it):
    return torch.from_numpy(np.ascontiguousarray(it).view(np.int32).reshape(-1, 2).copy()).cuda()


def host(x):
    return x if isinstance(x, np.ndarray) else x.cpu().numpy()


def check(a, x, it, c, want, what=""):
    """every entry point on one list (x: the items where the call reads them) against the restatement"""
    rec, labels, order, offsets, stats, G = want
    H = a.histogram(x)
    assert H.dtype == np.uint32 and H.shape == (c.U, c.V) and H.tobytes() == R.histogram(it, c).tobytes(), what
    roots = a.cell_roots(x)
    assert roots.dtype == np.int32 and roots.tobytes() == R.cell_roots(R.histogram(it, c), c)[0].tobytes(), what
    got_rec, got_labels, got_order, got_offsets = a.run(x)
    got_rec = cm.groups_to_numpy(got_rec)
    assert got_rec.dtype == cm.CLUSTER_GROUP_DTYPE and len(got_rec) == G == len(rec), (what, len(got_rec), G)
    assert got_rec.tobytes() == rec.tobytes(), (what, got_rec[:4], rec[:4])
    got_labels, got_order, got_offsets = host(got_labels), host(got_order), host(got_offsets)
    assert got_labels.dtype == np.int32 and got_labels.tobytes() == labels.tobytes(), what
    assert got_order.itemsize == 4 and got_order.tobytes() == order.tobytes(), (what, got_order[:16], order[:16])
    assert got_offsets.itemsize == 4 and got_offsets.tobytes() == offsets.tobytes(), (what, got_offsets, offsets)
    assert a.stats == stats, (what, a.stats, stats)
    # order and offsets may be left out together: everything else is the same
    r2, l2, o2, f2 = a.run(x, want_order=False)
    assert o2 is None and f2 is None and cm.groups_to_numpy(r2).tobytes() == rec.tobytes(), what
    assert host(l2).tobytes() == labels.tobytes() and a.stats == stats, what
    assert "pfb_cluster_part" not in a.last_kernel
    return got_rec


# -- the designed lists ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(n for n in CC.CASES if n != "isolated_65536"))
def test_the_designed_lists(torch, name):
    it, c = CC.inputs(name)
    want = CC.expected(name)
    tier = LDS if c.cells <= CC.LDS_CELLS else GLOBAL
    with make(c) as a:
        assert a.last_kernel == "" and a.stats == dict.fromkeys(cm.STATS_FIELDS, 0)
        p = a.plan
        assert (p.hist_tile, p.label_tile, p.part_tile, p.lds_cells) == (CC.HIST_TILE, CC.LABEL_TILE, CC.PART_TILE, CC.LDS_CELLS)
        assert p.histogram_kernel.decode() == tier and p.cells == c.cells
        check(a, it, it, c, want, what=name)
        a.run(it)
        ran = a.last_kernel.split("+")
        if len(it):
            assert ran[0] == tier and ("pfb_cluster_hook" in ran) == ("pfb_cluster_jump" in ran) == (want[4]["dense_cells"] > 0)
            assert ("pfb_cluster_part2" in ran) == (want[5] + 1 > 256) and ("pfb_cluster_part1" in ran) == (want[5] + 1 <= 256)
            assert ("pfb_cluster_emit" in ran) == (want[5] > 0) and "pfb_cluster_label" in ran
        a.histogram(it)
        assert a.last_kernel == (tier if len(it) else "")
        check(a, on_device(torch, it), it, c, want, what=name + " from device memory")
    if name in ("serpentine", "comb"):
        print("%s: %d hook rounds" % (name, want[4]["hook_rounds"]))


def test_both_tiers_give_the_same_bytes(torch):
    lib = L.load()
    for name in ("hist_tile_two_plus_1", "grid_lds_bound", "grid_lds_bound_1d", "one_cell", "alternating"):
        it, c = CC.inputs(name)
        want = CC.expected(name)
        with make(c) as a:
            seen = []
            for tier, kernel in ((0, LDS), (2, GLOBAL), (1, LDS), (2, GLOBAL)):
                assert lib.pfb_cluster_set_tier(a._h, tier) == L.PFB_OK
                seen.append(check(a, it, it, c, want, what=(name, tier)).tobytes())
                a.run(it)
                assert kernel in a.last_kernel.split("+") and (LDS in a.last_kernel) != (GLOBAL in a.last_kernel)
            assert len(set(seen)) == 1
            for bad in (3, -1):
                assert lib.pfb_cluster_set_tier(a._h, bad) == L.PFB_ERR_BAD_ARG
    it, c = CC.inputs("grid_over_lds_bound")
    with make(c) as a:
        assert lib.pfb_cluster_set_tier(a._h, 1) == L.PFB_ERR_UNSUPPORTED        # the LDS tier's bound
        assert lib.pfb_cluster_set_tier(a._h, 2) == L.PFB_OK
        check(a, it, it, c, CC.expected("grid_over_lds_bound"), what="over the LDS tier's bound")


def test_one_cell_takes_the_combining_path():
    it, c = CC.inputs("one_cell")
    with make(c) as a:
        rec = cm.groups_to_numpy(a.run(it)[0])
        assert rec["peak_count"].tolist() == [len(it)] == rec["pulses"].tolist() and rec["first_item"].tolist() == [0]
    it, c = CC.inputs("sum_past_2_32")
    with make(c) as a:
        rec = cm.groups_to_numpy(a.run(it)[0])
        assert int(rec["sum_u"][0]) == 5000 * ((1 << 20) - 1) > 1 << 32


# -- the calls ---------------------------------------------------------------------------------------------------------
def raw_run(a, ptr, n, mem, cap, torch=None, want_order=True):
    """pfb_cluster_run between guard bytes: (status, count, the four buffers as numpy bytes)"""
    lib = L.load()
    sizes = (64 * cap + 128, 4 * n + 128, 4 * n + 128, 4 * (cap + 2) + 128)
    count = C.c_uint64(77)
    if mem == L.PFB_MEM_HOST:
        bufs = [np.full(s, GUARD, np.uint8) for s in sizes]
        at = [b.ctypes.data + 64 for b in bufs]
    else:
        bufs = [torch.full((s,), GUARD, dtype=torch.uint8, device="cuda") for s in sizes]
        at = [b.data_ptr() + 64 for b in bufs]
    if not want_order:
        at[2] = at[3] = None
    rc = lib.pfb_cluster_run(a._h, C.c_void_p(ptr), n, mem, C.c_void_p(at[0]), cap, C.byref(count), C.c_void_p(at[1]),
                             C.c_void_p(at[2]), C.c_void_p(at[3]))
    return rc, count.value, [host(b) for b in bufs]


def inner(buf, nbytes):
    assert (buf[:64] == GUARD).all() and (buf[64 + nbytes:] == GUARD).all()
    return buf[64:64 + nbytes].tobytes()


@pytest.mark.parametrize("mem", ["host", "device"])
def test_guard_bytes_capacity_and_the_refusals(torch, mem):
    it, c = CC.inputs("min_pulses")
    rec, labels, order, offsets, stats, G = CC.expected("min_pulses")
    n = len(it)
    x = on_device(torch, it) if mem == "device" else it
    ptr = x.data_ptr() if mem == "device" else x.ctypes.data
    m = L.PFB_MEM_DEVICE if mem == "device" else L.PFB_MEM_HOST
    with make(c) as a:
        rc, count, bufs = raw_run(a, ptr, n, m, G + 3, torch)
        assert (rc, count) == (L.PFB_OK, G)
        assert inner(bufs[0], 64 * G) == rec.tobytes() and inner(bufs[1], 4 * n) == labels.tobytes()
        assert inner(bufs[2], 4 * n) == order.tobytes() and inner(bufs[3], 4 * (G + 2)) == offsets.tobytes()
        assert a.stats == stats
        # the same call twice
        again = raw_run(a, ptr, n, m, G + 3, torch)
        assert again[:2] == (rc, count) and all(x.tobytes() == y.tobytes() for x, y in zip(again[2], bufs))
        # without order and offsets
        rc, count, bufs = raw_run(a, ptr, n, m, G, torch, want_order=False)
        assert (rc, count) == (L.PFB_OK, G) and inner(bufs[0], 64 * G) == rec.tobytes()
        assert inner(bufs[2], 0) == b"" and inner(bufs[3], 0) == b""
        # a capacity one short: the count, nothing written, the stats of the run before
        other = R.Cfg(c.U, c.V, c.ru, c.rv, c.minc, 1)
        with make(other) as b:
            b.run(x)
            before = b.stats
            G1 = R.run(it, other)[5]
            assert G1 > G
            rc, count, bufs = raw_run(b, ptr, n, m, G1 - 1, torch)
            assert (rc, count) == (L.PFB_ERR_CAPACITY, G1) and all((buf == GUARD).all() for buf in bufs)
            assert b.stats == before
            # the handle grows its room by itself
            b.capacity = 1
            got = b.run(x)
            assert len(got[0]) == G1 == b.capacity
        if mem == "device":
            lib = L.load()
            count = C.c_uint64(77)
            good = [torch.zeros(4096, dtype=torch.uint8, device="cuda") for _ in range(4)]
            base = [g.data_ptr() for g in good]
            for k, off in ((-1, 4), (0, 4), (1, 2), (2, 2), (3, 2)):
                p = list(base)
                items = ptr
                if k < 0:
                    items = ptr + off
                else:
                    p[k] += off
                rc = lib.pfb_cluster_run(a._h, C.c_void_p(items), n - 1, m, C.c_void_p(p[0]), 8, C.byref(count),
                                         C.c_void_p(p[1]), C.c_void_p(p[2]), C.c_void_p(p[3]))
                assert rc == L.PFB_ERR_BAD_ARG and count.value == 77, k
            assert lib.pfb_cluster_histogram(a._h, C.c_void_p(ptr), n, m, C.c_void_p(base[0] + 2), c.cells) == L.PFB_ERR_BAD_ARG
            assert lib.pfb_cluster_cell_roots(a._h, C.c_void_p(ptr + 4), n - 1, m, C.c_void_p(base[0]), c.cells) == L.PFB_ERR_BAD_ARG
            assert lib.pfb_cluster_histogram(a._h, C.c_void_p(ptr), n, m, C.c_void_p(base[0]), c.cells - 1) == L.PFB_ERR_CAPACITY
            assert all(not g.any() for g in good)


def test_more_than_65535_clusters_are_refused(torch):
    it, c = CC.inputs("isolated_65536")
    assert CC.expected("isolated_65536")[5] == 65536
    with make(c) as a:
        for x, m in ((it, L.PFB_MEM_HOST), (on_device(torch, it), L.PFB_MEM_DEVICE)):
            ptr = x.ctypes.data if m == L.PFB_MEM_HOST else x.data_ptr()
            rc, count, bufs = raw_run(a, ptr, len(it), m, 65540, torch)
            assert (rc, count) == (L.PFB_ERR_CAPACITY, 65536) and all((buf == GUARD).all() for buf in bufs)
            assert a.stats == dict.fromkeys(cm.STATS_FIELDS, 0)
        with pytest.raises(L.PfbError) as e:
            a.run(it)
        assert e.value.status == L.PFB_ERR_CAPACITY
        # the grid itself is fine: the counts and roots of all 65536 cells
        assert a.histogram(it).tobytes() == R.histogram(it, c).tobytes()
        assert a.cell_roots(it).reshape(-1).tolist() == list(range(65536))


def test_a_handle_grows_and_a_stream_switch(torch):
    c = R.Cfg(40, 3, 1, 1, minc=2, border=True)
    with make(c) as a:
        for name in ("label_tile_at", "hist_tile_two_plus_1", "part_tile_plus_1", "label_tile_less_1"):
            it, cc = CC.inputs(name)
            assert cc == c
            check(a, it, it, c, CC.expected(name), what=name)
        s = torch.cuda.Stream()
        a.set_stream(s.cuda_stream)
        it, _ = CC.inputs("part_tile_two_plus_1")
        with torch.cuda.stream(s):
            check(a, on_device(torch, it), it, c, CC.expected("part_tile_two_plus_1"), what="on another stream")
        a.set_stream(0)
        check(a, it, it, c, CC.expected("part_tile_two_plus_1"), what="back on the first stream")


def test_gather_with_both_element_sizes(torch):
    it, c = CC.inputs("alternating")
    order = CC.expected("alternating")[2]
    rng = np.random.default_rng(2)
    with make(c) as a:
        d_order = a.run(on_device(torch, it))[2]
        assert host(d_order).tobytes() == order.tobytes()
        for dtype in (np.int32, np.float32, np.int64, np.float64):
            src = (rng.random(len(it)) * 1e6).astype(dtype)
            got = a.gather(torch.from_numpy(src).cuda(), d_order)
            assert a.last_kernel == "pfb_cluster_gather"
            assert host(got).dtype == dtype and host(got).tobytes() == src[order].tobytes()
        # a part of the order, from an offset: what a caller does with one cluster
        got = a.gather(torch.from_numpy(src).cuda(), d_order[5:105].contiguous())
        assert host(got).tobytes() == src[order[5:105]].tobytes()
        lib = L.load()
        src_d, dst_d = torch.zeros(64, dtype=torch.int64, device="cuda"), torch.zeros(64, dtype=torch.int64, device="cuda")
        args = lambda s=0, e=8, o=0, d=0, n=8: (a._h, C.c_void_p(src_d.data_ptr() + s), e, C.c_void_p(d_order.data_ptr() + o), n,  # noqa: E731
                                                C.c_void_p(dst_d.data_ptr() + d))
        for kw in (dict(e=2), dict(e=16), dict(s=4), dict(d=4), dict(o=2), dict(n=(1 << 20) + 1)):
            assert lib.pfb_cluster_gather(*args(**kw)) == L.PFB_ERR_BAD_ARG, kw
        assert lib.pfb_cluster_gather(*args(n=0)) == L.PFB_OK and not dst_d.any()


def test_one_list_of_2_20_items(torch):
    it, c = CC.big()
    want = R.run(it, c)
    assert len(it) == 1 << 20 and c.cells == 1 << 20 and want[5] > 256
    with make(c) as a:
        x = on_device(torch, it)
        got_rec, got_labels, got_order, got_offsets = a.run(x)
        assert cm.groups_to_numpy(got_rec).tobytes() == want[0].tobytes()
        assert host(got_labels).tobytes() == want[1].tobytes() and host(got_order).tobytes() == want[2].tobytes()
        assert host(got_offsets).tobytes() == want[3].tobytes() and a.stats == want[4]
        assert a.last_kernel.split("+")[0] == GLOBAL and "pfb_cluster_part2" in a.last_kernel
        h_rec, h_labels, h_order, h_offsets = a.run(it)
        assert h_rec.tobytes() == want[0].tobytes() and h_order.tobytes() == want[2].tobytes()


def test_cluster_pulses(torch):
    it, c = CC.inputs("grid_17_wide")
    rec, labels, order, offsets, stats, G = CC.expected("grid_17_wide")
    kw = dict(cells_u=c.U, cells_v=c.V, reach_u=c.ru, reach_v=c.rv, min_cell_count=c.minc, min_pulses=c.minp, border=c.border)
    got = cluster_pulses(it["u"], it["v"], **kw)
    assert got[0].tobytes() == rec.tobytes() and got[1].tobytes() == labels.tobytes() and got[2].tobytes() == order.tobytes()
    d = cluster_pulses(torch.from_numpy(it["u"].copy()).cuda(), torch.from_numpy(it["v"].copy()).cuda(), **kw)
    assert d[0].tobytes() == rec.tobytes() and d[1].is_cuda and host(d[1]).tobytes() == labels.tobytes()
    assert host(d[3]).tobytes() == offsets.tobytes()


# -- the chain ---------------------------------------------------------------------------------------------------------
def test_the_chain_on_the_device(torch):
    pdws, who, periods = CC.chain_table()
    D, K = CC.CHAIN_DEINT, CC.CHAIN_CLUSTER
    cells_u = 48
    cluster = R.Cfg(cells_u, 1, K["reach_u"], K["reach_v"], K["min_cell_count"], K["cluster_min_pulses"], K["border"])
    ref_emitters, ref_labels, ref_clusters, ref_stats = CC.reference_chain(pdws, D, CC.CHAIN_RATE, CC.CHAIN_STEP_HZ,
                                                                           CC.CHAIN_FREQ0, cells_u, cluster)
    # the reference's answer first: one cluster and one emitter per train, with the train's period and its pulses
    assert len(ref_clusters) == len(ref_emitters) == len(periods) == 8
    for k, (cl, e) in enumerate(ref_emitters):
        assert cl == k and abs(e["period"] - periods[k]) < 0.1
        mine = ref_labels == k
        assert (who[mine] == k).all() and mine.sum() >= 0.9 * (who == k).sum()
    assert ref_stats["candidates_tried"] == 8 and ref_stats["candidates_refused"] == 0
    emitters, labels, clusters = deinterleave_clustered(pdws, CC.CHAIN_RATE, D.pmin, D.pmax, D.W, freq_step_hz=CC.CHAIN_STEP_HZ,
                                                        freq0=CC.CHAIN_FREQ0, cells_u=cells_u, **K, **D.settings())
    assert labels.dtype == np.int32 and labels.tobytes() == ref_labels.tobytes()
    assert len(emitters) == 8 and emitters["cluster"].tolist() == list(range(8))
    for name in cm.EMITTER_DTYPE.names:
        if name != "first_pulse":
            assert emitters[name].tolist() == [e[name] for _, e in ref_emitters], name
    assert (labels[emitters["first_pulse"]] == np.arange(8)).all()
    for name in R.GROUP.names:
        assert clusters[name].tolist() == ref_clusters[name].tolist(), name
    assert int(clusters["candidates_tried"].sum()) == ref_stats["candidates_tried"]
    assert int(clusters["pulses_assigned"].sum()) == ref_stats["pulses_assigned"] == int((labels >= 0).sum())
    # measured frequencies in place of the table's own
    swapped = pdws.copy()
    swapped["freq"] = 0.0
    e2, l2, c2 = deinterleave_clustered(swapped, CC.CHAIN_RATE, D.pmin, D.pmax, D.W, freq_step_hz=CC.CHAIN_STEP_HZ,
                                        freq0=CC.CHAIN_FREQ0, cells_u=cells_u, freq=pdws["freq"], **K, **D.settings())
    assert l2.tobytes() == labels.tobytes() and e2.tobytes() == emitters.tobytes()
