"""The range-Doppler CFAR detector's contract without a GPU: the numpy restatement (rdcfar_ref) against a literal
per-cell loop, the training counts at the gate edges, the tie rule walked on a small map, the false-alarm rate on the
reference (and what a Hann window does to it: findings, printed), the designed inputs of rdcfar_cases proven on the
reference alone, every argument check that comes before the device, the struct layouts, the exports, the placement in
__all__, and pfb_rdcfar_to_pdw into pfb_event_fit."""
import ctypes as C
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import cfar_ref
import pd_cases
import pd_ref
import rdcfar_cases as K
import rdcfar_ref as R
from abi_symbols import declared_symbols
from sdr_channelizer_amd import _lib as L
from sdr_channelizer_amd import cfar, rd_cfar

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RDCFAR_EXPORTS = {"pfb_rdcfar_describe", "pfb_rdcfar_create", "pfb_rdcfar_destroy", "pfb_rdcfar_reset",
                  "pfb_rdcfar_set_stream", "pfb_rdcfar_sync", "pfb_rdcfar_get_device", "pfb_rdcfar_next_map",
                  "pfb_rdcfar_get_stats", "pfb_rdcfar_process", "pfb_rdcfar_process_async", "pfb_rdcfar_to_pdw",
                  "pfb_rdcfar_last_kernel"}


# -- the definition, cell by cell ---------------------------------------------------
def literal(maps, Wd, Gr, Tr, Pd, method, alpha, min_power, first_map=0):
    """The header text as a triple loop: every cell works its column sums, its noise and its peak box out from scratch."""
    f64, f32 = np.float64, np.float32
    out, n_over, without = [], 0, 0
    with np.errstate(all="ignore"):
        for m, P in enumerate(maps):
            ND, Rg = P.shape

            def A(d, g):
                a = f64(0.0)
                for j in range(-Wd, Wd + 1):
                    a = a + f64(P[(d + j) % ND][g])
                return a

            for d in range(ND):
                for r in range(Rg):
                    lead = [g for g in range(r - Gr - Tr, r - Gr) if g >= 0]
                    lag = [g for g in range(r + Gr + 1, r + Gr + Tr + 1) if g < Rg]
                    sl = sr = f64(0.0)
                    for g in lead:
                        sl = sl + A(d, g)
                    for g in lag:
                        sr = sr + A(d, g)
                    nl, nr, col = len(lead), len(lag), 2 * Wd + 1
                    if nl + nr == 0:
                        without += 1
                        continue
                    if method == R.CA:
                        noise = f32((sl + sr) / f64((nl + nr) * col))
                    else:
                        sides = ([sl / f64(nl * col)] if nl else []) + ([sr / f64(nr * col)] if nr else [])
                        if any(math.isnan(s) for s in sides):
                            noise = f32(np.nan)
                        else:
                            noise = f32(max(sides) if method == R.GO else min(sides))
                    p = P[d][r]
                    if not (bool(p > f32(alpha) * noise) and bool(p > f32(min_power))):
                        continue
                    n_over += 1
                    beaten = False
                    for j in range(-Pd, Pd + 1):
                        qd = (d + j) % ND
                        for g in range(max(r - Gr, 0), min(r + Gr, Rg - 1) + 1):
                            q = P[qd][g]
                            if q > p or (q == p and (qd, g) < (d, r)):
                                beaten = True
                    if not beaten:
                        out.append((first_map + m, d, r, p, noise, (nl + nr) * col, R.ONE_SIDED if nl + nr < 2 * Tr else 0))
    stats = {"maps_in": len(maps), "cells_over": n_over, "cells_without_noise": without, "detections": len(out),
             "dropped": 0}
    return (np.array(out, R.DET) if out else np.zeros(0, R.DET)), stats


@pytest.mark.parametrize("method", [R.CA, R.GO, R.SO])
@pytest.mark.parametrize("Wd,Gr,Tr,Pd", [(0, 0, 1, 0), (1, 1, 2, 1), (1, 2, 3, 0), (2, 0, 4, 2), (0, 5, 2, 1)])
def test_restatement_is_the_definition(method, Wd, Gr, Tr, Pd):
    need = 2 * max(Wd, Pd) + 1
    for seed, (ND, Rg) in enumerate(((1, 1), (1, 17), (3, 7), (5, 23), (6, 12))):
        if ND < need:
            continue
        maps = K.noise_maps(2, ND, Rg, seed, share=0.15, level=40.0)
        if Rg > 10:
            maps[0, ND // 2, 3] = np.nan
            maps[1, 0, 5] = np.inf
            maps[1, ND - 1, 8] = maps[1, ND - 1, 9] = maps[1].max() * 2    # equal neighbours
            maps[0, 0, Rg - 1] = -np.inf
        want, wstats = literal(maps, Wd, Gr, Tr, Pd, method, 3.0, 0.5, 7)
        got, gstats = R.detect(maps, Wd, Gr, Tr, Pd, method, 3.0, 0.5, 7)
        assert got.tobytes() == want.tobytes(), (ND, Rg)
        assert gstats == wstats, (ND, Rg)


def test_training_counts_at_the_gate_edges():
    Gr, Tr, Wd, Rg = 2, 4, 1, 20
    nl, nr = R.counts(Rg, Gr, Tr)
    assert list(nl[:8]) == [0, 0, 0, 1, 2, 3, 4, 4] and list(nr[-8:]) == [4, 4, 3, 2, 1, 0, 0, 0]
    p = np.ones((1, 3, Rg), np.float32)
    p[0, 1, [0, 3, 19]] = 50.0
    det, stats = R.detect(p, Wd, Gr, Tr, 0, R.CA, 4.0)
    assert [(int(d["gate"]), int(d["training_cells"]), int(d["flags"])) for d in det] == [(0, 12, 1), (3, 15, 1), (19, 12, 1)]
    assert stats["cells_without_noise"] == 0
    # R <= Gr + 1: no gate has a training gate on either side
    for Rg in (1, 2, 3):
        det, stats = R.detect(np.full((2, 3, Rg), 9.0, np.float32), 1, 2, 4, 0, R.CA, 1.0)
        assert len(det) == 0 and stats["cells_over"] == 0 and stats["cells_without_noise"] == 2 * 3 * Rg
    _, stats = R.detect(np.ones((1, 1, 4), np.float32), 0, 2, 4, 0)     # gates 0 and 3 train on one gate, 1 and 2 on none
    assert stats["cells_without_noise"] == 2


def test_the_tie_rule_on_a_3_by_5_map():
    """equal powers: the lowest (row, gate) of a box is reported; the box wraps in rows and is clipped in gates"""
    p = np.ones((1, 3, 5), np.float32)
    kw = dict(Wd=0, Gr=1, Tr=2, Pd=1, method=R.CA, alpha=2.0)
    p[0, 0, 2] = p[0, 2, 3] = 9.0            # rows 0 and 2 are neighbours through the wrap, gates 2 and 3 within Gr
    det, _ = R.detect(p, **kw)
    assert [(int(d["row"]), int(d["gate"])) for d in det] == [(0, 2)]
    p[0, 2, 3] = 1.0
    p[0, 2, 4] = 9.0                         # two gates apart: outside the box
    det, _ = R.detect(p, **kw)
    assert [(int(d["row"]), int(d["gate"])) for d in det] == [(0, 2), (2, 4)]
    p[0, 1, 4] = np.float32(9.0) + np.float32(1e-6)   # larger, next to (2, 4): that one is beaten, (0, 2) is not
    det, _ = R.detect(p, **kw)
    assert [(int(d["row"]), int(d["gate"])) for d in det] == [(0, 2), (1, 4)]
    p[0, 0, 1] = np.nan                      # a NaN neighbour beats nothing
    det, _ = R.detect(p, **kw)
    assert (0, 2) in [(int(d["row"]), int(d["gate"])) for d in det]


# -- the designed inputs ------------------------------------------------------------
def test_the_tie_map_is_what_it_is_taken_for():
    det, _ = R.detect(K.tie_map()[None], method=R.CA, min_power=0.0, **K.TIE)
    got = [(int(d["row"]), int(d["gate"])) for d in det]
    want = sorted([min(a, b) for a, b in K.TIE_INSIDE] + [c for pair in K.TIE_OUTSIDE for c in pair])
    assert got == want
    for a, b in K.TIE_INSIDE:
        assert max(a, b) not in got
    assert R.CA == L.PFB_CFAR_CA and rd_cfar.describe_rdcfar(*K.TIE_SHAPE, K.TIE["Wd"], K.TIE["Gr"], K.TIE["Tr"],
                                                            K.TIE["Pd"]).tile_rows == 8


def test_the_order_maps_depend_on_the_order_of_either_walk():
    """more than half the cells' noise bits change when a walk is reversed: bit-for-bit agreement of the device with
    the restatement then means the order, not luck"""
    p, c = K.order_map_gates(), K.ORDER_GATES
    A = R.column_sums(p, c["Wd"])
    fwd, _ = R.noise_of(p, c["Wd"], c["Gr"], c["Tr"], R.CA, A=A)
    rev, _ = R.noise_of(p, c["Wd"], c["Gr"], c["Tr"], R.CA, A=A, sums=R.side_sums(A, c["Gr"], c["Tr"], reverse=True))
    share = float((fwd.view(np.uint32) != rev.view(np.uint32)).mean())
    print(f"gate walk reversed: {share:.3f} of the noise values differ")
    assert share > 0.5
    p, c = K.order_map_rows(), K.ORDER_ROWS
    fwd, _ = R.noise_of(p, c["Wd"], c["Gr"], c["Tr"], R.CA)
    rev, _ = R.noise_of(p, c["Wd"], c["Gr"], c["Tr"], R.CA, A=R.column_sums(p, c["Wd"], reverse=True))
    share = float((fwd.view(np.uint32) != rev.view(np.uint32)).mean())
    print(f"row walk reversed: {share:.3f} of the noise values differ")
    assert share > 0.5


def test_the_nonfinite_map_reaches_every_role():
    p, c = K.nonfinite_map(), K.NONFINITE
    over, noise, _ = R.decide(p, c["Wd"], c["Gr"], c["Tr"], R.CA, c["alpha"], 0.0)
    assert not over[2, 30] and over[2, 90] and not over[2, 150]      # NaN never, +Inf is over, -Inf never
    assert np.isnan(noise[5, 30]) and not over[5, 30]                # a NaN training cell blinds
    assert np.isposinf(noise[5, 90]) and np.isneginf(noise[5, 150]) and over[5, 150]
    det, _ = R.detect(p[None], method=R.CA, **c)
    got = [(int(d["row"]), int(d["gate"])) for d in det]
    assert (6, 50) in got and (6, 110) not in got and (6, 170) in got   # a NaN or -Inf neighbour beats nothing, +Inf does
    assert (3, 250) in got and (3, 252) not in got                        # equal infinities: the lower gate


@pytest.fixture(scope="module")
def chain():
    iq = K.chain2_stream()
    return iq, K.chain_maps(iq)


def test_the_chain_design_on_the_reference(chain):
    """both trains stand at >= 2x their thresholds in every interval, no other cell exceeds 0.5x its own"""
    _iq, maps = chain
    Gr = pd_cases.chain_replica().size
    rows = (pd_cases.CHAIN_K // 2, pd_cases.CHAIN_K // 2 + K.CHAIN2_BIN)
    gate = pd_cases.CHAIN["first_pulse"]
    det, _ = K.chain_detect(maps, K.CHAIN_ALPHA)
    assert [(int(d["map"]), int(d["row"]), int(d["gate"])) for d in det] == \
        [(m, r, gate) for m in range(pd_cases.CHAIN_CPIS) for r in rows]
    assert det["power"][1::2].sum() < det["power"][0::2].sum()        # the second train is the weaker one
    for P in maps:
        noise, _ = R.noise_of(P, K.CHAIN_RD["Wd"], Gr, K.CHAIN_RD["Tr"], R.CA)
        q = P / (np.float32(K.CHAIN_ALPHA) * noise)
        assert min(q[r, gate] for r in rows) >= 2.0
        for r in rows:
            q[r, gate - Gr:gate + Gr + 1] = 0.0    # the trains' own range sidelobes: inside the guard, not noise
        print("peaks %.2f %.2f, largest other cell %.2f of its threshold" % (P[rows[0], gate] / (K.CHAIN_ALPHA * noise[rows[0], gate]),
                                                                              P[rows[1], gate] / (K.CHAIN_ALPHA * noise[rows[1], gate]), q.max()))
        assert q.max() <= 0.5


# -- false-alarm rate ---------------------------------------------------------------
FAR = dict(Wd=1, Gr=2, Tr=8)


def far_count(maps, alpha, Wd=FAR["Wd"]):
    """(over cells among the fully trained gates, how many such cells)"""
    count = cells = 0
    for P in maps:
        over, _noise, trained = R.decide(P, Wd, FAR["Gr"], FAR["Tr"], R.CA, alpha, 0.0)
        full = trained == 2 * FAR["Tr"]
        count += int(over[:, full].sum())
        cells += int(full.sum()) * P.shape[0]
    return count, cells


def test_design_false_alarm_rate():
    """2^22 i.i.d. exponential cells as 32 maps of 64 x 2048 against alpha = cfar_alpha(1e-4, 48): the over count among
    the fully trained cells lies within 5 sqrt(mu) of mu = pfa * cells"""
    pfa = 1e-4
    rng = np.random.default_rng(0)
    maps = rng.exponential(1.0, (32, 64, 2048)).astype(np.float32)
    alpha = cfar.cfar_alpha(pfa, 2 * FAR["Tr"] * (2 * FAR["Wd"] + 1))
    count, cells = far_count(maps, alpha)
    mu = pfa * cells
    print(f"{count} over of {cells} fully trained cells, expected {mu:.0f} +- {5 * math.sqrt(mu):.0f}")
    assert cells >= (1 << 22) * (2048 - 2 * (FAR["Gr"] + FAR["Tr"])) // 2048
    assert abs(count - mu) <= 5 * math.sqrt(mu)


def test_rate_under_a_hann_window_is_a_finding():
    """the same experiment on pd_ref.transform of complex white noise under a Hann window (rows correlated), and what
    detect_pulse_train's design factor gives on the same data: printed, DESIGN.md section 22 records them"""
    pfa, ND, Rg, n = 1e-4, 64, 2048, 32
    rng = np.random.default_rng(1)
    w = np.hanning(ND + 2)[1:-1].astype(np.float32)
    alpha = cfar.cfar_alpha(pfa, 2 * FAR["Tr"] * (2 * FAR["Wd"] + 1))
    harmonic = float(np.sum(1.0 / np.arange(1, ND + 1)))
    a_train = cfar.cfar_alpha(pfa / ND, 2 * 8 * 64) / harmonic          # detect_pulse_train's factor, per gate
    for name, win in (("rectangular", None), ("hann", w)):
        maps, best_over, gates = [], 0, 0
        for _ in range(n):
            A = (rng.standard_normal((ND, Rg)) + 1j * rng.standard_normal((ND, Rg))) / np.sqrt(2.0)
            P = pd_ref.power(pd_ref.transform(A, win, ND, True)).astype(np.float32)
            maps.append(P)
            bp, _bh = pd_ref.best(P, ND, True)
            over, _noise, trained = cfar_ref.decide(bp.astype(np.float32), Rg, True, 64, 1, 8, cfar_ref.CA, a_train, 0.0)
            full = np.repeat(trained == 16, 64)[:Rg]
            best_over += int(over[full].sum())
            gates += int(full.sum())
        count, cells = far_count(maps, alpha)
        count0, _ = far_count(maps, cfar.cfar_alpha(pfa, 2 * FAR["Tr"]), Wd=0)
        print(f"{name}: 2-D detector {count} over of {cells} cells = {count / cells:.2e} (asked {pfa:.0e}), "
              f"with Wd = 0 {count0 / cells:.2e}; "
              f"best-row route {best_over} over of {gates} gates = {best_over / max(gates, 1):.2e} per gate (asked {pfa:.0e})")
        assert cells > 0 and gates >= 0


# -- arguments, layouts, exports ----------------------------------------------------
def config(rows=64, gates=2048, pitch=0, Wd=1, Gr=2, Tr=8, Pd=1, method=0, alpha=5.0, min_power=0.0, flags=0, size=None,
           device=-1):
    return L.PfbRdcfarConfig(C.sizeof(L.PfbRdcfarConfig) if size is None else size, rows, gates, pitch, Wd, Gr, Tr, Pd,
                             method, alpha, min_power, flags, device)


def both(**kw):
    """the status of pfb_rdcfar_describe and of pfb_rdcfar_create for one config, their outputs untouched on failure"""
    lib = L.load()
    cfg = config(**kw)
    plan, h = L.PfbRdcfarPlan(), C.c_void_p()
    C.memset(C.byref(plan), 0x5a, C.sizeof(plan))
    d = lib.pfb_rdcfar_describe(C.byref(cfg), C.byref(plan))
    c = lib.pfb_rdcfar_create(C.byref(cfg), C.byref(h))
    assert d == L.PFB_OK or bytes(plan) == b"\x5a" * C.sizeof(plan)
    assert not h.value or c == L.PFB_OK
    if h.value:
        lib.pfb_rdcfar_destroy(h)
    return d, c


def test_arguments_are_checked_before_the_device_and_in_order():
    lib = L.load()
    BAD = L.PFB_ERR_BAD_ARG
    plan, h = L.PfbRdcfarPlan(), C.c_void_p()
    cfg = config()
    assert lib.pfb_rdcfar_describe(None, C.byref(plan)) == lib.pfb_rdcfar_describe(C.byref(cfg), None) == BAD
    assert lib.pfb_rdcfar_create(None, C.byref(h)) == lib.pfb_rdcfar_create(C.byref(cfg), None) == BAD
    bad = [dict(size=48), dict(size=56), dict(rows=0), dict(rows=1025), dict(gates=0), dict(gates=(1 << 20) + 1)]
    bad += [dict(pitch=2047), dict(pitch=1), dict(rows=1024, gates=1 << 16, pitch=(1 << 16) + 1), dict(rows=128, gates=1 << 20)]
    bad += [dict(Wd=17), dict(Wd=1 << 31), dict(rows=4, Wd=2, Pd=0), dict(rows=1, Wd=1, Pd=0), dict(Gr=1025)]
    bad += [dict(Tr=0), dict(Tr=257), dict(Pd=17), dict(rows=4, Wd=1, Pd=2), dict(method=3)]
    bad += [dict(alpha=a) for a in (0.0, -1.0, np.nan, np.inf, -np.inf)]
    bad += [dict(min_power=m) for m in (-1.0, np.nan, -np.inf)]
    bad += [dict(flags=f) for f in (1, 2, 1 << 31)]
    for kw in bad:
        assert both(**kw) == (BAD, BAD), kw
        assert both(device=1 << 20, **kw) == (BAD, BAD), kw   # before the device is looked at
    # the order: each refusal hides the ones behind it, so a config with two faults reports as the first alone does;
    # observable through describe only as BAD either way -- what can be told apart is BAD before NO_DEVICE
    u, st = C.c_uint64(7), L.PfbRdcfarStats()
    buf = np.zeros(64, np.float32)
    p = C.c_void_p(buf.ctypes.data)
    assert lib.pfb_rdcfar_destroy(None) == lib.pfb_rdcfar_reset(None) == lib.pfb_rdcfar_sync(None) == BAD
    assert lib.pfb_rdcfar_set_stream(None, None) == lib.pfb_rdcfar_get_device(None, None) == BAD
    assert lib.pfb_rdcfar_next_map(None, C.byref(u)) == lib.pfb_rdcfar_get_stats(None, C.byref(st)) == BAD
    assert lib.pfb_rdcfar_process(None, p, 1, p, 1, C.byref(u), L.PFB_MEM_HOST) == BAD
    assert lib.pfb_rdcfar_process(None, p, 1, p, 1, C.byref(u), 2) == BAD
    assert lib.pfb_rdcfar_process_async(None, p, 1, p, 1, p) == BAD
    assert u.value == 7 and lib.pfb_rdcfar_last_kernel(None) == b""


def test_a_valid_config_is_refused_only_for_want_of_a_device():
    have = L.load().pfb_device_count() > 0
    want = (L.PFB_OK, L.PFB_OK if have else L.PFB_ERR_NO_DEVICE)
    for kw in (dict(), dict(rows=1, gates=1, Wd=0, Gr=0, Tr=1, Pd=0), dict(rows=33, Wd=16, Pd=16, Gr=1024, Tr=256),
               dict(rows=1024, gates=1 << 16), dict(rows=64, gates=1 << 20), dict(pitch=4096), dict(method=2),
               dict(min_power=np.inf), dict(alpha=1e-30)):
        assert both(**kw) == want, kw


def test_describe():
    for (rows, gates, Wd, Gr, Tr, Pd), (band, kernel) in (
            ((64, 2048, 1, 2, 8, 1), (8, "lds")), ((1, 4096, 0, 0, 1, 0), (1, "lds")), ((3, 10, 1, 2, 4, 1), (4, "lds")),
            ((64, 2048, 1, 104, 16, 1), (8, "lds")), ((64, 2048, 16, 104, 128, 16), (8, "direct")),
            ((64, 4096, 1, 1024, 256, 1), (1, "lds")), ((64, 4096, 16, 1024, 256, 16), (2, "direct"))):
        plan = rd_cfar.describe_rdcfar(rows, gates, Wd, Gr, Tr, Pd)
        W, H = K.TILE + 2 * (Gr + Tr), max(Wd, Pd)
        assert plan.training_cells == 2 * Tr * (2 * Wd + 1) and plan.tile_gates == K.TILE
        assert (plan.tile_rows, plan.kernel.decode()) == (band, f"pfb_rdcfar_cells<{kernel}>"), (rows, gates, Wd, Gr, Tr, Pd)
        assert plan.lds_bytes == band * W * 8 + ((band + 2 * H) * W * 4 if kernel == "lds" else 0) <= 64 << 10
    base = bytes(rd_cfar.describe_rdcfar(64, 2048, 1, 2, 8, 1))
    for kw in (dict(alpha=9.0), dict(method="go"), dict(method="so"), dict(min_power=3.0), dict(pitch=4096)):
        assert bytes(rd_cfar.describe_rdcfar(64, 2048, 1, 2, 8, 1, **kw)) == base, kw
    with pytest.raises(ValueError):
        rd_cfar.RangeDopplerCfar(64, 2048, 1, 2, 8)
    with pytest.raises(ValueError):
        rd_cfar.RangeDopplerCfar(64, 2048, 1, 2, 8, 5.0, pfa=1e-3)


def test_exports():
    lib = L.load()
    declared = {n for n in declared_symbols() if n.startswith("pfb_rdcfar_")}
    assert declared == RDCFAR_EXPORTS == {n for n in L.EXPORTS if n.startswith("pfb_rdcfar_")}
    for name in RDCFAR_EXPORTS:
        assert hasattr(lib, name), name
    assert (C.sizeof(L.PfbRdcfarConfig), C.sizeof(L.PfbRdcfarPlan), C.sizeof(L.PfbRdcfarDet), C.sizeof(L.PfbRdcfarStats)) \
        == (52, 56, 32, 40)
    assert rd_cfar.DET_DTYPE.itemsize == R.DET.itemsize == 32 and rd_cfar.DET_DTYPE == R.DET
    assert [rd_cfar.DET_DTYPE.fields[n][1] for n, _ in L.PfbRdcfarDet._fields_] == [getattr(L.PfbRdcfarDet, n).offset
                                                                                   for n, _ in L.PfbRdcfarDet._fields_]
    assert L.PFB_RDCFAR_DET_ONE_SIDED == R.ONE_SIDED == 1
    hdr = open(os.path.join(ROOT, "include", "pfb_channelizer.h")).read()
    assert "#define PFB_RDCFAR_DET_ONE_SIDED 1u" in hdr
    assert "#define PFB_ABI_VERSION 2" in hdr and lib.pfb_abi_version() == 2
    assert hdr.index("pfb_rdcfar_describe(") > hdr.index("pfb_fold_last_kernel(")   # its own section, at the end
    import sdr_channelizer_amd as pkg
    names = ["RangeDopplerCfar", "detect_maps", "detect_targets", "targets_to_pdws"]
    at = pkg.__all__.index("PriFold")
    assert pkg.__all__[at - len(names):at] == names
    for name in names[:3]:
        assert getattr(pkg, name) is getattr(rd_cfar, name)
    assert pkg.targets_to_pdws is rd_cfar.detections_to_pdws and pkg.detections_to_pdws is cfar.detections_to_pdws


def test_the_struct_layouts_are_the_compilers(tmp_path):
    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.skip("no gcc")
    fields = [("pfb_rdcfar_config", L.PfbRdcfarConfig), ("pfb_rdcfar_plan", L.PfbRdcfarPlan),
              ("pfb_rdcfar_det", L.PfbRdcfarDet), ("pfb_rdcfar_stats", L.PfbRdcfarStats)]
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


def test_rdcfar_entry_points_sit_under_the_abi_guard():
    src = open(os.path.join(ROOT, "sdr_channelizer_amd", "csrc", "pfb_rdcfar.hip")).read()
    found = {}
    for m in re.finditer(r'^extern "C" int (\w+)\(', src, re.M):
        rest = src[m.start():]
        found[m.group(1)] = rest[: rest.index("\n}\n")]
    assert set(found) == RDCFAR_EXPORTS - {"pfb_rdcfar_last_kernel"}
    for name, body in found.items():
        assert "abi_guard" in body.split("{", 1)[1][:80], name
    assert src.count('extern "C"') == len(found) + 1
    from sdr_channelizer_amd import build
    assert "pfb_rdcfar.hip" in build.SOURCES
    # the unit's create checks the config first; the create path it shares with pfb_oscfar.hip takes the device, then memory
    create = found["pfb_rdcfar_create"]
    assert create.index("rdcfar_check(cfg") < create.index("create_detector(")
    assert "resolve_device" not in src and "hipMalloc" not in src
    core = open(os.path.join(ROOT, "sdr_channelizer_amd", "csrc", "pfb_rdmap.hpp")).read()
    shared = core[core.index("int create_detector("):]
    shared = shared[: shared.index("\n}\n")]
    assert shared.index("resolve_device") < shared.index("new H()") < shared.index("h->allocate()")


def test_to_pdw_and_event_fit():
    lib = L.load()
    fs, fc, t0, pri, Kp, ND, origin = 2.0e6, 915e6, 100.0, 2048, 64, 64, 11
    n = 9
    d = np.zeros(n, R.DET)
    d["map"] = np.arange(n)
    d["row"] = ND // 2 + 5
    d["gate"] = 700
    snr_db = 20.0 - 0.5 * (np.arange(n) - 4.0) ** 2            # a parabola with its top at interval 4
    d["noise"] = 2.0
    d["power"] = (2.0 * 10.0 ** (snr_db / 10.0)).astype(np.float32)
    pd = rd_cfar.detections_to_pdws(d, fs, fc, t0, pri, Kp, ND, origin=origin)
    assert pd.dtype == cfar.PDW_DTYPE and len(pd) == n
    assert np.array_equal(pd["toa"], (origin + np.arange(n) * Kp * pri + 700 + 1) / fs + t0)
    assert np.array_equal(pd["pw"], np.full(n, 1 / fs)) and not pd["sat"].any() and (pd["bin"] == 5).all()
    assert np.array_equal(pd["freq"], np.full(n, fc + 5 * fs / (ND * pri)))
    want_snr = 10 * np.log10(d["power"].astype(np.float64) / 2.0)
    assert np.abs(pd["snr"] - want_snr).max() < 1e-12 and np.abs(pd["mag"] - np.sqrt(d["power"].astype(np.float64))).max() < 1e-12
    from sdr_channelizer_amd import fit_event
    t_peak, snr_peak, coef = fit_event(pd)
    assert abs(t_peak - pd["toa"][4]) < 1e-6 and abs(snr_peak - 20.0) < 1e-3 and coef[2] < 0
    # the rows as the transform orders them without PFB_PD_CENTERED, for an odd and an even number of rows
    for rows in (64, 5):
        d["row"][:rows] = np.arange(min(rows, n))
        d["row"][rows:] = 0
        pb = rd_cfar.detections_to_pdws(d, fs, fc, t0, pri, Kp, rows, centered=False)
        assert list(pb["bin"][:5]) == ([0, 1, 2, 3, 4] if rows == 64 else [0, 1, 2, -2, -1])
        pc = rd_cfar.detections_to_pdws(d, fs, fc, t0, pri, Kp, rows, centered=True)
        assert list(pc["bin"][:5]) == [k - rows // 2 for k in range(5)]
    assert np.array_equal(rd_cfar.signed_bins(np.arange(5), 5, False), [0, 1, 2, -2, -1])
    # detect_targets' records go the same way
    t = np.zeros(n, rd_cfar.TARGET_DTYPE)
    t["cpi"], t["row"], t["gate"], t["power"], t["noise"] = d["map"], ND // 2 + 5, 700, d["power"], 2.0
    d["row"] = ND // 2 + 5
    assert rd_cfar.detections_to_pdws(t, fs, fc, t0, pri, Kp, ND, origin=origin).tobytes() == pd.tobytes()
    assert len(rd_cfar.detections_to_pdws(d[:0], fs, fc, t0, pri, Kp, ND)) == 0
    out = np.zeros(n, cfar.PDW_DTYPE)
    po = out.ctypes.data_as(C.POINTER(L.PfbPdw))
    dp = C.c_void_p(d.ctypes.data)
    for bad_fs in (0.0, -1.0, np.nan, np.inf):
        assert lib.pfb_rdcfar_to_pdw(dp, n, bad_fs, fc, t0, pri, Kp, 0, ND, 1, po) == L.PFB_ERR_BAD_ARG
    assert lib.pfb_rdcfar_to_pdw(None, n, fs, fc, t0, pri, Kp, 0, ND, 1, po) == L.PFB_ERR_BAD_ARG
    assert lib.pfb_rdcfar_to_pdw(dp, n, fs, fc, t0, pri, Kp, 0, ND, 1, None) == L.PFB_ERR_BAD_ARG
    assert lib.pfb_rdcfar_to_pdw(dp, n, fs, fc, t0, 0, Kp, 0, ND, 1, po) == L.PFB_ERR_BAD_ARG
    assert lib.pfb_rdcfar_to_pdw(dp, n, fs, fc, t0, pri, 0, 0, ND, 1, po) == L.PFB_ERR_BAD_ARG
    assert lib.pfb_rdcfar_to_pdw(dp, n, fs, fc, t0, pri, Kp, 0, 0, 1, po) == L.PFB_ERR_BAD_ARG
    assert lib.pfb_rdcfar_to_pdw(dp, n, fs, fc, t0, pri, Kp, 0, 8, 1, po) == L.PFB_ERR_BAD_ARG   # row 37 of 8
    assert not out.view(np.uint8).any()
