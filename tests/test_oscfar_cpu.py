"""The ordered-statistic CFAR detector's contract without a GPU: the numpy restatement (oscfar_ref) against a literal
per-cell loop that uses the counting form of the definition, the designed inputs of oscfar_cases proven on the
restatement alone (the masking scene with both of its margins), pfb_oscfar_alpha against the product formula, the
false-alarm rate on the reference (and what a Hann window does to it at Wd = 1: a finding, printed), every argument
check that comes before the device, the struct layouts, the exports and the placement in the header and in __all__."""
import ctypes as C
import inspect
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import oscfar_cases as K
import oscfar_ref as O
import pd_cases
import pd_ref
import rdcfar_ref as R
from abi_symbols import declared_symbols
from sdr_channelizer_amd import _lib as L
from sdr_channelizer_amd import cfar, os_cfar, rd_cfar

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OSCFAR_EXPORTS = {"pfb_oscfar_describe", "pfb_oscfar_alpha", "pfb_oscfar_create", "pfb_oscfar_destroy",
                  "pfb_oscfar_reset", "pfb_oscfar_set_stream", "pfb_oscfar_sync", "pfb_oscfar_get_device",
                  "pfb_oscfar_next_map", "pfb_oscfar_get_stats", "pfb_oscfar_process", "pfb_oscfar_process_async",
                  "pfb_oscfar_last_kernel"}


def cells(det):
    return [(int(d["row"]), int(d["gate"])) for d in det]


# -- the definition, cell by cell ---------------------------------------------------
def literal(maps, Wd, Gr, Tr, Pd, rank, alpha, min_power, first_map=0):
    """The header text as a loop over cells: the training set as a list, k' in integers, the noise as the smallest
    training value v with #{x <= v} >= k', the decision by counting alpha * x < p -- and by the product, which the
    header says is the same."""
    f32 = np.float32
    N = 2 * Tr * (2 * Wd + 1)
    out, n_over, without = [], 0, 0
    with np.errstate(all="ignore"):
        for m, P in enumerate(maps):
            ND, Rg = P.shape
            for d in range(ND):
                for r in range(Rg):
                    gates = [g for g in range(r - Gr - Tr, r - Gr) if g >= 0] + \
                            [g for g in range(r + Gr + 1, r + Gr + Tr + 1) if g < Rg]
                    xs = [P[(d + j) % ND][g] for j in range(-Wd, Wd + 1) for g in gates]
                    n = len(xs)
                    if n == 0:
                        without += 1
                        continue
                    kk = (rank * n + N - 1) // N
                    assert 1 <= kk <= n and (kk == rank or n < N)
                    noise = f32(np.nan)
                    for v in xs:      # the smallest v with enough values at or below it; NaN <= v never holds
                        if sum(1 for x in xs if x <= v) >= kk and not (noise <= v):
                            noise = v
                    if noise == 0:
                        noise = f32(0.0)
                    p = P[d][r]
                    counted = sum(1 for x in xs if f32(alpha) * x < p) >= kk
                    assert counted == bool(p > f32(alpha) * noise), (d, r)
                    if not (counted and bool(p > f32(min_power))):
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
                        out.append((first_map + m, d, r, p, noise, n, R.ONE_SIDED if n < N else 0))
    stats = {"maps_in": len(maps), "cells_over": n_over, "cells_without_noise": without, "detections": len(out),
             "dropped": 0}
    return (np.array(out, R.DET) if out else np.zeros(0, R.DET)), stats


@pytest.mark.parametrize("Wd,Gr,Tr,Pd", [(0, 0, 1, 0), (1, 1, 2, 1), (1, 2, 3, 0), (2, 0, 4, 2), (0, 5, 2, 1)])
def test_restatement_is_the_definition(Wd, Gr, Tr, Pd):
    need = 2 * max(Wd, Pd) + 1
    N = O.full_cells(Wd, Tr)
    for seed, (ND, Rg) in enumerate(((1, 1), (1, 17), (3, 7), (5, 23), (6, 12))):
        if ND < need:
            continue
        maps = K.noise_maps(2, ND, Rg, seed, share=0.15, level=40.0)
        quant = K.quantised_maps(2, ND, Rg, seed, raised=0.1)
        if Rg > 10:
            maps[0, ND // 2, 3] = np.nan
            maps[1, 0, 5] = np.inf
            maps[1, ND - 1, 8] = maps[1, ND - 1, 9] = maps[1].max() * 2    # equal neighbours
            maps[0, 0, Rg - 1] = -np.inf
            quant[0, 0, 4] = -0.0
        for rank in sorted({1, (N + 1) // 2, max(N - 1, 1), N}):
            for x, alpha, floor in ((maps, 3.0, 0.5), (quant, 1.5, 0.0)):
                want, wstats = literal(x, Wd, Gr, Tr, Pd, rank, alpha, floor, 7)
                got, gstats = O.detect(x, Wd, Gr, Tr, Pd, rank, alpha, floor, 7)
                assert got.tobytes() == want.tobytes(), (ND, Rg, rank)
                assert gstats == wstats, (ND, Rg, rank)


def test_the_rank_at_the_gate_edges():
    """k' = ceil(k n / N): Tr = 4, Gr = 2, rank 5 of 8 -- not a multiple of any count's divisor"""
    kk, n = O.ranks(20, 0, 2, 4, 5)
    assert list(n[:8]) == [4, 4, 4, 5, 6, 7, 8, 8] and list(kk[:8]) == [3, 3, 3, 4, 4, 5, 5, 5]
    assert list(n[-8:]) == [8, 8, 7, 6, 5, 4, 4, 4] and list(kk[-8:]) == [5, 5, 5, 4, 4, 3, 3, 3]
    kk, n = O.ranks(3, 1, 2, 4, 5)         # R <= Gr + 1: no cell trains
    assert not n.any() and not kk.any()
    p = np.ones((1, 3, 20), np.float32)
    p[0, 1, [0, 3, 19]] = 50.0
    det, stats = O.detect(p, 1, 2, 4, 0, 13, 4.0)
    assert [(int(d["gate"]), int(d["training_cells"]), int(d["flags"])) for d in det] == [(0, 12, 1), (3, 15, 1), (19, 12, 1)]
    assert stats["cells_without_noise"] == 0
    for Rg in (1, 2, 3):
        det, stats = O.detect(np.full((2, 3, Rg), 9.0, np.float32), 1, 2, 4, 0, 7, 1.0)
        assert len(det) == 0 and stats["cells_over"] == 0 and stats["cells_without_noise"] == 2 * 3 * Rg


# -- the designed inputs ------------------------------------------------------------
def test_the_quantised_maps_put_ties_at_every_rank():
    """with four values in 8 training cells every order statistic lies in a run of equal values: for most cells the
    (k-1)-th, k-th and (k+1)-th values are the same"""
    p = K.quantised_maps(1, 5, 70, seed=2)[0]
    S = O.sorted_training(p, 0, 1, 4)
    full = (O.ranks(70, 0, 1, 4, 1)[1] == 8)
    for k in range(2, 8):
        tied = (S[:, full, k - 2] == S[:, full, k - 1]) | (S[:, full, k - 1] == S[:, full, k])
        assert tied.mean() > 0.8, k
    seen = set()
    for k in range(1, 9):
        noise, _ = O.noise_of(p, 0, 1, 4, k, S)
        seen |= set(np.unique(noise[:, full]).tolist())
    assert {0.0, 1.0, 2.0, 3.0} <= seen


def test_the_nonfinite_map_puts_each_value_at_below_and_above_the_rank():
    p, c = K.nonfinite_map(), K.NONFINITE
    over, noise, n = O.decide(p, c["Wd"], c["Gr"], c["Tr"], c["rank"], c["alpha"], 0.0)
    det, _ = O.detect(p[None], c["Wd"], c["Gr"], c["Tr"], c["Pd"], c["rank"], c["alpha"])
    got = cells(det)
    for row in K.NONFINITE_ROWS:
        for i, (v, copies) in enumerate(K.NONFINITE_DESIGN):
            g = K.nonfinite_gate(i)
            assert n[g] == 8 and p[row, g] == 500.0
            x = noise[row, g]
            if np.isnan(v):       # 2 copies: ranks 7, 8; 3: the rank itself; 4: one below it too
                assert np.isnan(x) == (copies >= 3) and over[row, g] == (copies < 3)
            elif v > 0:
                assert np.isposinf(x) == (copies >= 3) and over[row, g] == (copies < 3)
            else:                 # -Inf: 5 copies are ranks 1 .. 5, the 6th value a number
                assert np.isneginf(x) == (copies >= 6) and over[row, g]
            assert np.isfinite(x) == (copies in (2, 5))
            assert ((row, g) in got) == bool(over[row, g])
    # what rdcfar_cases designed still plays its part: NaN never over, +Inf over, a NaN neighbour beats nothing
    assert not over[2, 30] and over[2, 90] and not over[2, 150]
    assert (3, 250) in got and (3, 252) not in got


def test_the_zeros_map_selects_zeros_of_either_sign():
    p, c = K.zeros_map(), K.ZEROS
    S = O.sorted_training(p, c["Wd"], c["Gr"], c["Tr"])
    kk, n = O.ranks(p.shape[1], c["Wd"], c["Gr"], c["Tr"], c["rank"])
    pick = np.take_along_axis(S, np.broadcast_to(np.maximum(kk - 1, 0)[None, :, None], p.shape + (1,)), axis=2)[:, :, 0]
    zero = (pick == 0) & (n[None, :] > 0)
    assert (zero & np.signbit(pick)).sum() > 100 and (zero & ~np.signbit(pick)).sum() > 100    # -0.0 and +0.0 selected
    assert ((pick == 1.0) & (n[None, :] > 0)).sum() > 10
    noise, _ = O.noise_of(p, c["Wd"], c["Gr"], c["Tr"], c["rank"], S)
    assert not np.signbit(noise[zero]).any()                                                    # reported as +0.0
    det, stats = O.detect(p[None], c["Wd"], c["Gr"], c["Tr"], c["Pd"], c["rank"], c["alpha"])
    z = det[det["noise"] == 0]
    assert len(z) > 100 and not z["noise"].view(np.uint32).any()
    assert stats["cells_over"] >= len(det) and (det["noise"] == 1.0).any()


def test_the_masking_scene():
    """the purpose of the unit: the CA restatement misses (3, 310), which stands under its threshold; the OS
    restatement reports all four at more than twice their thresholds while every other cell stays under 0.6 of its
    own.  GO misses one more; SO misses it too (an interferer stands on either side) and adds a false alarm."""
    p, c = K.mask_map(), K.MASK
    a_ca, a_os = K.mask_alphas()
    assert abs(a_ca - cfar.cfar_alpha(K.MASK_PFA, 32)) < 1e-5 and abs(a_os - os_cfar.os_cfar_alpha(K.MASK_PFA, 32, K.MASK_RANK)) < 1e-5
    ca, _ = R.detect(p[None], c["Wd"], c["Gr"], c["Tr"], c["Pd"], R.CA, a_ca)
    assert cells(ca) == [t for t in K.MASK_TARGETS if t != K.MASK_MISSED]
    noise, _ = R.noise_of(p, c["Wd"], c["Gr"], c["Tr"], R.CA)
    short = float(p[K.MASK_MISSED] / (np.float32(a_ca) * noise[K.MASK_MISSED]))
    go, _ = R.detect(p[None], c["Wd"], c["Gr"], c["Tr"], c["Pd"], R.GO, a_ca)
    so, _ = R.detect(p[None], c["Wd"], c["Gr"], c["Tr"], c["Pd"], R.SO, a_ca)
    assert K.MASK_MISSED not in cells(go) and len(go) < len(ca)
    assert K.MASK_MISSED not in cells(so) and set(cells(so)) - set(K.MASK_TARGETS)     # an interferer on either side
    det, _ = O.detect(p[None], c["Wd"], c["Gr"], c["Tr"], c["Pd"], K.MASK_RANK, a_os)
    assert cells(det) == K.MASK_TARGETS
    on, _ = O.noise_of(p, c["Wd"], c["Gr"], c["Tr"], K.MASK_RANK)
    with np.errstate(all="ignore"):
        q = p / (np.float32(a_os) * on)
    peaks = [float(q[t]) for t in K.MASK_TARGETS]
    for t in K.MASK_TARGETS:
        q[t] = 0.0
    print("CA: (3, 310) at %.2f of its threshold; OS: targets at %s of theirs, largest other cell %.2f"
          % (short, ", ".join("%.1f" % v for v in peaks), np.nanmax(q)))
    assert short < 0.8 and min(peaks) > 2.0 and np.nanmax(q) < 0.6


@pytest.fixture(scope="module")
def chain():
    iq = K.chain_stream()
    return iq, K.chain_maps(iq)


def test_the_chain_design_on_the_reference(chain):
    """CA misses the weaker (first) train in every interval, by a factor of ten; the ordered statistic reports both.
    The margins the chain's SNR allows are 1.7 and 0.6, not 2 and 0.5 (oscfar_cases has the figures)."""
    _iq, maps = chain
    Gr = pd_cases.chain_replica().size
    row, g1 = pd_cases.CHAIN_K // 2, pd_cases.CHAIN["first_pulse"]
    g2 = g1 + K.CHAIN_OFFSET
    assert Gr < K.CHAIN_OFFSET <= Gr + K.CHAIN_RD["Tr"]
    ca, _ = K.chain_detect_ca(maps)
    assert [(int(d["map"]), int(d["row"]), int(d["gate"])) for d in ca] == [(m, row, g2) for m in range(pd_cases.CHAIN_CPIS)]
    det, _ = K.chain_detect_os(maps)
    assert [(int(d["map"]), int(d["row"]), int(d["gate"])) for d in det] == \
        [(m, row, g) for m in range(pd_cases.CHAIN_CPIS) for g in (g1, g2)]
    assert (det["power"][0::2] < det["power"][1::2]).all()
    for P in maps:
        cn, _ = R.noise_of(P, K.CHAIN_RD["Wd"], Gr, K.CHAIN_RD["Tr"], R.CA)
        on, _ = O.noise_of(P, K.CHAIN_RD["Wd"], Gr, K.CHAIN_RD["Tr"], K.CHAIN_RANK)
        q = P / (np.float32(K.CHAIN_OS_ALPHA) * on)
        first_ca = float(P[row, g1] / (np.float32(K.CHAIN_CA_ALPHA) * cn[row, g1]))
        first_os = float(q[row, g1])
        for g in (g1, g2):
            q[row - 1:row + 2, g - Gr:g + Gr + 1] = 0.0     # the trains and their range sidelobes, inside the guard
        print("first train: %.3f of its CA threshold, %.2f of its OS threshold; largest other cell %.2f" % (first_ca, first_os, q.max()))
        assert first_ca < 0.1 and first_os >= 1.7 and q.max() <= 0.6


# -- the factor and the false-alarm rate ---------------------------------------------
def test_alpha_is_the_root_of_the_product_formula():
    for N in (1, 2, 16, 32, 768, 4096):
        for k in sorted({1, max(N // 2, 1), max(3 * N // 4, 1), N}):
            for pfa in (1e-2, 1e-4, 1e-6, 1e-9):
                a = os_cfar.os_cfar_alpha(pfa, N, k)
                prod = 1.0
                for i in range(k):
                    prod *= (N - i) / (N - i + a)
                assert abs(prod - pfa) <= 1e-9 * pfa, (N, k, pfa)
                if N <= 768:
                    assert abs(a - O.alpha_ref(pfa, N, k)) <= 1e-9 * a
    assert abs(os_cfar.os_cfar_alpha(1e-4, 16, 12) - 11.080) < 5e-4
    assert abs(os_cfar.os_cfar_alpha(1e-3, 5, 1) - 5 * (1e3 - 1)) < 1e-6     # k = 1: N / (N + alpha) = pfa
    lib, a = L.load(), C.c_double(7.0)
    for pfa, N, k in ((0.0, 16, 12), (1.0, 16, 12), (-1e-3, 16, 12), (math.nan, 16, 12), (1e-3, 0, 1), (1e-3, 16, 0),
                      (1e-3, 16, 17), (1e-3, (1 << 20) + 1, 1)):
        assert lib.pfb_oscfar_alpha(pfa, N, k, C.byref(a)) == L.PFB_ERR_BAD_ARG, (pfa, N, k)
    assert lib.pfb_oscfar_alpha(1e-3, 16, 12, None) == L.PFB_ERR_BAD_ARG and a.value == 7.0
    with pytest.raises(L.PfbError):
        os_cfar.os_cfar_alpha(2.0, 16, 12)


FAR = dict(Wd=0, Gr=2, Tr=8, rank=12)


def far_count(maps, alpha, Wd, rank):
    """(over cells among the fully trained gates, how many such cells)"""
    count = total = 0
    for P in maps:
        over, _noise, n = O.decide(P, Wd, FAR["Gr"], FAR["Tr"], rank, alpha, 0.0)
        full = n == O.full_cells(Wd, FAR["Tr"])
        count += int(over[:, full].sum())
        total += int(full.sum()) * P.shape[0]
    return count, total


def test_design_false_alarm_rate():
    """2^22 i.i.d. exponential cells as 32 maps of 64 x 2048 against alpha = os_cfar_alpha(1e-4, 16, 12): the over count
    among the fully trained cells lies within 5 sqrt(mu) of mu = pfa * cells"""
    pfa = 1e-4
    rng = np.random.default_rng(0)
    maps = rng.exponential(1.0, (32, 64, 2048)).astype(np.float32)
    alpha = os_cfar.os_cfar_alpha(pfa, 16, FAR["rank"])
    count, total = far_count(maps, alpha, FAR["Wd"], FAR["rank"])
    mu = pfa * total
    print(f"alpha {alpha:.3f}: {count} over of {total} fully trained cells, expected {mu:.0f} +- {5 * math.sqrt(mu):.0f}")
    assert total >= (1 << 22) * (2048 - 2 * (FAR["Gr"] + FAR["Tr"])) // 2048
    assert abs(count - mu) <= 5 * math.sqrt(mu)


def test_rate_under_a_hann_window_is_a_finding():
    """the same experiment at Wd = 1 (48 training cells, rank 36) on pd_ref.transform of complex white noise, with and
    without a Hann window, which correlates adjacent rows: printed, DESIGN.md section 23 records the figures"""
    pfa, ND, Rg, n = 1e-3, 64, 2048, 8
    rng = np.random.default_rng(1)
    w = np.hanning(ND + 2)[1:-1].astype(np.float32)
    for name, win in (("rectangular", None), ("hann", w)):
        maps = []
        for _ in range(n):
            A = (rng.standard_normal((ND, Rg)) + 1j * rng.standard_normal((ND, Rg))) / np.sqrt(2.0)
            maps.append(pd_ref.power(pd_ref.transform(A, win, ND, True)).astype(np.float32))
        c1, total = far_count(maps, os_cfar.os_cfar_alpha(pfa, 48, 36), 1, 36)
        c0, _ = far_count(maps, os_cfar.os_cfar_alpha(pfa, 16, 12), 0, 12)
        print(f"{name}: Wd = 1, rank 36 of 48: {c1} over of {total} cells = {c1 / total:.2e} (asked {pfa:.0e}); "
              f"Wd = 0, rank 12 of 16: {c0 / total:.2e}")
        assert total > 0


# -- arguments, layouts, exports ----------------------------------------------------
def config(rows=64, gates=2048, pitch=0, Wd=1, Gr=2, Tr=8, Pd=1, rank=36, alpha=5.0, min_power=0.0, flags=0, size=None,
           device=-1):
    return L.PfbOscfarConfig(C.sizeof(L.PfbOscfarConfig) if size is None else size, rows, gates, pitch, Wd, Gr, Tr, Pd,
                             rank, alpha, min_power, flags, device)


def both(**kw):
    """the status of pfb_oscfar_describe and of pfb_oscfar_create for one config, their outputs untouched on failure"""
    lib = L.load()
    cfg = config(**kw)
    plan, h = L.PfbOscfarPlan(), C.c_void_p()
    C.memset(C.byref(plan), 0x5a, C.sizeof(plan))
    d = lib.pfb_oscfar_describe(C.byref(cfg), C.byref(plan))
    c = lib.pfb_oscfar_create(C.byref(cfg), C.byref(h))
    assert d == L.PFB_OK or bytes(plan) == b"\x5a" * C.sizeof(plan)
    assert not h.value or c == L.PFB_OK
    if h.value:
        lib.pfb_oscfar_destroy(h)
    return d, c


def test_arguments_are_checked_before_the_device_and_in_order():
    lib = L.load()
    BAD = L.PFB_ERR_BAD_ARG
    plan, h = L.PfbOscfarPlan(), C.c_void_p()
    cfg = config()
    assert lib.pfb_oscfar_describe(None, C.byref(plan)) == lib.pfb_oscfar_describe(C.byref(cfg), None) == BAD
    assert lib.pfb_oscfar_create(None, C.byref(h)) == lib.pfb_oscfar_create(C.byref(cfg), None) == BAD
    # in the header's order
    bad = [dict(size=48), dict(size=56), dict(rows=0), dict(rows=1025), dict(gates=0), dict(gates=(1 << 20) + 1)]
    bad += [dict(pitch=2047), dict(pitch=1), dict(rows=1024, gates=1 << 16, pitch=(1 << 16) + 1), dict(rows=128, gates=1 << 20)]
    bad += [dict(Wd=17), dict(Wd=1 << 31), dict(rows=4, Wd=2, Pd=0, rank=1), dict(rows=1, Wd=1, Pd=0), dict(Gr=1025)]
    bad += [dict(Tr=0), dict(Tr=257), dict(Pd=17), dict(rows=4, Wd=1, Pd=2)]
    bad += [dict(Tr=256, Wd=4, rank=1), dict(Tr=256, Wd=16, rank=1), dict(Tr=82, Wd=12, rank=1)]    # N > 4096
    bad += [dict(rank=0), dict(rank=49), dict(rank=1 << 31), dict(Wd=0, rank=17)]
    bad += [dict(alpha=a) for a in (0.0, -1.0, np.nan, np.inf, -np.inf)]
    bad += [dict(min_power=m) for m in (-1.0, np.nan, -np.inf)]
    bad += [dict(flags=f) for f in (1, 2, 1 << 31)]
    for kw in bad:
        assert both(**kw) == (BAD, BAD), kw
        assert both(device=1 << 20, **kw) == (BAD, BAD), kw   # before the device is looked at
    u, st = C.c_uint64(7), L.PfbRdcfarStats()
    buf = np.zeros(64, np.float32)
    p = C.c_void_p(buf.ctypes.data)
    assert lib.pfb_oscfar_destroy(None) == lib.pfb_oscfar_reset(None) == lib.pfb_oscfar_sync(None) == BAD
    assert lib.pfb_oscfar_set_stream(None, None) == lib.pfb_oscfar_get_device(None, None) == BAD
    assert lib.pfb_oscfar_next_map(None, C.byref(u)) == lib.pfb_oscfar_get_stats(None, C.byref(st)) == BAD
    assert lib.pfb_oscfar_process(None, p, 1, p, 1, C.byref(u), L.PFB_MEM_HOST) == BAD
    assert lib.pfb_oscfar_process(None, p, 1, p, 1, C.byref(u), 2) == BAD
    assert lib.pfb_oscfar_process_async(None, p, 1, p, 1, p) == BAD
    assert u.value == 7 and lib.pfb_oscfar_last_kernel(None) == b""


def test_a_valid_config_is_refused_only_for_want_of_a_device():
    have = L.load().pfb_device_count() > 0
    want = (L.PFB_OK, L.PFB_OK if have else L.PFB_ERR_NO_DEVICE)
    for kw in (dict(), dict(rows=1, gates=1, Wd=0, Gr=0, Tr=1, Pd=0, rank=1), dict(rank=1), dict(rank=48),
               dict(rows=33, Wd=3, Pd=16, Gr=1024, Tr=256, rank=3584), dict(rows=1024, gates=1 << 16),
               dict(rows=64, gates=1 << 20), dict(pitch=4096), dict(min_power=np.inf), dict(alpha=1e-30)):
        assert both(**kw) == want, kw


def test_the_largest_training_set():
    """N = 2 Tr (2 Wd + 1) <= 4096.  With Tr <= 256 and Wd <= 16 no N is 4096 or 4098 (4096 = 2 * 2048 * 1 needs
    Tr = 2048; 4098 / 2 = 2049 = 3 * 683): the nearest settings either side of the limit are N = 4094 (Tr = 89,
    Wd = 11) and N = 4100 (Tr = 82, Wd = 12)"""
    reachable = {2 * Tr * (2 * Wd + 1) for Tr in range(1, 257) for Wd in range(17)}
    assert 4096 not in reachable and 4098 not in reachable
    assert max(n for n in reachable if n <= 4096) == 4094 and min(n for n in reachable if n > 4096) == 4100
    have = L.load().pfb_device_count() > 0
    ok = (L.PFB_OK, L.PFB_OK if have else L.PFB_ERR_NO_DEVICE)
    assert both(rows=64, Tr=89, Wd=11, rank=4094) == ok and both(rows=64, Tr=89, Wd=11, rank=1) == ok
    assert both(rows=64, Tr=89, Wd=11, rank=4095) == (L.PFB_ERR_BAD_ARG, L.PFB_ERR_BAD_ARG)
    assert both(rows=64, Tr=82, Wd=12, rank=1) == (L.PFB_ERR_BAD_ARG, L.PFB_ERR_BAD_ARG)
    assert os_cfar.describe_oscfar(64, 2048, 11, 2, 89, 4094).training_cells == 4094


def test_describe():
    for (rows, gates, Wd, Gr, Tr, Pd), (band, kernel) in (
            ((64, 2048, 1, 2, 8, 1), (16, "lds")), ((1, 4096, 0, 0, 1, 0), (1, "lds")), ((3, 10, 1, 2, 4, 1), (4, "lds")),
            ((64, 2048, 1, 104, 16, 1), (16, "lds")), ((64, 2048, 1, 104, 64, 16), (16, "direct")),
            ((64, 4096, 1, 1024, 256, 1), (2, "lds")), ((64, 4096, 2, 1024, 256, 2), (1, "lds")),
            ((64, 4096, 3, 1024, 256, 2), (16, "direct")), ((5, 4096, 2, 1024, 256, 2), (1, "lds")),
            ((7, 4096, 1, 1024, 256, 3), (8, "direct"))):
        N = 2 * Tr * (2 * Wd + 1)
        plan = os_cfar.describe_oscfar(rows, gates, Wd, Gr, Tr, (N + 1) // 2, Pd)
        W, H = K.TILE + 2 * (Gr + Tr), max(Wd, Pd)
        assert plan.training_cells == N and plan.tile_gates == K.TILE and plan.reserved == 0
        assert (plan.tile_rows, plan.kernel.decode()) == (band, f"pfb_oscfar_cells<{kernel}>"), (rows, gates, Wd, Gr, Tr, Pd)
        assert plan.lds_bytes == ((band + 2 * H) * W * 4 if kernel == "lds" else 0) <= 64 << 10
    base = bytes(os_cfar.describe_oscfar(64, 2048, 1, 2, 8, 36, 1))
    for kw in (dict(alpha=9.0), dict(min_power=3.0), dict(pitch=4096)):
        assert bytes(os_cfar.describe_oscfar(64, 2048, 1, 2, 8, 36, 1, **kw)) == base, kw
    assert bytes(os_cfar.describe_oscfar(64, 2048, 1, 2, 8, 1, 1)) == base     # the rank does not change the plan
    with pytest.raises(ValueError):
        os_cfar.OsCfar(64, 2048, 1, 2, 8, 36)
    with pytest.raises(ValueError):
        os_cfar.OsCfar(64, 2048, 1, 2, 8, 36, 5.0, pfa=1e-3)


def test_exports_and_placement():
    lib = L.load()
    declared = {n for n in declared_symbols() if n.startswith("pfb_oscfar_")}
    assert declared == OSCFAR_EXPORTS == {n for n in L.EXPORTS if n.startswith("pfb_oscfar_")}
    for name in OSCFAR_EXPORTS:
        assert hasattr(lib, name), name
    assert (C.sizeof(L.PfbOscfarConfig), C.sizeof(L.PfbOscfarPlan)) == (52, 56)
    assert [n for n, _ in L.PfbOscfarConfig._fields_] == [("rank" if n == "method" else n) for n, _ in L.PfbRdcfarConfig._fields_]
    assert [t for _, t in L.PfbOscfarConfig._fields_] == [t for _, t in L.PfbRdcfarConfig._fields_]
    hdr = open(os.path.join(ROOT, "include", "pfb_channelizer.h")).read()
    assert "#define PFB_ABI_VERSION 2" in hdr and lib.pfb_abi_version() == 2
    assert hdr.index("pfb_oscfar_describe(") > hdr.index("pfb_rdcfar_last_kernel(")   # its own section, at the end
    assert "pfb_oscfar_det" not in hdr and "pfb_oscfar_stats" not in hdr and "PFB_OSCFAR_DET" not in hdr   # rdcfar's
    import sdr_channelizer_amd as pkg
    names = ["OsCfar", "os_cfar_alpha", "detect_maps_os"]
    at = pkg.__all__.index("RangeDopplerCfar")
    assert pkg.__all__[at - len(names):at] == names
    for name in names:
        assert getattr(pkg, name) is getattr(os_cfar, name)
    assert issubclass(os_cfar.OsCfar, rd_cfar.RangeDopplerCfar) and os_cfar.records is rd_cfar.records


def test_detect_targets_without_a_rank_does_not_touch_the_unit():
    sig = inspect.signature(rd_cfar.detect_targets)
    assert sig.parameters["rank"].default is None and sig.parameters["rank"].kind is inspect.Parameter.KEYWORD_ONLY
    src = inspect.getsource(rd_cfar.detect_targets)
    branch = src[src.index("if rank is None:"):]
    assert branch.index("return RangeDopplerCfar(") < branch.index("from .os_cfar import OsCfar")
    assert "os_cfar" not in inspect.getsource(rd_cfar).replace(src, "")   # nothing else in the module knows it


def test_the_struct_layouts_are_the_compilers(tmp_path):
    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.skip("no gcc")
    fields = [("pfb_oscfar_config", L.PfbOscfarConfig), ("pfb_oscfar_plan", L.PfbOscfarPlan)]
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


def test_oscfar_entry_points_sit_under_the_abi_guard():
    src = open(os.path.join(ROOT, "sdr_channelizer_amd", "csrc", "pfb_oscfar.hip")).read()
    found = {}
    for m in re.finditer(r'^extern "C" int (\w+)\(', src, re.M):
        rest = src[m.start():]
        found[m.group(1)] = rest[: rest.index("\n}\n")]
    assert set(found) == OSCFAR_EXPORTS - {"pfb_oscfar_last_kernel"}
    for name, body in found.items():
        assert "abi_guard" in body.split("{", 1)[1][:80], name
    assert src.count('extern "C"') == len(found) + 1
    from sdr_channelizer_amd import build
    assert "pfb_oscfar.hip" in build.SOURCES
    # the unit's create checks the config first; the create path it shares with pfb_rdcfar.hip takes the device, then memory
    create = found["pfb_oscfar_create"]
    assert create.index("oscfar_check(cfg") < create.index("create_detector(")
    assert "resolve_device" not in src and "hipMalloc" not in src
    core = open(os.path.join(ROOT, "sdr_channelizer_amd", "csrc", "pfb_rdmap.hpp")).read()
    shared = core[core.index("int create_detector("):]
    shared = shared[: shared.index("\n}\n")]
    assert shared.index("resolve_device") < shared.index("new H()") < shared.index("h->allocate()")
    for text in (src, core):
        code = re.sub(r"//.*", "", text)
        assert "atomic" not in code.lower() and "asm" not in code
