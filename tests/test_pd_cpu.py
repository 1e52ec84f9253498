"""Pulse-Doppler integration without a GPU: the numpy restatement (pd_ref) against a literal triple loop and numpy's FFT,
Parseval, the completion rule walked sample by sample, every argument check that comes before the device, the struct
layouts, the exports, pfb_pd_doppler_frequencies, and -- on the restatement alone -- every input design the GPU module
relies on: the ties, the maxima that are clear of rounding, the train under the single-pulse threshold."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import pd_cases as P
import pd_ref as R
from abi_symbols import declared_symbols
from sdr_channelizer_amd import _lib as L
from sdr_channelizer_amd import cfar
from sdr_channelizer_amd import pulse_doppler as pd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PD_EXPORTS = {"pfb_pd_describe", "pfb_pd_doppler_frequencies", "pfb_pd_create", "pfb_pd_destroy", "pfb_pd_reset",
              "pfb_pd_set_stream", "pfb_pd_sync", "pfb_pd_get_device", "pfb_pd_cpis_for", "pfb_pd_next_index",
              "pfb_pd_set_index", "pfb_pd_process", "pfb_pd_process_async", "pfb_pd_flush", "pfb_pd_last_kernel"}


# -- the definition, term by term -----------------------------------------------------
def literal(x, c, o, L_, Rg, K, w, ND, centered):
    """the header's sums as loops: (Z, N) of interval c"""
    ds = range(-ND // 2, ND // 2) if centered else range(ND)
    Z = np.zeros((ND, Rg), np.complex128)
    N = np.zeros(Rg)
    for r in range(Rg):
        for k in range(K):
            a = complex(x[o + (c * K + k) * L_ + r])
            wk = 1.0 if w is None else float(w[k])
            N[r] += wk * wk * abs(a) ** 2
            for i, d in enumerate(ds):
                Z[i, r] += wk * a * np.exp(-2j * np.pi * d * k / ND)
    return Z, N


@pytest.mark.parametrize("centered", [False, True])
@pytest.mark.parametrize("K,ND,Rg,L_,o", [(1, 8, 1, 1, 0), (3, 8, 2, 5, 4), (8, 8, 3, 3, 1), (5, 16, 4, 7, 0), (16, 16, 1, 2, 9)])
def test_restatement_is_the_definition(K, ND, Rg, L_, o, centered):
    rng = np.random.default_rng(K * 100 + ND)
    x = (rng.standard_normal(o + 2 * K * L_ + Rg) + 1j * rng.standard_normal(o + 2 * K * L_ + Rg)).astype(np.complex64)
    w = None if K % 2 else rng.uniform(0.1, 1.0, K).astype(np.float32)
    for c in (0, 1):
        A = R.gates(x, c, o, L_, Rg, K)
        assert np.array_equal(A, np.array([[x[o + (c * K + k) * L_ + r] for r in range(Rg)] for k in range(K)]))
        Z, N = literal(x, c, o, L_, Rg, K, w, ND, centered)
        got = R.transform(A, w, ND, centered)
        assert np.abs(got - Z).max() <= 1e-12 * np.abs(Z).max()
        assert np.abs(R.noncoherent(A, w) - N).max() <= 1e-12 * N.max()
        # numpy's FFT of the zero-padded windowed columns, rows in FFT order or shifted
        pad = np.zeros((ND, Rg), np.complex128)
        pad[:K] = R.window(K, w).astype(np.float64)[:, None] * A
        F = np.fft.fft(pad, axis=0)
        F = np.fft.fftshift(F, axes=0) if centered else F
        assert np.abs(got - F).max() <= 1e-12 * np.abs(F).max()
        # Parseval: the rows' powers add up to ND times the noncoherent sum
        assert np.abs(R.power(got).sum(axis=0) / ND - R.noncoherent(A, w)).max() <= 1e-12 * N.max()
    assert np.array_equal(R.rows(ND, centered), np.arange(-ND // 2, ND // 2) if centered else np.arange(ND))


def test_best_walks_the_written_rows():
    nan, inf = np.nan, np.inf
    P_ = np.array([[1.0, nan, 2.0, 0.0, inf, 3.0],
                   [5.0, 9.0, 2.0, 0.0, inf, nan],
                   [5.0, 9.0, 1.0, 0.0, 1.0, 4.0],
                   [nan, 1.0, 2.0, 0.0, 2.0, 4.0]])
    bp, bh = R.best(P_, 4, False)
    assert bh.tolist() == [1, 0, 0, 0, 0, 2] and np.isnan(bp[1]) and bp[[0, 2, 3, 4, 5]].tolist() == [5.0, 2.0, 0.0, inf, 4.0]
    bp, bh = R.best(P_, 4, True)   # the same rows stand for d = -2, -1, 0, 1
    assert bh.tolist() == [-1, -2, -2, -2, -2, 0]


def test_the_completion_rule_sample_by_sample():
    for o, L_, Rg, K, start in ((0, 1, 1, 1, 0), (3, 5, 2, 3, 0), (0, 4, 4, 2, 0), (2, 7, 3, 4, 11), (5, 3, 1, 2, 5), (5, 3, 1, 2, 6)):
        span = R.cpi_samples(L_, Rg, K)
        plan = pd.describe_pulse_doppler(L_, K, Rg, o)
        assert plan.cpi_samples == span == (K - 1) * L_ + Rg
        done, held = 0, {}
        for total in range(start, o + 5 * K * L_ + 1):
            assert R.completed(total, o, L_, Rg, K, start) == done, (o, L_, Rg, K, start, total)
            i = total   # the sample that arrives now
            if i >= o:
                c, rem = divmod(i - o, K * L_)
                k, r = divmod(rem, L_)
                if r < Rg and o + c * K * L_ >= start:
                    held[c] = held.get(c, 0) + 1
                    if held[c] == K * Rg:                 # its last gate sample: o + ((c+1)K - 1)L + R - 1
                        assert i == o + ((c + 1) * K - 1) * L_ + Rg - 1
                        done += 1
        assert done >= 3
    x = np.arange(40) + 0j
    got = R.intervals(x, 33, True, 3, 5, 2, 3)       # intervals 0 and 1 whole, interval 2 opened by sample 33 - 1 >= 3 + 30
    assert len(got) == 2 and R.completed(33, 3, 5, 2, 3) == 2
    got = R.intervals(x, 34, True, 3, 5, 2, 3)
    assert len(got) == 3 and got[2][0].tolist() == [33, 0] and not got[2][1:].any()


def config(L_=64, o=0, Rg=16, K=8, ND=0, output=0, window=None, flags=0, size=None, device=-1):
    return L.PfbPdConfig(C.sizeof(L.PfbPdConfig) if size is None else size, L_, o, Rg, K, ND, output,
                         None if window is None else window.ctypes.data_as(C.POINTER(C.c_float)), flags, device)


def both(**kw):
    """the status of pfb_pd_describe and of pfb_pd_create for one config, their outputs untouched on failure"""
    lib = L.load()
    cfg = config(**kw)
    plan, h = L.PfbPdPlan(), C.c_void_p()
    C.memset(C.byref(plan), 0x5a, C.sizeof(plan))
    d = lib.pfb_pd_describe(C.byref(cfg), C.byref(plan))
    c = lib.pfb_pd_create(C.byref(cfg), C.byref(h))
    assert d == L.PFB_OK or bytes(plan) == b"\x5a" * C.sizeof(plan)
    assert not h.value or c == L.PFB_OK
    if h.value:
        lib.pfb_pd_destroy(h)
    return d, c


def test_arguments_are_checked_before_the_device_and_in_order():
    lib = L.load()
    BAD, UNS = L.PFB_ERR_BAD_ARG, L.PFB_ERR_UNSUPPORTED
    plan, h = L.PfbPdPlan(), C.c_void_p()
    cfg = config()
    assert lib.pfb_pd_describe(None, C.byref(plan)) == lib.pfb_pd_describe(C.byref(cfg), None) == BAD
    assert lib.pfb_pd_create(None, C.byref(h)) == lib.pfb_pd_create(C.byref(cfg), None) == BAD
    bad = [dict(size=44), dict(size=52), dict(L_=0), dict(Rg=0), dict(K=0), dict(Rg=65), dict(L_=5, Rg=6)]
    bad += [dict(K=9, ND=8), dict(K=1025), dict(K=1 << 31), dict(K=1025, ND=2048)]
    bad += [dict(ND=n) for n in (1, 2, 4, 7, 12, 24, 1000, 2048, 4096, 1 << 31)]
    bad += [dict(L_=(1 << 24) + 1, Rg=1), dict(L_=(1 << 32) - 1, Rg=1), dict(o=(1 << 62) + 1), dict(o=(1 << 64) - 1)]
    bad += [dict(output=4), dict(output=1 << 31), dict(flags=2), dict(flags=3), dict(flags=1 << 31)]
    for v in (np.nan, np.inf, -np.inf):
        w = np.ones(8, np.float32)
        w[5] = v
        bad.append(dict(window=w))
    for kw in bad:
        assert both(**kw) == (BAD, BAD), kw
        assert both(device=1 << 20, **kw) == (BAD, BAD), kw   # before the device is looked at
    # the carry: K R 8 bytes, 64 MiB allowed, one element more refused -- after every BAD_ARG check
    assert both(L_=1 << 24, Rg=(1 << 13) + 1, K=1024, device=1 << 20) == (UNS, UNS)
    assert both(L_=1 << 24, Rg=(1 << 13) + 1, K=1024, output=7, device=1 << 20) == (BAD, BAD)
    assert both(L_=1 << 24, Rg=(1 << 23) + 1, K=1, device=1 << 20) == (UNS, UNS)
    assert lib.pfb_pd_describe(C.byref(config(L_=1 << 24, Rg=1 << 13, K=1024)), C.byref(plan)) == L.PFB_OK
    assert plan.carry_bytes == 64 << 20
    # null handles and pointers
    u = C.c_uint64(7)
    buf = np.zeros(64, np.float32)
    p = C.c_void_p(buf.ctypes.data)
    assert lib.pfb_pd_destroy(None) == lib.pfb_pd_reset(None) == lib.pfb_pd_sync(None) == BAD
    assert lib.pfb_pd_set_stream(None, None) == lib.pfb_pd_get_device(None, None) == lib.pfb_pd_set_index(None, 0) == BAD
    assert lib.pfb_pd_next_index(None, C.byref(u)) == lib.pfb_pd_cpis_for(None, 5, C.byref(u)) == BAD
    assert lib.pfb_pd_process(None, p, 16, p, 1, C.byref(u), L.PFB_MEM_HOST) == BAD
    assert lib.pfb_pd_process(None, p, 16, p, 1, C.byref(u), 2) == BAD
    assert lib.pfb_pd_flush(None, p, 1, C.byref(u), L.PFB_MEM_HOST) == lib.pfb_pd_flush(None, p, 1, C.byref(u), 2) == BAD
    assert lib.pfb_pd_process_async(None, p, 16, p, 1, p) == BAD
    assert u.value == 7 and lib.pfb_pd_last_kernel(None) == b""
    with pytest.raises(ValueError):
        pd.describe_pulse_doppler(64, 8, 16, window=np.ones(7, np.float32))


def test_a_valid_config_needs_a_device():
    if L.load().pfb_device_count() > 0:
        pytest.skip("a GPU is present")
    for kw in (dict(), dict(L_=1, Rg=1, K=1), dict(L_=1 << 24, Rg=1 << 13, K=1024), dict(output=3, flags=1),
               dict(window=np.linspace(0, 1, 8).astype(np.float32)), dict(o=1 << 62), dict(K=8, ND=1024)):
        assert both(**kw) == (L.PFB_OK, L.PFB_ERR_NO_DEVICE), kw
    with pytest.raises(L.PfbError) as e:
        pd.PulseDoppler(64, 8, 16)
    assert e.value.status == L.PFB_ERR_NO_DEVICE
    with pytest.raises(L.PfbError) as e:
        pd.range_doppler(np.ones(1000, np.complex64), 64, 8)
    assert e.value.status == L.PFB_ERR_NO_DEVICE


def test_describe():
    for K in (1, 5, 8, 9, 100, 512, 513, 1024):
        assert pd.describe_pulse_doppler(4096, K, 10).doppler_length == R.doppler_length(K) == max(8, 1 << (K - 1).bit_length())
    names = {8: "<8>", 16: "<16>", 32: "<8,4>", 64: "<8,8>", 128: "<16,8>", 256: "<16,16>", 512: "<8,8,8>", 1024: "<16,8,8>"}
    for ND in R.LENGTHS:
        for output, per in (("complex", ND * 33), ("power", ND * 33), ("best", 33), ("noncoherent", 33)):
            for K in (1, ND):
                plan = pd.describe_pulse_doppler(100, K, 33, 5, None, ND, output, True)
                assert (plan.doppler_length, plan.carry_bytes, plan.cpi_samples, plan.cpi_outputs) == (ND, K * 33 * 8, (K - 1) * 100 + 33, per)
                if output == "noncoherent":
                    assert (plan.tile_gates, plan.kernel.decode()) == (256, "pfb_pd_noncoherent")
                else:
                    assert (plan.tile_gates, plan.kernel.decode()) == (P.tile_gates(ND), "pfb_pd_dft" + names[ND])
                    assert ND * plan.tile_gates * 8 <= 64 << 10    # two workgroups' tiles in a CU's 160 KiB
    base = bytes(pd.describe_pulse_doppler(100, 8, 33))
    assert bytes(pd.describe_pulse_doppler(100, 8, 33, origin=77, window=np.ones(8, np.float32), centered=True)) == base


def test_doppler_frequencies():
    lib = L.load()
    for ND in R.LENGTHS:
        for centered in (False, True):
            f = pd.doppler_frequencies(2048, ND, 56e6, centered)
            assert np.array_equal(f, R.frequencies(2048, ND, 56e6, centered)) and len(f) == ND
            assert f[ND // 2 if centered else 0] == 0.0 and abs((f[1] - f[0]) - 56e6 / (ND * 2048)) < 1e-9
    out = np.full(8, -1.0)
    po = out.ctypes.data_as(C.POINTER(C.c_double))
    cfg = config(K=5)   # doppler_length 0: the smallest of the set
    assert lib.pfb_pd_doppler_frequencies(C.byref(cfg), 64.0 * 8, po) == L.PFB_OK and out.tolist() == list(range(8))
    for kw, fs in ((dict(size=40), 1.0), (dict(L_=0), 1.0), (dict(K=0), 1.0), (dict(ND=12), 1.0), (dict(K=9, ND=8), 1.0),
                   (dict(flags=2), 1.0), (dict(), np.nan), (dict(), np.inf)):
        out[:] = -1.0
        assert lib.pfb_pd_doppler_frequencies(C.byref(config(**kw)), fs, po) == L.PFB_ERR_BAD_ARG and (out == -1.0).all()
    assert lib.pfb_pd_doppler_frequencies(None, 1.0, po) == lib.pfb_pd_doppler_frequencies(C.byref(cfg), 1.0, None) \
        == L.PFB_ERR_BAD_ARG


def test_doppler_frequencies_takes_a_resolved_length_only():
    """0, "the smallest length that holds num_pulses", names no length without num_pulses: the library would resolve it
    to 8 rows for the one pulse of the wrapper's config and write them into an array of 0 elements"""
    for centered in (False, True):
        with pytest.raises(ValueError):
            pd.doppler_frequencies(2048, 0, 56e6, centered)
        for bad in (4, 12, 2048):
            with pytest.raises(L.PfbError) as e:
                pd.doppler_frequencies(2048, bad, 56e6, centered)
            assert e.value.status == L.PFB_ERR_BAD_ARG
    # the array is as long as the plan says for every length the library takes
    for ND in R.LENGTHS:
        assert len(pd.doppler_frequencies(1, ND, 1.0)) == pd.describe_pulse_doppler(1, 1, 1, doppler_length=ND).doppler_length == ND


def test_exports():
    lib = L.load()
    declared = {n for n in declared_symbols() if n.startswith("pfb_pd_")}
    assert declared == PD_EXPORTS == {n for n in L.EXPORTS if n.startswith("pfb_pd_")}
    for name in PD_EXPORTS:
        assert hasattr(lib, name), name
    assert (C.sizeof(L.PfbPdConfig), C.sizeof(L.PfbPdPlan), pd.CELL_DTYPE.itemsize, C.sizeof(L.PfbMfbankCell)) == (48, 64, 8, 8)
    assert pd.CELL_DTYPE == R.CELL
    assert (L.PFB_PD_COMPLEX, L.PFB_PD_POWER, L.PFB_PD_BEST, L.PFB_PD_NONCOHERENT, L.PFB_PD_CENTERED) == (0, 1, 2, 3, 1)
    assert (R.COMPLEX, R.POWER, R.BEST, R.NONCOHERENT) == (0, 1, 2, 3)
    hdr = open(os.path.join(ROOT, "include", "pfb_channelizer.h")).read()
    assert "PFB_PD_COMPLEX = 0, PFB_PD_POWER = 1, PFB_PD_BEST = 2, PFB_PD_NONCOHERENT = 3" in hdr
    assert "PFB_PD_CENTERED = 1u << 0" in hdr
    assert "#define PFB_ABI_VERSION 2" in hdr and lib.pfb_abi_version() == 2
    assert hdr.index("pfb_pd_describe(") > hdr.index("pfb_cfar_last_kernel(")   # its own section, after the detector's
    assert "SAME BITS COME OUT UNDER ANY CUTTING" in hdr
    import sdr_channelizer_amd as pkg
    names = ["PulseDoppler", "range_doppler", "doppler_frequencies", "detect_pulse_train"]
    at = pkg.__all__.index("Cfar")
    assert pkg.__all__[at - len(names):at] == names
    for name in names:
        assert getattr(pkg, name) is getattr(pd, name)


def test_the_struct_layouts_are_the_compilers(tmp_path):
    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.skip("no gcc")
    lines, want = [], []
    for cname, cls in (("pfb_pd_config", L.PfbPdConfig), ("pfb_pd_plan", L.PfbPdPlan)):
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


def test_pd_entry_points_sit_under_the_abi_guard():
    src = open(os.path.join(ROOT, "sdr_channelizer_amd", "csrc", "pfb_pd.hip")).read()
    found = {}
    for m in re.finditer(r'^extern "C" int (\w+)\(', src, re.M):
        rest = src[m.start():]
        found[m.group(1)] = rest[: rest.index("\n}\n")]
    assert set(found) == PD_EXPORTS - {"pfb_pd_last_kernel"}
    for name, body in found.items():
        assert "abi_guard" in body.split("{", 1)[1][:80], name
    assert src.count('extern "C"') == len(found) + 1
    from sdr_channelizer_amd import build
    assert "pfb_pd.hip" in build.SOURCES
    create = src[src.index("int create_pd("):]
    create = create[: create.index("\n}\n")]
    assert create.index("pd_check(cfg") < create.index("resolve_device") < create.index("allocate_pd(")
    for word in ("atomic", "asm", "mfma"):
        assert word not in re.sub(r"//.*", "", src).lower(), word


# -- the designs test_gpu_pd.py relies on, on the restatement alone ----------------------------------------------
@pytest.mark.parametrize("nd", R.LENGTHS)
def test_the_grid_streams_have_a_clear_strongest_row(nd):
    """at most 5 % of the gates of the grid's streams (K > 1) have a maximum within twice the power allowance of the
    runner-up; K = 1 is the exact tie of test_ties_are_exact_in_the_reference and is checked as one"""
    T = P.tile_gates(nd)
    assert {s[1] for s in P.shapes(nd)} == {1, T - 1, T, T + 1, 2 * T + 3} and {s[0] for s in P.shapes(nd)} == {1, nd // 2 + 1, nd - 1, nd}
    gates = unclear = hits = 0
    for i, (K, Rg, L_) in enumerate(P.shapes(nd)):
        if K == 1:
            continue
        x, o = P.grid_stream(nd, K, Rg, L_, i)
        w = P.grid_window(K, i)
        for c in (0, 1):
            A = R.gates(x, c, o, L_, Rg, K)
            Pw = R.power(R.transform(A, w, nd, P.grid_flags(i)[0]))
            ok = P.clear_gates(Pw, A, w)
            gates += Rg
            unclear += int((~ok).sum())
            bp, bh = R.best(Pw, nd, P.grid_flags(i)[0])
            hits += int((bh % nd == P.tone_row(nd, c, np.arange(Rg))).sum())
    assert gates > 0 and unclear <= 0.05 * gates, (unclear, gates)
    assert hits > 0.9 * gates    # it is the tone that makes the maximum clear (the GPU module checks against best())


def test_ties_are_exact_in_the_reference():
    for nd in (8, 64, 1024):
        x = P.tie_stream(nd - 1, 5, 9, nd)
        A = R.gates(x, 0, 0, 9, 5, nd - 1)
        assert A[0].all() and not A[1:].any()
        Pw = R.power(R.transform(A, None, nd))
        assert (np.abs(Pw - Pw[0]) <= 1e-12 * Pw[0]).all()          # one value per gate, to float64 rounding
        assert R.best(np.tile(Pw[0], (nd, 1)), nd, False)[1].tolist() == [0] * 5
        assert R.best(np.tile(Pw[0], (nd, 1)), nd, True)[1].tolist() == [-nd // 2] * 5


@pytest.mark.parametrize("nd", [8, 64, 1024])
def test_designed_tones_land_in_their_rows(nd):
    d0 = (np.arange(nd) * 5 + 3) % nd if nd <= 64 else np.array([0, 1, nd // 2 - 1, nd // 2, nd // 2 + 1, nd - 1, 700 % nd])
    x = P.tone_stream(nd, len(d0), len(d0) + 2, d0)
    A = R.gates(x, 0, 0, len(d0) + 2, len(d0), nd)
    Pw = R.power(R.transform(A, None, nd))
    bp, bh = R.best(Pw, nd)
    assert bh.tolist() == d0.tolist() and np.abs(bp - nd * nd).max() < 1e-3 * nd * nd
    assert P.clear_gates(Pw, A, None).all()
    signed = R.best(R.power(R.transform(A, None, nd, True)), nd, True)[1]
    assert signed.tolist() == [int(d) - nd if d >= nd // 2 else int(d) for d in d0]


def test_the_train_is_under_the_single_pulse_threshold():
    a_single, a_train = P.chain_alphas(cfar.cfar_alpha)
    iq = P.chain_stream()
    r = P.chain_replica()
    assert r.size == 104 and iq.shape == (P.CHAIN_CPIS * P.CHAIN_K * P.CHAIN["pri"], 2)
    # per sample 20 dB under the noise; compressed, level with it: nothing for a detector of single pulses
    snr = P.CHAIN["amplitude"] ** 2 / (2 * P.CHAIN["noise_sigma"] ** 2)
    assert 0.9 < snr * r.size < 1.1
    gate = P.CHAIN["first_pulse"]
    for bins in (0, 5):
        single, train = P.chain_reference(iq if bins == 0 else P.chain_shift(iq, bins), a_single, a_train)
        assert len(single) == 0
        assert train == [(c, gate, bins) for c in range(P.CHAIN_CPIS)]
