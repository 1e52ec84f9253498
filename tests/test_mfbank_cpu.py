"""The matched-filter bank's contract without a GPU: the numpy restatement (mfbank_ref) against the definition, the
rotation identity and the -0.91 dB bound the kernel's header quotes, every argument check that comes before the device
and their order, the plan, the struct sizes, the exports and the ABI guard, and pfb_mfbank_frequencies."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import mf_ref as R
import mfbank_ref as B
from abi_symbols import declared_symbols
from sdr_channelizer_amd import _lib as L
from sdr_channelizer_amd import mf_bank as bank

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BANK_EXPORTS = {"pfb_mfbank_describe", "pfb_mfbank_frequencies", "pfb_mfbank_create", "pfb_mfbank_destroy",
                "pfb_mfbank_reset", "pfb_mfbank_set_stream", "pfb_mfbank_sync", "pfb_mfbank_get_device",
                "pfb_mfbank_outputs_for", "pfb_mfbank_next_index", "pfb_mfbank_process", "pfb_mfbank_process_async",
                "pfb_mfbank_process_iq_file", "pfb_mfbank_last_kernel"}


@pytest.mark.parametrize("K,first_bin,H,step", [(1, 0, 1, 1), (2, -1, 3, 1), (5, -8, 4, 3), (7, 30, 5, 1)])
@pytest.mark.parametrize("normalize", [False, True])
def test_restatement_is_the_definition(K, first_bin, H, step, normalize):
    nfft = 64   # q_h = 30 .. 34 wraps past nfft/2
    r = R.random_replica(K, K)
    for n in (0, K - 1, K, 2 * K + 5):
        x = R.unpack(R.random_raw("int16", 12, n, n + 1), "int16", 12)
        want = B.surface_loop(x, r, first_bin, H, step, nfft, normalize)
        got = B.surface(x, r, first_bin, H, step, nfft, normalize)
        assert got.shape == want.shape == (H, max(0, n - K + 1))
        if want.size:
            assert np.abs(got - want).max() <= 1e-12 * R.gain(r, normalize) * R.bound(x, r)
    # hypothesis 0 of a bank that starts at bin 0 is the matched filter itself
    x = R.unpack(R.random_raw("cf32", 1, 40, 3), "cf32", 1)
    assert np.array_equal(B.surface(x, r, 0, 2, 5, nfft, normalize)[0], R.compress(x, r, normalize))


def test_selection_rule():
    nan = np.nan
    p = np.array([[1.0, 2.0, nan, 1.0, 0.0],
                  [1.0, 3.0, 5.0, nan, 0.0],
                  [2.0, 3.0, 6.0, 0.5, 0.0]])
    bp, bh = B.best(p)
    assert bh.tolist() == [2, 1, 0, 0, 0] and bh.dtype == np.int32   # ties to the lowest h; a NaN at h = 0 stays
    assert bp[[0, 1, 3, 4]].tolist() == [2.0, 3.0, 1.0, 0.0] and np.isnan(bp[2])


@pytest.mark.parametrize("nfft", [1024, 2048, 4096])
def test_rotation_identity_and_the_midpoint_loss(nfft):
    """the two facts the kernel rests on, in float64"""
    K = nfft // 2
    r = R.random_replica(K, nfft).astype(np.complex128)
    n = np.arange(nfft)
    spec = np.fft.fft(np.conj(np.concatenate([r, np.zeros(nfft - K)])))   # R[c] = sum conj(r[n]) e^{-j 2 pi n c / N}
    for q in (1, 37, nfft // 2, nfft - 1, -5):
        rq = np.zeros(nfft, np.complex128)
        rq[:K] = B.modulated(r, q, nfft)
        assert np.abs(np.fft.fft(np.conj(rq)) - spec[(n + q) % nfft]).max() <= 1e-12 * np.abs(spec).max()
    # a constant-envelope pulse half a bin from the nearest hypothesis keeps sinc(K / (2 nfft)) of its amplitude
    for k, least in ((K, 0.900), (K // 2, 0.974), (13, 0.999)):
        pulse = np.exp(2j * np.pi * 0.5 * np.arange(k) / nfft)
        kept = abs(np.vdot(np.ones(k), pulse)) / k
        assert abs(kept - np.sinc(k / (2 * nfft))) < 1e-4 and kept >= least
    assert abs(20 * np.log10(np.sinc(0.25)) + 0.91) < 0.005


def config(K=13, replica=None, fmt=L.PFB_FMT_INT16_IQ, bw=12, output=0, flags=0, nfft=0, first_bin=0, H=1, step=1,
           size=None, device=-1, keep=[]):
    r = np.ones(2 * K, np.float32) if replica is None else np.ascontiguousarray(replica, np.float32)
    keep.append(r)  # the config holds a bare pointer
    return L.PfbMfbankConfig(C.sizeof(L.PfbMfbankConfig) if size is None else size, K,
                             r.ctypes.data_as(C.POINTER(C.c_float)), fmt, bw, output, flags, nfft, first_bin, H, step, device)


def both(**kw):
    """the status of pfb_mfbank_describe and of pfb_mfbank_create for one config: the same before the device"""
    lib = L.load()
    cfg = config(**kw)
    plan, h = L.PfbMfbankPlan(), C.c_void_p()
    d = lib.pfb_mfbank_describe(C.byref(cfg), C.byref(plan))
    c = lib.pfb_mfbank_create(C.byref(cfg), C.byref(h))
    assert not h.value or c == L.PFB_OK
    if h.value:
        lib.pfb_mfbank_destroy(h)
    return d, c


def test_arguments_are_checked_before_the_device_and_in_order():
    lib = L.load()
    BAD, FMT, UNS = L.PFB_ERR_BAD_ARG, L.PFB_ERR_BAD_FORMAT, L.PFB_ERR_UNSUPPORTED
    plan, h = L.PfbMfbankPlan(), C.c_void_p()
    cfg = config()
    assert lib.pfb_mfbank_describe(None, C.byref(plan)) == lib.pfb_mfbank_describe(C.byref(cfg), None) == BAD
    assert lib.pfb_mfbank_create(None, C.byref(h)) == lib.pfb_mfbank_create(C.byref(cfg), None) == BAD
    assert both(size=48) == (BAD, BAD)
    null = config()
    null.replica = None
    assert lib.pfb_mfbank_describe(C.byref(null), C.byref(plan)) == lib.pfb_mfbank_create(C.byref(null), C.byref(h)) == BAD
    assert both(K=0) == (BAD, BAD)
    assert both(output=2) == (BAD, BAD)
    for bit in (2, 4, 1 << 31):
        assert both(flags=bit) == (BAD, BAD)
    for nfft in (1, 512, 1023, 1025, 3072, 8192):
        assert both(nfft=nfft) == (BAD, BAD)
    assert both(step=0) == (BAD, BAD) and both(H=0) == (BAD, BAD)
    for nfft, H, step in ((1024, 1025, 1), (1024, 342, 3), (0, 4097, 1), (2048, 2, 1025), (4096, 1 << 31, 2)):
        assert both(nfft=nfft, H=H, step=step) == (BAD, BAD), (nfft, H, step)
    for bad in (np.nan, np.inf, -np.inf):
        r = np.ones(26, np.float32)
        r[7] = bad
        assert both(replica=r) == (BAD, BAD)
    assert both(replica=np.zeros(26, np.float32), flags=L.PFB_MF_NORMALIZE) == (BAD, BAD)
    assert both(fmt=3) == (FMT, FMT)
    for fmt, bad in ((L.PFB_FMT_INT8_IQ, (0, 9)), (L.PFB_FMT_INT16_IQ, (0, 17))):
        for bw in bad:
            assert both(fmt=fmt, bw=bw) == (FMT, FMT), (fmt, bw)
    # a replica too long for the bank: the code pfb_mf_create gives PFB_MF_ROUTE_FUSED with K > fft_length/2
    for nfft, K in ((0, 2049), (1024, 513), (2048, 1025), (4096, 2049), (0, 65537)):
        assert both(K=K, nfft=nfft) == (UNS, UNS), (nfft, K)
        if K <= 65536:
            r = np.ones(2 * K, np.float32)
            mcfg = L.PfbMfConfig(C.sizeof(L.PfbMfConfig), K, r.ctypes.data_as(C.POINTER(C.c_float)), L.PFB_FMT_INT16_IQ,
                                 12, 0, 0, nfft, L.PFB_MF_ROUTE_FUSED, -1)
            assert lib.pfb_mf_describe(C.byref(mcfg), C.byref(L.PfbMfPlan())) == UNS
    # the order of the list: arguments, then formats, then what is unsupported
    assert both(K=0, fmt=3) == (BAD, BAD) and both(output=2, fmt=3) == (BAD, BAD) and both(nfft=7, K=65537) == (BAD, BAD)
    assert both(H=0, fmt=3) == (BAD, BAD) and both(step=0, K=3000) == (BAD, BAD)
    assert both(fmt=3, K=3000) == (FMT, FMT) and both(fmt=L.PFB_FMT_INT8_IQ, bw=9, K=600, nfft=1024) == (FMT, FMT)
    r = np.ones(2 * 3000, np.float32)
    r[-1] = np.nan
    assert both(K=3000, replica=r) == (BAD, BAD)
    assert not h.value
    # null handles and pointers
    u = C.c_uint64()
    buf = np.zeros(64, np.int16)
    p = C.c_void_p(buf.ctypes.data)
    assert lib.pfb_mfbank_destroy(None) == lib.pfb_mfbank_reset(None) == lib.pfb_mfbank_sync(None) == BAD
    assert lib.pfb_mfbank_set_stream(None, None) == lib.pfb_mfbank_get_device(None, None) == BAD
    assert lib.pfb_mfbank_outputs_for(None, 5, C.byref(u)) == lib.pfb_mfbank_next_index(None, C.byref(u)) == BAD
    assert lib.pfb_mfbank_process(None, p, 32, p, 1, 1, C.byref(u), L.PFB_MEM_HOST) == BAD
    assert lib.pfb_mfbank_process_async(None, p, 32, p, 1, 1, C.byref(u)) == BAD
    assert lib.pfb_mfbank_process_iq_file(None, b"x.iq", p, 1, 1, C.byref(u), None) == BAD
    assert lib.pfb_mfbank_last_kernel(None) == b""


def test_a_valid_config_needs_a_device():
    lib = L.load()
    if lib.pfb_device_count() > 0:
        pytest.skip("a GPU is present")
    for kw in (dict(), dict(K=1), dict(K=2048), dict(K=512, nfft=1024), dict(fmt=L.PFB_FMT_CF32, bw=99),
               dict(nfft=1024, H=1024), dict(nfft=2048, H=512, step=4, first_bin=-(1 << 31)), dict(flags=1, output=1)):
        assert both(**kw) == (L.PFB_OK, L.PFB_ERR_NO_DEVICE), kw


def test_no_cpu_fallback():
    if L.load().pfb_device_count() > 0:
        pytest.skip("a GPU is present")
    with pytest.raises(L.PfbError) as e:
        bank.MatchedFilterBank(np.ones(13, np.complex64), first_bin=-2, num_hypotheses=5)
    assert e.value.status == L.PFB_ERR_NO_DEVICE
    with pytest.raises(L.PfbError) as e:
        bank.compress_bank(np.zeros((100, 2), np.int16), np.ones(13, np.complex64), first_bin=0, num_hypotheses=2)
    assert e.value.status == L.PFB_ERR_NO_DEVICE


@pytest.mark.parametrize("nfft", [0, 1024, 2048, 4096])
def test_describe(nfft):
    N = nfft or 4096
    for K in (1, 13, N // 2 - 1, N // 2):
        for H, output in ((1, "best"), (17, "surface"), (N, "best")):
            plan = bank.describe_bank(R.random_replica(K, K), first_bin=-3, num_hypotheses=H, output=output,
                                      fft_length=nfft)
            assert (plan.fft_length, plan.block_outputs, plan.num_hypotheses, plan.lds_bytes) == (N, N - K + 1, H, 16 * N)
    base = bank.describe_bank(R.random_replica(300, 1), first_bin=0, num_hypotheses=4, fft_length=nfft)
    for kw in (dict(sample_format="int8", bit_width=8), dict(sample_format="cf32"), dict(normalize=True)):
        assert bytes(bank.describe_bank(R.random_replica(300, 1), first_bin=9, num_hypotheses=4, fft_length=nfft, **kw)) \
            == bytes(base), kw


def test_frequencies():
    lib = L.load()
    fs = 56e6
    for nfft, first_bin, H, step in ((1024, -8, 17, 1), (0, -3, 7, 2), (2048, 1000, 30, 3), (4096, -(1 << 31), 2, 1)):
        got = bank.bank_frequencies(fs, first_bin=first_bin, num_hypotheses=H, bin_step=step, fft_length=nfft)
        want = B.frequencies(fs, first_bin, H, step, nfft or 4096)
        assert got.dtype == np.float64 and np.array_equal(got, want), (nfft, first_bin)
    got = bank.bank_frequencies(1024.0, first_bin=-2, num_hypotheses=5, fft_length=1024)
    assert got.tolist() == [-2.0, -1.0, 0.0, 1.0, 2.0]
    out = np.zeros(8)
    po = out.ctypes.data_as(C.POINTER(C.c_double))
    cfg = config(H=4)
    assert lib.pfb_mfbank_frequencies(None, fs, po) == lib.pfb_mfbank_frequencies(C.byref(cfg), fs, None) == L.PFB_ERR_BAD_ARG
    assert lib.pfb_mfbank_frequencies(C.byref(cfg), np.nan, po) == L.PFB_ERR_BAD_ARG
    for kw in (dict(size=8), dict(H=0), dict(step=0), dict(nfft=512), dict(nfft=1024, H=600, step=2)):
        assert lib.pfb_mfbank_frequencies(C.byref(config(**kw)), fs, po) == L.PFB_ERR_BAD_ARG, kw
    assert not out.any()


def test_exports():
    lib = L.load()
    declared = {n for n in declared_symbols() if n.startswith("pfb_mfbank_")}
    assert declared == BANK_EXPORTS == {n for n in L.EXPORTS if n.startswith("pfb_mfbank_")}
    for name in BANK_EXPORTS:
        assert hasattr(lib, name), name
    assert C.sizeof(L.PfbMfbankConfig) == 56 and C.sizeof(L.PfbMfbankPlan) == 16 and C.sizeof(L.PfbMfbankCell) == 8
    assert (L.PFB_MFBANK_BEST, L.PFB_MFBANK_SURFACE) == (0, 1)
    hdr = open(os.path.join(ROOT, "include", "pfb_channelizer.h")).read()
    assert "PFB_MFBANK_BEST = 0, PFB_MFBANK_SURFACE = 1" in hdr and "#define PFB_ABI_VERSION 2" in hdr
    assert hdr.index("pfb_mfbank_describe") > hdr.index("pfb_chsyn_last_kernel")   # its own section, after the synthesizer's
    import sdr_channelizer_amd as pkg
    names = ["MatchedFilterBank", "compress_bank", "bank_frequencies", "pulse_delay_and_offset_from_iq_files"]
    assert pkg.__all__[-4:] == names
    for name in names:
        assert getattr(pkg, name) is getattr(bank, name)


def test_the_struct_sizes_are_the_compilers(tmp_path):
    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.skip("no gcc")
    src = tmp_path / "sizes.c"
    src.write_text('#include "pfb_channelizer.h"\n#include <stdio.h>\n#include <stddef.h>\nint main(void) {\n'
                   '  printf("%zu %zu %zu %zu %zu %zu\\n", sizeof(pfb_mfbank_config), sizeof(pfb_mfbank_plan),\n'
                   '         sizeof(pfb_mfbank_cell), offsetof(pfb_mfbank_config, first_bin),\n'
                   '         offsetof(pfb_mfbank_config, device_id), offsetof(pfb_mfbank_cell, hypothesis));\n'
                   '  return 0;\n}\n')
    exe = tmp_path / "sizes"
    subprocess.run([gcc, "-std=c99", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)],
                   check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert r.stdout.split() == [str(C.sizeof(L.PfbMfbankConfig)), str(C.sizeof(L.PfbMfbankPlan)),
                                str(C.sizeof(L.PfbMfbankCell)), str(L.PfbMfbankConfig.first_bin.offset),
                                str(L.PfbMfbankConfig.device_id.offset), str(L.PfbMfbankCell.hypothesis.offset)]


def test_mfbank_entry_points_sit_under_the_abi_guard():
    src = open(os.path.join(ROOT, "sdr_channelizer_amd", "csrc", "pfb_mfbank.hip")).read()
    found = {}
    for m in re.finditer(r'^extern "C" int (\w+)\(', src, re.M):
        rest = src[m.start():]
        found[m.group(1)] = rest[: rest.index("\n}\n")]
    assert set(found) == BANK_EXPORTS - {"pfb_mfbank_last_kernel"}
    for name, body in found.items():
        assert "abi_guard" in body.split("{", 1)[1][:80], name
    rest = [ln for ln in src.splitlines() if ln.startswith('extern "C"') and not ln.startswith('extern "C" int ')]
    assert rest == ['extern "C" const char* pfb_mfbank_last_kernel(const pfb_mfbank_handle* h) '
                    '{ return h ? h->last_kernel : ""; }']
    assert src.count('extern "C"') == len(found) + 1
    from sdr_channelizer_amd import build
    assert "pfb_mfbank.hip" in build.SOURCES
    # the device is resolved after every argument check: NO_DEVICE comes last; the allocations are the shared ones
    create = src[src.index("int create_bank("):]
    create = create[: create.index("\n}\n")]
    assert create.index("bank_check(cfg") < create.index("resolve_device") < create.index("st.allocate(")
    shared = open(os.path.join(ROOT, "sdr_channelizer_amd", "csrc", "pfb_ols_host.cpp")).read()
    allocate = shared[shared.index("hipError_t OlsStream::allocate("):]
    assert "hipMalloc" in allocate[: allocate.index("\n}\n")] and "hipMalloc" not in create
    assert "atomic" not in src.split("#include", 1)[1]
