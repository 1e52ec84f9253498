"""The matched filter's contract without a GPU: the numpy restatement (mf_ref) against the definition, every argument
check that comes before the device and their order, the plan pfb_mf_describe reports, the exports and the ABI guard,
and the helpers the GPU tests derive local allowances and block sets from (mf_ref.span_tolerance, block_span,
outputs_seeing) against the plan and a plain enumeration."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import mf_ref as R
from abi_symbols import declared_symbols
from sdr_channelizer_amd import _lib as L
from sdr_channelizer_amd import matched_filter as mf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MF_EXPORTS = {"pfb_mf_describe", "pfb_mf_create", "pfb_mf_destroy", "pfb_mf_reset", "pfb_mf_set_stream", "pfb_mf_sync",
              "pfb_mf_get_device", "pfb_mf_outputs_for", "pfb_mf_next_index", "pfb_mf_process", "pfb_mf_process_async",
              "pfb_mf_process_iq_file", "pfb_mf_last_kernel"}
MIB64 = 64 << 20


@pytest.mark.parametrize("K", [1, 2, 13, 64])
@pytest.mark.parametrize("normalize", [False, True])
def test_restatement_is_the_definition(K, normalize):
    r = R.random_replica(K, K)
    for n in (0, K - 1, K, K + 1, 3 * K + 7):
        x = R.unpack(R.random_raw("int16", 12, n, n + 1), "int16", 12)
        want = R.compress_loop(x, r, normalize)
        got = R.compress(x, r, normalize)
        assert got.shape == want.shape == (max(0, n - K + 1),)
        if want.size:
            assert np.abs(got - want).max() <= 1e-12 * R.gain(r, normalize) * R.bound(x, r)
            assert np.abs(want).max() <= R.gain(r, normalize) * R.bound(x, r) * (1 + 1e-12)   # Cauchy-Schwarz
    # a copy of the replica with amplitude A gives A at the match under normalize
    x = np.zeros(5 * K + 3, np.complex128)
    x[K + 2: 2 * K + 2] = 0.25 * r
    y = R.compress(x, r, True)
    assert abs(y[K + 2] - 0.25) < 1e-12 and int(np.argmax(np.abs(y))) == K + 2


def test_bound_is_the_windowed_norm():
    x = R.unpack(R.random_raw("cf32", 1, 300, 3), "cf32", 1)
    r = R.random_replica(17, 4)
    direct = np.sqrt(np.sum(np.abs(r.astype(np.complex128)) ** 2)) * \
        max(np.sqrt(np.sum(np.abs(x[m:m + 17]) ** 2)) for m in range(300 - 17 + 1))
    assert abs(R.bound(x, r) - direct) <= 1e-12 * direct
    assert R.bound(x[:16], r) == 0.0 and R.tolerance(x, r) == 1e-5 * R.bound(x, r)


def test_span_tolerance_is_the_slice_alone():
    x = R.unpack(R.random_raw("cf32", 1, 400, 5), "cf32", 1)
    x[150:250] *= 1e3   # a loud stretch
    r = R.random_replica(17, 6)
    for normalize in (False, True):
        quiet = R.span_tolerance(x, r, 0, 150, normalize)
        assert quiet == R.tolerance(x[:150], r, normalize) == R.TOL * R.gain(r, normalize) * R.bound(x[:150], r)
        assert R.span_tolerance(x, r, 0, 151, normalize) > 10 * quiet   # one loud sample in the span
        assert R.span_tolerance(x, r, 0, 400, normalize) == R.tolerance(x, r, normalize) > 100 * quiet
    assert R.span_tolerance(x, r, 10, 26) == 0.0 and R.span_tolerance(x, r, 10, 27) > 0.0   # shorter than a window


@pytest.mark.parametrize("route,nfft,K", [("fused", 1024, 1), ("fused", 1024, 300), ("fused", 1024, 512),
                                          ("fused", 4096, 2048), ("partitioned", 1024, 1), ("partitioned", 1024, 512),
                                          ("partitioned", 1024, 513), ("partitioned", 1024, 700),
                                          ("partitioned", 4096, 5600)])
def test_block_spans_and_the_outputs_that_see_a_sample(route, nfft, K):
    plan = mf.describe(R.random_replica(K, 1), fft_length=nfft, route=route)
    V = R.block_outputs(route, nfft, K)
    assert V == plan.block_outputs
    for outputs in (1, V - 1, V, V + 1, 5 * V + 3):
        total = outputs + K - 1
        blocks = -(-outputs // V)
        spans = [R.block_span(route, nfft, K, b) for b in range(blocks)]
        for b, (lo, hi) in enumerate(spans):
            # a block's span holds the windows of all its outputs, and starts at its first output
            assert lo == b * V and hi >= lo + V + K - 1
            assert hi - lo == (nfft if route == "fused" else (plan.partitions + 1) * (nfft // 2))
        for s in sorted({0, 1, K - 1, V - 1, V, nfft - 1, nfft, total // 2, total - 1} & set(range(total))):
            seeing = [b for b, (lo, hi) in enumerate(spans) if lo <= s < hi]
            lo, hi = R.outputs_seeing(route, nfft, K, s, outputs)
            if not seeing:
                assert lo == hi
                continue
            assert seeing == list(range(seeing[0], seeing[-1] + 1))
            assert (lo, hi) == (seeing[0] * V, min((seeing[-1] + 1) * V, outputs))
            # every output whose window holds s is among them
            assert lo <= max(0, s - K + 1) and min(s, outputs - 1) < hi


def config(K=13, replica=None, fmt=L.PFB_FMT_INT16_IQ, bw=12, output=0, flags=0, nfft=0, route=0, size=None, device=-1,
           keep=[]):
    r = np.ones(2 * K, np.float32) if replica is None else np.ascontiguousarray(replica, np.float32)
    keep.append(r)  # the config holds a bare pointer
    return L.PfbMfConfig(C.sizeof(L.PfbMfConfig) if size is None else size, K, r.ctypes.data_as(C.POINTER(C.c_float)),
                         fmt, bw, output, flags, nfft, route, device)


def both(**kw):
    """the status of pfb_mf_describe and of pfb_mf_create for one config: the same before the device"""
    lib = L.load()
    cfg = config(**kw)
    plan, h = L.PfbMfPlan(), C.c_void_p()
    d = lib.pfb_mf_describe(C.byref(cfg), C.byref(plan))
    c = lib.pfb_mf_create(C.byref(cfg), C.byref(h))
    assert not h.value or c == L.PFB_OK
    if h.value:
        lib.pfb_mf_destroy(h)
    return d, c


def test_arguments_are_checked_before_the_device_and_in_order():
    lib = L.load()
    BAD, FMT, UNS = L.PFB_ERR_BAD_ARG, L.PFB_ERR_BAD_FORMAT, L.PFB_ERR_UNSUPPORTED
    plan, h = L.PfbMfPlan(), C.c_void_p()
    cfg = config()
    assert lib.pfb_mf_describe(None, C.byref(plan)) == lib.pfb_mf_describe(C.byref(cfg), None) == BAD
    assert lib.pfb_mf_create(None, C.byref(h)) == lib.pfb_mf_create(C.byref(cfg), None) == BAD
    assert both(size=40) == (BAD, BAD)
    null = config()
    null.replica = None
    assert lib.pfb_mf_describe(C.byref(null), C.byref(plan)) == lib.pfb_mf_create(C.byref(null), C.byref(h)) == BAD
    assert both(K=0) == (BAD, BAD)
    for bad in (np.nan, np.inf, -np.inf):
        r = np.ones(26, np.float32)
        r[7] = bad
        assert both(replica=r) == (BAD, BAD)
    assert both(replica=np.zeros(26, np.float32), flags=L.PFB_MF_NORMALIZE) == (BAD, BAD)
    assert both(output=2) == (BAD, BAD) and both(route=3) == (BAD, BAD)
    for bit in (2, 4, 1 << 31):
        assert both(flags=bit) == (BAD, BAD)
    for nfft in (1, 512, 1023, 1025, 3072, 8192):
        assert both(nfft=nfft) == (BAD, BAD)
    assert both(fmt=3) == (FMT, FMT)
    for fmt, bad in ((L.PFB_FMT_INT8_IQ, (0, 9)), (L.PFB_FMT_INT16_IQ, (0, 17))):
        for bw in bad:
            assert both(fmt=fmt, bw=bw) == (FMT, FMT), (fmt, bw)
    assert both(K=65537) == (UNS, UNS)
    for nfft, K in ((0, 2049), (1024, 513), (2048, 1025), (4096, 2049)):
        assert both(K=K, nfft=nfft, route=L.PFB_MF_ROUTE_FUSED) == (UNS, UNS), (nfft, K)
    # the order of the list: arguments, then formats, then what is unsupported
    assert both(K=0, fmt=3) == (BAD, BAD) and both(output=2, fmt=3) == (BAD, BAD) and both(nfft=7, K=65537) == (BAD, BAD)
    assert both(fmt=3, K=65537) == (FMT, FMT) and both(fmt=L.PFB_FMT_INT8_IQ, bw=9, K=600, nfft=1024, route=1) == (FMT, FMT)
    r = np.ones(2 * 65537, np.float32)
    r[-1] = np.nan
    assert both(K=65537, replica=r) == (BAD, BAD)
    assert not h.value
    # null handles and pointers
    u = C.c_uint64()
    buf = np.zeros(64, np.int16)
    p = C.c_void_p(buf.ctypes.data)
    assert lib.pfb_mf_destroy(None) == lib.pfb_mf_reset(None) == lib.pfb_mf_sync(None) == BAD
    assert lib.pfb_mf_set_stream(None, None) == lib.pfb_mf_get_device(None, None) == BAD
    assert lib.pfb_mf_outputs_for(None, 5, C.byref(u)) == lib.pfb_mf_next_index(None, C.byref(u)) == BAD
    assert lib.pfb_mf_process(None, p, 32, p, 1, C.byref(u), L.PFB_MEM_HOST) == BAD
    assert lib.pfb_mf_process_async(None, p, 32, p, 1, C.byref(u)) == BAD
    assert lib.pfb_mf_process_iq_file(None, b"x.iq", p, 1, C.byref(u), None) == BAD
    assert lib.pfb_mf_last_kernel(None) == b""


def test_a_valid_config_needs_a_device():
    lib = L.load()
    if lib.pfb_device_count() > 0:
        pytest.skip("a GPU is present")
    for kw in (dict(), dict(K=1), dict(K=65536), dict(fmt=L.PFB_FMT_CF32, bw=99), dict(K=2048, route=1),
               dict(K=513, nfft=1024, route=2), dict(flags=1, output=1)):
        assert both(**kw) == (L.PFB_OK, L.PFB_ERR_NO_DEVICE), kw


def test_no_cpu_fallback():
    if L.load().pfb_device_count() > 0:
        pytest.skip("a GPU is present")
    with pytest.raises(L.PfbError) as e:
        mf.MatchedFilter(np.ones(13, np.complex64))
    assert e.value.status == L.PFB_ERR_NO_DEVICE
    with pytest.raises(L.PfbError) as e:
        mf.compress(np.zeros((100, 2), np.int16), np.ones(13, np.complex64))
    assert e.value.status == L.PFB_ERR_NO_DEVICE


@pytest.mark.parametrize("K", [1, 13, 512, 513, 2048, 2049, 5600, 56000, 65536])
def test_describe_invariants(K):
    r = R.random_replica(K, K)
    seen = set()
    for route in ("auto", "fused", "partitioned"):
        for nfft in (0, 1024, 2048, 4096):
            try:
                plan = mf.describe(r, fft_length=nfft, route=route)
            except L.PfbError as e:
                assert e.status == L.PFB_ERR_UNSUPPORTED and route == "fused" and K > (nfft // 2 if nfft else 2048)
                continue
            N = plan.fft_length
            assert N in (1024, 2048, 4096) and (nfft == 0 or N == nfft)
            seen.add(plan.route)
            if plan.route == L.PFB_MF_ROUTE_FUSED:
                assert route != "partitioned" and K <= N // 2
                assert plan.partitions == 1 and plan.block_outputs == N - K + 1 and plan.workspace_bytes == 0
                if nfft == 0:   # the measured rule of the header
                    assert N == (1024 if K <= 64 else 2048 if K <= 1024 else 4096)
            else:
                assert plan.route == L.PFB_MF_ROUTE_PARTITIONED and route != "fused"
                assert route == "partitioned" or K > (nfft // 2 if nfft else 2048)
                assert plan.partitions == -(-K // (N // 2)) and plan.block_outputs == N // 2
                assert 0 < plan.workspace_bytes <= MIB64
                # one chunk of the walk holds at least one output block next to the P - 1 spectra it shares
                assert plan.workspace_bytes // (8 * N) >= plan.partitions
                if nfft == 0:
                    assert N == (2048 if K <= 1024 else 4096)
    assert L.PFB_MF_ROUTE_PARTITIONED in seen and (L.PFB_MF_ROUTE_FUSED in seen) == (K <= 2048)
    auto = mf.describe(r)
    assert auto.route == (L.PFB_MF_ROUTE_FUSED if K <= 2048 else L.PFB_MF_ROUTE_PARTITIONED)


def test_describe_does_not_depend_on_the_other_settings():
    r = R.random_replica(700, 1)
    base = mf.describe(r)
    for kw in (dict(sample_format="int8", bit_width=8), dict(sample_format="cf32"), dict(output="power"),
               dict(normalize=True)):
        p = mf.describe(r, **kw)
        assert bytes(p) == bytes(base), kw


def test_exports():
    lib = L.load()
    declared = {n for n in declared_symbols() if n.startswith("pfb_mf_")}
    assert declared == MF_EXPORTS == {n for n in L.EXPORTS if n.startswith("pfb_mf_")}
    for name in MF_EXPORTS:
        assert hasattr(lib, name), name
    assert C.sizeof(L.PfbMfConfig) == 48 and C.sizeof(L.PfbMfPlan) == 24
    assert (L.PFB_MF_COMPLEX, L.PFB_MF_POWER, L.PFB_MF_NORMALIZE) == (0, 1, 1)
    assert (L.PFB_MF_ROUTE_AUTO, L.PFB_MF_ROUTE_FUSED, L.PFB_MF_ROUTE_PARTITIONED) == (0, 1, 2)
    hdr = open(os.path.join(ROOT, "include", "pfb_channelizer.h")).read()
    for word in ("PFB_MF_COMPLEX = 0, PFB_MF_POWER = 1", "PFB_MF_NORMALIZE = 1u << 0",
                 "PFB_MF_ROUTE_AUTO = 0, PFB_MF_ROUTE_FUSED = 1, PFB_MF_ROUTE_PARTITIONED = 2"):
        assert word in hdr, word
    assert hdr.index("pfb_mf_describe") > hdr.index("pfb_trace_envelope_from_iq_file")   # its own section, after the traces
    import sdr_channelizer_amd as pkg
    for name in ("MatchedFilter", "compress", "compress_iq_file", "replica_from_pulse_train", "pulse_delay_from_iq_files"):
        assert name in pkg.__all__ and getattr(pkg, name) is getattr(mf, name)


def test_mf_entry_points_sit_under_the_abi_guard():
    src = open(os.path.join(ROOT, "sdr_channelizer_amd", "csrc", "pfb_mf.hip")).read()
    found = {}
    for m in re.finditer(r'^extern "C" int (\w+)\(', src, re.M):
        rest = src[m.start():]
        found[m.group(1)] = rest[: rest.index("\n}\n")]
    assert set(found) == MF_EXPORTS - {"pfb_mf_last_kernel"}
    for name, body in found.items():
        assert "abi_guard" in body.split("{", 1)[1][:80], name
    # the one entry point that does not return a status reads a field and builds nothing
    rest = [ln for ln in src.splitlines() if ln.startswith('extern "C"') and not ln.startswith('extern "C" int ')]
    assert rest == ['extern "C" const char* pfb_mf_last_kernel(const pfb_mf_handle* h) { return h ? h->last_kernel : ""; }']
    assert src.count('extern "C"') == len(found) + 1
    from sdr_channelizer_amd import build
    assert "pfb_mf.hip" in build.SOURCES
    # the device is resolved after every argument check: NO_DEVICE comes last; the allocations are the shared ones
    create = src[src.index("int create_mf("):]
    create = create[: create.index("\n}\n")]
    assert create.index("mf_check(cfg") < create.index("resolve_device") < create.index("st.allocate(")
    shared = open(os.path.join(ROOT, "sdr_channelizer_amd", "csrc", "pfb_ols_host.cpp")).read()
    allocate = shared[shared.index("hipError_t OlsStream::allocate("):]
    assert "hipMalloc" in allocate[: allocate.index("\n}\n")] and "hipMalloc" not in create
