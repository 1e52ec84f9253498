"""The PRI search without a GPU: the numpy restatement (fold_ref) against the literal per-cell loop, the counts against
np.bincount and pfb_fold_counts, the designed input whose sums depend on their order, every argument check that comes
before the device, the struct layouts, the exports, and -- on the restatement alone -- the chain design test_gpu_fold.py
relies on: the train under the single-pulse threshold folds to a clear peak at its PRI and nowhere else."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import fold_cases as FC
import fold_ref as R
from abi_symbols import declared_symbols
from sdr_channelizer_amd import _lib as L
from sdr_channelizer_amd import pri_search as ps

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FOLD_EXPORTS = {"pfb_fold_describe", "pfb_fold_counts", "pfb_fold_create", "pfb_fold_destroy", "pfb_fold_reset",
                "pfb_fold_set_stream", "pfb_fold_sync", "pfb_fold_get_device", "pfb_fold_next_index", "pfb_fold_process",
                "pfb_fold_process_async", "pfb_fold_scores", "pfb_fold_profile", "pfb_fold_last_kernel"}


# -- the definition, sentence by sentence -------------------------------------------------------------------------
@pytest.mark.parametrize("L_,C_", [(1, 1), (7, 1), (7, 2), (7, 3), (8, 4), (9, 4), (11, 4), (13, 5), (64, 64), (127, 64),
                                   (100, 7), (33, 16)])
def test_restatement_is_the_literal_loop(L_, C_):
    rng = np.random.default_rng(L_ * 100 + C_)
    for n in (0, 1, C_, L_ - 1, L_, L_ + 1, 2 * L_ + C_ + 1, 5 * L_ + 3):
        for start in (0, 3, L_ - 1, 2 * L_ + 1):
            p = R.spread_stream(n, int(rng.integers(1 << 30)))
            F, cnt = R.literal_fold(p, L_, C_, start)
            assert R.fold(p, L_, C_, start).tobytes() == F.tobytes()
            j = R.bins(start + np.arange(n), L_, C_)
            assert np.array_equal(np.bincount(j, minlength=L_ // C_).astype(np.uint64), cnt)
            assert np.array_equal(R.counts(start + n, L_, C_) - R.counts(start, L_, C_), cnt)
    # the last bin is C .. 2C-1 wide, every other one C
    widths = R.counts(L_, L_, C_)
    assert (widths[:-1] == C_).all() and C_ <= widths[-1] == C_ + L_ % C_ < 2 * C_ and widths.sum() == L_


def test_a_cut_stream_gives_the_same_profile():
    p = R.spread_stream(700, 3)
    for L_, C_ in ((37, 4), (64, 16), (101, 5)):
        whole = R.fold(p, L_, C_)
        for cuts in ((0, 1, 2, 3, 700), (0, 36, 37, 38, 300, 300, 700), tuple(range(0, 701, 7))):
            F = None
            for a, b in zip(cuts[:-1], cuts[1:]):
                F = R.fold(p[a:b], L_, C_, a, F)
            assert F.tobytes() == whole.tobytes()


def test_the_score_record():
    p = R.spread_stream(1000, 4)
    for L_, C_, N in ((37, 4, 1000), (37, 4, 36), (37, 4, 5), (64, 1, 1000), (200, 16, 150)):
        F, cnt = R.literal_fold(p[:N], L_, C_)
        rec = R.score(F, N, L_, C_)
        used = int((cnt > 0).sum())
        m = F[:used].astype(np.float64) / cnt[:used]
        assert (rec["period"], rec["num_bins"], rec["bins_used"], rec["cells"], rec["reserved"]) == (L_, L_ // C_, used, N, 0)
        assert rec["peak_bin"] == int(np.argmax(m)) and rec["peak_cells"] == cnt[rec["peak_bin"]]
        assert rec["peak_sum"] == F[rec["peak_bin"]] and rec["peak_mean"] == np.float32(m.max())
        assert abs(rec["sum_means"] - m.sum()) <= R.sums_bound(F, N, L_, C_)[0]
    zero = R.score(np.zeros(9, np.float32), 0, 37, 4)
    assert bytes(zero) == bytes(np.array((37, 9, 0, 0, 0, 0, 0, 0, 0, 0, 0), R.SCORE))
    # ties to the lowest j; a NaN never displaces; a NaN in the first used bin stays; Inf is a value like any other
    nan, inf = np.nan, np.inf
    for F, want in (([1, 5, 5, 2], 1), ([3, nan, 9, 9], 2), ([nan, 9, 1, 1], 0), ([1, -inf, inf, inf], 2), ([-inf, -inf, -inf, -inf], 0),
                    ([1, 2, nan, nan], 1)):
        assert R.score(np.array(F, np.float32), 16, 16, 4)["peak_bin"] == want, F
    rng = np.random.default_rng(8)
    for _ in range(200):                  # the vectorised peak is the literal walk, specials and ties included
        F = rng.choice(np.array([nan, inf, -inf, 0.0, -0.0, 1.0, 2.0, 3.0], np.float32), 12)
        assert R.score(F, 48, 48, 4)["peak_bin"] == R.literal_peak(F.astype(np.float64) / 4.0), F
    # equal means from different counts: the last bin of L = 9, C = 4 holds 5 cells
    assert R.score(np.array([8, 10], np.float32), 9, 9, 4)["peak_bin"] == 0
    assert R.score(np.array([8, 10.5], np.float32), 9, 9, 4)["peak_bin"] == 1


def test_z_and_rank():
    rec = np.zeros(4, ps.SCORE_DTYPE)
    rec["period"] = (30, 20, 20, 10)
    rec["bins_used"] = (16, 16, 16, 7)
    rec["peak_mean"] = (5.0, 5.0, 5.0, 99.0)
    rec["sum_means"] = 16.0
    rec["sum_sq_means"] = (32.0, 32.0, 16.0, 32.0)     # mu = 1, variance 1, 1, 0, -
    rec["peak_bin"] = (3, 4, 5, 6)
    assert ps.fold_z(rec).tolist() == [4.0, 4.0, 0.0, 0.0] == R.z(rec.astype(R.SCORE)).tolist()
    found = ps.rank(rec, 4)
    assert found["period"].tolist() == [20, 30, 10, 20] and found["origin"].tolist() == [16, 12, 24, 20]
    assert found["z"].tolist() == [4.0, 4.0, 0.0, 0.0]
    assert [int(rec[k]["peak_bin"]) for k in R.ranked(rec.astype(R.SCORE), 4)] == (found["origin"] // 4).tolist()
    assert ps.SCORE_DTYPE == R.SCORE and ps.SCORE_DTYPE.itemsize == C.sizeof(L.PfbFoldScore) == 56
    for (name, _), (cname, _) in zip(ps.SCORE_DTYPE.descr, L.PfbFoldScore._fields_):
        assert name == cname and ps.SCORE_DTYPE.fields[name][1] == getattr(L.PfbFoldScore, cname).offset


def test_the_designed_input_depends_on_the_order():
    """more than half the bins of the order-sensitive input differ under a pairwise tree, and under the reversed order:
    bit-for-bit agreement of the device with the restatement then means the order, not luck"""
    for L_, C_ in FC.ORDER_SHAPES:
        p = FC.order_stream(L_)
        F = R.fold(p, L_, C_)
        NB = L_ // C_
        assert (R.fold_pairwise(p, L_, C_) != F).sum() > NB / 2, (L_, C_)
        assert (R.fold_reversed(p, L_, C_) != F).sum() > NB / 2, (L_, C_)
        e = np.frexp(p)[1]
        assert e.max() - e.min() == 24 and np.isfinite(F).all()


# -- the arguments ---------------------------------------------------------------------------------------------------
def config(periods=(2048, 2049), C_=4, NC=None, flags=0, size=None, device=-1, null=False):
    p = np.ascontiguousarray(periods, np.uint32)
    cfg = L.PfbFoldConfig(C.sizeof(L.PfbFoldConfig) if size is None else size, C_, len(p) if NC is None else NC,
                          None if null else p.ctypes.data_as(C.POINTER(C.c_uint32)), flags, device)
    cfg._keep = p
    return cfg


def both(**kw):
    """the status of pfb_fold_describe and of pfb_fold_create for one config, their outputs untouched on failure"""
    lib = L.load()
    cfg = config(**kw)
    plan, h = L.PfbFoldPlan(), C.c_void_p()
    C.memset(C.byref(plan), 0x5a, C.sizeof(plan))
    d = lib.pfb_fold_describe(C.byref(cfg), C.byref(plan))
    c = lib.pfb_fold_create(C.byref(cfg), C.byref(h))
    assert d == L.PFB_OK or bytes(plan) == b"\x5a" * C.sizeof(plan)
    assert not h.value or c == L.PFB_OK
    if h.value:
        lib.pfb_fold_destroy(h)
    return d, c


def test_arguments_are_checked_before_the_device_and_in_order():
    lib = L.load()
    BAD, UNS = L.PFB_ERR_BAD_ARG, L.PFB_ERR_UNSUPPORTED
    plan, h = L.PfbFoldPlan(), C.c_void_p()
    cfg = config()
    assert lib.pfb_fold_describe(None, C.byref(plan)) == lib.pfb_fold_describe(C.byref(cfg), None) == BAD
    assert lib.pfb_fold_create(None, C.byref(h)) == lib.pfb_fold_create(C.byref(cfg), None) == BAD
    # one case per refusal, in the header's order: null list, struct_size, C, NC, a period, flags
    bad = [dict(null=True), dict(size=28), dict(size=40), dict(C_=0), dict(C_=65), dict(C_=1 << 31)]
    bad += [dict(NC=0), dict(periods=[2048] * 4097), dict(NC=1 << 31)]
    bad += [dict(periods=(2048, 3)), dict(periods=(0,)), dict(periods=((1 << 24) + 1,), C_=64), dict(periods=((1 << 32) - 1,), C_=64)]
    bad += [dict(periods=(65537,), C_=1), dict(periods=(2048, 65536 * 4 + 4)), dict(periods=((1 << 24),), C_=64)]
    bad += [dict(flags=1), dict(flags=1 << 31)]
    for kw in bad:
        assert both(**kw) == (BAD, BAD), kw
        assert both(device=1 << 20, **kw) == (BAD, BAD), kw    # before the device is looked at
    # each earlier refusal wins over a later one
    assert both(C_=0, periods=[2048] * 4097, flags=1) == (BAD, BAD)
    # the profiles: sum NB * 4 bytes, 64 MiB allowed, one bin more refused -- after every BAD_ARG check
    full = [65536] * 256
    assert both(periods=full + [1], C_=1, device=1 << 20) == (UNS, UNS)
    assert both(periods=full + [1], C_=1, flags=1, device=1 << 20) == (BAD, BAD)
    assert both(periods=[65536] * 4096, C_=1, device=1 << 20) == (UNS, UNS)
    assert lib.pfb_fold_describe(C.byref(config(periods=full, C_=1)), C.byref(plan)) == L.PFB_OK
    assert (plan.profile_bytes, plan.total_bins, plan.max_bins) == (64 << 20, 1 << 24, 65536)
    # the largest legal shape: L = 2^22 + 63 at C = 64 has 65536 bins
    assert lib.pfb_fold_describe(C.byref(config(periods=((1 << 22) + 63, 1 << 22), C_=64)), C.byref(plan)) == L.PFB_OK
    assert (plan.total_bins, plan.max_bins) == (2 << 16, 65536)
    # null handles and pointers
    u = C.c_uint64(7)
    buf = np.zeros(64, np.float32)
    p = C.c_void_p(buf.ctypes.data)
    assert lib.pfb_fold_destroy(None) == lib.pfb_fold_reset(None) == lib.pfb_fold_sync(None) == BAD
    assert lib.pfb_fold_set_stream(None, None) == lib.pfb_fold_get_device(None, None) == BAD
    assert lib.pfb_fold_next_index(None, C.byref(u)) == BAD and u.value == 7
    for mem in (L.PFB_MEM_HOST, L.PFB_MEM_DEVICE, 2):
        assert lib.pfb_fold_process(None, p, 16, mem) == lib.pfb_fold_scores(None, p, 2, mem) == BAD
        assert lib.pfb_fold_profile(None, 0, p, 64, mem) == BAD
    assert lib.pfb_fold_process_async(None, p, 16) == BAD
    assert lib.pfb_fold_last_kernel(None) == b""
    assert not buf.any()
    with pytest.raises(ValueError):
        ps.describe_fold([-1])
    with pytest.raises(ValueError):
        ps.describe_fold([1 << 32])


def test_a_valid_config_needs_a_device():
    if L.load().pfb_device_count() > 0:
        pytest.skip("a GPU is present")
    for kw in (dict(), dict(periods=(1,), C_=1), dict(periods=(64,), C_=64), dict(periods=[65536] * 256, C_=1),
               dict(periods=(2048, 2048, 2048)), dict(periods=((1 << 22) + 63,), C_=64)):
        assert both(**kw) == (L.PFB_OK, L.PFB_ERR_NO_DEVICE), kw
    with pytest.raises(L.PfbError) as e:
        ps.PriFold([2048, 2049])
    assert e.value.status == L.PFB_ERR_NO_DEVICE
    with pytest.raises(L.PfbError) as e:
        ps.find_pri(np.ones((1000, 2), np.float32), np.ones(13, np.complex64), 100, 110)
    assert e.value.status == L.PFB_ERR_NO_DEVICE


def test_describe():
    for C_, name in ((1, "direct<1>"), (2, "direct<2>"), (3, "direct<3>"), (4, "direct<4>"), (5, "direct<n>"), (7, "direct<n>"),
                     (8, "tile<8>"), (12, "direct<n>"), (16, "tile<16>"), (32, "tile<32>"), (63, "direct<n>"), (64, "tile<64>")):
        plan = ps.describe_fold([640, 641, 1000, 640], C_)
        nb = [640 // C_, 641 // C_, 1000 // C_, 640 // C_]
        assert (plan.total_bins, plan.profile_bytes, plan.max_bins) == (sum(nb), 4 * sum(nb), max(nb))
        assert plan.kernel.decode() == "pfb_fold_" + name == FC.kernel_name(C_)
    assert ps.describe_fold(range(1984, 2113)).total_bins == sum(L_ // 4 for L_ in range(1984, 2113))


def test_counts_are_the_closed_form():
    lib = L.load()
    periods = (9, 37, 64, 2048, 127)
    for C_ in (1, 3, 4, 5):
        for k, L_ in enumerate(periods):
            for N in (0, 1, C_, L_ - 1, L_, L_ + 1, 2 * L_ + C_ + 1, 5 * L_ + 3, (1 << 40) + 12345, 1 << 62):
                got = ps.fold_counts(periods, C_, k, N)
                assert got.dtype == np.uint64 and np.array_equal(got, R.counts(N, L_, C_)), (C_, L_, N)
                assert int(got.sum()) == N
    assert np.array_equal(ps.fold_counts(periods, 4, 1, 300), np.bincount(R.bins(np.arange(300), 37, 4), minlength=9))
    out = np.full(16, 77, np.uint64)
    po = out.ctypes.data_as(C.POINTER(C.c_uint64))
    cfg = config(periods=(9, 37))
    BAD = L.PFB_ERR_BAD_ARG
    assert lib.pfb_fold_counts(None, 0, 5, po) == lib.pfb_fold_counts(C.byref(cfg), 0, 5, None) == BAD
    assert lib.pfb_fold_counts(C.byref(cfg), 2, 5, po) == lib.pfb_fold_counts(C.byref(cfg), 0, (1 << 62) + 1, po) == BAD
    assert lib.pfb_fold_counts(C.byref(config(periods=(9, 3))), 0, 5, po) == BAD
    assert lib.pfb_fold_counts(C.byref(config(periods=[65536] * 257, C_=1)), 0, 5, po) == L.PFB_ERR_UNSUPPORTED
    assert (out == 77).all()
    assert lib.pfb_fold_counts(C.byref(cfg), 0, 5, po) == L.PFB_OK and out[:3].tolist() == [4, 1, 77]
    with pytest.raises(IndexError):
        ps.fold_counts(periods, 4, 5, 10)


def test_exports():
    lib = L.load()
    declared = {n for n in declared_symbols() if n.startswith("pfb_fold_")}
    assert declared == FOLD_EXPORTS == {n for n in L.EXPORTS if n.startswith("pfb_fold_")}
    for name in FOLD_EXPORTS:
        assert hasattr(lib, name), name
    assert (C.sizeof(L.PfbFoldConfig), C.sizeof(L.PfbFoldPlan), C.sizeof(L.PfbFoldScore)) == (32, 56, 56)
    hdr = open(os.path.join(ROOT, "include", "pfb_channelizer.h")).read()
    assert "#define PFB_ABI_VERSION 2" in hdr and lib.pfb_abi_version() == 2
    assert hdr.index("pfb_fold_describe(") > hdr.index("pfb_pd_last_kernel(")   # its own section, at the end
    assert "THE SAME BITS COME OUT UNDER ANY CUTTING OF THE STREAM" in hdr and "ONE AT A TIME IN ASCENDING i" in hdr
    import sdr_channelizer_amd as pkg
    names = ["PriFold", "find_pri", "fold_z", "describe_fold"]
    at = pkg.__all__.index("PulseDoppler")
    assert pkg.__all__[at - len(names):at] == names
    for name in names:
        assert getattr(pkg, name) is getattr(ps, name)


def test_the_struct_layouts_are_the_compilers(tmp_path):
    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.skip("no gcc")
    lines, want = [], []
    for cname, cls in (("pfb_fold_config", L.PfbFoldConfig), ("pfb_fold_plan", L.PfbFoldPlan), ("pfb_fold_score", L.PfbFoldScore)):
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


def test_fold_entry_points_sit_under_the_abi_guard():
    src = open(os.path.join(ROOT, "sdr_channelizer_amd", "csrc", "pfb_fold.hip")).read()
    found = {}
    for m in re.finditer(r'^extern "C" int (\w+)\(', src, re.M):
        rest = src[m.start():]
        found[m.group(1)] = rest[: rest.index("\n}\n")]
    assert set(found) == (FOLD_EXPORTS - {"pfb_fold_last_kernel"}) | {"pfb_fold_set_tier"}   # the dev header's switch
    for name, body in found.items():
        assert "abi_guard" in body.split("{", 1)[1][:80], name
    assert src.count('extern "C"') == len(found) + 1
    from sdr_channelizer_amd import build
    assert "pfb_fold.hip" in build.SOURCES
    create = src[src.index("int create_fold("):]
    create = create[: create.index("\n}\n")]
    assert create.index("fold_check(cfg") < create.index("resolve_device") < create.index("allocate_fold(")
    code = re.sub(r"//.*", "", src).lower()
    for word in ("atomic", "asm", "mfma", "fma("):     # additions only, one writer per element
        assert word not in code, word


# -- the chain design, on the restatement alone ---------------------------------------------------------------------
def test_the_train_folds_to_its_pri():
    """the stream of pd_cases, whose single pulses no detector finds: best 2048, at the train's first pulse, clear of
    every other candidate; the harmonics next; nothing else above 6"""
    p = FC.chain_powers()
    assert len(p) == FC.CHAIN_CELLS == 393113 and p.dtype == np.float32
    rec, _ = FC.chain_reference(p)
    z = R.z(rec)
    order = R.ranked(rec, FC.CHAIN_C)
    best = order[0]
    assert rec[best]["period"] == 2048 and rec[best]["peak_bin"] == 175 == FC.CHAIN_FIRST_PULSE // FC.CHAIN_C
    assert z[best] >= 8 and all(z[best] > z[k] for k in order[1:])
    harmonic = np.isin(rec["period"], (1024, 2048, 4096, 6144))
    assert z[~harmonic].max() <= 6 and (z[harmonic] > 6).all()
    assert sorted(int(rec[k]["period"]) for k in order[:4]) == [1024, 2048, 4096, 6144]
    print("z(2048) %.2f, best harmonic %.2f, best other %.2f" % (z[best], z[order[1]], z[~harmonic].max()))
    # the first interval alone already ranks it first
    rec1, _ = R.scores(p, FC.CHAIN_PERIODS, FC.CHAIN_C, N=131072)
    assert rec1[R.ranked(rec1, FC.CHAIN_C)[0]]["period"] == 2048


def test_noise_alone_folds_to_nothing():
    rng = np.random.default_rng(11)
    p = rng.exponential(1.0, FC.CHAIN_CELLS).astype(np.float32)
    rec, _ = FC.chain_reference(p)
    assert R.z(rec).max() <= 6
