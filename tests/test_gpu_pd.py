"""Pulse-Doppler integration on the MI355X (pfb_pd_*) against the float64 restatement (tests/pd_ref.py): the shape grid
of every Doppler length with all four outputs, both row orders, pointers on and off a 16-byte boundary and guard words;
exact ties, designed tones, samples that are not finite; every cutting byte for byte against one call; flush, capacity,
indices past 2^32, the host, async and carry-limit routes; and the chain from a train under the single-pulse threshold.

Allowances (the header's arithmetic, the formats' precision; none is taken from what the kernels give):
  complex      |Z - Zref| <= 1e-5 ||w||_2 ||A[:, r]||_2 per gate, the matched filter's allowance: the right-hand side is
               1e-5 of the Cauchy-Schwarz bound on |Z|, and one transform of <= 1024 points rounds less than the matched
               filter's forward transform, multiply and inverse at 4096
  power, best  the same carried through the square: |p - pref| <= b (2 B + b), B the bound on |Z|, b = 1e-5 B
  noncoherent  relative (K + 4) 2^-24: K terms of at most four roundings each (two window products squared, the
               square's own, the sum of the squares: to first order the term is off by 4 ulp/2), added by K - 1 float32
               additions
The grid crosses every ND with every K, R and L of the issue's sets and runs all four outputs on each shape; row order
and the two pointer alignments are drawn per shape by a hash, so each occurs with every ND, output, K and R class."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import pd_cases as P  # noqa: E402
import pd_ref as R  # noqa: E402
from gpu_support import Busy, cuda_torch  # noqa: E402
from sdr_channelizer_amd import (PulseDoppler, PulseTrain, cfar_alpha, detect_pulse_train, detect_pulses,  # noqa: E402
                                 range_doppler, replica_from_pulse_train)
from sdr_channelizer_amd import _lib as L  # noqa: E402
from sdr_channelizer_amd.pulse_doppler import TRAIN_DET_DTYPE, cells  # noqa: E402

KINDS = ("complex", "power", "best", "noncoherent")
SENTINEL = 0x7FC54321   # a NaN no kernel writes


@pytest.fixture(scope="module")
def torch():
    return cuda_torch()


def words_per_cpi(pd):
    return int(pd.plan.cpi_outputs) * (2 if pd.output in ("complex", "best") else 1)


def shaped(pd, words):
    """the float32 words of whole intervals as the array PulseDoppler.process returns"""
    w = np.ascontiguousarray(words)
    n = w.size // words_per_cpi(pd)
    if pd.output == "complex":
        return w.view(np.complex64).reshape(n, pd.doppler_length, pd.num_gates)
    if pd.output == "best":
        return w.view(R.CELL).reshape(n, pd.num_gates)
    return w.view(np.float32).reshape((n, pd.doppler_length, pd.num_gates) if pd.output == "power" else (n, pd.num_gates))


def raw_call(torch, pd, xin, lead_in, n, cpis, mis_out=False, capacity=None):
    """pfb_pd_process itself on device pointers: samples xin[lead_in : lead_in + n], an output buffer with sentinel
    words on both sides of the `cpis` intervals the call is to write.  Returns (status, count, the intervals' words)."""
    per = words_per_cpi(pd)
    lead_out = (2 if pd.output in ("complex", "best") else 1) if mis_out else 4   # one element past a 16-byte boundary
    out = torch.full((lead_out + cpis * per + 8,), SENTINEL, dtype=torch.int32, device="cuda")
    cnt = C.c_uint64(12345)
    rc = pd._lib.pfb_pd_process(pd._h, C.c_void_p(xin.data_ptr() + 8 * lead_in), n, C.c_void_p(out.data_ptr() + 4 * lead_out),
                                cpis if capacity is None else capacity, C.byref(cnt), L.PFB_MEM_DEVICE)
    host = out.cpu().numpy()
    assert (host[:lead_out] == SENTINEL).all() and (host[lead_out + cpis * per:] == SENTINEL).all()
    return rc, int(cnt.value), host[lead_out:lead_out + cpis * per]


def ratios(kind, got, A, w, nd, centered, Z=None):
    """the largest error of one interval over its allowance (<= 1 passes); best: also checks the bin.  Z: the
    reference transform of A when the caller has it already"""
    K, Rg = A.shape
    Z = R.transform(A, w, nd, centered) if Z is None else Z
    if kind == "complex":
        return float((np.abs(got - Z) / R.bound(A, w)).max())
    Pw = R.power(Z)
    if kind == "power":
        return float((np.abs(got.astype(np.float64) - Pw) / R.power_bound(A, w)).max())
    if kind == "noncoherent":
        N = R.noncoherent(A, w)
        return float((np.abs(got.astype(np.float64) - N) / ((K + 4) * 2.0 ** -24 * N)).max())
    bp, bh = R.best(Pw, nd, centered)
    if K == 1:   # every row holds w[0] A[0][r]: an exact tie, the first written row
        assert (got["hypothesis"] == R.rows(nd, centered)[0]).all()
    else:
        clear = P.clear_gates(Pw, A, w)
        assert (got["hypothesis"][clear] == bh[clear]).all()
    return float((np.abs(got["power"].astype(np.float64) - bp) / R.power_bound(A, w)).max())


@pytest.mark.parametrize("nd", R.LENGTHS)
def test_the_shape_grid(torch, nd):
    """every (K, R, L) of P.shapes(nd) with all four outputs, two CPIs a call.  R is laid around the tile of the
    transform kernels, T = P.tile_gates(nd), for all four outputs: pd_noncoherent's own tile is 256 gates whatever the
    length, so it meets R = 255, 256, 257 and 515 in the grids of ND = 8 and 16 only (the same kernel serves every
    length; ND reaches it only through K), and R well under its tile in the others."""
    worst = dict.fromkeys(KINDS, 0.0)
    seen = set()
    for i, (K, Rg, L_) in enumerate(P.shapes(nd)):
        x, o = P.grid_stream(nd, K, Rg, L_, i)
        w = P.grid_window(K, i)
        centered, mis_in, mis_out = P.grid_flags(i)
        lead_in = 1 if mis_in else 2
        xin = torch.zeros(len(x) + 4, dtype=torch.complex64, device="cuda")
        xin[lead_in:lead_in + len(x)] = torch.from_numpy(x).cuda()
        assert (xin.data_ptr() + 8 * lead_in) % 16 == (8 if mis_in else 0)
        A = [R.gates(x, c, o, L_, Rg, K) for c in (0, 1)]
        Z = [R.transform(a, w, nd, centered) for a in A]      # once per shape, shared by the four outputs
        for kind in KINDS:
            with PulseDoppler(L_, K, Rg, o, w, nd, kind, centered) as pd:
                assert pd.plan.tile_gates == (256 if kind == "noncoherent" else P.tile_gates(nd))
                assert pd.cpis_for(len(x)) == 2 and pd.cpis_for(len(x) - P.grid_tail(K, L_) - 1) == 1
                rc, cnt, words = raw_call(torch, pd, xin, lead_in, len(x), 2, mis_out)
                assert (rc, cnt) == (L.PFB_OK, 2) and pd.next_index == len(x)
                assert pd.last_kernel == pd.plan.kernel.decode() + "[stream]"
                got = shaped(pd, words)
                for c in (0, 1):
                    worst[kind] = max(worst[kind], ratios(kind, got[c], A[c], w, nd, centered, Z[c]))
            seen.add((kind, centered, mis_in, mis_out))
    print(f"ND {nd}: largest error over its allowance " + ", ".join(f"{k} {v:.4f}" for k, v in worst.items()))
    assert len(seen) == 4 * 8                      # every output met both row orders and all four pointer placements
    assert max(worst.values()) <= 1.0, worst


@pytest.mark.parametrize("nd", [8, 32, 64, 512, 1024])
def test_an_exact_tie(torch, nd):
    """one nonzero pulse at k = 0: every row of a gate holds the same bits, and the cell names the first written row"""
    K, Rg, L_ = nd - 1, P.tile_gates(nd) + 3, P.tile_gates(nd) + 8
    x = P.tie_stream(K, Rg, L_, nd)
    for centered in (False, True):
        z = range_doppler(torch.from_numpy(x).cuda(), L_, K, Rg, output="complex", centered=centered).cpu().numpy()
        assert z.shape == (1, nd, Rg) and (z.view(np.int64) == z[:, :1].view(np.int64)).all() and np.array_equal(z[0, 0], x[:Rg])
        c = cells(range_doppler(torch.from_numpy(x).cuda(), L_, K, Rg, output="best", centered=centered))
        assert (c["hypothesis"] == (-nd // 2 if centered else 0)).all()
        p = range_doppler(torch.from_numpy(x).cuda(), L_, K, Rg, output="power", centered=centered).cpu().numpy()
        assert np.array_equal(c["power"][0], p[0, 0]) and (p.view(np.int32) == p[:, :1].view(np.int32)).all()
        assert np.abs(p[0, 0] - np.abs(x[:Rg].astype(np.complex128)) ** 2).max() <= 2.0 ** -22 * p.max()


@pytest.mark.parametrize("nd", [8, 64, 1024])
def test_a_designed_bin(torch, nd):
    """the tone e^{j 2 pi d0 k / ND} across the pulses lands in row d0, for every d0"""
    every = np.arange(nd)
    for lo in range(0, nd, 256):
        d0 = every[lo:lo + 256]
        x = P.tone_stream(nd, len(d0), len(d0) + 2, d0)
        xd = torch.from_numpy(x).cuda()
        c = cells(range_doppler(xd, len(d0) + 2, nd, len(d0), output="best"))
        assert c["hypothesis"][0].tolist() == d0.tolist() and np.abs(c["power"][0] / nd ** 2 - 1).max() < 1e-4
        c = cells(range_doppler(xd, len(d0) + 2, nd, len(d0), output="best", centered=True))
        assert c["hypothesis"][0].tolist() == [int(d) - nd if d >= nd // 2 else int(d) for d in d0]
        p = range_doppler(xd, len(d0) + 2, nd, len(d0), output="power").cpu().numpy()[0]
        assert (p.argmax(axis=0) == d0).all() and (np.sort(p, axis=0)[-2] < 1e-6 * nd ** 2).all()


@pytest.mark.parametrize("nd,K", [(16, 16), (64, 50), (512, 512)])
def test_samples_that_are_not_finite(torch, nd, K):
    Rg, L_ = 2 * P.tile_gates(nd) + 3, 2 * P.tile_gates(nd) + 9
    x, o = P.grid_stream(nd, K, Rg, L_, 3, cpis=1)
    bad = x.copy()
    spots = {2: np.nan, Rg - 1: np.inf, P.tile_gates(nd): -np.inf}
    for k, (r, v) in enumerate(spots.items()):
        bad[o + (k * (K - 1) // 2) * L_ + r] = v           # pulses 0, (K-1)/2 and K-1
    bad[o + Rg:o + L_] = np.nan                            # between the gates: never read
    clean = sorted(set(range(Rg)) - set(spots))
    for kind in KINDS:
        want = range_doppler(x, L_, K, Rg, o, None, nd, kind)
        got = range_doppler(torch.from_numpy(bad).cuda(), L_, K, Rg, o, None, nd, kind)
        got = cells(got) if kind == "best" else got.cpu().numpy()
        assert got[..., clean].tobytes() == want[..., clean].tobytes()    # only its own gate column
        for r in spots:
            col = got[..., r]
            assert not np.isfinite(col["power"] if kind == "best" else col).any()
        if kind == "best":
            assert np.isnan(got["power"][0, 2]) and got["hypothesis"][0, 2] == 0    # NaN at d = 0 stays, as the bank's


def run_cuts(torch, pd, xd, cuts, flush=True):
    """the stream cut into calls of these lengths on a fresh stream position: (bytes of every interval in order, the
    flush's bytes, the kernels named after each call)"""
    pd.reset()
    got, names, pos = [], [], 0
    for m in cuts:
        want = pd.cpis_for(m)
        out = pd.process(xd[pos:pos + m])
        assert out.shape[0] == want
        got.append(out.cpu().numpy().tobytes())
        names.append(pd.last_kernel)
        pos += m
        assert pd.next_index == pos
    tail = pd.flush(xd.device).cpu().numpy() if flush else None
    return b"".join(got), tail, names


@pytest.mark.parametrize("kind", KINDS)
def test_cuttings_give_the_same_bytes(torch, kind):
    nd, K, Rg, L_, o = 64, 40, 131, 150, 11
    rng = np.random.default_rng(17)
    n = o + 3 * K * L_ + 7 * L_ + 60                     # three intervals and seven rows and a cut row of the fourth
    x = (rng.standard_normal(n) + 1j * rng.standard_normal(n)).astype(np.complex64)
    xd = torch.from_numpy(x).cuda()
    w = P.grid_window(K, 1)
    with PulseDoppler(L_, K, Rg, o, w, nd, kind, True) as pd:
        name = pd.plan.kernel.decode()
        one, tail, names = run_cuts(torch, pd, xd, [n])
        assert names == [name + "[stream]"] and len(one) == 3 * words_per_cpi(pd) * 4 and tail.shape[0] == 1
        As = R.intervals(x, n, True, o, L_, Rg, K)
        assert len(As) == 4 and not As[3][8:].any() and As[3][7, :60].all() and not As[3][7, 60:].any()
        whole = shaped(pd, np.frombuffer(one, np.float32))
        tail_np = cells(tail) if kind == "best" else tail
        for c in range(4):                               # the flush: the open interval, its missing samples as zeros
            assert ratios(kind, whole[c] if c < 3 else tail_np[0], As[c], w, nd, True) <= 1.0
        assert pd.flush(xd.device).shape[0] == 0 and pd.next_index == n    # none open: nothing, and nothing moves
        end0 = o + (K - 1) * L_ + Rg                      # one past the sample that completes interval 0
        cuttings = [
            [0, n, 0],
            [end0 - 1, 1, n - end0],                      # the completing sample alone
            [end0, n - end0],                             # nothing carried at all
            [o + 5, 0, 0, L_ * 3 + 7, K * L_, n - (o + 5 + L_ * 3 + 7 + K * L_)],   # a cut inside a gate row
            [o + 2 * L_ + Rg - 3] + [1] * 40 + [n - (o + 2 * L_ + Rg - 3) - 40],     # one by one across a row end
            [end0 - 20] + [1] * 40 + [n - end0 - 20],     # one by one across an interval's end
            [o + K * L_ - 20] + [1] * 40 + [n - (o + K * L_ - 20) - 40],              # and across the next one's start
        ]
        for seed in (1, 2, 3):
            r2 = np.random.default_rng(seed)
            cuts = np.sort(r2.integers(0, n + 1, 12))
            cuttings.append(np.diff(np.concatenate([[0], cuts, [n]])).tolist())
        cuttings.append(cuttings[-1])                     # the same cutting twice
        for cuts in cuttings:
            assert sum(cuts) == n
            got, t2, names = run_cuts(torch, pd, xd, cuts)
            assert got == one and t2.tobytes() == tail.tobytes(), cuts
            assert all(nm in (name + "[stream]", name + "[carry]") for nm in names)
        assert run_cuts(torch, pd, xd, [end0 - 1, 1], flush=False)[2][-1] == name + "[carry]"
        assert run_cuts(torch, pd, xd, [o, end0 - o], flush=False)[2][-1] == name + "[stream]"


def test_capacity_one_short_changes_nothing(torch):
    nd, K, Rg, L_ = 32, 20, 300, 301
    x, o = P.grid_stream(nd, K, Rg, L_, 9, cpis=3)
    xin = torch.from_numpy(x).cuda()
    cut = o + K * L_ + 50                                # interval 0 whole, interval 1 open
    for kind in ("power", "best"):
        with PulseDoppler(L_, K, Rg, o, None, nd, kind) as pd:
            rc, cnt, first = raw_call(torch, pd, xin, 0, cut, 1)
            assert (rc, cnt) == (L.PFB_OK, 1)
            rc, cnt, words = raw_call(torch, pd, xin, cut, len(x) - cut, 1, capacity=1)
            assert (rc, cnt) == (L.PFB_ERR_CAPACITY, 2) and pd.next_index == cut and pd.cpis_for(len(x) - cut) == 2
            cnt = C.c_uint64(9)
            assert pd._lib.pfb_pd_flush(pd._h, None, 0, C.byref(cnt), L.PFB_MEM_DEVICE) == L.PFB_ERR_CAPACITY and cnt.value == 1
            assert pd._lib.pfb_pd_process_async(pd._h, C.c_void_p(xin.data_ptr() + 8 * cut), len(x) - cut, C.c_void_p(xin.data_ptr()),
                                                1, C.c_void_p(xin.data_ptr())) == L.PFB_ERR_CAPACITY
            rc, cnt, rest = raw_call(torch, pd, xin, cut, len(x) - cut, 2)
            assert (rc, cnt) == (L.PFB_OK, 2) and pd.next_index == len(x)
            pd.reset()
            rc, cnt, one = raw_call(torch, pd, xin, 0, len(x), 3)
            assert np.concatenate([first, rest]).tobytes() == one.tobytes()
            # pointers off their element, a mem that does not exist: refused before anything is read
            cnt = C.c_uint64(9)
            for dx, dout in ((4, 0), (0, 2), (0, 4 if kind == "best" else 1)):
                assert pd._lib.pfb_pd_process(pd._h, C.c_void_p(xin.data_ptr() + dx), 8, C.c_void_p(xin.data_ptr() + dout), 1,
                                              C.byref(cnt), L.PFB_MEM_DEVICE) == L.PFB_ERR_BAD_ARG
            assert pd._lib.pfb_pd_process(pd._h, C.c_void_p(xin.data_ptr()), 8, C.c_void_p(xin.data_ptr()), 1, C.byref(cnt), 2) \
                == L.PFB_ERR_BAD_ARG and cnt.value == 9 and pd.next_index == len(x)


def test_indices_past_2_to_the_32(torch):
    nd, K, Rg, L_ = 16, 11, 70, 90
    x, _ = P.grid_stream(nd, K, Rg, L_, 4, cpis=3)        # its own origin is 4
    xd = torch.from_numpy(x).cuda()
    with PulseDoppler(L_, K, Rg, 4, None, nd, "complex") as low, \
            PulseDoppler(L_, K, Rg, (1 << 32) + 4, None, nd, "complex") as high:
        want = low.process(xd).cpu().numpy()
        assert want.shape[0] == 3
        high.set_index((1 << 32) - 100)
        lead = torch.full((100,), float("nan"), dtype=torch.complex64, device="cuda")   # before the origin: ignored
        assert high.process(lead).shape[0] == 0 and high.next_index == 1 << 32
        cut = 4 + K * L_ + 17
        got = [high.process(xd[:cut]), high.process(xd[cut:])]
        assert [g.shape[0] for g in got] == [1, 2] and high.next_index == (1 << 32) + len(x)
        assert np.concatenate([g.cpu().numpy() for g in got]).tobytes() == want.tobytes()
        # an index inside interval 0 drops it: the first interval taken is the one that starts at or after the index
        high.set_index((1 << 32) + 4 + 1)
        assert high.cpis_for(len(x) - 5) == 2
        assert high.process(xd[5:]).cpu().numpy().tobytes() == want[1:].tobytes()
        high.set_index((1 << 32) + 4)                    # on its first sample: taken
        assert high.process(xd[4:]).cpu().numpy().tobytes() == want.tobytes()
        with pytest.raises(L.PfbError):
            high.set_index((1 << 62) + 1)
        high.set_index(1 << 62)
        with pytest.raises(L.PfbError):
            high.process(xd[:8])                          # the index would pass 2^62


def test_host_memory_in_three_staging_steps(torch):
    """2^22 samples a step; with R = L = 1 and K = 3 an interval spans each seam (2^22 mod 3 = 1)"""
    n = 2 * (1 << 22) + 5
    rng = np.random.default_rng(31)
    x = (rng.standard_normal(n) + 1j * rng.standard_normal(n)).astype(np.complex64)
    m = n // 3
    A = x[:3 * m].reshape(m, 3).astype(np.complex128)
    with PulseDoppler(1, 3, 1, 0, None, 8, "best") as pd:
        host = pd.process(x)
        assert host.shape == (m, 1) and pd.last_kernel == "pfb_pd_dft<8>[stream]" and pd.next_index == n
        pd.reset()
        dev = cells(pd.process(torch.from_numpy(x).cuda()))
        assert host.tobytes() == dev.tobytes()
        Pw = R.power(A @ np.exp(-2j * np.pi * np.outer(np.arange(3), np.arange(8)) / 8))
        B2 = 3.0 * (np.abs(A) ** 2).sum(axis=1)            # ||w||^2 ||A||^2
        allow = 1e-5 * np.sqrt(B2) * (2 * np.sqrt(B2) + 1e-5 * np.sqrt(B2))
        assert (np.abs(host["power"][:, 0].astype(np.float64) - Pw.max(axis=1)) <= allow).all()
        top = np.sort(Pw, axis=1)
        clear = top[:, -1] - top[:, -2] > 2 * allow
        assert clear.mean() > 0.95 and (host["hypothesis"][:, 0][clear] == Pw.argmax(axis=1)[clear]).all()
    with PulseDoppler(1, 3, 1, 0, None, 8, "noncoherent") as pd:
        host = pd.process(x)
        N = (np.abs(A) ** 2).sum(axis=1)
        assert host.shape == (m, 1) and (np.abs(host[:, 0] - N) <= 7 * 2.0 ** -24 * N).all()
        assert pd.flush().shape == (1, 1)                  # the last sample opened interval m


def test_async_calls_across_a_stream_switch(torch):
    nd, K, Rg, L_ = 128, 100, 70, 75
    x, o = P.grid_stream(nd, K, Rg, L_, 6, cpis=4)
    xd = torch.from_numpy(x).cuda()
    cuts = [o + K * L_ + 9, 1, 0, 2 * K * L_, len(x) - (o + 3 * K * L_ + 10)]
    edges = np.cumsum([0] + cuts)
    with PulseDoppler(L_, K, Rg, o, None, nd, "power") as pd:
        want = pd.process(xd).cpu().numpy()
        per_call = [R.completed(int(e), o, L_, Rg, K) for e in edges]
        per_call = [b - a for a, b in zip(per_call, per_call[1:])]
        assert per_call == [1, 0, 0, 2, 1]
        pd.reset()
        side = torch.cuda.Stream()
        busy = Busy(torch)
        outs = [torch.full((2, nd, Rg), -1.0, device="cuda") for _ in cuts]
        counts = torch.full((len(cuts), 2), -1, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        busy.queue(torch.cuda.default_stream(), copies=2)   # the host runs ahead of the device
        for k, m in enumerate(cuts):
            if k == 3:
                pd.set_stream(side.cuda_stream)            # what is queued on the old stream comes first
            pd.process_async(xd[int(edges[k]):int(edges[k]) + m], outs[k], counts[k][:1])
        assert pd.next_index == len(x)
        pd.sync()
        torch.cuda.synchronize()
        got_counts = counts.cpu().numpy()
        assert got_counts[:, 0].tolist() == per_call and (got_counts[:, 1] == -1).all()
        got = np.concatenate([outs[k][:per_call[k]].cpu().numpy() for k in range(len(cuts))])
        assert got.tobytes() == want.tobytes()
        for k in range(len(cuts)):
            assert (outs[k][per_call[k]:] == -1.0).all()
        pd.set_stream(0)
        with pytest.raises(ValueError):
            pd.process_async(xd[:8], outs[0].to(torch.complex64), counts[0][:1])
        with pytest.raises(ValueError):
            pd.process_async(xd[:8], outs[0], counts[0][:1].to(torch.int32))


def test_a_carry_at_the_limit(torch):
    """K R 8 = 64 MiB is taken and used whole; one element more is refused"""
    K, Rg = 1024, 1 << 13
    with pytest.raises(L.PfbError) as e:
        PulseDoppler(Rg + 1, K, Rg + 1, output="best")
    assert e.value.status == L.PFB_ERR_UNSUPPORTED
    rng = np.random.default_rng(41)
    x = torch.from_numpy(rng.standard_normal(2 * K * Rg).astype(np.float32)).cuda().view(torch.complex64)
    with PulseDoppler(Rg, K, Rg, output="best") as pd:
        assert pd.plan.carry_bytes == 64 << 20
        one = pd.process(x)
        assert one.shape == (1, Rg, 2) and pd.last_kernel.endswith("[stream]")
        pd.reset()
        assert pd.process(x[:5]).shape[0] == 0
        two = pd.process(x[5:])
        assert pd.last_kernel.endswith("[carry]") and torch.equal(one.view(torch.int32), two.view(torch.int32))


def test_the_chain_from_a_train_under_the_single_pulse_threshold(torch):
    """A Barker-13 train 20 dB under the noise per sample, level with it after compression: nothing for detect_pulses,
    one detection per interval at the pulse's first sample for detect_pulse_train with K = 64 at L = 2048 -- in Doppler
    bin 0, and in bin 5 once the stream turns by 5 / (K L) of a cycle per sample."""
    c = P.CHAIN
    kw = dict(P.CHAIN_SYNTH, **{k: c[k] for k in ("fs", "pw", "pri", "amplitude", "bit_width")})
    r = replica_from_pulse_train(**kw)
    n = P.CHAIN_CPIS * P.CHAIN_K * c["pri"]
    with PulseTrain(first_pulse=c["first_pulse"], noise_sigma=c["noise_sigma"], seed=c["seed"], **kw) as pt:
        iq = pt.generate(n)
    host = iq.cpu().numpy()
    assert host.tobytes() == P.chain_stream().tobytes() and r.tobytes() == P.chain_replica().tobytes()
    a_single, a_train = P.chain_alphas(cfar_alpha)
    single, train = P.chain_reference(host, a_single, a_train)       # the reference first
    want = [(k, c["first_pulse"], 0) for k in range(P.CHAIN_CPIS)]
    assert len(single) == 0 and train == want
    assert len(detect_pulses(iq, r, normalize=True).records) == 0
    found = detect_pulse_train(iq, r, c["pri"], P.CHAIN_K, normalize=True, fs=c["fs"], chunk_samples=100000)
    assert found.dtype == TRAIN_DET_DTYPE
    assert [(int(d["cpi"]), int(d["gate"]), int(d["doppler_bin"])) for d in found] == want
    assert (found["frequency"] == 0.0).all() and (found["peak_power"] > a_train * found["noise"]).all()
    assert (found["first_gate"] <= found["gate"]).all() and (found["gate"] <= found["last_gate"]).all()
    assert detect_pulse_train(host, r, c["pri"], P.CHAIN_K, normalize=True, fs=c["fs"], chunk_samples=100000).tobytes() \
        == found.tobytes()                                            # the same from host memory
    turned = P.chain_shift(host, 5)
    for src in (torch.from_numpy(turned).cuda(), turned):
        found = detect_pulse_train(src, r, c["pri"], P.CHAIN_K, normalize=True, fs=c["fs"])
        assert [(int(d["cpi"]), int(d["gate"]), int(d["doppler_bin"])) for d in found] == [(k, g, 5) for k, g, _ in want]
        assert np.allclose(found["frequency"], 5 * c["fs"] / (P.CHAIN_K * c["pri"]), rtol=1e-12, atol=0)
