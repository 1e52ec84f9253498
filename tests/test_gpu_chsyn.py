"""The channel synthesizer on the GPU (pfb_chsyn_*), both routes, against the float64 restatement of tests/chsyn_ref.py.

Allowance.  With A[s] = |scale| sum_q |g[d + qD]| ||w o y[b-q, :]||_1 a kernel may differ from the float64 restatement
by C_ALLOW * 2^-24 * A[s].  C_ALLOW is 4 times the worst ratio |twin - float64| / (2^-24 A) that the float32 /
complex64 twin of chsyn_ref.py (the same sums in the stated order) shows on this module's own inputs, on the CPU:
measured 3.38 (at M = 256, D = 256, P_g = 1, with both flags and weights), so C_ALLOW = 13.6.  The 4 covers the different
summation trees and FMA contraction.  test_allowance_is_the_twins re-measures it without a GPU; nothing here is taken
from a kernel.
"""
import ctypes as C
import functools

import numpy as np
import pytest

import chsyn_ref as R
from gpu_support import Busy, cuda_torch
from oracle.pfb_oracle import OracleConfig, channelize_numpy
from sdr_channelizer_amd import _lib as L
from sdr_channelizer_amd import synthesizer as sy

gpu = pytest.mark.gpu
C_ALLOW = 13.6
EPS = 2.0 ** -24
FUSED_M = (56, 64, 128, 256)
GENERIC_M = (2, 3, 8, 12, 25, 56, 64, 130, 560, 1024)
P_ALL = (1, 2, 12, 24)


@pytest.fixture(scope="module")
def torch():
    return cuda_torch()


def decimations(M):
    return (M,) if M % 2 else (M, M // 2)


@functools.lru_cache(maxsize=None)
def frames_of(M, F, seed=0):
    rng = np.random.default_rng(1000 * M + seed)
    y = (rng.standard_normal((F, M)) + 1j * rng.standard_normal((F, M))).astype(np.complex64)
    y.setflags(write=False)
    return y


@functools.lru_cache(maxsize=None)
def taps_of(M, P, seed=0):
    g = np.random.default_rng(7 * M + P + seed).standard_normal(M * P).astype(np.float32)
    g.setflags(write=False)
    return g


@functools.lru_cache(maxsize=None)
def weights_of(M):
    w = np.random.default_rng(M).standard_normal(M).astype(np.float32)
    w.setflags(write=False)
    return w


@functools.lru_cache(maxsize=None)
def reference(M, D, P, F, flags=0, weighted=False, frame0=0):
    """(float64 result, allowance) of the module's inputs for one shape, computed once and shared"""
    y, g = frames_of(M, F), taps_of(M, P)
    w = weights_of(M) if weighted else None
    x = R.synthesize(y, g, M, D, flags=flags, weights=w, frame0=frame0)
    tol = C_ALLOW * EPS * R.allowance(y, g, M, D, weights=w)
    x.setflags(write=False)
    tol.setflags(write=False)
    return x, tol


def fused_frames(M, D, P):
    """frame counts 0 .. T + 2Q + 1 of a fused shape (T from the plan; None where the shape has no fused kernel)"""
    try:
        plan = sy.describe(M, taps_of(M, P), D, route="fused")
    except L.PfbError:
        return None
    return plan.tile_frames + 2 * plan.q + 1


# the shapes the twin is measured on: every (M, D, P) the GPU tests compare against float64, at a few frames
def twin_cases():
    for M in sorted(set(FUSED_M) | set(GENERIC_M)):
        for D in decimations(M):
            for P in P_ALL:
                yield M, D, P, (M * P // D) + 3 if M <= 256 else 3
    yield 4096, 2048, 2, 7


def test_allowance_is_the_twins():
    worst, where = 0.0, None
    for M, D, P, F in twin_cases():
        if M >= 560 and P > 2:
            continue  # the twin's M-term sums do not depend on P; the Q-term sum is covered at the smaller M
        y, g = frames_of(M, F), taps_of(M, P)
        for flags, w in ((0, None), (3, weights_of(M))):
            a = R.synthesize(y, g, M, D, flags=flags, weights=w)
            b = R.synthesize_f32(y, g, M, D, flags=flags, weights=w)
            A = R.allowance(y, g, M, D, weights=w)
            ratio = float((np.abs(a - b) / (EPS * A)).max())
            if ratio > worst:
                worst, where = ratio, (M, D, P, flags)
    print(f"worst twin ratio {worst:.3f} at {where}: C_ALLOW = 4 x = {4 * worst:.2f}")
    assert 4 * worst <= C_ALLOW <= 4 * worst * 1.05 + 0.05


# -- device helpers ----------------------------------------------------------------------------------------

class Checker:
    """Accumulates, on the device, the worst error over allowance of many calls; one read-back at the end."""

    def __init__(self, torch, x, tol, output="cf32", bit_width=12):
        self.t = torch
        self.full = float(1 << (bit_width - 1)) if output == "int16" else 1.0
        self.int16 = output == "int16"
        ref = torch.from_numpy(np.array(x)).cuda()   # writable copies for torch
        self.tol = torch.from_numpy(np.array(tol)).cuda()
        if self.int16:
            v = torch.view_as_real(ref) * self.full
            self.ref = torch.clamp(v, -self.full, self.full - 1)
            self.tol = (0.5 + self.tol * self.full)[:, None]
        else:
            self.ref = ref
        self.worst = torch.zeros((), dtype=torch.float64, device="cuda")
        self.calls = 0

    def add(self, out, first=0):
        n = out.shape[0]
        self.calls += 1
        if n == 0:
            return
        got = out.to(self.t.float64) if self.int16 else out.to(self.t.complex128)
        diff = (got - self.ref[first:first + n]).abs()
        tol = self.tol[first:first + n]
        ratio = self.t.where(diff <= tol, diff / (tol + 1e-300), self.t.full_like(diff, float("inf")))
        ratio = self.t.nan_to_num(ratio, nan=float("inf"))
        self.worst = self.t.maximum(self.worst, ratio.max())

    def done(self, what):
        worst = float(self.worst.item())
        print(f"{what}: {self.calls} calls, worst error / allowance = {worst:.3f}")
        assert worst <= 1.0, (what, worst)


def dev_frames(torch, M, F):
    return torch.from_numpy(np.array(frames_of(M, F))).cuda()   # a writable copy for torch


def make(M, D, P, route, output="cf32", **kw):
    return sy.ChannelSynthesizer(M, taps_of(M, P), D, route=route, output=output, **kw)


def raw_call(s, y_ptr, F, ld, out_ptr, cap, mem=L.PFB_MEM_DEVICE, async_=False):
    n = C.c_uint64(12345)
    if async_:
        rc = s._lib.pfb_chsyn_process_async(s._h, C.c_void_p(y_ptr), F, ld, C.c_void_p(out_ptr), cap, C.byref(n))
    else:
        rc = s._lib.pfb_chsyn_process(s._h, C.c_void_p(y_ptr), F, ld, C.c_void_p(out_ptr), cap, C.byref(n), mem)
    return rc, int(n.value)


def cut(rng, F, pieces, Q):
    """a cutting of F frames into calls: random lengths with calls of 0 frames and of fewer than Q - 1 among them"""
    lens, left = [0, min(1, F)], F - min(1, F)
    while left > 0:
        kind = rng.integers(4)
        n = 0 if kind == 0 else int(rng.integers(1, max(2, Q - 1))) if kind == 1 else int(rng.integers(1, max(2, F // pieces)))
        n = min(n, left)
        lens.append(n)
        left -= n
    return lens + [0]


def stream(s, y_t, lens):
    outs, at = [], 0
    for n in lens:
        outs.append(s.process(y_t[at:at + n]))
        at += n
    assert at == y_t.shape[0]
    return outs


def same_bits(torch, a, b):
    return a.shape == b.shape and a.dtype == b.dtype and bool(torch.equal(torch.view_as_real(a) if a.is_complex() else a,
                                                                          torch.view_as_real(b) if b.is_complex() else b))


# -- every shape, every route ------------------------------------------------------------------------------

@gpu
@pytest.mark.parametrize("route", ["fused", "generic"])
@pytest.mark.parametrize("M", FUSED_M)
def test_fused_shapes_every_frame_count(torch, M, route):
    """D = M and M/2, P_g in {1, 2, 12, 24}, both outputs, 0 .. T + 2Q + 1 frames, on every route the shape reaches"""
    for D in decimations(M):
        for P in P_ALL:
            Fmax = fused_frames(M, D, P)
            if Fmax is None:  # Q rows do not fit 64 KiB of LDS: the shape goes generic
                assert M * P // D >= 28 and sy.describe(M, taps_of(M, P), D).route == L.PFB_CHSYN_ROUTE_GENERIC
                with pytest.raises(L.PfbError):
                    make(M, D, P, "fused")
                if route == "fused":
                    continue
                Fmax = 2 * (M * P // D) + 18
            x, tol = reference(M, D, P, Fmax)
            y_t = dev_frames(torch, M, Fmax)
            for output in ("cf32", "int16"):
                scale = D if output == "cf32" else D / 4096.0  # int16: some samples inside the range, some saturated
                chk = Checker(torch, x * (scale / D), tol * (scale / D), output)
                with make(M, D, P, route, output, scale=scale) as s:
                    assert s.route == route and s.samples_for(7) == 7 * D
                    for F in range(Fmax + 1):
                        s.reset()
                        out = s.process(y_t[:F])
                        assert out.shape[0] == F * D
                        chk.add(out)
                    assert s.last_kernel.startswith(f"pfb_chsyn_{route}<") and s.frame_index == Fmax
                    assert ("int16" in s.last_kernel) == (output == "int16")
                    if route == "fused":
                        assert f"M{M}," in s.last_kernel
                chk.done(f"M={M} D={D} P={P} {route} {output}")


@gpu
@pytest.mark.parametrize("M", GENERIC_M + (4096,))
def test_generic_route_over_its_domain(torch, M):
    cases = [(D, P) for D in decimations(M) for P in P_ALL] if M < 4096 else [(2048, 2)]
    for D, P in cases:
        Q = M * P // D
        F = Q + 19 if M <= 256 else min(Q, 8) + 5
        x, tol = reference(M, D, P, F)
        y_t = dev_frames(torch, M, F)
        for output in ("cf32", "int16"):
            scale = D if output == "cf32" else D / 4096.0
            chk = Checker(torch, x * (scale / D), tol * (scale / D), output)
            with make(M, D, P, "generic", output, scale=scale) as s:
                assert s.route == "generic" and s.plan.q == Q
                whole = s.process(y_t)
                chk.add(whole)
                s.reset()
                rng = np.random.default_rng(M + P)
                parts = stream(s, y_t, cut(rng, F, 4, Q))
                assert same_bits(torch, torch.cat(parts), whole), (M, D, P, output)
                assert s.last_kernel == f"pfb_chsyn_generic<{output}>"
            chk.done(f"M={M} D={D} P={P} generic {output}")


# -- pointers, ld, guards ----------------------------------------------------------------------------------

@gpu
@pytest.mark.parametrize("M,route", [(64, "fused"), (56, "fused"), (256, "fused"), (64, "generic"), (25, "generic")])
def test_pointers_ld_and_guard_bytes(torch, M, route):
    D, P = (M // 2 if M % 2 == 0 else M), 2
    F = 3 * (M * P // D) + 37
    x, tol = reference(M, D, P, F)
    y = np.array(frames_of(M, F))
    for output, elem in (("cf32", 8), ("int16", 4)):
        scale = D if output == "cf32" else D / 4096.0
        chk = Checker(torch, x * (scale / D), tol * (scale / D), output)
        with make(M, D, P, route, output, scale=scale) as s:
            base = None
            for ld in (M, M + 1, M + 2, M + 7):
                for y_off in (0, 1):          # values of 8 bytes: 1 = a pointer that is not 16-byte aligned
                    for out_off in (0, 1, 2, 3):   # output samples
                        buf = torch.full((F * ld + 8,), float("nan"), dtype=torch.complex64, device="cuda")
                        view = buf[y_off:y_off + F * ld].view(F, ld)
                        view[:, :M] = torch.from_numpy(y).cuda()   # the columns past M stay NaN: never read
                        guard = 64
                        raw = torch.full((guard + F * D * elem + guard + 16,), 0xA5, dtype=torch.uint8, device="cuda")
                        first = guard + out_off * elem
                        s.reset()
                        rc, n = raw_call(s, buf.data_ptr() + 8 * y_off, F, ld, raw.data_ptr() + first, F * D)
                        assert (rc, n) == (L.PFB_OK, F * D)
                        body = raw[first:first + F * D * elem]
                        out = body.view(torch.complex64) if output == "cf32" else body.view(torch.int16).view(-1, 2)
                        chk.add(out.clone() if out_off == 0 else out.contiguous())
                        assert bool((raw[:first] == 0xA5).all()) and bool((raw[first + F * D * elem:] == 0xA5).all())
                        base = body.clone() if base is None else base
                        assert bool(torch.equal(body, base)), (ld, y_off, out_off)   # alignment changes no bit
            # what the checks refuse, with no state change
            good = torch.zeros(F * D * elem + 16, dtype=torch.uint8, device="cuda")
            yb = torch.zeros(F * M + 2, dtype=torch.complex64, device="cuda")
            before = s.frame_index
            assert raw_call(s, yb.data_ptr() + 4, F, M, good.data_ptr(), F * D)[0] == L.PFB_ERR_BAD_ARG
            assert raw_call(s, yb.data_ptr(), F, M, good.data_ptr() + elem // 2, F * D)[0] == L.PFB_ERR_BAD_ARG
            assert raw_call(s, yb.data_ptr(), F, M - 1, good.data_ptr(), F * D)[0] == L.PFB_ERR_BAD_ARG
            assert raw_call(s, yb.data_ptr(), F, M, good.data_ptr(), F * D, mem=2)[0] == L.PFB_ERR_BAD_ARG
            assert raw_call(s, 0, F, M, good.data_ptr(), F * D)[0] == L.PFB_ERR_BAD_ARG
            assert raw_call(s, yb.data_ptr(), F, M, 0, F * D)[0] == L.PFB_ERR_BAD_ARG
            assert raw_call(s, yb.data_ptr(), F, M, good.data_ptr(), F * D - 1) == (L.PFB_ERR_CAPACITY, F * D)
            assert raw_call(s, yb.data_ptr(), F, M, good.data_ptr(), F * D - 1, async_=True) == (L.PFB_ERR_CAPACITY, F * D)
            assert s.frame_index == before
        chk.done(f"M={M} {route} {output} pointers")


# -- int16: rounding and saturation ------------------------------------------------------------------------

@gpu
@pytest.mark.parametrize("M,route", [(64, "fused"), (128, "fused"), (64, "generic"), (8, "generic"), (3, "generic")])
@pytest.mark.parametrize("bit_width", [12, 16, 2])
def test_int16_rounds_halves_away_from_zero_and_saturates(torch, M, route, bit_width):
    """P_g = 1, D = M, g = 1, scale = 1 and only channel 0 fed: x[bM + d] = y[b, 0] with no rounding at all, so the
    stored integers are the definition's, exactly"""
    full = 1 << (bit_width - 1)
    vals = np.array([0.0, 0.5, -0.5, 1.5, -1.5, 2.5, -2.5, 0.25, -0.25, 0.75, full - 1, full - 1.5, full - 0.5, full, full + 3,
                     -full, -full + 0.5, -full - 0.5, -full - 7, 1e9, -1e9, 1.25, -0.75]) / full
    F = vals.size
    y = np.zeros((F, M), np.complex64)
    y[:, 0] = vals + 1j * vals[::-1]
    assert np.array_equal(y[:, 0].real.astype(np.float64) * full, vals * full)   # the inputs are exact in float32
    want = R.quantize_int16(np.repeat(y[:, 0], M), bit_width)
    r = np.sign(vals * full) * np.floor(np.abs(vals * full) + 0.5)
    assert want[::M, 0].tolist() == np.clip(r, -full, full - 1).astype(int).tolist()
    with sy.ChannelSynthesizer(M, np.ones(M, np.float32), M, scale=1.0, output="int16", bit_width=bit_width,
                               route=route) as s:
        out = s.process(torch.from_numpy(y).cuda()).cpu().numpy()
        s.reset()
        host = s.process(y)
    assert out.shape == (F * M, 2) and np.array_equal(out, want)
    assert np.array_equal(host, want)


# -- flags and weights -------------------------------------------------------------------------------------

@gpu
@pytest.mark.parametrize("M,D,route", [(64, 32, "fused"), (64, 32, "generic"), (56, 56, "fused"), (128, 64, "fused"),
                                        (12, 6, "generic"), (25, 25, "generic")])
def test_flags_and_weights(torch, M, D, route):
    P = 2
    Q = M * P // D
    F = 2 * Q + 21
    y_t = dev_frames(torch, M, F)
    for flags in (0, R.FFTSHIFT, R.DEROTATE, R.FFTSHIFT | R.DEROTATE):
        for weighted in (False, True):
            x, tol = reference(M, D, P, F, flags, weighted)
            chk = Checker(torch, x, tol)
            with make(M, D, P, route, fftshift=bool(flags & 1), derotate=bool(flags & 2),
                      weights=weights_of(M) if weighted else None) as s:
                chk.add(s.process(y_t))
            chk.done(f"M={M} D={D} {route} flags={flags} weights={weighted}")
    # a weight change between calls takes effect from the next frame: the frames already in keep theirs
    w0, w1 = weights_of(M), np.where(np.arange(M) % 3 == 0, 1.0, 0.0).astype(np.float32)
    y, g = frames_of(M, F), taps_of(M, P)
    k = Q + 3
    xa, hist = R.synthesize(y[:k], g, M, D, weights=w0, return_history=True)
    xb = R.synthesize(y[k:], g, M, D, weights=w1, history=hist, frame0=k)
    A = np.concatenate([R.allowance(y[:k], g, M, D, weights=w0),
                        np.maximum(R.allowance(y, g, M, D, weights=w0), R.allowance(y, g, M, D, weights=w1))[k * D:]])
    chk = Checker(torch, np.concatenate([xa, xb]), C_ALLOW * EPS * A)
    with make(M, D, P, route, weights=w0) as s:
        chk.add(s.process(y_t[:k]))
        s.set_weights(w1)
        chk.add(s.process(y_t[k:]), first=k * D)
        s.set_weights(None)   # all ones again
        s.reset()
        ones = s.process(y_t)
    chk.done(f"M={M} D={D} {route} weight change")
    chk = Checker(torch, *reference(M, D, P, F))
    chk.add(ones)
    chk.done(f"M={M} D={D} {route} weights back to ones")
    # a stream that starts at frame 7: the derotation index is the absolute one
    if D != M:
        x, tol = reference(M, D, P, F, R.DEROTATE)
        with make(M, D, P, route, derotate=True) as s:
            whole = s.process(y_t)
            s.reset()
            head = s.process(y_t[:7])
            assert s.frame_index == 7
            s.set_frame_index(0)
            wrong = s.process(y_t[7:])
            assert not same_bits(torch, wrong, whole[7 * D:])   # D = M/2 and an odd start: the rows are read half a turn off
        with make(M, D, P, route, derotate=True) as s:
            s.set_frame_index(100)
            first = s.process(y_t[:7])
            assert s.frame_index == 107
            s.set_frame_index(7)
            rest = s.process(y_t[7:])
        assert same_bits(torch, head, first) and same_bits(torch, rest, whole[7 * D:])   # an even shift changes nothing
        chk = Checker(torch, x, tol)
        chk.add(whole)
        chk.done(f"M={M} D={D} {route} derotate")


# -- cutting -----------------------------------------------------------------------------------------------

@gpu
@pytest.mark.parametrize("M,D,P", [(64, 32, 12), (128, 64, 12), (56, 56, 2), (256, 128, 2), (64, 64, 1)])
@pytest.mark.parametrize("output", ["cf32", "int16"])
def test_any_cutting_gives_the_same_bits(torch, M, D, P, output):
    Q = M * P // D
    F = fused_frames(M, D, P) * 2 + 5
    x, tol = reference(M, D, P, F)
    y_t = dev_frames(torch, M, F)
    scale = D if output == "cf32" else D / 4096.0
    got = {}
    for route in ("fused", "generic"):
        with make(M, D, P, route, output, scale=scale) as s:
            whole = s.process(y_t)
            rng = np.random.default_rng(M + D + P)
            for trial in range(4):
                lens = cut(rng, F, 2 + 3 * trial, Q)
                assert 0 in lens and (Q <= 2 or any(0 < n < Q - 1 for n in lens))
                for again in range(2):   # the same cutting twice
                    s.reset()
                    parts = torch.cat(stream(s, y_t, lens))
                    assert same_bits(torch, parts, whole), (route, trial, again)
            s.reset()
            one_by_one = torch.cat([s.process(y_t[i:i + 1]) for i in range(F)])
            assert same_bits(torch, one_by_one, whole), route
        chk = Checker(torch, x * (scale / D), tol * (scale / D), output)
        chk.add(whole)
        chk.done(f"M={M} D={D} P={P} {route} {output}")
        got[route] = whole
    if output == "cf32":   # the two routes differ by rounding only: twice the allowance
        diff = (got["fused"].to(torch.complex128) - got["generic"].to(torch.complex128)).abs().cpu().numpy()
        assert (diff <= 2 * tol).all(), float((diff / (2 * tol + 1e-300)).max())
    else:
        assert int((got["fused"].to(torch.int32) - got["generic"].to(torch.int32)).abs().max()) <= 1


# -- host, device, async -----------------------------------------------------------------------------------

@gpu
@pytest.mark.parametrize("M,D,P,route", [(64, 32, 12, "fused"), (64, 32, 12, "generic"), (25, 25, 2, "generic")])
def test_host_device_and_async_calls_agree(torch, M, D, P, route):
    Q = M * P // D
    F = 3 * Q + 50
    y = np.array(frames_of(M, F))
    y_t = torch.from_numpy(y).cuda()
    x, tol = reference(M, D, P, F)
    with make(M, D, P, route) as s:
        dev = s.process(y_t)
        s.reset()
        host = s.process(y)   # numpy in, numpy out, staged
        assert isinstance(host, np.ndarray) and np.array_equal(host.view(np.float32), dev.cpu().numpy().view(np.float32))
        s.reset()
        wide = np.full((F, M + 5), np.nan + 0j, np.complex64)
        wide[:, :M] = y
        assert np.array_equal(s.process(wide[:, :M]).view(np.float32), host.view(np.float32))   # ld = M + 5 on the host
        s.reset()
        exact = np.full((F - 1) * (M + 5) + M, np.nan + 0j, np.complex64)   # the buffer ends with the last frame's M values
        rows = np.lib.stride_tricks.as_strided(exact, (F, M), ((M + 5) * 8, 8))
        rows[:] = y
        assert np.array_equal(s.process(rows).view(np.float32), host.view(np.float32))
        # async on a stream of the caller's, the host ahead of the device, then a switch to another stream mid-stream
        busy = Busy(torch)
        s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
        s.reset()
        s.sync()
        s.set_stream(s1.cuda_stream)
        busy.queue(s1, copies=2)
        a = s.process(y_t[:Q + 7], sync=False)
        b = s.process(y_t[Q + 7:Q + 9], sync=False)
        s.set_stream(s2.cuda_stream)
        c = s.process(y_t[Q + 9:], sync=False)
        s.sync()
        s1.synchronize()
        assert same_bits(torch, torch.cat([a, b, c]), dev)
        s.set_stream(0)
        # PFB_ERR_CAPACITY changes no state: the call that follows continues the stream
        s.reset()
        out = torch.empty(F * D, dtype=torch.complex64, device="cuda")
        k = Q + 1
        assert raw_call(s, y_t.data_ptr(), k, M, out.data_ptr(), k * D) == (L.PFB_OK, k * D)
        assert raw_call(s, y_t[k:].data_ptr(), F - k, M, out[k * D:].data_ptr(), 5) == (L.PFB_ERR_CAPACITY, (F - k) * D)
        assert raw_call(s, y[k:].ctypes.data, F - k, M, host.ctypes.data, 5, mem=L.PFB_MEM_HOST) == (L.PFB_ERR_CAPACITY, (F - k) * D)
        assert s.frame_index == k
        assert raw_call(s, y_t[k:].data_ptr(), F - k, M, out[k * D:].data_ptr(), (F - k) * D)[0] == L.PFB_OK
        assert same_bits(torch, out, dev)
    chk = Checker(torch, x, tol)
    chk.add(dev)
    chk.done(f"M={M} D={D} {route} host/device/async")


@gpu
@pytest.mark.parametrize("route", ["fused", "generic"])
def test_a_host_call_of_three_staging_steps(torch, route):
    """rows 64 KiB apart: 1024 frames fill a 64 MiB staging step, 2100 frames take three"""
    M, D, P, ld, F = 64, 32, 2, 8192, 2100
    rng = np.random.default_rng(5)
    wide = np.zeros((F, ld), np.complex64)
    y = (rng.standard_normal((F, M)) + 1j * rng.standard_normal((F, M))).astype(np.complex64)
    wide[:, :M] = y
    with make(M, D, P, route) as s:
        host = s.process(wide[:, :M])
        s.reset()
        dev = s.process(torch.from_numpy(y).cuda()).cpu().numpy()
    assert np.array_equal(host.view(np.float32), dev.view(np.float32))
    g = taps_of(M, P)
    x = R.synthesize(y, g, M, D)
    assert (np.abs(host - x) <= C_ALLOW * EPS * R.allowance(y, g, M, D)).all()


@gpu
def test_the_generic_workspace_grows_and_is_walked_in_chunks(torch):
    """M = 1024: the 64 MiB workspace holds 8192 frames; a call of 8192 + 37 after a short one grows it and takes two
    chunks, with the same bits as the stream cut into short calls"""
    M, D, P = 1024, 1024, 2
    F = 8192 + 37
    gen = torch.Generator(device="cuda").manual_seed(3)
    y_t = torch.view_as_complex(torch.randn((F, M, 2), generator=gen, device="cuda", dtype=torch.float32))
    with make(M, D, P, "generic") as s:
        assert s.plan.workspace_bytes == 64 << 20
        small = s.process(y_t[:5])
        big = s.process(y_t[5:])
        whole = torch.cat([small, big])
        s.reset()
        parts = torch.cat([s.process(y_t[i:i + 1000]) for i in range(0, F, 1000)])
    assert same_bits(torch, parts, whole)
    tail = y_t[F - 40:].cpu().numpy()   # the frames around the chunk boundary at local frame 8192 of the second call
    g = taps_of(M, P)
    x = R.synthesize(tail, g, M, D)[D:]   # Q = 2: the first block lacks its history
    got = whole[(F - 39) * D:].cpu().numpy()
    assert (np.abs(got - x) <= C_ALLOW * EPS * R.allowance(tail, g, M, D)[D:]).all()


# -- elements that are not finite --------------------------------------------------------------------------

@gpu
@pytest.mark.parametrize("M,D,P,route", [(64, 32, 2, "fused"), (128, 128, 2, "fused"), (64, 32, 2, "generic"),
                                          (12, 6, 2, "generic")])
def test_non_finite_elements_poison_only_what_their_frame_reaches(torch, M, D, P, route):
    Q = M * P // D
    F = 4 * Q + 30
    x, tol = reference(M, D, P, F)
    for output, elem in (("cf32", 8), ("int16", 4)):
        scale = D if output == "cf32" else D / 4096.0
        for bad, m0 in ((np.nan, Q + 5), (np.inf, 0), (-np.inf, F - 1)):
            y = frames_of(M, F).copy()
            y[m0, 3 % M] = bad
            raw = torch.full((64 + F * D * elem + 64,), 0x5A, dtype=torch.uint8, device="cuda")
            with make(M, D, P, route, output, scale=scale) as s:
                rc, n = raw_call(s, torch.from_numpy(y).cuda().data_ptr(), F, M, raw.data_ptr() + 64, F * D)
            assert (rc, n) == (L.PFB_OK, F * D)
            assert bool((raw[:64] == 0x5A).all()) and bool((raw[64 + F * D * elem:] == 0x5A).all())
            body = raw[64:64 + F * D * elem]
            out = body.view(torch.complex64) if output == "cf32" else body.view(torch.int16).view(-1, 2)
            lo, hi = m0 * D, min(F, m0 + Q) * D
            chk = Checker(torch, x * (scale / D), tol * (scale / D), output)
            chk.add(out[:lo].contiguous())
            chk.add(out[hi:].contiguous(), first=hi)
            chk.done(f"M={M} {route} {output} {bad} in frame {m0}")


# -- end to end --------------------------------------------------------------------------------------------

@gpu
@pytest.mark.parametrize("route", ["fused", "generic"])
def test_end_to_end_isolates_a_pulse(torch, route):
    """An LFM pulse around column 5 and a tone ten columns away through Channelizer(64, D = 32), a mask and the synthesizer:
    equal to the float64 chain within the allowances of both stages, the tone gone; isolate_band puts the matched
    filter's peak at the pulse's true start."""
    import sdr_channelizer_amd as pkg
    M, D, bw, N = 64, 32, 12, 32 * 640
    fs, f0, pw, start = 64e6, 5e6, 2000, 5000
    kw = dict(sample_format="int16", bit_width=bw, fs=fs, f0=f0, pw=pw, pri=N, first_pulse=start, lfm_extent_hz=2e6,
              amplitude=0.4, noise_sigma=0.0)
    pulse = pkg.pulse_train(N, device=False, **kw).astype(np.int32)
    n = np.arange(N)
    tone = np.round(0.4 * 2047 * np.exp(2j * np.pi * 15 * n / M))
    iq = (pulse + np.stack([tone.real, tone.imag], axis=1).astype(np.int32)).astype(np.int16)
    h, g = pkg.design_prototype(M, 12), sy.design_synthesis_taps(M, D)
    mask = np.zeros(M, np.float32)
    mask[3:9] = 1.0
    # the float64 chain
    x64 = (iq[:, 0].astype(np.float64) + 1j * iq[:, 1]) / 2 ** (bw - 1)
    y64 = channelize_numpy(x64, h.astype(np.float64), OracleConfig(M, 12, D))
    want = R.synthesize(y64, g.astype(np.float64), M, D, weights=mask)
    with pkg.Channelizer(M, taps=h, decimation=D, sample_format="int16", bit_width=bw) as ch, \
            sy.ChannelSynthesizer(M, g, D, weights=mask, route=route) as s:
        y_t = ch(torch.from_numpy(iq).cuda())
        got = s.process(y_t).cpu().numpy()
        assert s.route == route
    y_gpu = y_t.cpu().numpy()
    e1 = 1e-5 * np.abs(y64).max()   # the channelizer's own bound, as smoke() states it
    assert np.abs(y_gpu - y64).max() <= e1
    allow = C_ALLOW * EPS * R.allowance(y64, g, M, D, weights=mask) + R.allowance(np.full_like(y64, e1), g, M, D, weights=mask)
    assert got.shape == want.shape and (np.abs(got - want) <= allow).all()
    # the tone is gone, the pulse is there
    delay = sy.synthesis_delay(h.size, g.size, D - 1)
    seg = got[delay:]
    on, off = seg[start + 200:start + pw - 200], seg[start + pw + 2000:]
    assert abs(np.abs(on).mean() - 0.4) < 0.01 and np.abs(off).max() < 1e-3
    # isolate_band: aligned with its input, on the host and on the device
    host = sy.isolate_band(iq, M, range(3, 9), bit_width=bw, route=route)
    dev = sy.isolate_band(torch.from_numpy(iq).cuda(), M, range(3, 9), bit_width=bw, route=route)
    assert host.shape == (N,) and host.dtype == np.complex64 and tuple(dev.shape) == (N,)
    assert (np.abs(host - dev.cpu().numpy())[:N - delay] <= 2 * allow[delay:]).all()
    assert (np.abs(host[:N - delay] - got[delay:]) <= 2 * allow[delay:]).all()
    replica = pkg.replica_from_pulse_train(**kw)
    assert replica.size == pw
    with pkg.MatchedFilter(replica, "cf32", output="power") as mf:
        p = mf.process(dev)
    assert int(torch.argmax(p).item()) == start
    clean = pulse[start:start + pw]
    ref = (clean[:, 0] + 1j * clean[:, 1]) / 2 ** (bw - 1)
    # away from the pulse's edges (whose splatter the mask cuts off) the band is the pulse, sample for sample: one sample
    # of misalignment would be half a radian at 5 MHz
    assert np.abs(host[start + 600:start + pw - 600] - ref[600:pw - 600]).max() < 0.05
