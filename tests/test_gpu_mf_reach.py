"""The matched filter on the MI355X where tests/test_gpu_mf.py does not reach: every pfb_mf_spectra / pfb_mf_combine row
at its partition and output-count boundaries and the library's own fft_length choices on the device; quiet stretches of a
stream next to a loud one held to the quiet stretch's own allowance; designed cuttings with carries that span blocks and
runs of calls shorter than the carry; the staging steps of host-pointer and file calls and a workspace chunk walk with
several shared slots, byte for byte against the same steps made by hand; bit widths, samples that are not finite, async
calls that grow the workspace and a stream switch between two calls.  Everything against tests/mf_ref.py in float64
with TOL = 1e-5."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import mf_ref as R  # noqa: E402
from gpu_support import Busy, cuda_torch  # noqa: E402
from mf_support import WORST, check, on_device, reset_worst, run_guarded  # noqa: E402
from sdr_channelizer_amd import MatchedFilter, iqfile  # noqa: E402
from sdr_channelizer_amd import _lib as L  # noqa: E402

LOCAL = {"ratio": 0.0, "where": ""}   # the loud / quiet tests: the largest error in units of the quiet stretch's allowance


@pytest.fixture(scope="module")
def torch():
    t = cuda_torch()
    reset_worst()
    yield t
    # DESIGN.md section 15 quotes both figures
    print(f"\nmf reach worst error / (g Bnd) = {WORST['of_bound']:.3e} ({WORST['ratio']:.3f} of the allowance) at {WORST['where']}")
    print(f"mf reach worst quiet-stretch error = {LOCAL['ratio']:.3f} of the local allowance at {LOCAL['where']}")


@pytest.fixture(scope="module")
def busy(torch):
    b = Busy(torch)
    yield b
    del b.src, b.dst
    torch.cuda.empty_cache()


# ---- A. every table row, at its own boundaries ---------------------------------------------------------------------

@pytest.mark.parametrize("nfft", [1024, 2048, 4096])
@pytest.mark.parametrize("fmt,bw", R.FORMATS)
def test_partitioned_rows_at_their_boundaries(torch, fmt, bw, nfft):
    """pfb_mf_spectra<nfft, fmt> and pfb_mf_combine<nfft> with P = 1, 1 | 2 and 2 | 3 partitions, at output counts around
    one block: the store's min(B, outputs - m0) and the trailing spectra blocks that hold no sample"""
    B = nfft // 2
    counts = (0, 1, B - 1, B, B + 1, 2 * B + 3)
    for K in (1, B, B + 1, 2 * B, 2 * B + 1):
        r = R.random_replica(K, K + nfft)
        raw = R.random_raw(fmt, bw, K - 1 + counts[-1], K + bw)
        x = R.unpack(raw, fmt, bw)
        for normalize in (False, True):
            ref = R.compress(x, r, normalize)
            for output in ("complex", "power"):
                with MatchedFilter(r, fmt, bw, output, normalize, fft_length=nfft, route="partitioned") as mf:
                    assert mf.plan.partitions == -(-K // B) and mf.plan.block_outputs == B
                    assert mf.plan.route == L.PFB_MF_ROUTE_PARTITIONED and mf.plan.fft_length == nfft
                    for i, outs in enumerate(counts):
                        n = K - 1 + outs
                        for misalign in (False, True):
                            mf.reset()
                            assert mf.outputs_for(n) == outs
                            y = run_guarded(torch, mf, on_device(torch, raw[: 2 * n], misalign), outs, output,
                                            misalign ^ (i % 2 == 1))
                            check(y, ref[:outs], x[:n], r, normalize, output, ("rows", fmt, nfft, K, n, output, normalize))
                            assert mf.next_index == outs
                            if outs:
                                assert mf.last_kernel == f"pfb_mf_partitioned<N{nfft},{fmt}>"


DEFAULT_PLANS = [("auto", 64, 1024, "fused"), ("auto", 65, 2048, "fused"), ("auto", 1024, 2048, "fused"),
                 ("auto", 1025, 4096, "fused"), ("auto", 2048, 4096, "fused"), ("auto", 2049, 4096, "partitioned"),
                 ("partitioned", 1024, 2048, "partitioned"), ("partitioned", 1025, 4096, "partitioned")]


@pytest.mark.parametrize("route,K,nfft,kind", DEFAULT_PLANS)
def test_the_librarys_own_fft_lengths_on_the_device(torch, route, K, nfft, kind):
    """fft_length = 0 on either side of each threshold of the header's rule: the plan, the kernel that ran, the result"""
    n = K + 2 * nfft + 5
    r = R.random_replica(K, K + 7)
    for fmt, bw in (R.FORMATS[0], R.FORMATS[2]):
        raw = R.random_raw(fmt, bw, n, K + 8)
        x = R.unpack(raw, fmt, bw)
        for normalize, output in ((False, "complex"), (True, "power")):
            with MatchedFilter(r, fmt, bw, output, normalize, fft_length=0, route=route) as mf:
                assert mf.plan.fft_length == nfft
                assert mf.plan.route == (L.PFB_MF_ROUTE_FUSED if kind == "fused" else L.PFB_MF_ROUTE_PARTITIONED)
                y = run_guarded(torch, mf, on_device(torch, raw, normalize), n - K + 1, output, not normalize)
                assert mf.last_kernel == f"pfb_mf_{kind}<N{nfft},{fmt}>"
            check(y, R.compress(x, r, normalize), x, r, normalize, output, ("default plan", route, K, fmt, output))


# ---- B. a loud stretch next to a quiet one, held to the quiet one's allowance --------------------------------------

QUIET = {"int16": (16, 3), "int8": (8, 1), "cf32": (1, 1e-6)}   # bit width; quiet I/Q in -q .. q, or normal * q


def loud_and_quiet(fmt, n, lo, hi, seed):
    """n samples, loud (the full container, or standard normal) on [lo, hi) and quiet elsewhere"""
    rng = np.random.default_rng(seed)
    bw, q = QUIET[fmt]
    if fmt == "cf32":
        raw = rng.standard_normal(2 * n).astype(np.float32)
        raw[: 2 * lo] *= np.float32(q)
        raw[2 * hi:] *= np.float32(q)
        return raw
    full = 2 ** (bw - 1)
    raw = rng.integers(-q, q + 1, size=2 * n)
    raw[2 * lo: 2 * hi] = rng.integers(-full, full, size=2 * (hi - lo))
    return raw.astype(np.int8 if fmt == "int8" else np.int16)


def run_cut(mf, d, edges, route, nfft, K, lo, hi):
    """One cutting of the stream on a reset handle.  Returns the outputs and, for the leading (samples before lo) and the
    trailing (from hi on) stretch, the stream-absolute output ranges of the blocks whose whole input span -- what the
    block reads of the call's carry and samples -- lies in that stretch, with the number of whole blocks among them."""
    V = R.block_outputs(route, nfft, K)
    mf.reset()
    parts, quiet = [], {"lead": [], "trail": []}
    whole = {"lead": 0, "trail": 0}
    for a, b in zip(edges[:-1], edges[1:]):
        origin = a - min(a, K - 1)   # the stream index of the call's first carried sample
        assert mf.next_index == origin
        outs = mf.outputs_for(b - a)
        parts.append(mf.process(d[2 * a: 2 * b]))
        for blk in range(-(-outs // V)):
            s0, s1 = R.block_span(route, nfft, K, blk)
            s0, s1 = origin + s0, min(origin + s1, b)   # past the call's end the block holds zeros
            m0, m1 = origin + blk * V, origin + min((blk + 1) * V, outs)
            which = "lead" if s1 <= lo else "trail" if s0 >= hi else None
            if which:
                quiet[which].append((m0, m1))
                whole[which] += m1 - m0 == V
    return np.concatenate([p.cpu().numpy() for p in parts]), quiet, whole


@pytest.mark.parametrize("route,nfft,K", [("fused", 1024, 1), ("fused", 1024, 300), ("fused", 4096, 2048),
                                          ("partitioned", 1024, 700), ("partitioned", 4096, 5600)])
@pytest.mark.parametrize("fmt", list(QUIET))
def test_quiet_stretches_next_to_a_loud_one(torch, fmt, route, nfft, K):
    """A block is computed from its own input span, so the outputs of a block whose span is quiet meet the quiet
    stretch's allowance -- 90 (int8) to 10^6 (cf32) times tighter than the stream's -- whatever stale LDS, a wrong
    workspace slot or a wrong carry offset might leak in from the loud third; in one call, cut inside the leading quiet
    stretch, cut inside the loud one, where the carry of the next call holds loud samples, and cut at both."""
    bw = QUIET[fmt][0]
    V = R.block_outputs(route, nfft, K)
    n = 12 * V + 7 + K - 1   # twelve whole blocks and a partial one
    lo, hi = n // 3, 2 * n // 3
    raw = loud_and_quiet(fmt, n, lo, hi, K + nfft)
    x = R.unpack(raw, fmt, bw)
    r = R.random_replica(K, K + 1)
    ref = R.compress(x, r)
    stretches = {"lead": (0, R.compress(x[:lo], r), R.span_tolerance(x, r, 0, lo)),
                 "trail": (hi, R.compress(x[hi:], r), R.span_tolerance(x, r, hi, n))}
    assert 0.0 < max(s[2] for s in stretches.values()) < R.tolerance(x, r) / 50
    d = torch.from_numpy(raw).cuda()
    with MatchedFilter(r, fmt, bw, "complex", fft_length=nfft, route=route) as mf:
        assert mf.plan.block_outputs == V
        for edges in ([0, n], [0, lo // 2 + 1, n], [0, n // 2 + 1, n], [0, lo // 2 + 1, n // 2 + 1, n]):
            where = ("loud and quiet", fmt, route, nfft, K, tuple(edges[1:]))
            y, quiet, whole = run_cut(mf, d, edges, route, nfft, K, lo, hi)
            check(y, ref, x, r, False, "complex", where)
            for which, (first, own, e) in stretches.items():
                assert whole[which] >= 1, (where, which, quiet)
                for m0, m1 in quiet[which]:
                    ratio, _ = R.worst_ratio(y[m0:m1], own[m0 - first: m1 - first], e, "complex")
                    if ratio > LOCAL["ratio"]:
                        LOCAL.update(ratio=ratio, where=str(where + (which, m0)))
                    assert ratio <= 1.0, (where, which, m0, m1, ratio)


# ---- C. carries that span blocks, and runs of short calls ----------------------------------------------------------

@pytest.mark.parametrize("route,nfft,K", [("fused", 1024, 512), ("fused", 4096, 2048), ("partitioned", 1024, 2567),
                                          ("partitioned", 4096, 5600)])
@pytest.mark.parametrize("fmt,bw", [R.FORMATS[0], R.FORMATS[2]])
def test_designed_cuttings(torch, fmt, bw, route, nfft, K):
    """Calls of 1, K-2, 0, 1, 1, B, K-1, 1, 3B+1 samples and a rest: three calls and an empty one that only feed the
    carry (the history update reads its own output), the first output from a call that is all carry but one sample, a
    carry that spans blocks"""
    B = nfft // 2
    lengths = [1, K - 2, 0, 1, 1, B, K - 1, 1, 3 * B + 1, B + 77]
    edges = np.concatenate([[0], np.cumsum(lengths)]).tolist()
    n = edges[-1]
    raw = R.random_raw(fmt, bw, n, K + 3)
    x = R.unpack(raw, fmt, bw)
    r = R.random_replica(K, K + 4)
    ref = R.compress(x, r)
    e = R.tolerance(x, r)
    d = torch.from_numpy(raw).cuda()
    with MatchedFilter(r, fmt, bw, "complex", fft_length=nfft, route=route) as mf:
        runs = []
        for _ in range(2):
            mf.reset()
            assert mf.next_index == 0
            parts = []
            for a, b in zip(edges[:-1], edges[1:]):
                want = max(0, b - K + 1) - max(0, a - K + 1)
                assert mf.outputs_for(b - a) == want
                y = mf.process(d[2 * a: 2 * b])
                assert y.numel() == want and mf.next_index == max(0, b - K + 1)
                parts.append(y)
            assert [p.numel() for p in parts[:5]] == [0, 0, 0, 1, 1]
            runs.append(torch.cat(parts).cpu().numpy())
        assert runs[0].size == n - K + 1 and runs[0].tobytes() == runs[1].tobytes()
        check(runs[0], ref, x, r, False, "complex", ("designed cutting", fmt, route, nfft, K))
        mf.reset()
        one = mf.process(d).cpu().numpy()
        check(one, ref, x, r, False, "complex", ("designed cutting, one call", fmt, route, nfft, K))
        assert np.abs(runs[0].astype(np.complex128) - one).max() <= 2 * e


# ---- D. staging steps and workspace chunks -------------------------------------------------------------------------

def check_windows(y, raw, fmt, bw, r, normalize, output, seams, where):
    """the first and last 4096 outputs and [seam - K - 100, seam + 200) around each seam, each against the restatement
    of its own slice of the stream"""
    K, outputs = r.size, y.size
    spans = [(0, min(4096, outputs)), (max(0, outputs - 4096), outputs)]
    spans += [(seam - K - 100, seam + 200) for seam in seams]
    for a, b in spans:
        assert 0 <= a < b <= outputs
        xs = R.unpack(raw[2 * a: 2 * (b + K - 1)], fmt, bw)
        check(y[a:b], R.compress(xs, r, normalize), xs, r, normalize, output, (where, a, b))


def same_bytes(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


@pytest.mark.parametrize("K,output", [(300, "power"), (3000, "complex")])
def test_host_call_longer_than_a_staging_step(torch, K, output):
    """a host-pointer call of 2^23 + 5000 samples is staged in two steps, each one enqueue: a device-pointer run cut at
    2^23 gives the same bytes"""
    step = 1 << 23
    n = step + 5000
    raw = R.random_raw("int8", 8, n, K)
    r = R.random_replica(K, K + 1)
    with MatchedFilter(r, "int8", 8, output, True) as mf:
        assert mf.plan.route == (L.PFB_MF_ROUTE_FUSED if K == 300 else L.PFB_MF_ROUTE_PARTITIONED)
        y = mf.process(raw)
        assert isinstance(y, np.ndarray) and y.size == n - K + 1 and mf.next_index == n - K + 1
    with MatchedFilter(r, "int8", 8, output, True) as mf:
        d = torch.from_numpy(raw).cuda()
        z = torch.cat([mf.process(d[: 2 * step]), mf.process(d[2 * step:])]).cpu().numpy()
    assert same_bytes(y, z)
    check_windows(y, raw, "int8", 8, r, True, output, [step], ("host steps", K))


def test_file_longer_than_a_staging_step(torch, tmp_path):
    """a record of 2^22 + 5000 samples is staged in steps of 2^22 with the carry across the step"""
    K, step, bw = 3000, 1 << 22, 12
    n = step + 5000
    raw = R.random_raw("int16", bw, n, 91)
    r = R.random_replica(K, 92)
    path = str(tmp_path / "long.iq")
    iqfile.write_iq(path, raw.reshape(-1, 2), 56e6, 1e9, bw)
    with MatchedFilter(r, "int16", bw, "power") as mf:
        y, info = mf.process_iq_file(path)
        assert info.file_format == 3 and info.packet.numSamples == n and y.size == n - K + 1
        assert mf.next_index == n - K + 1
    with MatchedFilter(r, "int16", bw, "power") as mf:
        d = torch.from_numpy(raw).cuda()
        z = torch.cat([mf.process(d[: 2 * step]), mf.process(d[2 * step:])]).cpu().numpy()
    assert same_bytes(y, z)
    check_windows(y, raw, "int16", bw, r, False, "power", [step], "file steps")


def test_chunk_walk_with_several_shared_slots(torch):
    """4096 points, P = 3: a chunk of the workspace holds 2046 output blocks and the 2 spectra it shares with the next"""
    K, B = 5600, 2048
    n = 2048 * B + K + 100
    raw = R.random_raw("int8", 8, n, 93)
    r = R.random_replica(K, 94)
    with MatchedFilter(r, "int8", 8, "complex") as mf:
        P = mf.plan.partitions
        assert mf.plan.fft_length == 4096 and P == 3 and mf.plan.route == L.PFB_MF_ROUTE_PARTITIONED
        per_chunk = mf.plan.workspace_bytes // (8 * 4096) - (P - 1)
        assert per_chunk == 2046 and -(-(n - K + 1) // B) > per_chunk
        y = mf.process(torch.from_numpy(raw).cuda()).cpu().numpy()
        assert mf.last_kernel == "pfb_mf_partitioned<N4096,int8>"
    check_windows(y, raw, "int8", 8, r, False, "complex", [per_chunk * B], "chunk walk, P = 3")


# ---- E. small contract tests ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("fmt,bw", [("int8", 1), ("int8", 5), ("int16", 1), ("int16", 9), ("int16", 16)])
def test_bit_width_is_a_scale_and_nothing_else(torch, fmt, bw):
    """x = I / 2^(bit_width-1) whatever the raw values are: they fill the container here"""
    container = 8 if fmt == "int8" else 16
    n = 3000
    raw = R.random_raw(fmt, container, n, 80 + bw)
    x = R.unpack(raw, fmt, bw)
    assert np.abs(x.real).max() > (1.0 if bw < container else 0.99)
    assert np.array_equal(x.real * 2.0 ** (bw - 1), raw[0::2].astype(np.float64))
    for route, K in (("fused", 300), ("partitioned", 700)):
        r = R.random_replica(K, K + bw)
        for normalize, output in ((False, "complex"), (True, "power")):
            with MatchedFilter(r, fmt, bw, output, normalize, fft_length=1024, route=route) as mf:
                y = mf.process(torch.from_numpy(raw).cuda()).cpu().numpy()
            check(y, R.compress(x, r, normalize), x, r, normalize, output, ("bit width", fmt, bw, route, output))


@pytest.mark.parametrize("route,K", [("fused", 300), ("partitioned", 700)])
def test_a_sample_that_is_not_finite_stays_in_its_blocks(torch, route, K):
    """One NaN, then one +Inf, in a cf32 stream: every output whose window holds it is not finite; every output of the
    blocks whose input spans do not hold it is finite and right (the allowance of the stream with that sample zero);
    after reset() the handle is as good as new."""
    nfft = 1024
    V = R.block_outputs(route, nfft, K)
    n = 5 * V + 9 + K - 1
    n1 = 2 * V + 50 + K - 1   # where the two-call placement cuts: the sample sits in the second call's carry
    raw = R.random_raw("cf32", 1, n, K + 5)
    x = R.unpack(raw, "cf32", 1)
    r = R.random_replica(K, K + 6)
    outputs = n - K + 1
    with MatchedFilter(r, "cf32", 1, "complex", fft_length=nfft, route=route) as mf:
        for edges, s in (([0, n], 2 * V + 100), ([0, n], 2 * V), ([0, n1, n], n1 - 5)):
            x0 = x.copy()
            x0[s] = 0.0
            ref0 = R.compress(x0, r)
            for bad, part in ((np.nan, 0), (np.inf, 1)):
                where = ("not finite", route, len(edges), s, bad)
                spoiled = raw.copy()
                spoiled[2 * s + part] = bad
                d = torch.from_numpy(spoiled).cuda()
                mf.reset()
                parts, may = [], np.zeros(outputs, bool)
                for a, b in zip(edges[:-1], edges[1:]):
                    origin = a - min(a, K - 1)
                    outs = mf.outputs_for(b - a)
                    parts.append(mf.process(d[2 * a: 2 * b]).cpu().numpy())
                    if origin <= s < b:   # call-local, carry included
                        m0, m1 = R.outputs_seeing(route, nfft, K, s - origin, outs)
                        may[origin + m0: origin + m1] = True
                y = np.concatenate(parts)
                assert y.size == outputs
                must = np.zeros(outputs, bool)
                must[max(0, s - K + 1): min(s, outputs - 1) + 1] = True
                assert must.sum() == K and not (must & ~may).any() and (~may).sum() >= V, where
                assert not np.isfinite(y[must]).any(), where
                assert np.isfinite(y[~may]).all(), where
                check(y[~may], ref0[~may], x0, r, False, "complex", where)
        mf.reset()
        y = mf.process(torch.from_numpy(raw).cuda()).cpu().numpy()
        check(y, R.compress(x, r), x, r, False, "complex", ("finite again", route))


def test_async_calls_that_grow_the_workspace(torch, busy):
    """two sync=False partitioned calls on a busy stream, of 2 blocks and then of 40: the second replaces the workspace
    the first one's kernels use"""
    K, B = 700, 512
    n1, n2 = K - 1 + 2 * B, 40 * B
    raw = R.random_raw("int8", 8, n1 + n2, 95)
    x = R.unpack(raw, "int8", 8)
    r = R.random_replica(K, 96)
    d = torch.from_numpy(raw).cuda()
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    with MatchedFilter(r, "int8", 8, "complex", fft_length=1024, route="partitioned") as mf:
        mf.set_stream(s.cuda_stream)
        busy.queue(s)
        first = mf.process(d[: 2 * n1], sync=False)
        assert first.numel() == 2 * B and not s.query(), "the device caught up: the call was not issued ahead of it"
        second = mf.process(d[2 * n1:], sync=False)
        assert second.numel() == 40 * B
        mf.sync()
        y = torch.cat([first, second]).cpu().numpy()
        mf.set_stream(0)
    check(y, R.compress(x, r), x, r, False, "complex", "async workspace growth")


@pytest.mark.parametrize("route,K", [("fused", 300), ("partitioned", 700)])
def test_stream_switch_between_two_calls(torch, busy, route, K):
    """a call on a busy stream, set_stream, a call on the new stream: the second reads the carry the first writes"""
    n1, n2 = 5000, 3000
    raw = R.random_raw("int16", 12, n1 + n2, 97)
    x = R.unpack(raw, "int16", 12)
    r = R.random_replica(K, 98)
    d = torch.from_numpy(raw).cuda()
    sa, sb = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    with MatchedFilter(r, "int16", 12, "complex", fft_length=1024, route=route) as mf:
        mf.set_stream(sa.cuda_stream)
        busy.queue(sa)
        first = mf.process(d[: 2 * n1], sync=False)
        mf.set_stream(sb.cuda_stream)
        second = mf.process(d[2 * n1:], sync=False)
        assert not sb.query(), "the device caught up: the calls were not issued ahead of it"
        mf.sync()
        assert sa.query()   # the new stream waited for what the old one had queued
        y = torch.cat([first, second]).cpu().numpy()
        mf.set_stream(0)
    check(y, R.compress(x, r), x, r, False, "complex", ("stream switch", route))
