"""The calls nobody waits for: pfb_process_async / pfb_sync / pfb_stft_process_async on non-blocking streams with the
host ahead of the device -- how bench.py and every rate meter drive the library.  This is where the two-buffer history
hand-over (d_hist[cur] / d_carry[cur]), the event ordering of pfb_set_stream, the regrowth of the slab scratch and the
state calls (get_state / reset / prime / set_frame_index) run behind queued work.  Every check compares bits with a
synchronous run of the same stream."""
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from gpu_support import Busy, cuda_torch  # noqa: E402
from pdw_checks import synthetic_matrix  # noqa: E402
from plan_support import device_input  # noqa: E402
from sdr_channelizer_amd import Channelizer, Stft, synth  # noqa: E402
from sdr_channelizer_amd import _lib as L  # noqa: E402
from sdr_channelizer_amd.pdw import extract_pdws, extract_pdws_raw  # noqa: E402

# (M, P, D, format, bit width, channel-major, expected kernel prefix): the wave-pair tiles, a 2x-oversampled shape, a
# team plan whose channel-major output goes by slabs, the smallest cf32 shape, and a band count only the generic
# kernel takes
CASES = [(64, 12, 64, "int16", 12, False, "pfb_fast<M64,"), (128, 12, 64, "int16", 12, False, "pfb_fast<M128,"),
         (560, 12, 560, "int8", 8, True, "pfb_fast<M560,"), (8, 12, 8, "cf32", 1, False, "pfb_fast<M8,"),
         (36, 12, 36, "int16", 12, False, "pfb_generic")]
IDS = [f"M{c[0]}-D{c[2]}-{c[3]}{'-cm' if c[5] else ''}" for c in CASES]


@pytest.fixture(scope="module")
def torch():
    return cuda_torch()


def make_handle(case, seed=3, **extra):
    M, P, D, fmt, bw, cm, _ = case
    h = (np.random.default_rng(seed).standard_normal(M * P) / M).astype(np.float32)
    return Channelizer(M, taps=h, decimation=D, sample_format=fmt, bit_width=bw, channel_major=cm, fftshift=True, **extra)


def ragged_lengths(rng, D, hist, count=44):
    """Call lengths in samples: empty, one sample, less than a frame, less than the history, exact multiples of D, and
    ragged ones of up to a few hundred frames."""
    fixed = [0, 1, D - 1, 1, max(1, hist // 2), hist - 1, D, 7 * D, 64 * D, 0, D + 1, 2 * hist + 3]
    lens = fixed + [int(rng.integers(1, 300 * D)) for _ in range(count - len(fixed))]
    order = rng.permutation(len(lens))
    return [lens[i] for i in order]


def size_slab_scratch(ch, bufs):
    """A handle that goes by slabs synchronises its stream whenever a call needs a larger scratch than the last: size
    it once up front with the longest call, so that the calls under test run with the host ahead (the regrowth itself is
    test_slab_scratch_regrown_behind_queued_calls)."""
    if ch.channel_major:
        ch(max(bufs, key=lambda x: x.shape[0]))
        ch.reset()


@pytest.fixture(scope="module")
def busy(torch):
    b = Busy(torch)
    yield b
    del b.src, b.dst
    torch.cuda.empty_cache()


def join(torch, parts, cm):
    parts = [p for p in parts if p.numel()]
    return torch.cat(parts, dim=1 if cm else 0)


def rows(y, a, b, cm):
    return y[:, a:b] if cm else y[a:b]


@pytest.mark.parametrize("switch", [False, True], ids=["one-stream", "stream-switch"])
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_back_to_back_async_calls(torch, busy, case, switch):
    """44 sync=False calls of ragged lengths from distinct buffers into distinct outputs with no host synchronisation
    in between; with `switch`, the handle moves to a second stream after a third of them and back after two thirds."""
    M, P, D, fmt, bw, cm, kernel = case
    rng = np.random.default_rng(M + D)
    with make_handle(case) as ref, make_handle(case) as ch:
        rep = ch.last_launch
        assert all(getattr(rep, f) == 0 for f, _ in L.PfbLaunchReport._fields_)   # nothing launched yet
        lens = ragged_lengths(rng, D, ch.history_samples)
        iq = device_input(sum(lens), fmt, bw, 77)
        want = ref(iq)
        assert ref.last_kernel.startswith(kernel), ref.last_kernel
        cuts = np.concatenate([[0], np.cumsum(lens)])
        bufs = [iq[a:b].clone() for a, b in zip(cuts[:-1], cuts[1:])]
        size_slab_scratch(ch, bufs)
        s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
        torch.cuda.synchronize()
        ch.set_stream(s1.cuda_stream)
        busy.queue(s1)
        outs, last = [], s1
        for i, x in enumerate(bufs):
            if switch and i == len(bufs) // 3:
                ch.set_stream(s2.cuda_stream)
                last = s2
            if switch and i == 2 * len(bufs) // 3:
                ch.set_stream(s1.cuda_stream)
                last = s1
            outs.append(ch(x, sync=False))
        assert not last.query(), "the device caught up: the calls were not issued ahead of it"
        ch.sync()
        torch.cuda.synchronize()
        assert ch.last_kernel.startswith(kernel)
        got = join(torch, outs, cm)
        assert got.shape == want.shape and torch.equal(got, want), case
        assert sum(o.numel() == 0 for o in outs) >= 3   # the empty calls were in there


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_state_calls_behind_queued_work(torch, busy, case):
    """get_state(), reset() and prime() on device data directly behind queued async calls."""
    M, P, D, fmt, bw, cm, kernel = case
    rng = np.random.default_rng(2 * M + D)
    with make_handle(case) as ref, make_handle(case) as ch, make_handle(case) as resumed:
        lens = ragged_lengths(rng, D, ch.history_samples, count=24)
        iq = device_input(sum(lens), fmt, bw, 78)
        want = ref(iq)
        cuts = np.concatenate([[0], np.cumsum(lens)])
        bufs = [iq[a:b].clone() for a, b in zip(cuts[:-1], cuts[1:])]
        size_slab_scratch(ch, bufs)
        s = torch.cuda.Stream()
        torch.cuda.synchronize()
        ch.set_stream(s.cuda_stream)

        # get_state() behind the first ten calls: the blob resumes in a second handle to the one-shot's remaining
        # rows, and the handle it was taken from goes on to the same rows
        busy.queue(s)
        outs = [ch(x, sync=False) for x in bufs[:10]]
        assert not s.query()
        blob = ch.get_state()
        outs += [ch(x, sync=False) for x in bufs[10:]]
        ch.sync()
        assert torch.equal(join(torch, outs, cm), want), case
        done = sum(o.shape[1 if cm else 0] for o in outs[:10])
        resumed.set_state(blob)
        rest = resumed(iq[cuts[10]:])
        assert torch.equal(rest, rows(want, done, want.shape[1 if cm else 0], cm).contiguous()), case

        # reset() behind queued calls (the handle is mid-stream, a partial frame carried): the fresh-handle bits
        busy.queue(s)
        junk = [ch(x, sync=False) for x in bufs[3:9]]
        ch.reset()
        outs = [ch(x, sync=False) for x in bufs]
        assert not s.query()
        ch.sync()
        assert torch.equal(join(torch, outs, cm), want), case

        # prime() on device data behind queued calls: sections 8 ... 15 go in as history only, the calls after them
        # produce the one-shot's rows
        ch.reset()
        busy.queue(s)
        outs = [ch(x, sync=False) for x in bufs[:8]]
        done = sum(o.shape[1 if cm else 0] for o in outs)
        skipped = 0
        for x in bufs[8:16]:
            skipped += ch.frames_for(x.shape[0])
            ch.prime(x)
        tail = [ch(x, sync=False) for x in bufs[16:]]
        assert not s.query()
        ch.sync()
        total = want.shape[1 if cm else 0]
        assert torch.equal(join(torch, outs, cm), rows(want, 0, done, cm).contiguous())
        assert torch.equal(join(torch, tail, cm), rows(want, done + skipped, total, cm).contiguous()), case
        del junk


def test_set_frame_index_behind_queued_work(torch, busy):
    """set_frame_index() with derotate at D = M/2 directly behind a queued call: the later calls take the new index (an
    odd shift flips the sign of every odd channel), as in a synchronous run of the same sequence."""
    case = CASES[1]
    M, P, D = case[:3]
    n1, n2 = 5000 * D + 17, 3000 * D + 5
    iq = device_input(n1 + n2, "int16", 12, 79)
    a, b = iq[:n1].clone(), iq[n1:].clone()
    with make_handle(case, derotate=True) as ref, make_handle(case, derotate=True) as ch:
        one = ref(iq)
        ref.reset()
        w1 = ref(a)
        ref.set_frame_index(w1.shape[0] + 1)
        w2 = ref(b)
        assert torch.equal(w1, one[:w1.shape[0]]) and not torch.equal(w2, one[w1.shape[0]:])
        s = torch.cuda.Stream()
        torch.cuda.synchronize()
        ch.set_stream(s.cuda_stream)
        busy.queue(s)
        g1 = ch(a, sync=False)
        ch.set_frame_index(g1.shape[0] + 1)
        g2 = ch(b, sync=False)
        assert not s.query()
        ch.sync()
        assert torch.equal(g1, w1) and torch.equal(g2, w2)


def test_slab_scratch_regrown_behind_queued_calls(torch, busy):
    """A channel-major handle that goes by slabs: async calls of growing length, so the slab scratch is freed and
    allocated again while earlier calls that use it are still queued."""
    case = CASES[2]
    M, P, D, fmt, bw, cm, kernel = case
    frames = [70, 300, 1500, 9000, 40000, 150000, 100]
    lens = [f * D + 3 for f in frames]
    with make_handle(case) as ref, make_handle(case) as ch:
        iq = device_input(sum(lens), fmt, bw, 80)
        want = ref(iq)
        assert ref.last_kernel.startswith(kernel) and ref.last_launch.by_slabs == 1
        cuts = np.concatenate([[0], np.cumsum(lens)])
        bufs = [iq[a:b].clone() for a, b in zip(cuts[:-1], cuts[1:])]
        s = torch.cuda.Stream()
        torch.cuda.synchronize()
        ch.set_stream(s.cuda_stream)
        busy.queue(s)
        outs, slabs = [], []
        for x in bufs:
            outs.append(ch(x, sync=False))
            slabs.append(int(ch.last_launch.slab_frames))
        ch.sync()
        assert all(ch_slab > 0 for ch_slab in slabs) and slabs[:6] == sorted(slabs[:6]) and len(set(slabs)) >= 5, slabs
        assert torch.equal(join(torch, outs, cm), want)


@pytest.mark.parametrize("case", [CASES[0], CASES[2], CASES[4]], ids=[IDS[0], IDS[2], IDS[4]])
def test_profiled_async_launches(torch, busy, case):
    """PFB_OPT_PROFILE: one positive finite time per launch, in order, same outputs.  The order is read off the sizes:
    the third launch is 2^20 frames among launches of 300 at the most, 3500 times the work of any other (at least
    0.75 GB of memory traffic, hundreds of microseconds, against a few microseconds), so its time must be the largest by far if the times come back in
    launch order; nothing is asserted about times of comparable launches."""
    M, P, D, fmt, bw, cm, kernel = case
    frames = [100, 300, 1 << 20, 200, 0, 300]
    lens = [f * D for f in frames]
    with make_handle(case) as ref, make_handle(case) as ch:
        iq = device_input(sum(lens), fmt, bw, 81)
        want = ref(iq)
        cuts = np.concatenate([[0], np.cumsum(lens)])
        bufs = [iq[a:b].clone() for a, b in zip(cuts[:-1], cuts[1:])]
        s = torch.cuda.Stream()
        torch.cuda.synchronize()
        ch.set_stream(s.cuda_stream)
        ch.set_option(L.PFB_OPT_PROFILE, 1)
        busy.queue(s, copies=2)
        outs = [ch(x, sync=False) for x in bufs]
        times = ch.kernel_times_ms()
        launches = sum(f > 0 for f in frames)
        assert len(times) == launches and all(math.isfinite(t) and t > 0 for t in times), times
        assert int(np.argmax(times)) == 2, times
        assert ch.kernel_times_ms() == []
        ch.set_option(L.PFB_OPT_PROFILE, 0)
        assert torch.equal(join(torch, outs, cm), want)


# -- STFT ---------------------------------------------------------------------------------------------------------

def stft_cuts(rng, n, Lw, H):
    cuts = {0, 1, min(n, Lw // 3), min(n, Lw), min(n, Lw + 2 * H), n}   # as tests/test_gpu_stft.py cuts its streams
    cuts |= set(rng.integers(0, n + 1, size=40).tolist())
    return sorted(cuts)


@pytest.mark.parametrize("switch", [False, True], ids=["one-stream", "stream-switch"])
@pytest.mark.parametrize("nfft,Lw,H,fmt,kernel", [(768, 768, 192, "int16", "pfb_stft_fused<N768,"),
                                                  (700, 700, 350, "cf32", "pfb_stft_generic")])
def test_stft_back_to_back_async_calls(torch, busy, nfft, Lw, H, fmt, kernel, switch):
    rng = np.random.default_rng(nfft + H)
    n = 60 * Lw + 37
    if fmt == "cf32":
        raw = rng.standard_normal(2 * n).astype(np.float32)
    else:
        raw = rng.integers(-2048, 2048, size=2 * n).astype(np.int16)
    x = torch.from_numpy(raw).cuda()
    w = np.hamming(Lw)
    kw = dict(hop=H, fft_length=nfft, sample_format=fmt, bit_width=12, output="complex")
    with Stft(w, **kw) as ref, Stft(w, **kw) as st:
        want = ref(x)
        assert ref.last_kernel.startswith(kernel), ref.last_kernel
        edges = [0] + stft_cuts(rng, n, Lw, H) + [n]
        bufs = [x[2 * a:2 * b].clone() for a, b in zip(edges[:-1], edges[1:])]
        assert len(bufs) >= 40
        s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
        torch.cuda.synchronize()
        st.set_stream(s1.cuda_stream)
        busy.queue(s1)
        outs, last = [], s1
        for i, b in enumerate(bufs):
            if switch and i == len(bufs) // 3:
                st.set_stream(s2.cuda_stream)
                last = s2
            if switch and i == 2 * len(bufs) // 3:
                st.set_stream(s1.cuda_stream)
                last = s1
            outs.append(st(b, sync=False))
        assert not last.query(), "the device caught up: the calls were not issued ahead of it"
        st.sync()
        torch.cuda.synchronize()
        assert st.last_kernel.startswith(kernel)
        got = torch.cat([o for o in outs if o.numel()])
        assert got.shape == want.shape and torch.equal(got, want)


# -- PDW ----------------------------------------------------------------------------------------------------------

def test_pdw_extraction_on_a_busy_stream(torch, busy):
    """extract_pdws / extract_pdws_raw on a device tensor while a non-default stream is current and still busy with the
    kernel that wrote the tensor: the PDWs of the same data extracted after a full synchronise."""
    y_src = torch.from_numpy(synthetic_matrix(F=40000, M=64, seed=11)).cuda()
    iq_src = synth.pulsed_iq_torch(1 << 22, 12, device="cuda")
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        busy.queue(s)
        y = y_src * 1.0   # written on s, behind the copies
        assert not s.query()
        got, nf = extract_pdws(y, 16e6, 2.4e9, 3.0, return_noise_floor=True)
        busy.queue(s)
        iq = iq_src + 0
        assert not s.query()
        got_raw, nf_raw = extract_pdws_raw(iq, 56e6, 915e6, 0.0, snr_threshold_db=12.0, return_noise_floor=True)
    torch.cuda.synchronize()
    assert torch.equal(y, y_src) and torch.equal(iq, iq_src)
    want, want_nf = extract_pdws(y, 16e6, 2.4e9, 3.0, return_noise_floor=True)
    want_raw, want_nf_raw = extract_pdws_raw(iq, 56e6, 915e6, 0.0, snr_threshold_db=12.0, return_noise_floor=True)
    assert len(want) > 5 and got.tobytes() == want.tobytes() and np.array_equal(nf, want_nf)
    assert len(want_raw) > 5 and got_raw.tobytes() == want_raw.tobytes() and nf_raw == want_nf_raw
