"""What the trace / envelope GPU modules share: the comparison of records with the numpy restatement (trace_ref), the
random device streams made once per format, a caller's output buffers with guard bytes or guard floats around them,
and the record of the largest cf32 mean error a module saw.  Imported by basename like trace_ref."""
import numpy as np

import trace_ref as R
from sdr_channelizer_amd import trace

RECORD = R.BIN_DTYPE.itemsize


def same(got, want, fmt):
    got, want = trace.as_records(got), np.asarray(want)
    if got.shape != want.shape:
        return False
    return R.mean_close(got, want) if fmt == "cf32" else np.array_equal(got.view(np.uint8), want.view(np.uint8))


_streams = {}


def stream(torch, fmt, bw, n=8 * 100003 + 4):
    """One random stream per format and length, on the host and on the device; made once, never written."""
    if (fmt, bw, n) not in _streams:
        iq = R.random_iq(fmt, bw, n, seed=bw + len(fmt))
        iq[5000:5040] = iq[5000]   # a run of equal powers
        _streams[fmt, bw, n] = (iq, torch.from_numpy(iq).cuda())
    return _streams[fmt, bw, n]


MEAN = {}   # label -> the largest |power_mean - reference| / (count * 2^-52 * reference) of the cf32 records seen


def note_mean(label, got, want):
    """Keep the largest cf32 mean error under `label`, as a fraction of mean_close's allowance (asserts nothing)."""
    got, want = trace.as_records(got), np.asarray(want)
    ok = want["power_mean"] > 0
    if got.shape != want.shape or not ok.any():
        return
    frac = np.abs(got["power_mean"][ok] - want["power_mean"][ok]) / (want["count"][ok] * 2.0 ** -52 * want["power_mean"][ok])
    MEAN[label] = max(MEAN.get(label, 0.0), float(frac.max()))


class Slots:
    """One uint8 device tensor cut into a slot per call: a record of guard bytes, room for counts[k] records, a record
    of guard bytes, all 0xA5 before the calls."""

    def __init__(self, torch, counts):
        self.counts = [int(c) for c in counts]
        self.at = np.concatenate([[0], np.cumsum([(c + 2) * RECORD for c in self.counts])]).astype(np.int64)
        self.buf = torch.full((int(self.at[-1]),), 0xA5, dtype=torch.uint8, device="cuda")

    def out(self, k):
        lo = int(self.at[k]) + RECORD
        return self.buf[lo:lo + self.counts[k] * RECORD]

    def records(self):
        """every slot's records, after the guards on both sides of each were found untouched"""
        host = self.buf.cpu().numpy()
        got = []
        for k, c in enumerate(self.counts):
            lo, hi = int(self.at[k]), int(self.at[k + 1])
            assert np.all(host[lo:lo + RECORD] == 0xA5) and np.all(host[hi - RECORD:hi] == 0xA5), k
            got.append(host[lo + RECORD:hi - RECORD].copy().view(R.BIN_DTYPE))
        return got


class GuardedFloats:
    """n float32 outputs inside a buffer of 7.0s, from a 16-byte boundary (lead 4) or one float past it (lead 5)."""

    def __init__(self, torch, n, lead):
        self.n, self.lead = n, lead
        self.buf = torch.full((n + 12,), 7.0, dtype=torch.float32, device="cuda")
        assert self.buf.data_ptr() % 16 == 0

    def ptr(self):
        return self.buf.data_ptr() + 4 * self.lead

    def values(self):
        host = self.buf.cpu().numpy()
        assert np.all(host[:self.lead] == 7.0) and np.all(host[self.lead + self.n:] == 7.0)
        return host[self.lead:self.lead + self.n]
