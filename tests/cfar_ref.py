"""The CFAR detector restated in numpy from the header text (include/pfb_channelizer.h, the pfb_cfar section), not from
the device code: tree sums by repeated pairwise adds in float32, a float64 sequential walk over the training blocks,
one float32 multiply, runs by a plain scan.  ``detect`` takes a cell count and a "flushed" flag and returns what has
closed by then."""
import numpy as np

DET = np.dtype([("first_index", "u8"), ("last_index", "u8"), ("peak_index", "u8"), ("peak_power", "f4"), ("noise", "f4"),
                ("hypothesis", "i4"), ("cells_over", "u4"), ("flags", "u4"), ("reserved", "u4")])
CELL = np.dtype([("power", "f4"), ("hypothesis", "i4")])
CA, GO, SO = 0, 1, 2
ONE_SIDED = 1


def block_sums(p, C):
    """S[b] of the complete blocks of p: the balanced binary tree, every node one float32 addition."""
    nb = len(p) // C
    x = np.asarray(p[: nb * C], np.float32).reshape(nb, C)
    with np.errstate(all="ignore"):
        while x.shape[1] > 1:
            x = x[:, 0::2] + x[:, 1::2]
    return x[:, 0] if nb else np.zeros(0, np.float32)


def block_noise(S, nblocks, C, G, T, method):
    """(noise float32, trained-on count) of blocks 0 .. nblocks-1 given the sums of the complete blocks; NaN where a
    block has no noise.  The walk over the training blocks is sequential in ascending index, in float64."""
    nbc = len(S)
    b = np.arange(nblocks)
    S64 = np.concatenate([S.astype(np.float64), [0.0]])  # [nbc]: a slot for "not there"
    sums, counts = [], []
    with np.errstate(all="ignore"):
        for first in (b - G - T, b + G + 1):
            s, n = np.zeros(nblocks), np.zeros(nblocks, np.int64)
            for t in range(T):
                j = first + t
                ok = (j >= 0) & (j < nbc)
                s = s + np.where(ok, S64[np.where(ok, j, nbc)], 0.0)  # + 0.0 leaves a float64 as it is
                n += ok
            sums.append(s)
            counts.append(n)
        (sl, sr), (nl, nr) = sums, counts
        nan = np.full(nblocks, np.nan)
        if method == CA:
            m = np.where(nl + nr > 0, (sl + sr) / ((nl + nr) * float(C)), nan)
        else:
            a, c = sl / (nl * float(C)), sr / (nr * float(C))
            both = np.maximum(a, c) if method == GO else np.minimum(a, c)  # NaN on either side gives NaN
            m = np.where((nl > 0) & (nr > 0), both, np.where(nl > 0, a, np.where(nr > 0, c, nan)))
        return m.astype(np.float32), nl + nr


def decide(p, n, flushed, C, G, T, method, alpha, min_power):
    """(over[0 .. decided), noise per block, trained-on count per block) for the first n cells of p."""
    p = np.asarray(p[:n], np.float32)
    nbc = n // C
    nblocks = -(-n // C) if flushed else max(0, nbc - G - T)
    decided = n if flushed else nblocks * C
    noise, trained = block_noise(block_sums(p, C), nblocks, C, G, T, method)
    with np.errstate(all="ignore"):
        thr = np.float32(alpha) * noise  # one float32 multiply
        cells = p[:decided]
        over = (cells > np.repeat(thr, C)[:decided]) & (cells > np.float32(min_power))
    return over, noise, trained


def detect(p, n, flushed, C, G, T, method=CA, alpha=1.0, min_power=0.0, merge_gap=0, hyp=None):
    """(records closed by cell count n, stats) -- flushed: pfb_cfar_flush came after the n cells."""
    over, noise, trained = decide(p, n, flushed, C, G, T, method, alpha, min_power)
    p = np.asarray(p, np.float32)
    decided = len(over)
    idx = np.flatnonzero(over)
    runs, cur = [], []
    for i in idx:  # the plain scan: a gap of more than merge_gap cells of not-over starts the next run
        if cur and i - cur[-1] - 1 > merge_gap:
            runs.append(cur)
            cur = []
        cur.append(int(i))
    open_run = 0
    if cur:
        if flushed or decided - 1 - cur[-1] >= merge_gap + 1:
            runs.append(cur)
        else:
            open_run = 1
    out = np.zeros(len(runs), DET)
    for k, r in enumerate(runs):
        pk = r[int(np.argmax(p[r]))]  # the first of equal maxima: the lowest index
        blk = pk // C
        out[k] = (r[0], r[-1], pk, p[pk], noise[blk], -1 if hyp is None else int(hyp[pk]), min(len(r), 2 ** 32 - 1),
                  ONE_SIDED if trained[blk] < 2 * T else 0, 0)
    without = int(sum(min(C, n - b * C) for b in np.flatnonzero(trained == 0)))
    stats = {"cells_in": n, "cells_decided": decided, "cells_over": int(over.sum()), "cells_without_noise": without,
             "detections": len(runs), "dropped": 0, "open_run": open_run}
    return out, stats


def alpha_ca(pfa, N):
    return N * (pfa ** (-1.0 / N) - 1.0)
