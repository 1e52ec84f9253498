"""float64 numpy restatement of the matched-filter bank (pfb_mfbank_* in include/pfb_channelizer.h), built on mf_ref,
and the checks of its tests.  Imported by basename like mf_ref.

    q_h    = (first_bin + h) * bin_step                    h = 0 .. H-1
    y_h[m] = g * sum_{n=0}^{K-1} conj(r[n]) * exp(-2j pi q_h n / nfft) * x[m+n]
    p_h[m] = |y_h[m]|^2

Hypothesis h is mf_ref.compress with the replica r[n] exp(+2j pi q_h n / nfft).  The allowance is the matched filter's
own, e = mf_ref.tolerance = 1e-5 g ||r|| max ||x window||: the modulation does not change ||r||, and the device runs each
hypothesis through the same forward, multiply and inverse chain.  A power p against |ref|^2 is allowed e (2 |ref| + e),
as mf_ref.worst_ratio allows it.
"""
import numpy as np

import mf_ref as R

WORST = {"ratio": 0.0, "of_bound": 0.0, "where": ""}


def reset_worst():
    WORST.update(ratio=0.0, of_bound=0.0, where="")


def bins(first_bin, H, bin_step):
    return (first_bin + np.arange(H, dtype=np.int64)) * bin_step


def modulated(r, q, nfft):
    r = np.asarray(r, np.complex128)
    return r * np.exp(2j * np.pi * float(q) * np.arange(r.size) / nfft)


def surface(x, r, first_bin, H, bin_step, nfft, normalize=False):
    """y_h[m] as an (H, outputs) complex128 array"""
    g = R.gain(r, normalize)   # of the plain replica; the modulated one has the same energy
    rows = [g * R.compress(x, modulated(r, q, nfft)) for q in bins(first_bin, H, bin_step)]
    return np.stack(rows) if rows[0].size else np.zeros((H, 0), np.complex128)


def surface_loop(x, r, first_bin, H, bin_step, nfft, normalize=False):
    """the definition, literally"""
    x, r = np.asarray(x, np.complex128), np.asarray(r, np.complex128)
    K, N = r.size, x.size
    y = np.zeros((H, max(0, N - K + 1)), np.complex128)
    for h in range(H):
        q = (first_bin + h) * bin_step
        for m in range(y.shape[1]):
            acc = 0j
            for n in range(K):
                acc += np.conj(r[n]) * np.exp(-2j * np.pi * q * n / nfft) * x[m + n]
            y[h, m] = acc
    return R.gain(r, normalize) * y


def best(p):
    """The selection rule of PFB_MFBANK_BEST on an (H, outputs) array of powers: start from h = 0, replace only on a
    strictly greater power (ties keep the lowest h, a NaN displaces nothing).  Returns (power, hypothesis)."""
    p = np.asarray(p)
    bp, bh = p[0].copy(), np.zeros(p.shape[1], np.int32)
    for h in range(1, p.shape[0]):
        with np.errstate(invalid="ignore"):
            m = p[h] > bp
        bp[m], bh[m] = p[h][m], h
    return bp, bh


def frequencies(fs, first_bin, H, bin_step, nfft):
    return bins(first_bin, H, bin_step).astype(np.float64) * fs / nfft


def _record(ratio, where):
    if ratio > WORST["ratio"]:
        WORST.update(ratio=ratio, of_bound=ratio * R.TOL, where=str(where))


def check_surface(p, yref, e, where, keep=None):
    """every p[h, m] against |yref[h, m]|^2 as mf_ref.worst_ratio compares power; keep: a boolean mask over m of the
    outputs that are checked (the rest may be spoiled by a sample that is not finite)"""
    p = np.asarray(p)
    assert p.shape == yref.shape and p.dtype == np.float32, (where, p.shape, yref.shape, p.dtype)
    if keep is not None:
        p, yref = p[:, keep], yref[:, keep]
    if p.size == 0:
        return
    ratio, _ = R.worst_ratio(p.reshape(-1), yref.reshape(-1), e, "power")
    _record(ratio, where)
    assert ratio <= 1.0, (where, ratio)


def check_best(power, hyp, yref, e, where, keep=None):
    """With h* the device's choice at output m and a(v) = e (2 |v| + e) the power allowance at a reference value v:
      1  0 <= h* < H, and the device's power is within a(yref[h*, m]) of |yref[h*, m]|^2;
      2  |yref[h*, m]|^2 is within a(yref[h*, m]) of max_h |yref[h, m]|^2;
      3  where the reference's largest power stands more than 2 a(its value) over every other hypothesis (the most two
         rounded powers can move towards each other), h* is the reference's."""
    power, hyp = np.asarray(power), np.asarray(hyp)
    H, F = yref.shape
    assert power.shape == hyp.shape == (F,) and power.dtype == np.float32 and hyp.dtype == np.int32, \
        (where, power.shape, hyp.shape, F, power.dtype, hyp.dtype)
    if keep is not None:
        power, hyp, yref = power[keep], hyp[keep], yref[:, keep]
        F = power.size
    if F == 0:
        return
    assert hyp.min() >= 0 and hyp.max() < H, (where, hyp.min(), hyp.max())
    cols = np.arange(F)
    pref = np.abs(yref) ** 2
    chosen, mag = pref[hyp, cols], np.abs(yref[hyp, cols])
    if e == 0.0:
        assert not power.any(), where
        return
    allow = e * (2 * mag + e)
    r1 = np.abs(power.astype(np.float64) - chosen) / allow
    top = pref.max(axis=0)
    r2 = (top - chosen) / allow
    ratio = float(max(r1.max(), r2.max()))
    _record(ratio, where)
    assert r1.max() <= 1.0, (where, "power", float(r1.max()), int(np.argmax(r1)))
    assert r2.max() <= 1.0, (where, "choice", float(r2.max()), int(np.argmax(r2)))
    if H > 1:
        want = np.argmax(pref, axis=0)
        second = np.partition(pref, H - 2, axis=0)[H - 2]
        clear = top - second > 2 * e * (2 * np.sqrt(top) + e)
        assert np.array_equal(hyp[clear], want[clear]), (where, "hypothesis", int(np.flatnonzero(hyp[clear] != want[clear])[0]))
