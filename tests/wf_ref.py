"""The waterfall contract (pfb_wf_* in include/pfb_channelizer.h) restated in numpy: float64 power, max / min / first
argmax over each bin of rows, sum / count, and one rounding to float32.  Imported by basename like trace_ref."""
import numpy as np

CELL_DTYPE = np.dtype([("power_max", "<f4"), ("power_mean", "<f4"), ("power_min", "<f4"), ("peak_row", "<u4")])
ELEMENTS = ("complex", "magnitude", "power")
NP_DTYPE = {"complex": np.complex64, "magnitude": np.float32, "power": np.float32}


def powers(x, element):
    """float64 power of every element of a complex64 / float32 array"""
    x = np.asarray(x)
    if element == "complex":
        re, im = x.real.astype(np.float64), x.imag.astype(np.float64)
        return re * re + im * im
    a = x.astype(np.float64)
    return a * a if element == "magnitude" else a


def cells_of(p, B, partial=True):
    """(bins, W) cells of a (rows, W) float64 power matrix whose first row starts a bin; the final partial bin is
    included unless partial=False"""
    p = np.asarray(p, dtype=np.float64)
    rows, W = p.shape
    nb = rows // B + (1 if partial and rows % B else 0)
    out = np.zeros((nb, W), CELL_DTYPE)
    for b in range(nb):
        blk = p[b * B:(b + 1) * B]
        out["power_max"][b] = blk.max(axis=0).astype(np.float32)
        out["power_min"][b] = blk.min(axis=0).astype(np.float32)
        out["power_mean"][b] = (blk.sum(axis=0) / float(blk.shape[0])).astype(np.float32)
        out["peak_row"][b] = blk.argmax(axis=0)      # numpy's argmax is the first of equal values
    return out


def waterfall(x, element, B, partial=True):
    return cells_of(powers(x, element), B, partial)


def random_matrix(element, rows, W, seed):
    """finite values with normal float32 powers"""
    rng = np.random.default_rng(seed)
    if element == "complex":
        return (rng.standard_normal((rows, W)) + 1j * rng.standard_normal((rows, W))).astype(np.complex64)
    a = np.abs(rng.standard_normal((rows, W))).astype(np.float32) + np.float32(0.01)
    return a


def ulps32(a, b):
    """distance in float32 steps between finite values of one sign"""
    a = np.ascontiguousarray(a, dtype=np.float32).view(np.int32).astype(np.int64)
    b = np.ascontiguousarray(b, dtype=np.float32).view(np.int32).astype(np.int64)
    return np.abs(a - b)


def same_selections(got, want):
    return all(np.array_equal(got[k].view(np.uint32), want[k].view(np.uint32))
               for k in ("power_max", "power_min", "peak_row"))


def check_cells(got, want, where=""):
    """The pass condition: power_max, power_min and peak_row bit for bit, power_mean within 1 float32 ulp.  A double sum
    of at most 2^24 non-negative terms in any order is within 2^-29 relative of the exact sum, 1/32 of a float32 ulp,
    so two roundings of such sums differ only across a rounding boundary: by one step."""
    assert got.shape == want.shape, (where, got.shape, want.shape)
    for k in ("power_max", "power_min", "peak_row"):
        bad = np.argwhere(got[k].view(np.uint32) != want[k].view(np.uint32))
        assert bad.size == 0, (where, k, bad[:5].tolist(), got[k][tuple(bad[0])], want[k][tuple(bad[0])])
    d = ulps32(got["power_mean"], want["power_mean"])
    assert d.size == 0 or d.max() <= 1, (where, "power_mean", int(d.max()), np.argwhere(d > 1)[:5].tolist())
