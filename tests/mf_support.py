"""What the matched filter's GPU modules share: the check against the float64 restatement (mf_ref) with the record of
the largest error a module saw, samples placed on or off a 16-byte boundary, and a caller's output buffer with guard
elements around it.  Imported by basename like mf_ref."""
import numpy as np

import mf_ref as R

WORST = {"ratio": 0.0, "of_bound": 0.0, "where": ""}


def reset_worst():
    """a module's `torch` fixture starts its own record"""
    WORST.update(ratio=0.0, of_bound=0.0, where="")


def check(y, ref, x, r, normalize, output, where):
    y = np.asarray(y)
    assert y.shape == ref.shape, (where, y.shape, ref.shape)
    assert y.dtype == (np.complex64 if output == "complex" else np.float32)
    if y.size == 0:
        return
    ratio, of_bound = R.worst_ratio(y, ref, R.tolerance(x, r, normalize), output)
    if ratio > WORST["ratio"]:
        WORST.update(ratio=ratio, of_bound=of_bound, where=str(where))
    assert ratio <= 1.0, (where, ratio, of_bound)


def on_device(torch, raw, misalign):
    """the raw samples in device memory, 16-byte aligned or one sample past a 16-byte boundary"""
    if not misalign:
        return torch.from_numpy(raw).cuda()
    buf = torch.empty(raw.size + 2, dtype=torch.from_numpy(raw[:0]).dtype, device="cuda")
    assert buf.data_ptr() % 16 == 0
    view = buf[2:]
    view.copy_(torch.from_numpy(raw))
    return view


GUARD = 5   # output elements on either side: 40 or 20 bytes, so the guarded output starts off a 16-byte boundary


def run_guarded(torch, mf, d_in, outputs, output, misalign):
    """process into a caller's buffer with guard elements around it that must survive"""
    dt = torch.complex64 if output == "complex" else torch.float32
    lead = GUARD if misalign else GUARD + 3   # 8 elements: a multiple of 16 bytes for both kinds
    buf = torch.full((lead + outputs + GUARD,), -77.0, dtype=dt, device="cuda")
    out = buf[lead: lead + outputs]
    got = mf.process(d_in, out=out)
    assert got.numel() == outputs and (outputs == 0 or got.data_ptr() == out.data_ptr())
    host = buf.cpu().numpy()
    assert np.all(host[:lead] == -77.0) and np.all(host[lead + outputs:] == -77.0)
    return host[lead: lead + outputs]
