"""What the GPU tests of the two range-Doppler detectors (RangeDopplerCfar, OsCfar) share: maps placed on the device
as a pitched view off a 256-byte boundary, and one process_async call with guard words around its outputs.  A support
module, not a test."""
from sdr_channelizer_amd.rd_cfar import records

SENTINEL = 0x5A5A5A5A5A5A5A5A


def place(torch, maps, pitch=0, offset=0):
    """the maps on the device as a view with `pitch` floats from row to row, its first cell `offset` cells off a
    256-byte boundary; what lies between the rows is NaN"""
    n, ND, Rg = maps.shape
    pitch = pitch or Rg
    flat = torch.full((offset + max(n, 1) * ND * pitch + 64,), float("nan"), dtype=torch.float32, device="cuda")
    assert flat.data_ptr() % 256 == 0
    view = flat[offset:].as_strided((n, ND, Rg), (ND * pitch, pitch, 1))
    view.copy_(torch.from_numpy(maps))
    return view


def run_async(torch, det, x, capacity):
    """(records, count) of one process_async call of the detector (pfb_rdcfar_process_async or
    pfb_oscfar_process_async), with guard words around the records and the count"""
    out = torch.full((capacity + 2, 4), SENTINEL, dtype=torch.int64, device="cuda")
    count = torch.full((3,), SENTINEL, dtype=torch.int64, device="cuda")
    det.process_async(x, out[1:capacity + 1], count[1:2])
    det.sync()
    n = int(count[1].item())
    assert int(count[0].item()) == int(count[2].item()) == SENTINEL
    assert (out[0] == SENTINEL).all() and (out[capacity + 1] == SENTINEL).all()
    assert (out[1 + min(n, capacity):] == SENTINEL).all()          # nothing behind the last record
    return records(out[1:1 + min(n, capacity)]), n
