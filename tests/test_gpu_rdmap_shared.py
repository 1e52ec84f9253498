"""The two range-Doppler detectors run on one core (pfb_rdmap.hpp): four handles of both units in one process, their
calls interleaved, keep their state apart.  Every handle's records and stats are its restatement's on the whole input,
byte for byte, whatever the others did in between."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import oscfar_ref as O  # noqa: E402
import rdcfar_ref as R  # noqa: E402
from gpu_support import cuda_torch  # noqa: E402
from rdmap_support import place  # noqa: E402
from sdr_channelizer_amd import OsCfar, RangeDopplerCfar  # noqa: E402
from sdr_channelizer_amd.rd_cfar import records  # noqa: E402

N_MAPS, ND, RG = 5, 3, 300            # two gate tiles, the second partial; ND below the band height
WD, GR, TR, PD, ALPHA = 1, 2, 8, 1, 8.0
RANK = 36                             # of N = 2 Tr (2 Wd + 1) = 48


def scene():
    rng = np.random.default_rng(11)
    maps = rng.exponential(size=(N_MAPS, ND, RG)).astype(np.float32)
    maps.reshape(-1)[rng.choice(maps.size, 40, replace=False)] *= 200
    return maps


def test_four_handles_of_two_units_keep_their_state_apart():
    torch = cuda_torch()
    maps = scene()
    want = {"ca": R.detect(maps, WD, GR, TR, PD, R.CA, ALPHA), "go": R.detect(maps, WD, GR, TR, PD, R.GO, ALPHA),
            "os": O.detect(maps, WD, GR, TR, PD, RANK, ALPHA)}
    assert [len(want[k][0]) for k in ("ca", "go", "os")] == [35, 33, 35]
    for rec, _ in want.values():
        assert set(rec["map"].tolist()) == set(range(N_MAPS)) and int((rec["gate"] >= 256).sum()) == 4
    x = place(torch, maps)
    got = {k: [] for k in ("ca", "go", "os", "os_host")}
    with RangeDopplerCfar(ND, RG, WD, GR, TR, ALPHA, peak_half_width=PD, method="ca") as ca, \
            RangeDopplerCfar(ND, RG, WD, GR, TR, ALPHA, peak_half_width=PD, method="go") as go, \
            OsCfar(ND, RG, WD, GR, TR, RANK, ALPHA, peak_half_width=PD) as os_dev, \
            OsCfar(ND, RG, WD, GR, TR, RANK, ALPHA, peak_half_width=PD) as os_host:
        # the first cut: device tensors for the first handle of each unit, numpy for the second
        got["ca"].append(records(ca.process(x[:2])))
        got["os_host"].append(records(os_host.process(maps[:2])))
        got["os"].append(records(os_dev.process(x[:2])))
        got["go"].append(records(go.process(maps[:2])))
        # one handle starts over while the others go on
        os_host.reset()
        got["os_host"] = [records(os_host.process(maps[:2]))]
        got["go"].append(records(go.process(maps[2:])))
        got["os"].append(records(os_dev.process(x[2:])))
        got["os_host"].append(records(os_host.process(maps[2:])))
        got["ca"].append(records(ca.process(x[2:])))
        for name, det in (("ca", ca), ("go", go), ("os", os_dev), ("os_host", os_host)):
            rec, stats = want[name[:2]]
            assert np.concatenate(got[name]).tobytes() == rec.tobytes(), name
            assert det.stats == stats and det.next_map == N_MAPS, name
