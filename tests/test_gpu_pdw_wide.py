"""The channelized PDW extractor (pfb_pdw_extract) on wide banks -- M = 128, 130, 256, 560, 1024: two to sixteen column
groups of 64, all full or a full one followed by a partial one -- against the float64 oracle.  Everything that depends
on the column-group index runs here and nowhere else in the suite: col = blockIdx.x * 64 + lane for blockIdx.x >= 2 in
the sample gather, the bracket pass, the digit histograms, the collect and the mask kernels, the grids sized by
8192 / cgroups, the parts per channel of the candidate select, pdw_pick_kernel's (M + 3) / 4 workgroups, the scan
kernel on either side of `M >= 32 && ntiles < 2048`, and the M-column tile kernels at tile_words = 16.

  F  short and wide: pdw_cases.edges_chan(M), F = 3109 -- the full-select route (noise-floor path 2), the oracle run on
     the matrix itself
  G  long and wide: pdw_cases.wide_base(F), an (F, 9) base expanded on the device to M columns (column j = base column
     j mod 9) -- the sampled-bracket route (path 1; path 3 on the tied background).  The oracle runs on the base, once
     per base, and pdw_cases.widen_expected maps its answer to the wide matrix; tests/test_pdw_cases_cpu.py proves that
     rule, and the designs, with the oracle alone.

Tolerances are the ones pdw_checks.py holds (compare, check_case), unchanged and without phase_col."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import pdw_cases as pc  # noqa: E402
from pdw_checks import check_case, compare  # noqa: E402
from sdr_channelizer_amd import _lib as L  # noqa: E402
from sdr_channelizer_amd.pdw import extract_pdws  # noqa: E402

_WANT = {}   # the oracle's answer per case, computed once and shared by every M (and by host and device input)


def oracle_of(oracle, case):
    if case.name not in _WANT:
        _WANT[case.name] = pc.run_oracle(oracle, case)
    return _WANT[case.name]


# ---- F: short and wide -----------------------------------------------------------------------------------------------

def run_short(case, data, **kw):
    a = case.args
    out = extract_pdws(data, a["fs_in"], a["fc"], a["t0"], snr_threshold_db=a["snr_db"], matlab_quirks=a["matlab_quirks"],
                       return_noise_floor=True, **kw)
    assert L.load().pfb_pdw_last_noise_floor_path() == 2
    return out


@pytest.mark.parametrize("where", ["host", "device"])
@pytest.mark.parametrize("M", pc.WIDE_M)
def test_short_wide_edges_staggered_over_columns(oracle, M, where):
    import torch
    case = pc.edges_chan(M)
    got, nf = run_short(case, torch.from_numpy(case.data).cuda() if where == "device" else case.data)
    check_case(case, got, nf, *oracle_of(oracle, case))


def test_short_wide_channel_major_gives_the_same_bytes(oracle):
    """PFB_PDW_CHANNEL_MAJOR at M = 560: nine column groups through the transpose, the same PDWs and floors to the bit"""
    import torch
    case = pc.edges_chan(560)
    y = torch.from_numpy(case.data).cuda()
    got, nf = run_short(case, y)
    check_case(case, got, nf, *oracle_of(oracle, case))
    got_cm, nf_cm = run_short(case, y.T.contiguous(), channel_major=True)
    assert got_cm.tobytes() == got.tobytes() and nf_cm.tobytes() == nf.tobytes()


# ---- G: long and wide ------------------------------------------------------------------------------------------------

def check_wide(oracle, base, M, path):
    import torch
    F, M0 = base.data.shape
    need = F * M * 8
    if torch.cuda.mem_get_info()[0] < need * 1.5:
        pytest.skip(f"needs {need >> 20} MiB of HBM")
    want_base, nf_base = oracle_of(oracle, base)
    a = base.args
    want = pc.widen_expected(oracle, want_base, M, M0, a["fs_in"])
    pulses = pc.widen_pulses(base.pulses, M, M0)
    assert len(want) == len(pulses)
    lib = L.load()
    try:
        y = torch.from_numpy(base.data).cuda().repeat(1, -(-M // M0))[:, :M].contiguous()
        assert y.shape == (F, M)
        got, nf = extract_pdws(y, a["fs_in"], a["fc"], a["t0"], decimation=M0, snr_threshold_db=a["snr_db"],
                               matlab_quirks=a["matlab_quirks"], capacity=len(pulses) + 64, return_noise_floor=True)
        del y
        assert lib.pfb_pdw_last_noise_floor_path() == path
        assert np.allclose(nf, nf_base[np.arange(M) % M0], rtol=1e-12, atol=0)
        assert len(got) == len(pulses)
        compare(got, want, base.fs)
        assert pc.triples(got, base.fs) == pulses
    finally:
        lib.pfb_pdw_release_workspace(-1)
        torch.cuda.empty_cache()


@pytest.mark.parametrize("quirks", [True, False])
@pytest.mark.parametrize("M", pc.WIDE_M)
def test_long_wide_sampled_bracket(oracle, M, quirks):
    """F = 8 * 65536 + 300: the smallest sampled-route length with a ragged last word; 1025 tiles of 8 words,
    pdw_tilescan_kernel<64>"""
    check_wide(oracle, pc.wide_base(pc.WIDE_F1, quirks=quirks), M, path=1)


def test_long_wide_tied_background_takes_the_full_select(oracle):
    """a background on a grid of 1 / 200 at M = 130: the bracket's count check fails, the digit histograms, the pick and
    the collect run over three column groups (the last with two live lanes) on the long stream"""
    check_wide(oracle, pc.wide_base(pc.WIDE_F1, tied=True, quirks=False), 130, path=3)


@pytest.mark.parametrize("F", pc.WIDE_FS[1:])
def test_wide_around_2_20_frames(oracle, F):
    """M = 128 on either side of the scan kernels' switch (2047 tiles: one wave per column, 32 tiles per thread; 2048:
    1024 threads per column) and at the first length with 16-word tiles, where the candidate select takes two parts per
    channel (tests/test_pdw_cases_cpu.py::test_routes_of_the_wide_lengths asserts which case takes which)"""
    try:
        check_wide(oracle, pc.wide_base(F), 128, path=1)
    finally:
        _WANT.pop(pc.wide_base(F).name, None)
        pc._wide_data.cache_clear()
