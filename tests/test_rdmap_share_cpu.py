"""The two detectors over range-Doppler maps share one core (pfb_rdmap.hpp): both units include it and keep no copy of
what it holds, and the grow-only buffer and the grid clamp of every detector unit have one definition."""
import glob
import os
import re

import pytest

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "sdr_channelizer_amd", "csrc")
UNITS = ("pfb_rdcfar.hip", "pfb_oscfar.hip")
DEFINITION = r"^[^\n;=]*\b(%s)\s*\([^;{]*\)\s*(?:const\s*)?\{"    # a name, its parameter list and a body's opening brace


def source(name):
    return open(os.path.join(CSRC, name)).read()


def definitions(names, text):
    return re.findall(DEFINITION % names, text, re.M)


@pytest.mark.parametrize("unit", UNITS)
def test_the_unit_keeps_no_copy_of_the_core(unit):
    src = source(unit)
    assert "pfb_rdmap.hpp" in re.findall(r'^#include "([^"]+)"', src, re.M)
    own = definitions(r"block_sum_excl|wrap|grow|grid_for|\w*tile_counts|\w*_scan|\w*_emit|\w*sync_call|\w*enqueue|\w*_step", src)
    assert own == [], own
    assert not re.search(r"\bstruct (DevState|Tiling)\b", src)
    for call in ("sync_call", "async_call", "create_detector"):
        assert len(re.findall(r"return (?:rc != PFB_OK \? rc : )?%s\((?:h|\*cfg), " % call, src)) == 1, (unit, call)
    assert len(re.findall(r"^struct pfb_\w+_handle : MapDetector \{", src, re.M)) == 1


def test_the_core_holds_what_the_units_call():
    core = source("pfb_rdmap.hpp")
    for name in ("block_sum_excl", "wrap", "rdmap_tile_counts", "rdmap_scan", "rdmap_emit", "create_detector", "step",
                 "enqueue", "check_call", "sync_call", "async_call"):
        assert len(definitions(name, core)) == 1, name
    for name in ("DevState", "Tiling", "MapParams", "MapDetector"):
        assert len(re.findall(r"^struct %s \{" % name, core, re.M)) == 1, name
    # internal to each unit: the two are separate code objects whose host stubs must not meet at link time
    assert core.index("namespace {") < core.index("constexpr") and core.rstrip().endswith("}  // namespace")
    users = [os.path.basename(p) for p in sorted(glob.glob(os.path.join(CSRC, "*"))) if '"pfb_rdmap.hpp"' in open(p, errors="replace").read()]
    assert users == sorted(UNITS)


def test_grow_and_grid_for_are_defined_once():
    defs = {}
    for path in sorted(glob.glob(os.path.join(CSRC, "*"))):
        for name in definitions("grow|grid_for", open(path, errors="replace").read()):
            defs.setdefault(name, []).append(os.path.basename(path))
    assert defs == {"grow": ["pfb_host.cpp"], "grid_for": ["pfb_host.cpp"]}
    from sdr_channelizer_amd import build
    assert "pfb_host.cpp" in build.SOURCES and "pfb_rdmap.hpp" in build.HEADERS
    for unit in ("pfb_cfar.hip", "pfb_pd.hip", "pfb_rdmap.hpp"):
        assert "grow(&h->d_stage, &h->stage_bytes, " in source(unit), unit
