"""The STFT, the matched filter and its bank share one input loader, and the two filters one overlap-save core: the
units include the shared headers and keep no copy of what the headers hold."""
import glob
import os
import re

import pytest

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "sdr_channelizer_amd", "csrc")
UNITS = ("pfb_stft.hip", "pfb_mf.hip", "pfb_mfbank.hip")


def source(name):
    return open(os.path.join(CSRC, name)).read()


@pytest.mark.parametrize("unit", UNITS)
def test_the_unit_loads_its_input_through_the_span_header(unit):
    src = source(unit)
    includes = re.findall(r'^#include "([^"]+)"', src, re.M)
    assert "pfb_iq_span.hpp" in includes
    assert ("pfb_ols.hpp" in includes) == (unit != "pfb_stft.hip")    # the STFT's passes are multi-frame: its own
    assert "iq_load_span<FMT, " in src
    # no fetch or load function of its own: a name followed by its parameter list and a body's opening brace
    own = re.findall(r"^[^\n;=]*\b(\w+_fetch|\w+_load_\w+)\s*\([^;{]*\)\s*\{", src, re.M)
    assert own == [], own


def test_the_shared_headers_hold_what_the_units_call():
    span, core = source("pfb_iq_span.hpp"), source("pfb_ols.hpp")
    for name in ("iq_fetch", "iq_load_span"):
        assert re.search(r"^PFB_DEV \w+ %s\(" % name, span, re.M), name
    for name in ("ols_first_pass", "ols_pass", "ols_power", "ols_store_power"):
        assert re.search(r"^PFB_DEV \w+ %s\(" % name, core, re.M), name
    for unit in ("pfb_mf.hip", "pfb_mfbank.hip"):
        src = source(unit)
        for call in ("ols_first_pass<", "ols_pass<", "ols_store_power("):
            assert call in src, (unit, call)


def test_dft_minus_is_defined_once():
    defs = {}
    for path in sorted(glob.glob(os.path.join(CSRC, "*"))):
        n = len(re.findall(r"^\w[\w:<> ]*\bdft_minus\s*\([^;{]*\)\s*\{", open(path, errors="replace").read(), re.M))
        if n:
            defs[os.path.basename(path)] = n
    assert defs == {"pfb_ols_host.cpp": 1}
    from sdr_channelizer_amd import build
    assert "pfb_ols_host.cpp" in build.SOURCES
