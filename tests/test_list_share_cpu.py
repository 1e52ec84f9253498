"""The three list units (deinterleaver, associator, clusterer) share one core (pfb_list.hpp): each includes it and keeps
no copy of what it holds, and the carving of a scratch block (pfb_host.h), which pfb_mop.hip takes too, has one
definition."""
import glob
import os
import re

import pytest

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "sdr_channelizer_amd", "csrc")
UNITS = ("pfb_deint.hip", "pfb_assoc.hip", "pfb_cluster.hip")
DEFINITION = r"^[^\n;=]*\b(%s)\s*\([^;{]*\)\s*(?:const\s*)?\{"    # a name, its parameter list and a body's opening brace
CORE_FUNCTIONS = ("block_scan", "list_scan", "misaligned", "check_list", "copy_out", "fetch", "hook_until_still", "ensure",
                  "release", "ran", "destroy_list", "set_list_stream", "sync_list", "list_device", "list_stats")


def source(name):
    return open(os.path.join(CSRC, name)).read()


def definitions(names, text):
    return re.findall(DEFINITION % names, text, re.M)


@pytest.mark.parametrize("unit", UNITS + ("pfb_mop.hip",))
def test_the_unit_keeps_no_copy_of_the_core(unit):
    src = source(unit)
    includes = re.findall(r'^#include "([^"]+)"', src, re.M)
    assert ("pfb_list.hpp" in includes) == (unit in UNITS)
    code = re.sub(r"//.*", "", src)
    assert definitions(r"block_scan|round_up|copy_out|copy_control|ensure_scratch|misaligned", src) == []
    assert not re.search(r"\btake\(|\btake =|\bLayout\b|\bkTier\w+ =", code)
    if unit in UNITS:
        own = definitions(r"\w+_scan|check_list|fetch|free_\w+|ran", src)
        assert own in ([], ["part_scan"]), own                # the radix pass of the clusterer scans its own table
        assert " kThreads = " not in src and "using u64" not in src
        assert len(re.findall(r"^struct pfb_\w+_handle : ListHandle \{", src, re.M)) == 1
        assert len(re.findall(r"^struct Call : ListCall \{", src, re.M)) == 1
        # every array of the scratch is named once, with its type and its count: one carving function, which the
        # size (a carver without a base) and the call (the handle's scratch) both go through
        assert len(definitions("carve", src)) == 1 and len(re.findall(r"\bcarve\(c, ", src)) == 2
        assert "reinterpret_cast<char*>" not in src and "d_scratch +" not in src
        assert re.findall(r"hipLaunchKernelGGL\(list_scan<(\w+)>, dim3\(1\), ", src) == ["false" if unit == "pfb_deint.hip" else "true"]
        for body in ("destroy_list(h)", "set_list_stream(h, hip_stream)", "sync_list(h)", "list_device(h, device_id)",
                     "list_stats(h, stats_out)"):
            assert src.count("    return %s;\n" % body) == 1, (unit, body)
    if unit != "pfb_deint.hip" and unit in UNITS:
        assert src.count("hook_until_still(h->stream, c.a.ctl->hooked, kMaxRounds, ") == 1
        assert "for (;;)" not in src and "hooked[round] = 1u;" in src


def test_the_parameter_structs_are_pinned():
    for unit, names in (("pfb_deint.hip", ("Control", "CompactParams", "HistParams", "SuccParams")),
                        ("pfb_assoc.hip", ("Control", "Arrays")), ("pfb_cluster.hip", ("Control", "Arrays"))):
        src = source(unit)
        for name in names:
            assert re.search(r"static_assert\([^;]*sizeof\(%s\) == \d+" % name, src), (unit, name)


def test_the_core_holds_what_the_units_call():
    core = source("pfb_list.hpp")
    for name in CORE_FUNCTIONS:
        assert len(definitions(name, core)) == 1, name
    for name in ("ListHandle", "ListCall"):
        assert len(re.findall(r"^struct %s \{" % name, core, re.M)) == 1, name
    assert len(re.findall(r"^enum \{ kTierAuto = 0, kTierLds = 1, kTierGlobal = 2 \};", core, re.M)) == 1
    assert len(re.findall(r"^constexpr int kThreads = 256;", core, re.M)) == 1
    for field in ("int device", "hipStream_t stream", "hipEvent_t ev_switch", "char\\* d_scratch", "size_t cap", "std::string last_kernel"):
        assert re.search(r"^  %s\b" % field, core, re.M), field
    # internal to each unit: the three are separate code objects whose host stubs must not meet at link time
    assert core.index("namespace {") < core.index("constexpr") and core.rstrip().endswith("}  // namespace")
    users = [os.path.basename(p) for p in sorted(glob.glob(os.path.join(CSRC, "*"))) if '"pfb_list.hpp"' in open(p, errors="replace").read()]
    assert users == sorted(UNITS)
    from sdr_channelizer_amd import build
    assert "pfb_list.hpp" in build.HEADERS


def test_the_carver_is_defined_once():
    defs = {}
    for path in sorted(glob.glob(os.path.join(CSRC, "*"))):
        text = open(path, errors="replace").read()
        for name in definitions("round_up", text) + re.findall(r"^struct (Carver) \{", text, re.M):
            defs.setdefault(name, []).append(os.path.basename(path))
    assert defs == {"round_up": ["pfb_host.h"], "Carver": ["pfb_host.h"]}
    host = source("pfb_host.h")
    carver = host[host.index("struct Carver {"):]
    carver = carver[:carver.index("\n};")]
    # the next round_up(count * sizeof(T), 256) bytes; no arithmetic on a null base
    assert "at += round_up(count * sizeof(T), 256);" in carver
    assert "return base ? reinterpret_cast<T*>(base + here) : nullptr;" in carver
    for unit in UNITS + ("pfb_mop.hip",):
        assert re.search(r"\bCarver c(\{[\w>-]+\})?;", source(unit)), unit

