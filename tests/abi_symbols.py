"""The function names the C headers under include/ declare, read out of their text."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def declared_symbols(headers=("pfb_channelizer.h", "pfb_iq_packet.h")):
    names = set()
    for hdr in headers:
        text = open(os.path.join(ROOT, "include", hdr)).read()
        text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
        names |= set(re.findall(r"\b(pfb_[a-z0-9_]+)\s*\(", text))
    return names
