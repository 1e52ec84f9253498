"""Generates tests/golden/record_format_ref.json.

What the reference's own record-format code (cpp/IqPacket.h + cpp/Helper.cpp, compiled into oracle/_ref by
oracle/Makefile where the reference tree is present) answers to the questions tests/test_record_format.py asks: the
IqPacket size and field offsets, the 112 header bytes the recorders write for a set of field values, and
getFilenameStr for a set of times.  The tests compare our restatements with this file everywhere, and with the live
oracle/_ref build too where it exists.

Run from the repo root after building oracle/_ref:  python tests/golden/make_record_format.py
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from oracle.pfb_oracle import RefIqPacket  # noqa: E402

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "record_format_ref.json")

# make_header arguments: marker, link speed, frequency, bandwidth, sample rate, gain, samples, bit width, board, serial,
# fpga version, firmware version, start time
HEADERS = [(marker, 5000, 2_412_000_000, 56_000_000, 56_000_000, 31.5, 123456, bw,
            b"bladerf", b"0123456789abcde", b"v0.15.0", b"v2.4.0", 1.7e9 + 0.25)
           for marker, bw in ((0x02020202, 12), (0x03030303, 16), (0x03030303, 8), (0x02020202, 8))]
HEADERS.append((0x03030303, 0, 915_000_000, 20_000_000, 20_000_000, 12.0, 10, 16, b"usrp", b"s1", b"", b"", 99.0))
FILENAME_MS = [0, 1_700_000_000_123, 951_782_400_000, 1_709_251_199_999]


def as_json(args):
    return [a.decode() if isinstance(a, bytes) else a for a in args]


def main():
    ref = RefIqPacket()
    rec = {"sizeof": ref.sizeof(), "offsets": ref.offsets(),
           "headers": [{"args": as_json(a), "bytes": ref.make_header(*a).hex()} for a in HEADERS],
           "filenames": {str(ms): ref.filename(ms) for ms in FILENAME_MS}}
    with open(OUT, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print("wrote", OUT)


if __name__ == "__main__":
    main()
