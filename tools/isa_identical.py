#!/usr/bin/env python3
"""isa_identical.py OLD_TREE NEW_TREE -- is the device code of two checkouts the same?

Compiles the kernel translation units (FILES) of both trees to gfx950 assembly with the flags of
sdr_channelizer_amd/build.py and compares them per kernel symbol: the instruction text with its
.amdhsa_kernel block, and the kernel's entry in the code object's metadata.  Comments, .ident, .file, the
per-compilation __hip_cuid_<hash> symbol and the file's .AMDGPU.* trailer sections (which follow whichever kernel was
emitted last) are dropped; local labels lose the function's ordinal, so that the order
in which kernels are emitted does not matter.  Exit status 0 = every kernel of every file exists in both trees and
is identical.  A refactor that only moves device code between structs and headers must pass with no difference.  A unit
that one of the trees does not have yet counts as a difference and is reported by name.
"""
import os
import re
import shutil
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

FILES = ["pfb_kernels.hip", "pfb_kernels_mid.hip", "pfb_kernels_big.hip", "pfb_kernels_mixed.hip", "pfb_stft.hip",
         "pfb_pdw.hip", "pfb_trace.hip"]
CSRC = os.path.join("sdr_channelizer_amd", "csrc")
FIELDS = [".vgpr_count", ".sgpr_count", ".vgpr_spill_count", ".sgpr_spill_count", ".private_segment_fixed_size",
          ".group_segment_fixed_size"]
LABEL = re.compile(r"(\.L[A-Za-z_]+)\d+")                    # .LBB12_3 -> .LBB_3, .Lfunc_end12 -> .Lfunc_end
SYMBOL = re.compile(r"\s*\.type\s+(\S+),@(function|object)")
PLACEMENT = (".text", ".section", ".globl", ".weak", ".protected", ".hidden", ".p2align")  # in front of a symbol's .type


def assemble(job):
    tree, name, out = job
    csrc = os.path.join(tree, CSRC)
    hipcc = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    subprocess.check_call([hipcc, "-x", "hip", "--offload-arch=gfx950", "-std=c++20", "-O3", "-fPIC",
                           f"-I{os.path.join(tree, 'include')}", f"-I{csrc}", "--cuda-device-only", "-S",
                           os.path.join(csrc, name), "-o", out])
    return out


def kernels(path):
    """symbol -> [lines of its code and .amdhsa_kernel block, lines of its metadata entry]; kernels only"""
    code, meta, cur, pending, entry, in_meta = {}, {}, None, [], None, False
    with open(path) as f:
        for raw in f:
            line = LABEL.sub(r"\1", raw.split(";")[0].rstrip())
            word = line.split()[0] if line.strip() else ""
            if not word or word in (".ident", ".file"):
                continue
            if "__hip_cuid_" in line or (word == ".section" and ".AMDGPU." in line):  # the file's trailer, no kernel's
                cur, pending = None, []
            elif word == ".amdgpu_metadata":
                in_meta = True
            elif in_meta:
                if line.startswith("  - "):
                    entry = []
                elif not line.startswith(" "):
                    entry = None
                if entry is not None:
                    entry.append(line)
                    if line.strip().startswith(".name:"):
                        meta[line.split()[1]] = entry
            elif SYMBOL.match(line):
                cur = code.setdefault(SYMBOL.match(line).group(1), [])
                cur += pending + [line]
                pending = []
            elif word in PLACEMENT:
                pending.append(line)
            elif cur is not None:
                cur += pending + [line]
                pending = []
    return {k: [code.get(k, []), meta[k]] for k in meta}


def figures(entry):
    vals = {ln.split(":")[0].strip(): ln.split(":")[1].strip() for ln in entry if ":" in ln}
    return " ".join(f"{f[1:]}={vals.get(f, '?')}" for f in FIELDS)


def main():
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    trees = [os.path.abspath(t) for t in sys.argv[1:]]
    tmp = tempfile.mkdtemp(prefix="isa_identical_")
    missing = [f for f in FILES if not all(os.path.exists(os.path.join(t, CSRC, f)) for t in trees)]
    both = [f for f in FILES if f not in missing]
    jobs = [(t, f, os.path.join(tmp, f"{i}_{f}.s")) for f in both for i, t in enumerate(trees)]
    with ThreadPoolExecutor(max_workers=min(5, os.cpu_count() or 1)) as pool:
        list(pool.map(assemble, jobs))
    bad = len(missing)
    for f in missing:
        print(f"{f}: not in both trees")
    for f in both:
        old, new = (kernels(os.path.join(tmp, f"{i}_{f}.s")) for i in (0, 1))
        print(f"{f}: {len(old)} kernels in OLD_TREE, {len(new)} in NEW_TREE")
        for sym in sorted(set(old) | set(new)):
            if sym not in old or sym not in new:
                print(f"  only in {'NEW_TREE' if sym in new else 'OLD_TREE'}: {sym}")
            elif old[sym] != new[sym]:
                print(f"  differs: {sym}\n    old: {figures(old[sym][1])}\n    new: {figures(new[sym][1])}")
            else:
                continue
            bad += 1
    shutil.rmtree(tmp)
    print("identical" if not bad else f"{bad} kernels differ or are missing")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
