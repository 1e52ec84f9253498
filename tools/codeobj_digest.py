#!/usr/bin/env python3
"""codeobj_digest.py [TREE] -- digests of the gfx950 device code of every .hip source of a checkout.

Compiles each .hip file of sdr_channelizer_amd/build.py's SOURCES with --cuda-device-only and build.py's flags,
takes the gfx950 code object (unbundled where the compiler wraps it) and prints the sha256 of its .text section and,
per kernel symbol, the demangled name, the size and the sha256 of the function's bytes.  Two builds of one source
differ as whole files (the per-compilation id) but not in .text, so compare this output, never the objects:

    tools/codeobj_digest.py OLD_TREE > old.txt; tools/codeobj_digest.py NEW_TREE > new.txt; diff old.txt new.txt

A host-side refactor must leave every unit's .text digest equal; where only the order in which the host code takes
kernel addresses moved, the kernels' names and per-kernel digests are still equal (compare the sorted kernel lines).
Bytes are hashed; no instruction text is parsed.
"""
import hashlib
import importlib.util
import os
import shutil
import struct
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

BUNDLE_MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"


def load_build(tree):
    spec = importlib.util.spec_from_file_location("_digest_build", os.path.join(tree, "sdr_channelizer_amd", "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def llvm_tool(hipcc, *names):
    """the first of `names` on PATH or next to the compiler's LLVM; None when there is none"""
    for name in names:
        cands = [shutil.which(name), os.path.join(os.path.dirname(os.path.realpath(hipcc)), "..", "lib", "llvm", "bin", name),
                 os.path.join("/opt/rocm/lib/llvm/bin", name)]
        for c in cands:
            if c and os.path.exists(c):
                return c
    return None


def demangle(hipcc, names):
    tool = llvm_tool(hipcc, "llvm-cxxfilt", "c++filt")
    if not tool or not names:
        return list(names)  # no demangler on this machine: the mangled names, which compare just as well
    return subprocess.run([tool], input="\n".join(names) + "\n", text=True, capture_output=True, check=True).stdout.splitlines()


def code_object(job):
    """compile one source for the device only; return the path of its gfx950 ELF"""
    build, hipcc, src, tmp = job
    obj = os.path.join(tmp, src + ".co")
    common = ["-O3", "-fPIC", f"-I{os.path.join(build.ROOT, 'include')}", f"-I{build.CSRC}"]
    common += os.environ.get("PFB_EXTRA_CXXFLAGS", "").split()
    subprocess.check_call([hipcc, "-x", "hip", f"--offload-arch={build.ARCH}", "-std=c++20"] + common +
                          ["--cuda-device-only", "-c", os.path.join(build.CSRC, src), "-o", obj])
    with open(obj, "rb") as f:
        wrapped = f.read(len(BUNDLE_MAGIC)) == BUNDLE_MAGIC
    if wrapped:
        elf = obj + ".elf"
        subprocess.check_call([llvm_tool(hipcc, "clang-offload-bundler"), "--unbundle", "--type=o", f"--input={obj}",
                               f"--targets=hipv4-amdgcn-amd-amdhsa--{build.ARCH}", f"--output={elf}"])
        return elf
    return obj


def elf_text_and_kernels(path):
    """(.text bytes, [(mangled name, size, bytes)]) of a 64-bit little-endian ELF; kernels = functions with a NAME.kd"""
    with open(path, "rb") as f:
        b = f.read()
    assert b[:6] == b"\x7fELF\x02\x01", "64-bit little-endian ELF expected"
    shoff, = struct.unpack_from("<Q", b, 0x28)
    shentsize, shnum, shstrndx = struct.unpack_from("<HHH", b, 0x3A)
    secs = []
    for i in range(shnum):
        name, typ, _flags, _addr, off, size, link, _info, _align, entsize = struct.unpack_from("<IIQQQQIIQQ", b, shoff + i * shentsize)
        secs.append(dict(name=name, type=typ, off=off, size=size, link=link, entsize=entsize, addr=_addr))

    def cstr(tab, at):
        start = tab["off"] + at
        return b[start:b.index(b"\0", start)].decode()

    for s in secs:
        s["sname"] = cstr(secs[shstrndx], s["name"])
    text_i = next(i for i, s in enumerate(secs) if s["sname"] == ".text")
    text = secs[text_i]
    symtab = next(s for s in secs if s["type"] == 2)  # SHT_SYMTAB
    funcs, descriptors = [], set()
    for k in range(symtab["size"] // symtab["entsize"]):
        nm, info, _other, shndx, value, size = struct.unpack_from("<IBBHQQ", b, symtab["off"] + k * symtab["entsize"])
        name = cstr(secs[symtab["link"]], nm)
        if name.endswith(".kd"):
            descriptors.add(name[:-3])
        elif (info & 0xF) == 2 and shndx == text_i:  # STT_FUNC in .text
            funcs.append((name, value - text["addr"], size))
    tb = b[text["off"]:text["off"] + text["size"]]
    return tb, [(n, sz, tb[o:o + sz]) for n, o, sz in funcs if n in descriptors]


def main():
    tree = os.path.abspath(sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(__file__), ".."))
    build = load_build(tree)
    hipcc = build._hipcc()
    units = [s for s in build.SOURCES if s.endswith(".hip")]
    tmp = tempfile.mkdtemp(prefix="codeobj_digest_")
    try:
        with ThreadPoolExecutor(max_workers=min(5, os.cpu_count() or 1)) as pool:
            objs = list(pool.map(code_object, [(build, hipcc, u, tmp) for u in units]))
        for unit, obj in zip(units, objs):
            text, kernels = elf_text_and_kernels(obj)
            names = demangle(hipcc, [k[0] for k in kernels])
            print(f"unit {unit} text_bytes={len(text)} text_sha256={hashlib.sha256(text).hexdigest()} kernels={len(kernels)}")
            for name, (_, size, body) in sorted(zip(names, kernels)):
                print(f"  kernel {size:7d} {hashlib.sha256(body).hexdigest()} {name}")
    finally:
        shutil.rmtree(tmp)
    return 0


if __name__ == "__main__":
    sys.exit(main())
