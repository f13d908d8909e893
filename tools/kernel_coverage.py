"""Which kernel instantiations of librpeflow_hip.so a run launched.

    python tools/kernel_coverage.py list <lib.so>
        every kernel instantiation in the library's gfx950 code object, one normalised name per line
    python tools/kernel_coverage.py diff <lib.so> <kernel_trace.csv> [more traces...]
        the instantiations no trace launched, grouped by the source file that defines them

The instantiations are the ``.kd`` (kernel descriptor) symbols of the gfx950 entries of the offload bundles in
``.hip_fatbin`` (one bundle per translation unit); the ELF and bundles are read here, only the demangling is left to llvm-cxxfilt.  Library and trace
are compared on one normalised name: demangled, ``(anonymous namespace)::`` removed, return type and argument list
dropped, template arguments kept (``corr_backward_kernel<4, true>``).  Trace rows that are not kernels of the
library (MIOpen, rocBLAS, ATen) play no part.
"""
import argparse
import csv
import os
import re
import shutil
import struct
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "rpeflow_amd", "csrc")
TARGET = "gfx950"
_BUNDLE_MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"


def _sections(elf):
    """{name: (offset, size, sh_type, sh_link, sh_entsize)} of a little-endian ELF64 image."""
    if elf[:4] != b"\x7fELF" or elf[4] != 2 or elf[5] != 1:
        raise ValueError("not a little-endian ELF64 file")
    shoff, = struct.unpack_from("<Q", elf, 0x28)
    shentsize, shnum, shstrndx = struct.unpack_from("<HHH", elf, 0x3A)
    hdrs = [struct.unpack_from("<IIQQQQIIQQ", elf, shoff + i * shentsize) for i in range(shnum)]
    stroff = hdrs[shstrndx][4]
    out = []
    for h in hdrs:
        name = elf[stroff + h[0]:elf.index(b"\0", stroff + h[0])].decode()
        out.append((name, h[4], h[5], h[1], h[6], h[9]))
    return out


def code_objects(lib_path, target=TARGET):
    """The ``target`` code objects bundled into a HIP shared library: without -fgpu-rdc every translation unit
    brings its own offload bundle, and .hip_fatbin holds them one after another."""
    with open(lib_path, "rb") as f:
        elf = f.read()
    fat = [s for s in _sections(elf) if s[0] == ".hip_fatbin"]
    if not fat:
        raise ValueError(f"{lib_path}: no .hip_fatbin section")
    _, off, size, *_ = fat[0]
    blob = elf[off:off + size]
    if not blob.startswith(_BUNDLE_MAGIC):
        raise ValueError(f"{lib_path}: .hip_fatbin is not an uncompressed clang offload bundle")
    cos, start = [], 0
    while start >= 0:
        n, = struct.unpack_from("<Q", blob, start + len(_BUNDLE_MAGIC))
        pos, end = start + len(_BUNDLE_MAGIC) + 8, start
        for _ in range(n):
            e_off, e_size, t_len = struct.unpack_from("<QQQ", blob, pos)
            triple = blob[pos + 24:pos + 24 + t_len].decode()
            pos += 24 + t_len
            end = max(end, start + e_off + e_size)
            if triple.startswith("hip") and triple.split("--")[-1].split(":")[0] == target:
                cos.append(blob[start + e_off:start + e_off + e_size])
        start = blob.find(_BUNDLE_MAGIC, max(end, start + 1))
    if not cos:
        raise ValueError(f"{lib_path}: no {target} entry in the offload bundles")
    return cos


def kd_symbols(co):
    """Mangled names of the kernels (the symbols ``<name>.kd``) of an AMDGPU code object."""
    secs = _sections(co)
    names = set()
    for _, off, size, sh_type, link, entsize in secs:
        if sh_type not in (2, 11):  # SHT_SYMTAB, SHT_DYNSYM
            continue
        str_off = secs[link][1]
        for i in range(size // entsize):
            st_name, = struct.unpack_from("<I", co, off + i * entsize)
            name = co[str_off + st_name:co.index(b"\0", str_off + st_name)].decode()
            if name.endswith(".kd"):
                names.add(name[:-3])
    return sorted(names)


def _cxxfilt():
    for cand in (shutil.which("llvm-cxxfilt"), "/opt/rocm/llvm/bin/llvm-cxxfilt", "/opt/rocm/lib/llvm/bin/llvm-cxxfilt",
                 shutil.which("c++filt")):
        if cand and os.path.exists(cand):
            return cand
    raise FileNotFoundError("no llvm-cxxfilt or c++filt to demangle with")


def demangle(names):
    if not names:
        return []
    out = subprocess.run([_cxxfilt()], input="\n".join(names) + "\n", capture_output=True, text=True, check=True).stdout
    return out.splitlines()


def normalise(demangled):
    """``void (anonymous namespace)::k<4, true>(float const*, int)`` -> ``k<4, true>``."""
    s = demangled.strip().replace("(anonymous namespace)::", "")
    # drop the argument list: the last top-level "(...)" (a trace may already have dropped it)
    if s.endswith(")"):
        depth = 0
        for i in range(len(s) - 1, -1, -1):
            depth += {")": 1, "(": -1}.get(s[i], 0)
            if depth == 0:
                s = s[:i]
                break
    # drop the return type: keep what follows the last top-level space
    depth, cut = 0, 0
    for i, ch in enumerate(s):
        if ch in "<(":
            depth += 1
        elif ch in ">)":
            depth -= 1
        elif ch == " " and depth == 0:
            cut = i + 1
    return s[cut:].strip()


def list_kernels(lib_path):
    """Sorted normalised names of every kernel instantiation in the library's gfx950 code object."""
    mangled = sorted(set(m for co in code_objects(lib_path) for m in kd_symbols(co)))
    return sorted(set(normalise(d) for d in demangle(mangled)))


def launched(trace_paths):
    """Normalised names of every kernel a rocprofv3 kernel_trace.csv (or several) recorded."""
    names = set()
    for p in trace_paths:
        with open(p, newline="") as f:
            for row in csv.DictReader(f):
                name = row.get("Kernel_Name") or row.get("KernelName") or ""
                if name:
                    names.add(normalise(name))
    return names


def base_name(norm):
    """``ns::k<4, (X)1>`` -> ``k``."""
    return norm.split("<", 1)[0].split("::")[-1]


def source_of(norm, src_dir=CSRC):
    """The .hip/.h file under src_dir whose ``__global__`` defines the kernel, or '?'."""
    pat = re.compile(r"__global__[^;{}]{0,400}?\b" + re.escape(base_name(norm)) + r"\s*\(", re.S)
    for fn in sorted(os.listdir(src_dir)):
        if fn.endswith((".hip", ".h")):
            with open(os.path.join(src_dir, fn)) as f:
                if pat.search(f.read()):
                    return fn
    return "?"


def never_launched(lib_path, trace_paths):
    seen = launched(trace_paths)
    return [k for k in list_kernels(lib_path) if k not in seen]


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    sub = ap.add_subparsers(dest="cmd", required=True)
    p = sub.add_parser("list", help="every kernel instantiation in the library")
    p.add_argument("lib")
    p = sub.add_parser("diff", help="instantiations that no trace launched, by source file")
    p.add_argument("lib")
    p.add_argument("traces", nargs="+")
    p.add_argument("--src", default=CSRC, help="directory of the .hip sources (default: the package's csrc)")
    a = ap.parse_args(argv)
    if a.cmd == "list":
        for k in list_kernels(a.lib):
            print(k)
        return 0
    allk = list_kernels(a.lib)
    missing = never_launched(a.lib, a.traces)
    by_file = {}
    for k in missing:
        by_file.setdefault(source_of(k, a.src), []).append(k)
    print(f"# {len(missing)} of {len(allk)} kernel instantiations never launched")
    for fn in sorted(by_file):
        print(f"{fn}:")
        for k in by_file[fn]:
            print(f"  {k}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
