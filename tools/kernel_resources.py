"""Register / scratch / LDS use of every kernel in libdpr.so, read from the code-object metadata
(llvm-readelf --notes on the gfx950 bundles of the shared library).  Runs without a GPU.

    python tools/kernel_resources.py            # kernels with spills or scratch
    python tools/kernel_resources.py --all      # every kernel
    python tools/kernel_resources.py --compare OTHER.so   # libdpr.so against another build: kernels in one library
                                                          # only, other resources, other instruction bytes (exit 1
                                                          # if any) -- the check that a host-side change left the
                                                          # device code alone

`tests/test_abi.py::test_scratch_use_matches_the_allow_list` uses `kernel_resources()` as the
zero-scratch gate of the shipped library."""
import hashlib
import os
import re
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LLVM = "/opt/rocm/lib/llvm/bin"
LIB = os.path.join(ROOT, "diffpointrasterisation.jl_amd", "libdpr.so")


def demangle(names):
    try:
        out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout
        return out.splitlines()
    except Exception:
        return list(names)


def _readelf(path, *args):
    return subprocess.run([os.path.join(LLVM, "llvm-readelf"), "-W", *args, path], check=True, capture_output=True,
                          text=True).stdout


def code_digests(path):
    """{symbol: sha256 of its bytes} for every function of the code object `path`: the section table gives the file
    offset of a symbol's section, the symbol table its address and size."""
    sections = {}  # index -> (address, file offset)
    for m in re.finditer(r"^\s*\[\s*(\d+)\]\s+\S+\s+\S+\s+([0-9a-f]{16})\s+([0-9a-f]+)\s", _readelf(path, "-S"), re.M):
        sections[int(m.group(1))] = (int(m.group(2), 16), int(m.group(3), 16))
    with open(path, "rb") as f:
        blob = f.read()
    out = {}
    for m in re.finditer(r"^\s*\d+:\s+([0-9a-f]{16})\s+(\d+)\s+FUNC\s+\S+\s+\S+\s+(\d+)\s+(\S+)$",
                         _readelf(path, "--dyn-syms"), re.M):
        value, size, (addr, off) = int(m.group(1), 16), int(m.group(2)), sections[int(m.group(3))]
        out[m.group(4)] = hashlib.sha256(blob[off + value - addr:off + value - addr + size]).hexdigest()
    return out


def kernel_resources(lib=LIB, code=False):
    """[{name, vgpr, agpr, sgpr, vgpr_spill, sgpr_spill, scratch, lds}] for every kernel of `lib`; with `code` also
    code: the sha256 of the kernel's instruction bytes."""
    tmp = tempfile.mkdtemp(prefix="dpr_co_")
    try:
        copy = os.path.join(tmp, "lib.so")
        shutil.copy(lib, copy)
        subprocess.run([os.path.join(LLVM, "llvm-objdump"), "--offloading", copy], check=True,
                       capture_output=True, cwd=tmp)
        kernels = []
        for f in sorted(os.listdir(tmp)):
            if "amdgcn" not in f:
                continue
            notes = _readelf(os.path.join(tmp, f), "--notes")
            digests = code_digests(os.path.join(tmp, f)) if code else {}
            # one YAML map per kernel under amdhsa.kernels; fields are flat "  .key: value" lines
            for block in re.split(r"\n\s*- \.agpr_count:", notes)[1:]:
                block = ".agpr_count:" + block
                get = lambda k, b=block: re.search(rf"\.{k}:\s*(\S+)", b)
                name = get("name")
                if not name:
                    continue
                num = lambda k: int(get(k).group(1)) if get(k) else 0
                kernels.append(dict(name=name.group(1), vgpr=num("vgpr_count"), agpr=num("agpr_count"),
                                    sgpr=num("sgpr_count"), vgpr_spill=num("vgpr_spill_count"),
                                    sgpr_spill=num("sgpr_spill_count"),
                                    scratch=num("private_segment_fixed_size"),
                                    lds=num("group_segment_fixed_size")))
                if code:
                    kernels[-1]["code"] = digests[name.group(1)]
        for k, d in zip(kernels, demangle([k["name"] for k in kernels])):
            k["demangled"] = d
        return kernels
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


RESOURCES = ("vgpr", "agpr", "sgpr", "vgpr_spill", "sgpr_spill", "scratch", "lds")


def compare(lib, other):
    """Prints the kernel symbols that only one of the two libraries holds, those whose resources differ and those
    whose instruction bytes differ; returns their number.  Names, metadata and bytes only: which instructions a kernel
    uses is not looked at.  A name compiled in several units (tests/test_abi.py lists them) is compared as the sorted
    list of its copies."""
    def table(path):
        t = {}
        for k in kernel_resources(path, code=True):
            t.setdefault(k["name"], []).append((tuple(k[r] for r in RESOURCES), k["code"]))
        return {n: sorted(v) for n, v in t.items()}

    a, b = table(lib), table(other)
    label = dict(zip(list(a) + list(b), map(short, demangle(list(a) + list(b)))))
    only_a, only_b = sorted(set(a) - set(b)), sorted(set(b) - set(a))
    both = sorted(set(a) & set(b))
    res = [n for n in both if [r for r, _ in a[n]] != [r for r, _ in b[n]]]
    code = [n for n in both if n not in res and a[n] != b[n]]
    for title, names in ((f"only in {lib}", only_a), (f"only in {other}", only_b)):
        for n in names:
            print(f"{title}: {label[n]}")
    for n in res:
        print(f"resources differ: {label[n]}\n    {[r for r, _ in a[n]]}\n    {[r for r, _ in b[n]]}   {RESOURCES}")
    for n in code:
        print(f"code bytes differ (resources equal): {label[n]}")
    print(f"{len(a)} / {len(b)} kernel symbols; {len(only_a)} + {len(only_b)} in one library only, {len(res)} with "
          f"other resources, {len(code)} with other code bytes, {len(both) - len(res) - len(code)} identical")
    return len(only_a) + len(only_b) + len(res) + len(code)


def short(d):
    """`dpr::k_name<template args>` without the parameter list"""
    m = re.match(r"(?:void )?(dpr::\w+(?:<.*?>)?)\(", d)
    return m.group(1) if m else d


if __name__ == "__main__":
    if "--compare" in sys.argv:
        sys.exit(1 if compare(LIB, sys.argv[sys.argv.index("--compare") + 1]) else 0)
    ks = kernel_resources()
    show_all = "--all" in sys.argv
    n = 0
    for k in sorted(ks, key=lambda k: (-k["scratch"], k["demangled"])):
        if show_all or k["vgpr_spill"] or k["scratch"] or k["sgpr_spill"]:
            n += 1
            print(f"vgpr {k['vgpr']:3d} agpr {k['agpr']:3d} spill v{k['vgpr_spill']:3d} s{k['sgpr_spill']:3d} "
                  f"scratch {k['scratch']:4d} B  lds {k['lds']:6d}  {short(k['demangled'])}")
    print(f"{len(ks)} kernels, {n} listed")
