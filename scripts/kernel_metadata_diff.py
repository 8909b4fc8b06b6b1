#!/usr/bin/env python
"""Registers, LDS, scratch and code size of every kernel of two builds of libogg_hip.so, from the code objects' own metadata
(the amdhsa.kernels note and the symbol table of the gfx950 code object inside the library): which kernels changed, appeared or went.

    python scripts/kernel_metadata_diff.py BEFORE.so AFTER.so [--all] > profiles/<name>.md

Needs the ROCm LLVM tools (llvm-objdump --offloading, llvm-readelf); cross-checks nothing on a GPU.
"""
import os
import re
import subprocess
import sys
import tempfile

LLVM = os.environ.get("OGG_LLVM_BIN", "/opt/rocm/llvm/bin")
FIELDS = (".vgpr_count", ".agpr_count", ".sgpr_count", ".vgpr_spill_count", ".sgpr_spill_count", ".group_segment_fixed_size",
          ".private_segment_fixed_size")


def kernels(lib):
    """{kernel name: {field: value, 'code_bytes': size of the kernel's function symbol}}"""
    with tempfile.TemporaryDirectory() as d:
        copy = os.path.join(d, "lib.so")
        with open(lib, "rb") as f, open(copy, "wb") as g:
            g.write(f.read())
        subprocess.run([os.path.join(LLVM, "llvm-objdump"), "--offloading", copy], check=True, stdout=subprocess.DEVNULL, cwd=d)
        cos = [os.path.join(d, f) for f in os.listdir(d) if "amdgcn" in f]
        assert cos, "no device code object in %s" % lib
        out = {}
        for co in cos:
            notes = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", co], check=True, capture_output=True, text=True).stdout
            for block in re.split(r"\n\s*- \.agpr_count:", notes)[1:]:
                block = "  - .agpr_count:" + block
                m = re.search(r"^\s*\.name:\s*(\S+)", block, flags=re.M)
                if not m:
                    continue
                rec = {}
                for f in FIELDS:
                    v = re.search(r"^\s*(?:- )?%s:\s*(\d+)" % re.escape(f), block, flags=re.M)
                    rec[f] = int(v.group(1)) if v else -1
                out[m.group(1)] = rec
            syms = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "-sW", co], check=True, capture_output=True, text=True).stdout
            for line in syms.splitlines():
                p = line.split()
                if len(p) >= 8 and p[3] == "FUNC" and p[7] in out:
                    out[p[7]]["code_bytes"] = int(p[2])
        return out


def demangle(names):
    for tool in (os.path.join(LLVM, "llvm-cxxfilt"), "c++filt"):
        try:
            r = subprocess.run([tool], input="\n".join(names), capture_output=True, text=True)
        except OSError:
            continue
        if r.returncode == 0:
            return dict(zip(names, r.stdout.splitlines()))
    return {n: n for n in names}


def main(argv):
    before, after = kernels(argv[1]), kernels(argv[2])
    show_all = "--all" in argv
    names = sorted(set(before) | set(after))
    nice = demangle(names)
    cols = FIELDS + ("code_bytes",)
    same = [n for n in names if before.get(n) == after.get(n)]
    print("# Kernel resources, before -> after\n")
    print("%d kernels before, %d after, %d identical in every column (%s).\n" % (len(before), len(after), len(same),
                                                                                 ", ".join(c.lstrip(".") for c in cols)))
    print("| kernel | " + " | ".join(c.lstrip(".") for c in cols) + " |")
    print("|---|" + "---|" * len(cols))
    for n in names:
        b, a = before.get(n), after.get(n)
        if b == a and not show_all:
            continue
        cells = []
        for c in cols:
            vb = "-" if b is None else str(b.get(c, "?"))
            va = "-" if a is None else str(a.get(c, "?"))
            cells.append(vb if vb == va else "%s -> %s" % (vb, va))
        tag = "new: " if b is None else ("gone: " if a is None else "")
        print("| %s`%s` | %s |" % (tag, nice[n][:150], " | ".join(cells)))
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
