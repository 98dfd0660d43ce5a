#!/usr/bin/env python3
"""Are the kernels of two builds the same?  Given two object directories (charls_amd/lib/obj of each build), checks that

  * both have the same set of kernel names, and each name exactly once across all device objects of a build,
  * every kernel has the same (VGPRs, SGPRs, static LDS, scratch),
  * every kernel has the same instruction text: llvm-objdump -d of the gfx950 code objects, cut at the kernel symbols, without
    addresses and encodings (everything from `//`) and without the running number at the end of the labels of inline assembly
    (`L_<name><n>`: it follows the order in which a unit instantiates its templates).

A refactoring of the launch code must leave all three alone.  Prints one line per difference and a summary; exit status 1 when
there is a difference.

    python tools/compare_kernels.py <parent>/charls_amd/lib/obj charls_amd/lib/obj
"""
import glob
import os
import re
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from charls_amd import build as b  # noqa: E402

LABEL = re.compile(r"\b(L_[A-Za-z_]+?)\d+\b")
PADDING = ("s_nop 0", "s_code_end", "...")
SYMBOL = re.compile(r"^[0-9a-f]+ <([^>]+)>:$")


def kernels_of(obj_dir):
    """{name: [(resources, instruction text), ...]} over the device objects of one build."""
    table = {}
    for obj in sorted(glob.glob(os.path.join(obj_dir, "*.hip.o"))):
        resources = {k["name"]: (k["vgprs"], k["sgprs"], k["lds"], k["scratch"]) for k in b.kernel_resources(obj)}
        with tempfile.TemporaryDirectory() as tmp:
            text = "".join(subprocess.check_output([os.path.join(b.LLVM_BIN, "llvm-objdump"), "-d", dev]).decode()
                           for dev in b.device_code_objects(obj, tmp))
        bodies, current = {}, None
        for line in text.splitlines():
            m = SYMBOL.match(line)
            if m:  # (local labels are symbols too: only a kernel's name starts a new body)
                if m.group(1) in resources:
                    current = bodies.setdefault(m.group(1), [])
                elif current is not None:
                    current.append("<" + LABEL.sub(r"\1", m.group(1)) + ">:")
                continue
            if current is not None and line.strip():
                current.append(LABEL.sub(r"\1", line.split("//")[0].strip()))
        for name, res in resources.items():
            body = bodies.get(name, [])
            while body and body[-1] in PADDING:  # (what fills the section up behind a unit's last kernel is not the kernel's)
                body.pop()
            table.setdefault(name, []).append((res, "\n".join(body)))
    return table


def compare(dir_a, dir_b, out=sys.stdout):
    a, c = kernels_of(dir_a), kernels_of(dir_b)
    differences = 0
    for label, table in ((dir_a, a), (dir_b, c)):
        for name, found in table.items():
            if len(found) != 1:
                differences += 1
                print(f"{name}: {len(found)} times in {label}", file=out)
    for name in sorted(set(a) | set(c)):
        if name not in a or name not in c:
            differences += 1
            print(f"{name}: only in {dir_a if name in a else dir_b}", file=out)
        elif a[name][0][0] != c[name][0][0]:
            differences += 1
            print(f"{name}: (vgprs, sgprs, lds, scratch) {a[name][0][0]} -> {c[name][0][0]}", file=out)
        elif a[name][0][1] != c[name][0][1]:
            differences += 1
            print(f"{name}: instruction text differs", file=out)
    empty = sum(1 for found in a.values() if not found[0][1])
    print(f"{len(a)} kernels against {len(c)} ({empty} without instruction text): "
          f"{'no difference' if differences == 0 else str(differences) + ' differences'}", file=out)
    return differences


if __name__ == "__main__":
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    sys.exit(1 if compare(sys.argv[1], sys.argv[2]) else 0)
