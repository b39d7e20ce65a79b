#!/usr/bin/env python3
"""Compare the kernels of two device-assembly files body by body.

    hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off --cuda-device-only -S vqvdb_amd/csrc/vq_runtime.hip -o before.s   (old tree)
    hipcc ... -o after.s                                                                                                            (new tree)
    python tools/kernel_isa_diff.py before.s after.s > profiles/<change>_isa_diff.txt

For a change that must not move an instruction (a refactor of host code, a renamed template parameter).  A kernel is the text from
its `_Z...:` label to the following `.Lfunc_end`.  Comments are dropped, every mangled symbol becomes `SYM`, and the function number
of a local label (`.LBB12_3` -> `.LBB_3`, `.Lfunc_end12` -> `.Lfunc_end`) goes, so that a renamed kernel compares equal; the kernels
are paired in order of appearance.  Exit status 0: same number of kernels, every body identical.
"""
import re
import subprocess
import sys

LABEL = re.compile(r"^(_Z\w+):")
END = re.compile(r"^\.Lfunc_end\d+:")
SYMBOL = re.compile(r"\b_Z\w+")
LOCAL = re.compile(r"\.L([A-Za-z_]+?)\d+(_\d+)?\b")


def kernels(path):
    """[(mangled name, normalised body lines)] in order of appearance"""
    out, name, body = [], None, []
    with open(path) as f:
        for line in f:
            if name is None:
                m = LABEL.match(line)
                if m:
                    name, body = m.group(1), []
                continue
            if END.match(line):
                out.append((name, body))
                name = None
                continue
            line = line.split(";", 1)[0].rstrip()
            if not line:
                continue
            line = SYMBOL.sub("SYM", line)
            body.append(LOCAL.sub(lambda m: ".L" + m.group(1) + (m.group(2) or ""), line))
    return out


def demangle(names):
    try:
        r = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True)
        return r.stdout.split("\n")[: len(names)]
    except (OSError, subprocess.CalledProcessError):
        return list(names)


def short(name):
    return re.sub(r"\(.*$", "", re.sub(r"^void ", "", name))


def main():
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    a, b = kernels(sys.argv[1]), kernels(sys.argv[2])
    print(f"kernels: {len(a)} before, {len(b)} after")
    differ, renamed = [], []
    for i, ((na, ba), (nb, bb)) in enumerate(zip(a, b)):
        if ba != bb:
            first = next((k for k, (x, y) in enumerate(zip(ba, bb)) if x != y), min(len(ba), len(bb)))
            differ.append((i, na, nb, len(ba), len(bb), first))
        if na != nb:
            renamed.append((i, na, nb))
    print(f"bodies compared in order of appearance: {min(len(a), len(b)) - len(differ)} identical, {len(differ)} differ")
    print(f"renamed: {len(renamed)}")
    da, db = demangle([r[1] for r in renamed]), demangle([r[2] for r in renamed])
    for (i, _, _), x, y in zip(renamed, da, db):
        print(f"  #{i:<3} {short(x)}\n    -> {short(y)}   ({len(a[i][1])} lines)")
    for i, na, nb, la, lb, first in differ:
        print(f"DIFFERENT #{i}: {na} ({la} lines) / {nb} ({lb} lines), first difference at body line {first}")
    ok = len(a) == len(b) and not differ
    print("RESULT: " + ("identical" if ok else "NOT identical"))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
