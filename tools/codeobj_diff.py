#!/usr/bin/env python3
"""Compare the device code of two builds kernel by kernel.

    python tools/codeobj_diff.py A_DIR B_DIR [--alias B_TEXT=A_TEXT ...]

A_DIR and B_DIR hold gfx950 assembly files of the same names (one per object: the compile line of csrc/build.py with
`--offload-device-only -S -o NAME.s`).  Each file is split at its kernel symbols; a kernel is its instruction text
and the resource lines of its `.amdhsa_kernel` block (`<symbol>:` up to `.end_amdhsa_kernel`).  Compiler-local label numbers
(`.LBB<n>_<m>`, `.Lfunc_end<n>`, ... -- they follow the order of emission, which host code can change) are normalised.
Prints one line per object and a total; the exit status is 0 only when every object has the same kernel symbols with
identical text.  --alias replaces B_TEXT by A_TEXT in B's files first: for a kernel that became one instantiation of a
template, whose mangled name changed and nothing else should have (the other instantiations then count as kernels of B only).
Device functions that are not kernels (none in this project: everything is inlined) are not compared."""
import os
import re
import sys

LABEL = re.compile(r"\.L(BB|func_begin|func_end|tmp|JTI)(\d+)(_\d+)?")


ALIASES = []


def kernels(path, aliases=()):
    text = open(path).read()
    for new, old in aliases:
        text = text.replace(new, old)
    lines = text.split("\n")
    names = [m.group(1) for m in (re.match(r"\s*\.amdhsa_kernel\s+(\S+)", ln) for ln in lines) if m]
    out = {n: [] for n in names}
    cur = None
    for ln in lines:
        t = ln.split(";")[0].strip()            # comments carry emission-order details (function numbers)
        if cur is None:
            if t.endswith(":") and t[:-1] in out:
                cur = out[t[:-1]]               # the resource block follows the instructions, in front of .Lfunc_end
            continue
        if t:
            cur.append(t)
        if t == ".end_amdhsa_kernel":
            cur = None
    norm = {}
    for n, body in out.items():
        ids = {}
        def sub(m):
            return ".L%s%d%s" % (m.group(1), ids.setdefault((m.group(1), m.group(2)), len(ids)), m.group(3) or "")
        norm[n] = [LABEL.sub(sub, ln) for ln in body]
    return norm


def main(a_dir, b_dir):
    files = sorted(f for f in os.listdir(a_dir) if f.endswith(".s"))
    missing = sorted(set(f for f in os.listdir(b_dir) if f.endswith(".s")) ^ set(files))
    total = diffs = len(missing)
    for f in missing:
        print("%s: in one directory only" % f)
    for f in files:
        if f in missing:
            continue
        a, b = kernels(os.path.join(a_dir, f)), kernels(os.path.join(b_dir, f), ALIASES)
        bad = sorted(set(a) ^ set(b)) + sorted(n for n in set(a) & set(b) if a[n] != b[n] or len(a[n]) < 2)
        for n in bad:
            print("  %s: %s %s" % (f, "only in one build:" if (n in a) != (n in b) else "differs:", n))
        print("%s: %d kernels compared, %d differences" % (f, len(set(a) | set(b)), len(bad)))
        total += len(set(a) | set(b))
        diffs += len(bad)
    print("objects %d, kernels compared %d, differences %d" % (len(files), total, diffs))
    return 1 if diffs or not files else 0


if __name__ == "__main__":
    while "--alias" in sys.argv:
        i = sys.argv.index("--alias")
        ALIASES.append(tuple(sys.argv[i + 1].split("=", 1)))
        del sys.argv[i:i + 2]
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    sys.exit(main(sys.argv[1], sys.argv[2]))
