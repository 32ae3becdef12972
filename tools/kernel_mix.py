#!/usr/bin/env python3
"""Resource figures and static instruction mix of the kernels in gfx950 assembly files.

    python tools/kernel_mix.py ASM_DIR [PATTERN]

ASM_DIR holds NAME.s files (one per object: the compile line of csrc/build.py with `--offload-device-only -S -o NAME.s`, as
tools/codeobj_diff.py expects).  For every kernel whose (demangled, if c++filt is there) name contains PATTERN (default: every
kernel) prints
  - VGPRs, AGPRs, SGPRs, spilled SGPRs / VGPRs, scratch bytes per lane and the waves per SIMD the compiler reports;
  - the static instruction counts by class of (a) the whole kernel, (b) its outermost loop and (c) the innermost loop that holds
    ALL of the kernel's MFMAs (for a conv kernel: the k loop).
Classes, by mnemonic prefix only: mfma = v_mfma*, valu = every other v_*, salu = s_*, lds = ds_*, vmem = global_* / buffer_* /
flat_* / scratch_*.  Loops are the natural loops of the control-flow graph (a loop's blocks may lie anywhere in the text); counts are
static: an inner rolled loop counts once, and both sides of a branch count."""
import os
import re
import subprocess
import sys

CLASSES = ("mfma", "valu", "salu", "lds", "vmem", "other")


def klass(mn):
    if mn.startswith("v_mfma"):
        return "mfma"
    for pre, k in (("v_", "valu"), ("s_", "salu"), ("ds_", "lds"), ("global_", "vmem"), ("buffer_", "vmem"), ("flat_", "vmem"),
                   ("scratch_", "vmem")):
        if mn.startswith(pre):
            return k
    return "other"


def demangle(names):
    try:
        out = subprocess.run(["c++filt"], input="\n".join(names), stdout=subprocess.PIPE, text=True, check=True).stdout.split("\n")
        return dict(zip(names, out))
    except (OSError, subprocess.CalledProcessError):
        return {n: n for n in names}


def metadata(lines):
    """{symbol: {field: value}} of the amdhsa.kernels list"""
    out, cur = {}, None
    for ln in lines:
        if re.match(r"\s+- \.\w+:", ln):
            cur = {}
            ln = ln.replace("- ", "  ", 1)
        m = re.match(r"\s+\.(\w+):\s+(\S+)\s*$", ln)
        if cur is not None and m:
            cur[m.group(1)] = m.group(2)
            if m.group(1) == "symbol":
                out[m.group(2)[:-3] if m.group(2).endswith(".kd") else m.group(2)] = cur
    return out


def kernels(path):
    lines = open(path).read().split("\n")
    names = [m.group(1) for m in (re.match(r"\s*\.amdhsa_kernel\s+(\S+)", ln) for ln in lines) if m]
    meta = metadata(lines)
    out = {}
    for n in names:
        start = next(i for i, ln in enumerate(lines) if ln.split(";")[0].strip() == n + ":")
        body, notes, i = [], {}, start + 1
        end = next(j for j in range(start, len(lines)) if lines[j].strip().startswith(".end_amdhsa_kernel"))
        for ln in lines[end:end + 40]:                  # the compiler's resource comments follow the descriptor
            m = re.match(r";\s*(TotalNumSgprs|NumVgprs|NumAgprs|ScratchSize|Occupancy):\s*(\d+)", ln)
            if m:
                notes.setdefault(m.group(1), int(m.group(2)))
        while i < end:
            ln = lines[i]
            t = ln.split(";")[0].strip()
            if t and not t.startswith("."):
                body.append(t)
            elif t.startswith(".LBB") and t.endswith(":"):
                body.append(t)
            i += 1
        out[n] = (body, notes, meta.get(n, {}))
    return out


def count(body, idx):
    c = dict.fromkeys(CLASSES, 0)
    for i in idx:
        if not body[i].endswith(":"):
            c[klass(body[i].split()[0])] += 1
    return c


def loops(body):
    """natural loops of the kernel's control-flow graph as sets of line indices (block placement may put a loop's blocks
    anywhere in the text): basic blocks end at branches and start at labels; a back edge is a branch to a label not after
    it whose target reaches it; loops of one header are one loop"""
    starts = sorted({0} | {i for i, t in enumerate(body) if t.endswith(":")} |
                    {i + 1 for i, t in enumerate(body) if t.split()[0].startswith(("s_cbranch", "s_branch", "s_endpgm", "s_setpc"))})
    starts = [x for x in starts if x < len(body)]
    blk = {}
    for k, x in enumerate(starts):
        for i in range(x, starts[k + 1] if k + 1 < len(starts) else len(body)):
            blk[i] = k
    at = {t[:-1]: blk[i] for i, t in enumerate(body) if t.endswith(":")}
    succ = {k: set() for k in range(len(starts))}
    for k, x in enumerate(starts):
        last = (starts[k + 1] if k + 1 < len(starts) else len(body)) - 1
        w = body[last].split()
        if w[0].startswith(("s_cbranch", "s_branch")) and w[-1] in at:
            succ[k].add(at[w[-1]])
        if not w[0].startswith(("s_branch", "s_endpgm", "s_setpc")) and k + 1 < len(starts):
            succ[k].add(k + 1)
    pred = {k: set() for k in succ}
    for k, ss in succ.items():
        for t in ss:
            pred[t].add(k)
    by_header = {}
    for u, ss in succ.items():
        for h in ss:
            if starts[h] > starts[u]:
                continue
            seen, todo = {h}, [u]                      # blocks that reach u without passing h
            while todo:
                n = todo.pop()
                if n not in seen:
                    seen.add(n)
                    todo.extend(pred[n])
            fwd, todo = set(), [h]                     # ... and that h reaches: drops the blocks in front of a mere backward jump
            while todo:
                n = todo.pop()
                if n in seen and n not in fwd:
                    fwd.add(n)
                    todo.extend(succ[n])
            if u in fwd:
                by_header.setdefault(h, set()).update(fwd)
    return [sorted(i for i in blk if blk[i] in bs) for bs in by_header.values()]


def fmt(c):
    return "  ".join("%s %5d" % (k, c[k]) for k in CLASSES if k != "other" or c[k])


def main(d, pat):
    for f in sorted(x for x in os.listdir(d) if x.endswith(".s")):
        ks = kernels(os.path.join(d, f))
        pretty = demangle(list(ks))
        for n in sorted(ks, key=lambda k: pretty[k]):
            if pat not in pretty[n] and pat not in n:
                continue
            body, notes, meta = ks[n]
            print("%s: %s" % (f, pretty[n]))
            print("  vgpr %s  agpr %s  sgpr %s  sgpr_spill %s  vgpr_spill %s  scratch %s  waves/simd %s" % (
                notes.get("NumVgprs", "?"), notes.get("NumAgprs", "?"), notes.get("TotalNumSgprs", "?"), meta.get("sgpr_spill_count", "?"),
                meta.get("vgpr_spill_count", "?"), notes.get("ScratchSize", "?"), notes.get("Occupancy", "?")))
            print("  kernel           %s" % fmt(count(body, range(len(body)))))
            lp = loops(body)
            mf = {i for i, t in enumerate(body) if t.startswith("v_mfma")}
            if lp:
                print("  outermost loop   %s" % fmt(count(body, max(lp, key=len))))
            inner = [r for r in lp if mf and mf <= set(r)]
            if inner:
                print("  all-MFMA loop    %s" % fmt(count(body, min(inner, key=len))))


if __name__ == "__main__":
    if len(sys.argv) not in (2, 3):
        sys.exit(__doc__)
    main(sys.argv[1], sys.argv[2] if len(sys.argv) == 3 else "")
