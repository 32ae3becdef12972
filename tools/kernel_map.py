"""Which kernels each configuration of tests/test_isolation_gpu.py reaches.

Run under a kernel trace, then read the trace back:
    rocprofv3 --kernel-trace --output-format csv -d OUT -o trace -- python tools/kernel_map.py run
    python tools/kernel_map.py parse OUT
`run` does one forward + predict per (configuration, mode) and one forward per one-kernel network and launches a small torch sort between two of them as a
separator; `parse` splits the dispatches (in dispatch order) at the separators and prints the conv / op kernels of each."""
import glob
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def _runs():
    import test_isolation_gpu as t
    out = [(c, "fp32") for c in t.CFG]
    out += [(c, m) for c, m, _ in t.CASES if m != "fp32"]
    seen, res = set(), []
    for r in out:
        if r not in seen and not (r[1] == "store_f16" and r[0] in t._FP16_REFUSED):
            seen.add(r); res.append(r)
    return res + [("kernel:" + n, "fp32") for n in sorted(t.KERNEL_TARGETS)]


def run():
    import torch
    import test_isolation_gpu as t
    from yololite_amd import _lib
    sep = torch.rand(4099, device=t.DEV)
    for cid, mode in _runs():
        if cid.startswith("kernel:"):                 # the one-kernel networks of test_masked_channel_tail_kernel_keeps_images_apart
            ctx, S = t._kernel_context(cid[7:])
            x = t._x(3, S, seed=17).to(t.DEV)
            torch.sort(sep)
            torch.cuda.synchronize()
            ctx.forward(x)
            torch.cuda.synchronize()
            continue
        m = t._model(cid)
        S, B = t.CFG[cid][1], t.CFG[cid][2]
        ctx = m._ctx_for(S)
        t._configure(ctx, cid, mode, "eager")
        x = t._x(B, S, seed=7).to(t.DEV)
        torch.sort(sep)
        torch.cuda.synchronize()
        m(x)
        ctx.predict(x, _lib.POST_MAIN, 0.01, 0.5, 300)
        torch.cuda.synchronize()
        t._configure(ctx, cid, "fp32", "eager")
    torch.sort(sep)
    torch.cuda.synchronize()
    print("\n".join(f"{c} {m}" for c, m in _runs()))


def parse(d):
    import csv
    files = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)
    assert files, d
    rows = []
    for f in files:
        with open(f) as fh:
            rows += list(csv.DictReader(fh))
    rows.sort(key=lambda r: int(r.get("Dispatch_Id") or r.get("Correlation_Id") or 0))
    groups, cur = [], None
    for r in rows:
        name = r["Kernel_Name"]
        if "sort" in name.lower() and "yl_" not in name:        # the separator: torch's sort kernels, never one of ours
            if cur is not None and cur:
                groups.append(cur)
            cur = set() if cur is None or cur else cur
            continue
        if cur is not None and name.startswith(("void yl_", "yl_")):
            cur.add(re.sub(r"^void ", "", name).split("(")[0])
    runs = _runs()
    for (cid, mode), g in zip(runs, groups):
        print(f"{cid:28s} {mode:10s} " + " ".join(sorted({k.split('<')[0] for k in g})))
    if len(groups) != len(runs):
        print(f"(groups {len(groups)} != runs {len(runs)})")


if __name__ == "__main__":
    if sys.argv[1] == "run":
        run()
    else:
        parse(sys.argv[2])
