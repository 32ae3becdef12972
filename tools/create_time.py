#!/usr/bin/env python3
"""Time yl_create (validate, pack, upload) of two builds of the library in ONE process, alternating.

    python tools/create_time.py _variants/libyololite_hip_parent.so [--n 9] [--out FILE.json]

For edge_n and yololite_m (80 classes, 640 x 640): one descriptor per model, then n rounds of [other library, in-tree
library], each a yl_create + yl_destroy timed on the host around the create alone.  One untimed create per library and
model comes first (the per-device kernel attributes, the runtime's first allocations).  Prints and optionally writes per
model and library: every time in ms, the median, and the spread (max - min)."""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from yololite_amd import _lib  # noqa: E402
from yololite_amd.model import model_desc  # noqa: E402
from yololite_amd.program import SynthStateDict, build_program, zoo_meta  # noqa: E402


def create_ms(lib, d):
    h = ctypes.c_void_p()
    t0 = time.perf_counter()
    st = lib.yl_create(ctypes.byref(d), 0, ctypes.byref(h))
    t1 = time.perf_counter()
    if h:
        lib.yl_destroy(h)
    if st != 0:
        raise RuntimeError(f"yl_create: status {st}")
    return (t1 - t0) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("other")
    ap.add_argument("--n", type=int, default=9)
    ap.add_argument("--out")
    a = ap.parse_args()
    libs = {"other": ctypes.CDLL(os.path.abspath(a.other)), "in_tree": ctypes.CDLL(_lib.LIB_PATH)}
    for lib in libs.values():
        lib.yl_destroy.argtypes = [ctypes.c_void_p]
        lib.yl_destroy.restype = None
    res = {"other": os.path.basename(a.other), "n": a.n, "models": {}}
    for name in ("edge_n", "yololite_m"):
        prog = build_program(zoo_meta(name, num_classes=80, img_size=640), SynthStateDict(seed=0, num_classes=80))
        d, keep = model_desc(prog.img_size, prog.num_classes, prog.level_size, prog.level_anchors, prog)
        times = {k: [] for k in libs}
        for k, lib in libs.items():
            create_ms(lib, d)
        for _ in range(a.n):
            for k, lib in libs.items():
                times[k].append(round(create_ms(lib, d), 3))
        res["models"][name] = {k: {"ms": v, "median_ms": statistics.median(v), "spread_ms": round(max(v) - min(v), 3)}
                               for k, v in times.items()}
        print(name, json.dumps(res["models"][name]))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
