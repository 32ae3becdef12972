#!/usr/bin/env python3
"""Dump every tensor the trainable modules return on the module-level parity cases, and compare two such dumps bit by
bit: the training side's counterpart of `bench.py --dump-outputs`, for changes that must not move a bit.

    python tools/train_bits.py DIR            one forward + backward of every case -> DIR/<module>/<case>/<mode>/<precision>.npz
    python tools/train_bits.py --compare A B  exit status 0 only if both trees hold the same files with bitwise-equal arrays;
                                              prints the first difference otherwise

Cases: CASES + WIDE of tests/_head_cases.py, _neck_cases.py, _dense_neck_cases.py, _stage_cases.py and _stem_cases.py, and the
whole tiny backbone (_stem_cases.TINY), built and run by the builders and `run` functions of tests/_*_dev.py.  Every mode
of the case; fp32, and fp16 and bf16 where the module runs in them (all but the depthwise neck).  A file holds y (p), dx (dc), the BatchNorm buffers
and every gradient; the tensors of level k of a module with levels are named "<k>:<tensor>".  The cases are the fixtures'
tiny shapes: the whole dump takes seconds on the device."""
import os
import sys

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)


def modules():
    """-> [(module name, its precisions, cases, modes(case), case -> inputs, (case, inputs, train) -> module,
    (module, case, inputs) -> tensors)].  The depthwise neck has `.precision` and refuses all but fp32: it has no dense GEMM
    of its own"""
    import _dense_neck_cases as dc
    import _dense_neck_dev as dd
    import _head_cases as hc
    import _head_dev as hd
    import _neck_cases as nc
    import _neck_dev as nd
    import _stage_cases as sc
    import _stage_dev as sd
    import _stem_cases as tc
    import _stem_dev as td
    tiny = dict(name=tc.TINY["name"])
    one, amp = ("fp32",), ("fp32", "fp16", "bf16")
    return [
        ("heads", amp, hc.CASES + hc.WIDE, hc.modes, hc.case_inputs, hd.heads_of, lambda m, c, i: hd.run(m, i)),
        ("neck", one, nc.CASES + nc.WIDE, nc.modes, nc.case_inputs, nd.neck_of, lambda m, c, i: nd.run(m, i)),
        ("dense_neck", amp, dc.CASES + dc.WIDE, dc.modes, dc.case_inputs, dd.neck_of, lambda m, c, i: dd.run(m, i)),
        ("stage", amp, sc.CASES + sc.WIDE, sc.modes, sc.case_inputs, sd.stack_of, lambda m, c, i: sd.run(m, i)),
        ("stem", amp, tc.CASES + tc.WIDE, tc.modes, tc.case_inputs, td.stack_of, td.run),
        ("backbone", amp, [tiny], lambda c: ("train",), lambda c: tc.tiny_inputs(), lambda c, i, train: td.tiny_backbone(i),
         lambda m, c, i: td.run_tiny(m, i)),
    ]


def dump(out_dir):
    files = 0
    for name, precisions, cases, modes, inputs_of, module_of, run in modules():
        for case in cases:
            inputs = inputs_of(case)
            for mode in modes(case):
                for precision in precisions:
                    m = module_of(case, inputs, mode == "train")      # a fresh module: its buffers start at the case's
                    m.precision = precision
                    got = run(m, case, inputs)
                    if isinstance(got, dict):
                        flat = dict(got)
                    else:
                        flat = {f"{k}:{n}": v for k, d in enumerate(got) for n, v in d.items()}
                    d = os.path.join(out_dir, name, case["name"], mode)
                    os.makedirs(d, exist_ok=True)
                    np.savez(os.path.join(d, precision + ".npz"), **{n: v.numpy() for n, v in flat.items()})
                    files += 1
    print(f"{files} files under {out_dir}")
    return 0


def _files(root):
    return sorted(os.path.relpath(os.path.join(d, f), root) for d, _, fs in os.walk(root) for f in fs if f.endswith(".npz"))


def compare(a_dir, b_dir):
    fa, fb = _files(a_dir), _files(b_dir)
    if fa != fb or not fa:
        print("the two trees hold different files:", sorted(set(fa) ^ set(fb))[:5] if fa or fb else "none at all")
        return 1
    arrays = 0
    for f in fa:
        a, b = np.load(os.path.join(a_dir, f)), np.load(os.path.join(b_dir, f))
        if sorted(a.files) != sorted(b.files):
            print(f"{f}: different tensors: {sorted(set(a.files) ^ set(b.files))[:5]}")
            return 1
        for n in a.files:
            x, y = a[n], b[n]
            if x.dtype != y.dtype or x.shape != y.shape:
                print(f"{f}: {n}: {x.dtype}{x.shape} against {y.dtype}{y.shape}")
                return 1
            if x.tobytes() != y.tobytes():
                bad = np.flatnonzero(np.frombuffer(x.tobytes(), np.uint8) != np.frombuffer(y.tobytes(), np.uint8))
                i = int(bad[0]) // x.dtype.itemsize
                print(f"{f}: {n}: {len(np.unique(bad // x.dtype.itemsize))} of {x.size} elements differ, the first at "
                      f"{i}: {x.reshape(-1)[i]!r} against {y.reshape(-1)[i]!r}")
                return 1
            arrays += 1
    print(f"{len(fa)} files, {arrays} arrays: bitwise equal")
    return 0


if __name__ == "__main__":
    if len(sys.argv) == 4 and sys.argv[1] == "--compare":
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    if len(sys.argv) != 2 or sys.argv[1].startswith("-"):
        sys.exit(__doc__)
    sys.exit(dump(sys.argv[1]))
