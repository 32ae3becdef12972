#!/usr/bin/env python3
"""Generate tests/golden/head_amp.npz by RUNNING THE REFERENCE's own make_head, init_detect_bias and
YOLOLiteMS._forward_head as make_head_fixtures.py does, with one change: the 1x1 convolutions of the heads make_head
builds (the trunk blocks' pointwise convolution and out.box / out.obj / out.cls) are made to compute
tests/_head_amp_cases.Rounded1x1 (x, W and dz rounded to fp16 / bf16, nearest even; the products of the rounded values
in the run's dtype; the bias and its gradient unrounded).  Everything else is the reference's modules, unmodified.

    python tests/golden/make_head_amp_fixtures.py --reference /path/to/YoloLite-Official-Repo

Per case, mode, precision and level: r64 (the float64 run), max64, and the flip allowance of tests/_head_amp_cases.py:
the largest max|r32_j - r64| over FLIP_RUNS fp32 runs with jittered rounding inputs.

Admission rule (that of make_head_fixtures.py), asserted for every case, mode, precision, level and block: the ReLU masks of
the plain fp32 run and of the float64 run of the rounded model are identical, and the smallest |BatchNorm output| of the
float64 run is at least 1e-5 and at least 64 x the plain fp32 run's error in that tensor -- otherwise a case pins a ReLU
tie.  Asserted besides: none of the FLIP_RUNS jittered runs has another ReLU mask than the float64 run (a flipped rounding
moves a BatchNorm output by far more than an fp32 error; a case in which that crosses zero would pin the tie after all).
bf16 rule, asserted for every case, mode and level.  A bf16 rounding flips once per 2^15 values and fp32 ulp of difference,
so the eight jittered runs of a small level often flip none, and its allowance is then a plain fp32 error that ONE flip
on another fp32 implementation exceeds a hundredfold.  The jitter is +-1 ulp of the value; two correct fp32 sums of the
depthwise 3x3 differ by far more where the nine terms cancel (hundreds of ulps of a small d), and the kernel's order is
not torch's.  So: a level whose jittered runs flipped no forward rounding must have no element of block 0's d that the
kernel's own order (_head_amp_cases.device_order_d, restated from csrc/yl_block.h) rounds to another bf16 value than the
float64 d.  (fp16 flips eight times as often: its allowances see flips wherever the shapes are large enough to matter.)
A case that fails any rule gets another seed in tests/_head_amp_cases.py."""
import argparse
import os
import sys

os.environ["PYTHONDONTWRITEBYTECODE"] = "1"
sys.dont_write_bytecode = True
import numpy as np
import torch
from torch import nn

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
from _head_amp_cases import (AMP_CASES, FLIP_RUNS, FLIP_SEED, FORWARD_FLIPS, PRECISIONS, Rounded1x1, amp_modes,  # noqa: E402
                             d_flips)
from _head_cases import case_inputs, stored_indices, tensor_shapes  # noqa: E402
from make_head_fixtures import load_reference, run_reference  # noqa: E402

OUT = os.environ.get("YL_FIXTURE_OUT") or HERE


class Rounded:
    """the reference's module with make_head's 1x1 convolutions computing Rounded1x1; every other name is the reference's"""

    def __init__(self, mod, precision, jitter=None):
        self._mod, self._precision, self._jitter = mod, precision, jitter

    def __getattr__(self, name):
        return getattr(self._mod, name)

    def make_head(self, *args, **kw):
        head = self._mod.make_head(*args, **kw)
        n = 0
        for layer in head.modules():
            if isinstance(layer, nn.Conv2d) and layer.kernel_size == (1, 1):
                assert layer.padding == (0, 0) and layer.stride == (1, 1) and layer.groups == 1
                layer.forward = (lambda x, layer=layer: Rounded1x1.apply(x, layer.weight, layer.bias, self._precision, self._jitter))
                n += 1
        assert n == len(head["trunk"]) + 3, n
        return head


def level_run(mod, case, lv, li, mode, precision):
    """-> (r64 {name: array}, flip {name: float}, BatchNorm outputs of the float64 run); asserts the admission rule"""
    train = mode == "train"
    tag = (case["name"], mode, precision, li)
    r64, bn64 = run_reference(Rounded(mod, precision), case, lv, train, torch.float64)
    _, bn32 = run_reference(Rounded(mod, precision), case, lv, train, torch.float32)
    for t, (b32, b64) in enumerate(zip(bn32, bn64)):           # admission rule: change the seed in _head_amp_cases.py
        margin, err = np.abs(b64).min(), np.abs(b32.astype(np.float64) - b64).max()
        assert np.array_equal(b32 > 0, b64 > 0), tag + (t, "ReLU masks differ")
        assert margin >= 1e-5 and margin >= 64 * err, tag + (t, margin, err)
    flips = {n: 0.0 for n in r64}
    FORWARD_FLIPS["n"] = 0
    for j in range(FLIP_RUNS):
        g = torch.Generator().manual_seed(FLIP_SEED + j)
        r32, bn32 = run_reference(Rounded(mod, precision, g), case, lv, train, torch.float32)
        for n in r64:
            flips[n] = max(flips[n], float(np.abs(r32[n].astype(np.float64) - r64[n]).max()))
        for t, (b32, b64) in enumerate(zip(bn32, bn64)):
            assert np.array_equal(b32 > 0, b64 > 0), tag + (t, "ReLU masks differ in jittered run", j)
    if precision == "bf16" and FORWARD_FLIPS["n"] == 0:       # the bf16 rule: the allowance saw no flip, so d must not have one
        assert d_flips(lv, precision) == 0, tag + ("the kernel's order of the depthwise sum flips a rounding of d",)
    return r64, flips, bn64


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="checkout of the reference repository")
    a = ap.parse_args()
    mod = load_reference(a.reference)
    arrays = {}
    for case in AMP_CASES:
        inputs = case_inputs(case)
        for mode in amp_modes(case):
            for precision in PRECISIONS:
                for li, lv in enumerate(inputs):
                    r64, flips, bn64 = level_run(mod, case, lv, li, mode, precision)
                    key = f"{case['name']}/{mode}/{precision}/L{li}"
                    vals, fl, m64s = [], [], []
                    shapes = tensor_shapes(case, lv["k"], lv["S"])
                    assert set(shapes) == set(r64), sorted(set(shapes) ^ set(r64))
                    for n, shape in shapes.items():
                        v64 = r64[n]
                        assert v64.shape == tuple(shape), (n, v64.shape, shape)
                        fl.append(flips[n])
                        m64s.append(np.abs(v64).max())
                        flat = v64.reshape(-1).astype(np.float64)
                        idx = stored_indices(f"{case['name']}/{mode}/L{li}", n, shape)
                        vals.append(flat if idx is None else flat[idx])
                    arrays[key + "/r64"] = np.concatenate(vals)
                    arrays[key + "/flip"] = np.asarray(fl, np.float64)
                    arrays[key + "/max64"] = np.asarray(m64s, np.float64)
                    worst = max(f / max(m, 1e-300) for f, m in zip(fl, m64s))
                    print(f"{case['name']:6s} {mode:5s} {precision} L{li} S={lv['S']:2d}  min|bn|={min(np.abs(b).min() for b in bn64):.1e}  "
                          f"worst flip/max64={worst:.1e}")
    path = os.path.join(OUT, "head_amp.npz")
    np.savez_compressed(path, **arrays)
    print(path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < (1 << 20)


if __name__ == "__main__":
    main()
