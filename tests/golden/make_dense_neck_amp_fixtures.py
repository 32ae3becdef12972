#!/usr/bin/env python3
"""Generate tests/golden/dense_neck_amp.npz by RUNNING THE REFERENCE's own YOLOLiteMS.forward as
make_dense_neck_fixtures.py does, with one change: the 3x3 convolutions of the reference's conv_block are made to compute
tests/_dense_neck_amp_np.RoundedConv3x3 (x, W and dz rounded to fp16 / bf16, nearest even; the products of the rounded
values in the run's dtype).  Everything else is the reference's modules, unmodified.

    python tests/golden/make_dense_neck_amp_fixtures.py --reference /path/to/YoloLite-Official-Repo

Per case, mode, precision and level: r64 (the float64 run), max64, and the flip allowance of
tests/_dense_neck_amp_cases.py: the largest max|r32_j - r64| over FLIP_RUNS fp32 runs with jittered rounding inputs."""
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
from _dense_neck_amp_cases import AMP_CASES as CASES, AMP_PRECISIONS, FLIP_RUNS, FLIP_SEED, amp_stored_indices  # noqa: E402
from _dense_neck_amp_np import RoundedConv3x3  # noqa: E402
from _dense_neck_cases import case_inputs, modes, tensor_shapes  # noqa: E402
from make_dense_neck_fixtures import run_reference  # noqa: E402
from make_neck_fixtures import load_reference  # noqa: E402

OUT = os.environ.get("YL_FIXTURE_OUT") or HERE


class Rounded:
    """the reference's module with conv_block's 3x3 convolutions computing RoundedConv3x3; every other name is the reference's"""

    def __init__(self, mod, precision, jitter=None):
        self._mod, self._precision, self._jitter = mod, precision, jitter

    def __getattr__(self, name):
        return getattr(self._mod, name)

    def conv_block(self, *args, **kw):
        block = self._mod.conv_block(*args, **kw)
        for layer in block:
            if isinstance(layer, nn.Conv2d):
                assert layer.kernel_size == (3, 3) and layer.padding == (1, 1) and layer.bias is None and layer.groups == 1
                layer.forward = (lambda x, layer=layer: RoundedConv3x3.apply(x, layer.weight, self._precision, self._jitter))
        return block


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="checkout of the reference repository")
    a = ap.parse_args()
    mod = load_reference(a.reference)
    arrays = {}
    for case in CASES:
        inputs = case_inputs(case)
        for mode in modes(case):
            for precision in AMP_PRECISIONS:
                r64s = run_reference(Rounded(mod, precision), case, inputs, mode == "train", torch.float64)
                flips = None
                for j in range(FLIP_RUNS):
                    g = torch.Generator().manual_seed(FLIP_SEED + j)
                    r32s = run_reference(Rounded(mod, precision, g), case, inputs, mode == "train", torch.float32)
                    e = [{n: np.abs(r32[n].astype(np.float64) - r64[n]).max() for n in r64} for r32, r64 in zip(r32s, r64s)]
                    flips = e if flips is None else [{n: max(f[n], d[n]) for n in f} for f, d in zip(flips, e)]
                for li, lv in enumerate(inputs):
                    r64 = r64s[li]
                    key = f"{case['name']}/{mode}/{precision}/L{li}"
                    vals, fl, m64s = [], [], []
                    shapes = tensor_shapes(case, lv["k"], lv["S"], lv["Cin"])
                    assert set(shapes) == set(r64), sorted(set(shapes) ^ set(r64))
                    for n, shape in shapes.items():
                        v64 = r64[n]
                        assert v64.shape == tuple(shape), (n, v64.shape, shape)
                        fl.append(flips[li][n])
                        m64s.append(np.abs(v64).max())
                        flat = v64.reshape(-1).astype(np.float64)
                        idx = amp_stored_indices(f"{case['name']}/{mode}/L{li}", n, shape)
                        vals.append(flat if idx is None else flat[idx])
                    arrays[key + "/r64"] = np.concatenate(vals)
                    arrays[key + "/flip"] = np.asarray(fl, np.float64)
                    arrays[key + "/max64"] = np.asarray(m64s, np.float64)
                    worst = max(f / max(m, 1e-300) for f, m in zip(fl, m64s))
                    print(f"{case['name']:6s} {mode:5s} {precision} L{li} S={lv['S']:2d}  worst flip/max64={worst:.1e}")
    path = os.path.join(OUT, "dense_neck_amp.npz")
    np.savez_compressed(path, **arrays)
    print(path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < (1 << 20)


if __name__ == "__main__":
    main()
