#!/usr/bin/env python3
"""Generate tests/golden/stem_train.npz from the oracle/backbones.py modules (ConvBnAct, FeatureBackbone; pure torch, CPU,
torch autograd), forward and backward, in fp32 and in float64 on the SAME fp32-valued inputs.

    python tests/golden/make_stem_fixtures.py [--wide] [--search]

--wide writes stem_train_wide.npz from the WIDE cases and leaves stem_train.npz alone.

Inputs come from the seeds of tests/_stem_cases.py; the archive's layout is described there.

Admission rule, asserted for every case, mode and ReLU (none is dropped; change the seed in _stem_cases.py and say so
there): the ReLU masks of the fp32 and the float64 run are identical, and the smallest |BatchNorm output| in front of the
ReLU in the float64 run is at least 64 x the fp32 run's error in that tensor -- otherwise a case pins a ReLU tie.
--search prints, per case of CASES and WIDE, the first seed of 101, 202, 303, ... that is admitted, and writes nothing."""
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
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from _stem_cases import (CASES, EPS, FIXTURE, FIXTURE_WIDE, TINY, WIDE, case_inputs, modes, stored_indices, tensor_shapes, tiny_inputs,  # noqa: E402
                         tiny_tensor_shapes, units)
from oracle.backbones import BatchNormAct2d, ConvBnAct, FeatureBackbone  # noqa: E402

OUT = os.environ.get("YL_FIXTURE_OUT") or HERE
torch.set_num_threads(1)                                   # the fp32 run's sums in one order, whatever the machine's cores


def oracle_stack(case):
    """-> (root module, the modules to run in order).  A case under `backbone.` is the oracle_tiny FeatureBackbone's own
    conv_stem / bn1 / stages 0 and 1; any other is ConvBnAct modules under units.{i}"""
    root = nn.Module()
    if case.get("prefix") == "backbone.":
        bb = FeatureBackbone("oracle_tiny")
        root.add_module("backbone", bb)
        last = max(int(u["conv"].split(".")[2]) for u in units(case) if ".blocks." in u["conv"])
        return root, [bb.conv_stem, bb.bn1] + [bb.blocks[i] for i in range(last + 1)]
    root.add_module("units", nn.Module())
    cin, run = case["cin"], []
    for i, u in enumerate(case["units"]):
        m = ConvBnAct(cin, u["c"], u["k"], u["s"], "relu", EPS, False)
        root.units.add_module(str(i), m)
        run.append(m)
        cin = u["c"]
    return root, run


def hook_relus(root, pre_relu):
    hooks = []
    for m in root.modules():
        if isinstance(m, BatchNormAct2d) and isinstance(m.act, nn.ReLU):
            m.act.inplace = False
            hooks.append(m.act.register_forward_hook(lambda mod, i, o: pre_relu.append(i[0].detach().clone())))
    return hooks


def load(root, inputs, dtype):
    sd = {n: torch.from_numpy(np.asarray(v)) for n, v in {**inputs["params"], **inputs["buffers"]}.items()}
    missing, unexpected = root.load_state_dict({n: v.to(dtype) if v.dtype.is_floating_point else v for n, v in sd.items()},
                                               strict=False)
    assert not unexpected, unexpected
    return set(sd)


def nhwc(t):
    return t.detach().permute(0, 2, 3, 1).contiguous().numpy()


def collect(root, own):
    out = {}
    for n, v in root.state_dict().items():
        if n in own and ("running_" in n or "num_batches" in n):
            out["b." + n] = v.numpy().copy()
    for n, p in root.named_parameters():
        if n in own:
            out["g." + n] = p.grad.numpy()
    return out


def run_oracle(case, inputs, train, dtype):
    """-> {tensor name: array}, [(BatchNorm output in front of a ReLU)] in running order"""
    root, run = oracle_stack(case)
    root = root.to(dtype)
    own = load(root, inputs, dtype)
    root.train(train)
    pre_relu = []
    hooks = hook_relus(root, pre_relu)
    x = torch.from_numpy(inputs["x"]).to(dtype).permute(0, 3, 1, 2).contiguous().requires_grad_(True)
    h = x
    for m in run:
        h = m(h)
    h.backward(torch.from_numpy(inputs["gy"]).to(dtype).permute(0, 3, 1, 2))
    for hk in hooks:
        hk.remove()
    out = {"y": nhwc(h)}
    if not case["planar"]:
        out["dx"] = nhwc(x.grad)
    out.update(collect(root, own))
    return out, [b.numpy() for b in pre_relu]


def run_tiny(inputs, dtype):
    """the whole oracle_tiny FeatureBackbone in train mode: loss = sum_k <c_k, g_k>"""
    root = nn.Module()
    bb = FeatureBackbone("oracle_tiny")
    root.add_module("backbone", bb)
    root = root.to(dtype)
    own = load(root, inputs, dtype)
    assert own == set(root.state_dict()), sorted(own ^ set(root.state_dict()))[:4]
    root.train(True)
    pre_relu = []
    hooks = hook_relus(root, pre_relu)
    x = torch.from_numpy(inputs["x"]).to(dtype).permute(0, 3, 1, 2).contiguous()
    c3, c4, c5 = bb(x)[-3:]
    loss = sum((c * torch.from_numpy(inputs[g]).to(dtype).permute(0, 3, 1, 2)).sum() for c, g in ((c3, "g3"), (c4, "g4"), (c5, "g5")))
    loss.backward()
    for hk in hooks:
        hk.remove()
    out = {"y.c3": nhwc(c3), "y.c4": nhwc(c4), "y.c5": nhwc(c5)}
    out.update(collect(root, own))
    return out, [b.numpy() for b in pre_relu]


def admitted(runner):
    r32, bn32 = runner(torch.float32)
    r64, bn64 = runner(torch.float64)
    why = None
    for t, (b32, b64) in enumerate(zip(bn32, bn64)):
        margin, err = np.abs(b64).min(), np.abs(b32.astype(np.float64) - b64).max()
        if not np.array_equal(b32 > 0, b64 > 0):
            why = (t, "ReLU masks differ")
        elif not margin >= 64 * err:
            why = (t, float(margin), float(err))
    return r32, r64, bn64, why


def runners(which=("cases", "wide")):
    """(case name, modes, seed -> {mode: runner(dtype)}, shapes, the case's own seed)"""
    for case in (CASES if "cases" in which else []) + (WIDE if "wide" in which else []):
        def make(seed, case=case):
            inputs = case_inputs(case, seed)
            return {mode: (lambda dt, mode=mode: run_oracle(case, inputs, mode == "train", dt)) for mode in modes(case)}
        yield case["name"], make, tensor_shapes(case), case["seed"]
    if "cases" in which:
        yield TINY["name"], (lambda seed: {"train": lambda dt: run_tiny(tiny_inputs(seed), dt)}), tiny_tensor_shapes(), TINY["seed"]


def search():
    for name, make, _, own in runners():
        for k in range(1, 400):
            seed = 101 * k
            if all(admitted(r)[3] is None for r in make(seed).values()):
                print(f"{name:14s} first admitted seed {seed}" + ("" if seed == own else f"   (the case says {own})"))
                break


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--search", action="store_true")
    ap.add_argument("--wide", action="store_true", help="write stem_train_wide.npz (the WIDE cases) instead")
    a = ap.parse_args()
    if a.search:
        return search()
    arrays = {}
    for name, make, shapes, seed in runners(("wide",) if a.wide else ("cases",)):
        for mode, runner in make(seed).items():
            r32, r64, bn64, why = admitted(runner)
            assert why is None, (name, mode, why)          # admission rule: change the seed in _stem_cases.py
            key = f"{name}/{mode}"
            vals, e32s, m64s = [], [], []
            assert set(shapes) == set(r64), sorted(set(shapes) ^ set(r64))
            for n, shape in shapes.items():
                v32, v64 = r32[n], r64[n]
                assert v32.shape == v64.shape == tuple(shape), (n, v64.shape, shape)
                e32s.append(np.abs(v32.astype(np.float64) - v64).max())
                m64s.append(np.abs(v64).max())
                flat = v64.reshape(-1).astype(np.float64)
                idx = stored_indices(key, n, shape)
                vals.append(flat if idx is None else flat[idx])
            arrays[key + "/r64"] = np.concatenate(vals)
            arrays[key + "/e32"] = np.asarray(e32s, np.float64)
            arrays[key + "/max64"] = np.asarray(m64s, np.float64)
            worst = max(e / max(m, 1e-300) for e, m in zip(e32s, m64s))
            print(f"{name:14s} {mode:5s} min|bn|={min(np.abs(b).min() for b in bn64):.1e}  worst e32/max64={worst:.1e}")
    path = os.path.join(OUT, os.path.basename(FIXTURE_WIDE if a.wide else FIXTURE))
    np.savez_compressed(path, **arrays)
    print(path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < (1 << 20)


if __name__ == "__main__":
    main()
