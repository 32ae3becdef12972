#!/usr/bin/env python3
"""Generate tests/golden/dense_neck_train.npz by RUNNING THE REFERENCE's own YOLOLiteMS.forward (scripts/model/model_v2.py
of the reference checkout, imported unmodified; pure torch, CPU), forward and backward, in fp32 and in fp64 on the SAME
fp32-valued inputs.

    python tests/golden/make_dense_neck_fixtures.py --reference /path/to/YoloLite-Official-Repo [--wide]

--wide writes dense_neck_train_wide.npz (the WIDE cases: their tensors only, no `keys`, no `e2e/losses`) and leaves
dense_neck_train.npz alone.

As make_neck_fixtures.py: an empty module named timm is placed in sys.modules first (model_v2.py imports timm at module
level and uses it only in the constructors), and the model is made without its constructor (__new__ +
nn.Module.__init__): nn.Conv2d laterals, the reference's own conv_block(F, F, n=d) smooth blocks, make_head heads and a
stub backbone that returns the case's feature maps are attached, use_p6 = False, and forward() is called.  p_k is taken
from forward hooks on smooth<k>, and sum <p_k, gp_k> is backpropagated.  A case of two levels runs as p4 / p5 with a
dummy p3 whose gradient is zero.  Inputs come from the seeds of tests/_dense_neck_cases.py; the archive's layout is
described there.  SiLU has no ties: no admission rule."""
import argparse
import json
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
from _dense_neck_cases import (CASES, E2E, FIXTURE, FIXTURE_WIDE, KEYS, WIDE, case_inputs, head_inputs, modes,  # noqa: E402
                               stored_indices, tensor_shapes)
from _dense_neck_np import fit_reference  # noqa: E402
from make_neck_fixtures import _Feats, load_reference  # noqa: E402

OUT = os.environ.get("YL_FIXTURE_OUT") or HERE


def build_reference(mod, F, depth, cins, ks, dtype):
    """a YOLOLiteMS without its constructor: the neck of levels `ks` (input channels `cins`) and one-anchor heads"""
    m = mod.YOLOLiteMS.__new__(mod.YOLOLiteMS)
    nn.Module.__init__(m)
    m.use_p2, m.use_p6 = 2 in ks, False
    m.num_classes, m.num_anchors_per_level = 1, (1,) * len(ks)
    m.export_concat = m.export_decode = False
    rest = [(k, ci) for k, ci in zip(ks, cins) if k != 2]
    if 2 in ks:                                              # the constructor's order (model_v2.py:115-127)
        m.lateral2 = nn.Conv2d(cins[0], F, 1)
    for k, ci in rest:
        setattr(m, f"lateral{k}", nn.Conv2d(ci, F, 1))
    if 2 in ks:
        m.smooth2 = mod.conv_block(F, F, n=depth)
    for k, ci in rest:
        setattr(m, f"smooth{k}", mod.conv_block(F, F, n=depth))
    for k in ks:
        setattr(m, f"head{k}", mod.make_head(1, 1, 1, F))
    return m.to(dtype)


def run_reference(mod, case, inputs, train, dtype):
    """-> per level {tensor name: array}"""
    F, depth, B = case["F"], case["depth"], case["B"]
    ks = [lv["k"] for lv in inputs]
    dummy = len(ks) == 2                                     # p4, p5: forward() wants a c3 as well
    all_ks = ([3] if dummy else []) + ks
    m = build_reference(mod, F, depth, ([4] if dummy else []) + [lv["Cin"] for lv in inputs], all_ks, dtype)
    sd = {}
    for lv in inputs:
        sd.update(lv["params"]); sd.update(lv["buffers"])
    own = m.state_dict()
    assert all(n in own for n in sd), sorted(set(sd) - set(own))
    m.load_state_dict({n: torch.from_numpy(np.asarray(v)).to(own[n].dtype) for n, v in sd.items()}, strict=False)
    m.train(train)
    cs = [torch.from_numpy(lv["c"]).to(dtype).permute(0, 3, 1, 2).contiguous().requires_grad_(True) for lv in inputs]
    feats = list(cs)
    if dummy:
        S3 = 2 * inputs[0]["S"]
        feats.insert(0, torch.from_numpy(np.random.RandomState(1).standard_normal((B, 4, S3, S3))).to(dtype))
    m.backbone = _Feats(feats)
    ps, hooks = {}, []
    for k in ks:                                             # the SiLU is in place: the hook's output is the final tensor
        hooks.append(getattr(m, f"smooth{k}").register_forward_hook(lambda mod_, i, o, k=k: ps.__setitem__(k, o)))
    m(torch.zeros(B, 3, 8, 8, dtype=dtype))
    for h in hooks:
        h.remove()
    loss = sum((ps[lv["k"]] * torch.from_numpy(lv["gp"]).to(dtype).permute(0, 3, 1, 2)).sum() for lv in inputs)
    loss.backward()
    out = []
    named = dict(m.named_parameters())
    for lv, c in zip(inputs, cs):
        k = lv["k"]
        d = {"p": ps[k].detach().permute(0, 2, 3, 1).contiguous().numpy(),
             "dc": c.grad.permute(0, 2, 3, 1).contiguous().numpy()}
        sm = getattr(m, f"smooth{k}")
        for t in range(depth):
            bn = sm[3 * t + 1]
            d[f"running_mean.{t}"] = bn.running_mean.numpy().copy()
            d[f"running_var.{t}"] = bn.running_var.numpy().copy()
            d[f"num_batches_tracked.{t}"] = bn.num_batches_tracked.numpy().copy()
        for n in lv["params"]:
            d["g." + n] = named[n].grad.numpy()
        out.append(d)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="checkout of the reference repository")
    ap.add_argument("--wide", action="store_true", help="write the WIDE cases' file instead")
    a = ap.parse_args()
    mod = load_reference(a.reference)
    arrays = {}
    for case in (WIDE if a.wide else CASES):
        inputs = case_inputs(case)
        for mode in modes(case):
            r32s = run_reference(mod, case, inputs, mode == "train", torch.float32)
            r64s = run_reference(mod, case, inputs, mode == "train", torch.float64)
            for li, lv in enumerate(inputs):
                r32, r64 = r32s[li], r64s[li]
                key = f"{case['name']}/{mode}/L{li}"
                vals, e32s, m64s = [], [], []
                shapes = tensor_shapes(case, lv["k"], lv["S"], lv["Cin"])
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
                print(f"{case['name']:6s} {mode:5s} L{li} S={lv['S']:2d}  worst e32/max64={worst:.1e}")
    if not a.wide:
        # the key list DetectNeckMS is held to: the reference's names, shapes and dtypes of laterals and smooth blocks
        m = build_reference(mod, KEYS["F"], KEYS["depth"], KEYS["Cin"], [3, 4, 5], torch.float32)
        keys = [[n, list(v.shape), str(v.dtype)] for n, v in m.state_dict().items() if n.startswith(("lateral", "smooth"))]
        arrays["keys"] = np.asarray(json.dumps(keys))
        losses = fit_reference(E2E, case_inputs(E2E), head_inputs(E2E))
        drop = (losses[0] - losses[-1]) / losses[0]
        print("e2e losses", losses[0], "->", losses[-1], f"drop {100 * drop:.1f} %")
        assert drop >= 0.2, "the CPU loop's own drop must be at least 20 % of L0: choose another lr / batch"
        arrays["e2e/losses"] = losses
    path = os.path.join(OUT, os.path.basename(FIXTURE_WIDE if a.wide else FIXTURE))
    np.savez_compressed(path, **arrays)
    print(path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < (1 << 20)


if __name__ == "__main__":
    main()
