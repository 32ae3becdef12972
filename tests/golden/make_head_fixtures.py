#!/usr/bin/env python3
"""Generate tests/golden/head_train.npz by RUNNING THE REFERENCE's own make_head, init_detect_bias and
YOLOLiteMS._forward_head (scripts/model/model_v2.py of the reference checkout, imported unmodified; pure torch, CPU),
forward and backward, in fp32 and in fp64 on the SAME fp32-valued inputs.

    python tests/golden/make_head_fixtures.py --reference /path/to/YoloLite-Official-Repo [--wide]

--wide writes head_train_wide.npz (the WIDE cases: their tensors only, no `keys`, no `e2e/losses`) and leaves
head_train.npz alone.

model_v2.py imports timm at module level and uses it only in the model constructors; an empty module named timm is
placed in sys.modules first.  Inputs come from the seeds of tests/_head_cases.py; the archive's layout is described
there.  Also stored: `keys` (name, shape, dtype of every state_dict entry of three reference heads, the list
DetectHeads is held to) and `e2e/losses`, the float64 CPU loop of the end-to-end test (tests/_head_np.py).

Admission rule, asserted for every case, level and block (none is dropped; change the seed and say so here): the ReLU
masks of the fp32 and the fp64 run are identical, and the smallest |BatchNorm output| of the fp64 run is at least 1e-5
and at least 64 x the fp32 run's error in that tensor -- otherwise a case pins a ReLU tie."""
import argparse
import importlib.util
import json
import os
import sys
import types

os.environ["PYTHONDONTWRITEBYTECODE"] = "1"
sys.dont_write_bytecode = True
import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
from _head_cases import (CASES, E2E, FIXTURE, FIXTURE_WIDE, WIDE, case_inputs, modes, stored_indices,  # noqa: E402
                         tensor_shapes)
from _head_np import fit_reference  # noqa: E402

OUT = os.environ.get("YL_FIXTURE_OUT") or HERE


def load_reference(root):
    sys.modules.setdefault("timm", types.ModuleType("timm"))
    spec = importlib.util.spec_from_file_location("ref_model_v2", os.path.join(root, "scripts", "model", "model_v2.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def run_reference(mod, case, lv, train, dtype):
    """one level through the reference's modules -> {tensor name: array}, BatchNorm outputs per block"""
    F, C, A, depth, k = case["F"], case["C"], case["A"], case["depth"], lv["k"]
    head = mod.make_head(A, depth, C, F)
    mod.init_detect_bias(head, C)
    head = head.to(dtype)
    pre = f"head{k}."
    sd = {n[len(pre):]: torch.from_numpy(np.asarray(v)) for n, v in {**lv["params"], **lv["buffers"]}.items()}
    head.load_state_dict({n: v.to(dtype) if v.dtype.is_floating_point else v for n, v in sd.items()}, strict=True)
    head.train(train)
    bn_out = []
    hooks = [blk.block[2].register_forward_hook(lambda m, i, o: bn_out.append(o.detach().clone()))
             for blk in head["trunk"]]
    x = torch.from_numpy(lv["x"]).to(dtype).permute(0, 3, 1, 2).contiguous().requires_grad_(True)
    y = mod.YOLOLiteMS._forward_head(types.SimpleNamespace(num_classes=C), x, head, A)
    y.backward(torch.from_numpy(lv["gy"]).to(dtype))
    for h in hooks:
        h.remove()
    out = {"y": y.detach().numpy(), "dx": x.grad.permute(0, 2, 3, 1).contiguous().numpy()}
    for t, blk in enumerate(head["trunk"]):
        bn = blk.block[2]
        out[f"running_mean.{t}"] = bn.running_mean.numpy().copy()
        out[f"running_var.{t}"] = bn.running_var.numpy().copy()
        out[f"num_batches_tracked.{t}"] = bn.num_batches_tracked.numpy().copy()
    for n, p in head.named_parameters():
        out["g." + pre + n] = p.grad.numpy()
    return out, [b.numpy() for b in bn_out]


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
            for li, lv in enumerate(inputs):
                r32, bn32 = run_reference(mod, case, lv, mode == "train", torch.float32)
                r64, bn64 = run_reference(mod, case, lv, mode == "train", torch.float64)
                for t, (b32, b64) in enumerate(zip(bn32, bn64)):       # admission rule: change the seed, say so above
                    margin, err = np.abs(b64).min(), np.abs(b32.astype(np.float64) - b64).max()
                    assert np.array_equal(b32 > 0, b64 > 0), (case["name"], mode, li, t, "ReLU masks differ")
                    assert margin >= 1e-5 and margin >= 64 * err, (case["name"], mode, li, t, margin, err)
                key = f"{case['name']}/{mode}/L{li}"
                vals, e32s, m64s = [], [], []
                shapes = tensor_shapes(case, lv["k"], lv["S"])
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
                print(f"{case['name']:6s} {mode:5s} L{li} S={lv['S']:2d}  min|bn|={min(np.abs(b).min() for b in bn64):.1e}  "
                      f"worst e32/max64={worst:.1e}")
    if not a.wide:
        # the key list DetectHeads is held to: three reference heads as YOLOLiteMS names them
        keys = []
        for k in (3, 4, 5):
            head = mod.make_head(1, 2, 3, 16)
            keys += [[f"head{k}.{n}", list(v.shape), str(v.dtype)] for n, v in head.state_dict().items()]
        arrays["keys"] = np.asarray(json.dumps(keys))
        losses = fit_reference(E2E, case_inputs(E2E))
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
