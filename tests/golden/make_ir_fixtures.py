#!/usr/bin/env python3
"""Generate tests/golden/ir_train.npz from oracle.backbones.InvertedResidual (pure torch, CPU, torch autograd) with
same=True, act="relu6", eps=1e-3, forward and backward, in fp32 and in float64 on the SAME fp32-valued inputs.

    python tests/golden/make_ir_fixtures.py [--wide] [--search]

--wide writes ir_train_wide.npz from the WIDE cases and leaves ir_train.npz alone; without it only the CASES file is
written.  Inputs come from the seeds of tests/_ir_cases.py; the archive's layout is the stage fixture's and is described
there.

Admission rule, asserted for every case, mode and unit with a ReLU6 (none is dropped; change the seed in _ir_cases.py and
say so there): the fp32 and the float64 run agree on both masks, y > 0 and y < 6, and every BatchNorm output in front of
the ReLU6 is, in the float64 run, at least 64 x the fp32 run's error in that tensor away from 0 AND from 6 -- otherwise a
case pins a tie at one of the two kinks.
Coverage, asserted likewise (conditions on the inputs, not tolerances): in the float64 run every ReLU6 unit has at least
2 % of its outputs clamped at 6 and at least 10 % clamped at 0 -- a ReLU6 that is really a ReLU does not pass these cases.
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
from _ir_cases import CASES, EPS, FIXTURE, FIXTURE_WIDE, WIDE, case_inputs, modes, stored_indices, tensor_shapes, units  # noqa: E402
from oracle.backbones import InvertedResidual  # noqa: E402

OUT = os.environ.get("YL_FIXTURE_OUT") or HERE
MIN_AT_6, MIN_AT_0 = 0.02, 0.10


def oracle_stack(case):
    """the case's blocks as oracle modules under the case's key names"""
    root, cin = nn.Module(), case["cin"]
    for b in case["blocks"]:
        m = InvertedResidual(cin, b["c"], b["k"], b["s"], b["mid"] / cin, "relu6", EPS, True)
        assert m.conv_pw.out_channels == b["mid"], (b, m.conv_pw.out_channels)
        node = root
        parts = (case.get("prefix", "") + "blocks." + b["name"]).split(".")
        for p in parts[:-1]:
            if not hasattr(node, p):
                node.add_module(p, nn.Module())
            node = getattr(node, p)
        node.add_module(parts[-1], m)
        cin = b["c"]
    return root


def run_oracle(case, inputs, train, dtype):
    """-> {tensor name: array}, [(BatchNorm output in front of a ReLU6)] in running order"""
    root = oracle_stack(case).to(dtype)
    sd = {n: torch.from_numpy(np.asarray(v)) for n, v in {**inputs["params"], **inputs["buffers"]}.items()}
    root.load_state_dict({n: v.to(dtype) if v.dtype.is_floating_point else v for n, v in sd.items()}, strict=True)
    root.train(train)
    mods = dict(root.named_modules())
    pre_act, hooks = [], []
    for u in units(case):
        if u["act"]:
            bn = mods[u["key"] + u["bn"]]
            assert isinstance(bn.act, nn.ReLU6)
            hooks.append(bn.act.register_forward_hook(lambda m, i, o: pre_act.append(i[0].detach().clone())))
            bn.act.inplace = False
    x = torch.from_numpy(inputs["x"]).to(dtype).permute(0, 3, 1, 2).contiguous().requires_grad_(True)
    h = x
    for b in case["blocks"]:
        h = mods[case.get("prefix", "") + "blocks." + b["name"]](h)
    h.backward(torch.from_numpy(inputs["gy"]).to(dtype).permute(0, 3, 1, 2))
    for hk in hooks:
        hk.remove()
    out = {"y": h.detach().permute(0, 2, 3, 1).contiguous().numpy(), "dx": x.grad.permute(0, 2, 3, 1).contiguous().numpy()}
    for n, v in root.state_dict().items():
        if "running_" in n or "num_batches" in n:
            out["b." + n] = v.numpy().copy()
    for n, p in root.named_parameters():
        out["g." + n] = p.grad.numpy()
    return out, [b.numpy() for b in pre_act]


def admitted(case, inputs, mode):
    r32, bn32 = run_oracle(case, inputs, mode == "train", torch.float32)
    r64, bn64 = run_oracle(case, inputs, mode == "train", torch.float64)
    why = None
    for t, (b32, b64) in enumerate(zip(bn32, bn64)):
        err = np.abs(b32.astype(np.float64) - b64).max()
        margin = min(np.abs(b64).min(), np.abs(b64 - 6.0).min())
        at6, at0 = float((b64 >= 6).mean()), float((b64 <= 0).mean())
        if not (np.array_equal(b32 > 0, b64 > 0) and np.array_equal(b32 < 6, b64 < 6)):
            why = (case["name"], mode, t, "ReLU6 masks differ")
        elif not margin >= 64 * err:
            why = (case["name"], mode, t, "margin", float(margin), float(err))
        elif not (at6 >= MIN_AT_6 and at0 >= MIN_AT_0):
            why = (case["name"], mode, t, "coverage", at6, at0)
    return r32, r64, bn64, why


def search():
    for case in CASES + WIDE:
        for k in range(1, 1000):
            seed = 101 * k
            inputs = case_inputs(case, seed)
            whys = [admitted(case, inputs, mode)[3] for mode in modes(case)]
            if all(w is None for w in whys):
                print(f"{case['name']:14s} first admitted seed {seed}" + ("" if seed == case["seed"] else f"   (the case says {case['seed']})"),
                      flush=True)
                break
            if any(w is not None and w[3] == "coverage" for w in whys):
                print(f"{case['name']:14s} seed {seed}: {[w for w in whys if w is not None]}", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--search", action="store_true")
    ap.add_argument("--wide", action="store_true", help="write ir_train_wide.npz (the WIDE cases) instead")
    a = ap.parse_args()
    if a.search:
        return search()
    arrays = {}
    for case in (WIDE if a.wide else CASES):
        inputs = case_inputs(case)
        for mode in modes(case):
            r32, r64, bn64, why = admitted(case, inputs, mode)
            assert why is None, why                        # admission and coverage: change the seed in _ir_cases.py
            key = f"{case['name']}/{mode}"
            vals, e32s, m64s = [], [], []
            shapes = tensor_shapes(case)
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
            cov = [(round(float((b >= 6).mean()), 3), round(float((b <= 0).mean()), 3)) for b in bn64]
            print(f"{case['name']:14s} {mode:5s} worst e32/max64={worst:.1e}  (at 6, at 0) per ReLU6 unit {cov}")
    path = os.path.join(OUT, os.path.basename(FIXTURE_WIDE if a.wide else FIXTURE))
    np.savez_compressed(path, **arrays)
    print(path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < (1 << 20)


if __name__ == "__main__":
    main()
