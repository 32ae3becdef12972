#!/usr/bin/env python3
"""Time the detection heads' forward + backward (yololite_amd.DetectHeads, csrc/yl_head.hip) against the same module
in torch -- nn.Conv2d / nn.BatchNorm2d / nn.ReLU built here as the reference's make_head builds them, channels-last
input, same weights -- in one process on one device.

Shapes: edge_n (F 96, head_depth 1, batch 64, levels 80 / 40 / 20) and yololite_m (F 328, head_depth 2, batch 32),
80 classes, one anchor.  One step = train-mode forward of the three levels on fixed feature maps that do not require
grad, backward from fixed level-tensor gradients into every parameter.

Block protocol: --blocks times, alternating the two sides, each block = synchronise, --steps steps, synchronise, host
clock around it.  Per side: median and minimum over the blocks of the time per step.  Prints one JSON line, with the
launches per step of the device side and an estimate of the bytes its kernels read and write per step.

With --parity F the cases of tests/_head_cases.py are run and device error, bar and ratio of every tensor are written
to F.  With --trace only --steps steps per side are run once (for `rocprofv3 --kernel-trace --stats -- python
tools/head_train_time.py --trace ...`).

--precision fp16 | bf16: the device side is DetectHeads(precision=...), the torch side the same module under
torch.autocast of that dtype (its parameters stay fp32, as the reference trains); the line names the mode on both sides.
The gradient errors are against the unrounded float64 module in every mode: in a reduced one they show the rounding.

    python tools/head_train_time.py [--models edge_n,yololite_m] [--blocks 7] [--steps 20] [--out F] [--parity F] [--trace]
                                    [--precision fp32|fp16|bf16]"""
import contextlib
import json
import os
import sys

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

from tools import _train_time as tt  # noqa: E402

SHAPES = {"edge_n": dict(F=96, depth=1, B=64, sizes=(80, 40, 20)), "yololite_m": dict(F=328, depth=2, B=32, sizes=(80, 40, 20))}
NC, A = 80, 1
PRECISIONS = ("fp32", "fp16", "bf16")


def take_precision(argv):
    """--precision P (or --precision=P) out of argv -> P; the rest of the command line is tools/_train_time.py's"""
    p = "fp32"
    for i, v in enumerate(argv):
        if v == "--precision" and i + 1 < len(argv):
            p = argv[i + 1]
            del argv[i:i + 2]
            break
        if v.startswith("--precision="):
            p = v.split("=", 1)[1]
            del argv[i]
            break
    if p not in PRECISIONS:
        raise SystemExit(f"--precision must be one of {PRECISIONS}, got {p!r}")
    return p


PRECISION = "fp32"


def torch_heads(F, depth, nlevels):
    """the reference's make_head per level, in torch (model_v2.py:23-53), and its _forward_head (:182-192)"""
    import torch
    from torch import nn

    class Heads(nn.Module):
        def __init__(self):
            super().__init__()
            for i in range(nlevels):
                setattr(self, f"head{3 + i}", nn.ModuleDict({
                    "trunk": nn.Sequential(*[tt.torch_block(F, 1) for _ in range(depth)]),
                    "out": nn.ModuleDict({"box": nn.Conv2d(F, A * 4, 1), "obj": nn.Conv2d(F, A, 1),
                                          "cls": nn.Conv2d(F, A * NC, 1)})}))

        def forward(self, feats):
            outs = []
            for i, p in enumerate(feats):
                h = getattr(self, f"head{3 + i}")
                p = h["trunk"](p)
                box, obj, cls = h["out"]["box"](p), h["out"]["obj"](p), h["out"]["cls"](p)
                B, _, S, _ = box.shape
                out = torch.cat([box.view(B, A, 4, S, S), obj.view(B, A, 1, S, S), cls.view(B, A, NC, S, S)], dim=2)
                outs.append(out.permute(0, 1, 3, 4, 2).contiguous())
            return outs

    return Heads()


def run_model(name, blocks, steps, trace):
    import torch
    import yololite_amd as ya
    from yololite_amd import headops
    sh = SHAPES[name]
    F, depth, B, sizes = sh["F"], sh["depth"], sh["B"], sh["sizes"]
    dev = "cuda:0"
    torch.manual_seed(3)
    ours = ya.DetectHeads(F, NC, A, depth, precision=PRECISION).to(dev).train()
    ref = torch_heads(F, depth, len(sizes)).to(dev).to(memory_format=torch.channels_last).train()
    ref.load_state_dict(ours.state_dict())
    gen = torch.Generator().manual_seed(5)
    feats = [torch.randn(B, S, S, F, generator=gen).to(dev) for S in sizes]                  # NHWC
    feats_cl = [f.permute(0, 3, 1, 2) for f in feats]                                        # the same memory, NCHW shape
    gys = [(1e-3 * torch.randn(B, A, S, S, 5 + NC, generator=gen)).to(dev) for S in sizes]

    cast = {"fp16": torch.float16, "bf16": torch.bfloat16}.get(PRECISION)

    def step(m, x):
        for p in m.parameters():
            p.grad = None
        if m is ours:
            ys = m(x, layout="nhwc")
        else:                                              # the level tensors come out in the autocast dtype: gys follow
            with torch.autocast("cuda", dtype=cast) if cast else contextlib.nullcontext():
                ys = m(x)
        torch.autograd.backward(ys, gys if m is ours or not cast else [g.to(y.dtype) for g, y in zip(gys, ys)])

    plans = [headops.plan(F, NC, A, depth, B, S) for S in sizes]
    saved = sum(p["saved_bytes"] for p in plans)
    act = sum(4 * p["rows"] * F for p in plans)
    res = {"model": name, "device_precision": PRECISION, "torch_autocast": PRECISION if cast else "off", "F": F, "head_depth": depth, "batch": B, "sizes": list(sizes), "steps_per_block": steps,
           "saved_bytes": saved, "workspace_bytes": sum(p["workspace_bytes"] for p in plans),
           # activation-sized tensors (M x F fp32) read or written per block: forward 7 (depthwise 2, 1x1 2, statistics 1,
           # normalisation 2), backward 20 (dh 1, its two sums 3, dz 4, 1x1 weight gradient 2, dd 2, depthwise weight
           # gradient 6 over its three tap rows, and the output convolutions' 2 reads of h counted once per level below),
           # the input gradient of every block but the first 2; the level tensor is written once and its gradient read twice
           "bytes_moved_estimate": act * (27 * depth + 2 * (depth - 1) + 2) + 3 * sum(4 * p["rows"] * A * (5 + NC) for p in plans)}
    launches = lambda: sum(l["forward"] + l["backward"] for l in ours.last_launches())    # noqa: E731
    if not tt.time_sides(res, lambda: step(ours, feats), lambda: step(ref, feats_cl), launches, blocks, steps, trace):
        return res
    ref64 = torch_heads(F, depth, len(sizes)).to(dev).double().train()
    ref64.load_state_dict(ours.state_dict())
    # A BatchNorm output within fp32 rounding of zero gets another ReLU mask in fp32 than in float64.  One such element
    # moves one row of a weight gradient by one row's term, 1 / sqrt(M) of an entry that sums M random-signed terms:
    # the largest error shows it, the L2 error does not.  Counted here for the torch side, whose masks a hook can see.
    masks = {}
    def keep(tag):
        return lambda mod, i, o: masks.setdefault(tag, []).append(o > 0)
    bns = lambda m: [b for b in m.modules() if isinstance(b, torch.nn.BatchNorm2d)]      # noqa: E731
    hooks = [b.register_forward_hook(keep(t)) for t, m in (("f32", ref), ("f64", ref64)) for b in bns(m)]
    with torch.no_grad():
        ref(feats_cl)
    torch.autograd.backward(ref64([f.double() for f in feats_cl]), [g.double() for g in gys])
    for h in hooks:
        h.remove()
    flips = sum(int((a != b).sum()) for a, b in zip(masks["f32"], masks["f64"]))
    elements = sum(a.numel() for a in masks["f64"])
    del masks
    res.update(tt.grad_errors(ours, ref, ref64, between=True))
    at = res["device_max_rel_grad_error_at"]
    # of the device's worst gradient: how many of its rows (output channels) carry an error above 1e-4 of its largest entry
    pw, rw = dict(ours.named_parameters())[at].grad.double(), dict(ref64.named_parameters())[at].grad
    rows_off = int((((pw - rw).abs().reshape(pw.shape[0], -1).amax(1) / rw.abs().max()) > 1e-4).sum())
    del ref64
    res.update({"device_worst_gradient_rows_above_1e-4": rows_off, "device_worst_gradient_rows": int(pw.shape[0]),
                "torch_relu_masks_differing_from_float64": flips, "batchnorm_outputs": elements})
    return res


def parity(path):
    import numpy as np
    import _head_cases as hc
    import _head_dev as t
    z = np.load(hc.FIXTURE)
    rows, worst = [], (0.0, "")
    for case in hc.CASES:
        for mode in hc.modes(case):
            for (li, n), (err, b) in t.parity_ratios(case, mode, z).items():
                rows.append({"case": case["name"], "mode": mode, "level": li, "tensor": n, "error": err, "bar": b,
                             "ratio": round(err / b, 4)})
                worst = max(worst, (err / b, f"{case['name']}/{mode}/L{li}/{n}"))
    with open(path, "w") as f:
        json.dump(rows, f, indent=1)
    return {"worst_ratio": round(worst[0], 4), "at": worst[1], "tensors": len(rows)}


if __name__ == "__main__":
    PRECISION = take_precision(sys.argv)
    tt.main("head_train_time.py", "edge_n,yololite_m", run_model, header={"num_classes": NC, "precision": PRECISION},
            parity=parity)
