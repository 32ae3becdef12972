#!/usr/bin/env python3
"""Time the FPN neck's forward + backward (yololite_amd.DetectNeck, csrc/yl_neck.hip) against the same module in torch
-- nn.Conv2d laterals, F.interpolate(mode="nearest") + add, nn.Conv2d / nn.BatchNorm2d / nn.ReLU smooth blocks built
here as the reference's YOLOLiteMS_CPU builds them, channels-last input, same weights -- in one process on one device.

Shapes: edge_n (F 96, depth 1, input channels 32 / 48 / 480, batch 64, levels 80 / 40 / 20) and edge_l (F 320, depth 2,
input channels 64 / 96 / 960, batch 32).  One step = train-mode forward of the neck on fixed feature maps that do not
require grad, backward from fixed gradients of p3, p4, p5 into every parameter.

Block protocol: --blocks times, alternating the two sides, each block = synchronise, --steps steps, synchronise, host
clock around it.  Per side: median and minimum over the blocks of the time per step.  Prints one JSON line, with the
launches per step of the device side, what yl_neck_plan says the handle holds, and an estimate of the bytes its
kernels read and write per step.

With --trace only --steps steps per side are run once (for `rocprofv3 --kernel-trace --stats -- python
tools/neck_train_time.py --trace ...`).

    python tools/neck_train_time.py [--models edge_n,edge_l] [--blocks 7] [--steps 20] [--out F] [--trace]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

SHAPES = {"edge_n": dict(F=96, depth=1, Cin=(32, 48, 480), B=64, sizes=(80, 40, 20)),
          "edge_l": dict(F=320, depth=2, Cin=(64, 96, 960), B=32, sizes=(80, 40, 20))}


def torch_neck(F, depth, cins):
    """the reference's laterals, smooth blocks and top-down pass in torch (model_v2.py:23-39, 285-294, 337-361)"""
    import torch.nn.functional as TF
    from torch import nn

    class Block(nn.Module):
        def __init__(self):
            super().__init__()
            layers = []
            for _ in range(depth):
                layers += [nn.Conv2d(F, F, 3, padding=1, groups=F, bias=False), nn.Conv2d(F, F, 1, bias=False),
                           nn.BatchNorm2d(F), nn.ReLU(inplace=True)]
            self.block = nn.Sequential(*layers)

        def forward(self, x):
            return self.block(x)

    class Neck(nn.Module):
        def __init__(self):
            super().__init__()
            for i, ci in enumerate(cins):
                setattr(self, f"lateral{3 + i}", nn.Conv2d(ci, F, 1))
            for i in range(len(cins)):
                setattr(self, f"smooth{3 + i}", Block())

        def forward(self, feats):
            ps, prev = [None] * len(feats), None
            for i in range(len(feats) - 1, -1, -1):
                t = getattr(self, f"lateral{3 + i}")(feats[i])
                if prev is not None:
                    t = TF.interpolate(prev, size=t.shape[-2:], mode="nearest") + t
                prev = ps[i] = getattr(self, f"smooth{3 + i}")(t)
            return ps

    return Neck()


def run_model(name, blocks, steps, trace):
    import numpy as np
    import torch
    import yololite_amd as ya
    from yololite_amd import neckops
    sh = SHAPES[name]
    F, depth, cins, B, sizes = sh["F"], sh["depth"], sh["Cin"], sh["B"], sh["sizes"]
    dev = "cuda:0"
    torch.manual_seed(3)
    ours = ya.DetectNeck(cins, F, depth).to(dev).train()
    ref = torch_neck(F, depth, cins).to(dev).to(memory_format=torch.channels_last).train()
    ref.load_state_dict(ours.state_dict())
    gen = torch.Generator().manual_seed(5)
    feats = [torch.randn(B, S, S, ci, generator=gen).to(dev) for S, ci in zip(sizes, cins)]       # NHWC
    feats_cl = [f.permute(0, 3, 1, 2) for f in feats]                                             # the same memory, NCHW shape
    gps = [(1e-3 * torch.randn(B, S, S, F, generator=gen)).to(dev) for S in sizes]
    gps_cl = [g.permute(0, 3, 1, 2) for g in gps]

    def step(m):
        for p in m.parameters():
            p.grad = None
        if m is ours:
            torch.autograd.backward(m(feats, layout="nhwc"), gps)
        else:
            torch.autograd.backward(m(feats_cl), gps_cl)

    def block(m, n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            step(m)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / n

    plan = neckops.plan(cins, F, depth, B, sizes)
    rows = [lp["rows"] for lp in plan["levels"]]
    act = sum(4 * M * F for M in rows)
    cact = sum(4 * M * ci for M, ci in zip(rows, cins))
    res = {"model": name, "F": F, "depth": depth, "in_channels": list(cins), "batch": B, "sizes": list(sizes),
           "steps_per_block": steps, "saved_bytes": plan["saved_bytes"], "workspace_bytes": plan["workspace_bytes"],
           # activation-sized tensors (M x F fp32) read or written per block: forward 7, backward 20 and 2 for the input
           # gradient of every block (tools/head_train_time.py counts them).  Per level besides, 8: t written 1, p copied
           # out of the handle 2, G = gp + gathered gt (read 2, written 1; the finer level's gt is charged to this
           # level's size, the finest level has none), gt read by the lateral's weight and bias gradient 2; the
           # coarser p read by the lateral's epilogue is a quarter and left out.  The feature maps (M x Cin) are read by
           # the lateral and by its weight gradient; no dc is asked for.
           "bytes_moved_estimate": act * (29 * depth + 8) + 2 * cact}
    if trace:
        block(ours, steps); block(ref, steps)
        res["launches_per_step"] = sum(ours.last_launches().values())
        return res
    for _ in range(2):
        block(ours, 3); block(ref, 3)
    to, tr = [], []
    for _ in range(blocks):
        to.append(block(ours, steps)); tr.append(block(ref, steps))
    # same weights, same inputs: both sides against the torch module in float64, one step (largest error over the
    # parameter gradients, relative to the gradient's largest element; and the L2 error, which a flipped ReLU mask of
    # a BatchNorm output within fp32 rounding of zero does not dominate)
    ref64 = torch_neck(F, depth, cins).to(dev).double().train()
    ref64.load_state_dict(ours.state_dict())
    torch.autograd.backward(ref64([f.double() for f in feats_cl]), [g.double() for g in gps_cl])
    worst, worst_t, l2, l2_t = (0.0, ""), (0.0, ""), 0.0, 0.0
    for (n, p), q, r in zip(ours.named_parameters(), ref.parameters(), ref64.parameters()):
        m = r.grad.abs().max().clamp_min(1e-300)
        worst = max(worst, (float((p.grad.double() - r.grad).abs().max() / m), n))
        worst_t = max(worst_t, (float((q.grad.double() - r.grad).abs().max() / m), n))
        l2 = max(l2, float((p.grad.double() - r.grad).norm() / r.grad.norm().clamp_min(1e-300)))
        l2_t = max(l2_t, float((q.grad.double() - r.grad).norm() / r.grad.norm().clamp_min(1e-300)))
    del ref64
    res.update({"blocks": blocks, "launches_per_step": sum(ours.last_launches().values()),
                "device_ms": round(float(np.median(to)), 4), "device_ms_min": round(float(np.min(to)), 4),
                "torch_ms": round(float(np.median(tr)), 4), "torch_ms_min": round(float(np.min(tr)), 4),
                "ratio": round(float(np.median(tr)) / float(np.median(to)), 3),
                "device_ms_blocks": [round(v, 4) for v in to], "torch_ms_blocks": [round(v, 4) for v in tr],
                "device_max_rel_grad_error_vs_float64": worst[0], "device_max_rel_grad_error_at": worst[1],
                "torch_max_rel_grad_error_vs_float64": worst_t[0], "torch_max_rel_grad_error_at": worst_t[1],
                "device_max_rel_l2_grad_error_vs_float64": l2, "torch_max_rel_l2_grad_error_vs_float64": l2_t})
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--models", default="edge_n,edge_l")
    ap.add_argument("--blocks", type=int, default=7)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--out", default="")
    ap.add_argument("--trace", action="store_true")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("neck_train_time.py needs a HIP device")
    res = {"gpu": torch.cuda.get_device_name(0), "runs": []}
    for name in [m for m in args.models.split(",") if m]:
        res["runs"].append(run_model(name, args.blocks, args.steps, args.trace))
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
