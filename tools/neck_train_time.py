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
import os
import sys

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

from tools import _train_time as tt  # noqa: E402

SHAPES = {"edge_n": dict(F=96, depth=1, Cin=(32, 48, 480), B=64, sizes=(80, 40, 20)),
          "edge_l": dict(F=320, depth=2, Cin=(64, 96, 960), B=32, sizes=(80, 40, 20))}


def torch_neck(F, depth, cins):
    """the reference's laterals, smooth blocks and top-down pass in torch (model_v2.py:23-39, 285-294, 337-361)"""
    import torch.nn.functional as TF
    from torch import nn

    class Neck(nn.Module):
        def __init__(self):
            super().__init__()
            for i, ci in enumerate(cins):
                setattr(self, f"lateral{3 + i}", nn.Conv2d(ci, F, 1))
            for i in range(len(cins)):
                setattr(self, f"smooth{3 + i}", tt.torch_block(F, depth))

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
    launches = lambda: sum(ours.last_launches().values())    # noqa: E731
    if not tt.time_sides(res, lambda: step(ours), lambda: step(ref), launches, blocks, steps, trace):
        return res
    ref64 = torch_neck(F, depth, cins).to(dev).double().train()
    ref64.load_state_dict(ours.state_dict())
    torch.autograd.backward(ref64([f.double() for f in feats_cl]), [g.double() for g in gps_cl])
    res.update(tt.grad_errors(ours, ref, ref64))
    return res


if __name__ == "__main__":
    tt.main("neck_train_time.py", "edge_n,edge_l", run_model)
