#!/usr/bin/env python3
"""Time the dense FPN neck's forward + backward (yololite_amd.DetectNeckMS, csrc/yl_dneck.hip) against the same module in
torch -- nn.Conv2d laterals, F.interpolate(mode="nearest") + add, dense 3x3 nn.Conv2d / nn.BatchNorm2d / nn.SiLU smooth
blocks built here as the reference's YOLOLiteMS builds them, channels-last input, same weights -- in one process on one
device.

Shapes: yololite_n (F 196, depth 2, input channels 40 / 112 / 320, batch 32, levels 80 / 40 / 20) and yololite_m (F 328,
depth 2, input channels 48 / 120 / 352, batch 16).  One step = train-mode forward of the neck on fixed feature maps that
do not require grad, backward from fixed gradients of p3, p4, p5 into every parameter.

Block protocol (tools/_train_time.py): two short warm-up rounds of both sides, so that the torch side's kernel search is
not timed; then --blocks times, alternating the two sides, each block = synchronise, --steps steps, synchronise, host
clock around it.  Per side: median and minimum over the blocks of the time per step.  Prints one JSON line, with the
launches per step of the device side, what yl_dneck_plan says the handle holds, the convolution work per step, and the
gradient error of both sides against a float64 run of the torch module.

--precision fp16 | bf16: the device side runs DetectNeckMS(precision=...) (the three 3x3 GEMMs on 16-bit MFMA, operands
rounded to nearest even, fp32 accumulation) and the torch side runs the SAME module under torch.autocast("cuda",
dtype=...) -- the reference's AMP, tools/train.py:284-357 -- channels-last, in the same process.  The JSON line names the
mode on both sides ("device_precision", "torch_autocast").

With --trace only --steps steps per side are run once (for `rocprofv3 --kernel-trace --stats -- python
tools/dense_neck_train_time.py --trace ...`).

    python tools/dense_neck_train_time.py [--models yololite_n,yololite_m] [--precision fp32|fp16|bf16] [--blocks 7]
                                          [--steps 20] [--out F] [--trace]"""
import os
import sys

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

from tools import _train_time as tt  # noqa: E402

PRECISION = "fp32"                       # --precision, read off the command line before tools/_train_time.py's own arguments

SHAPES = {"yololite_n": dict(F=196, depth=2, Cin=(40, 112, 320), B=32, sizes=(80, 40, 20)),
          "yololite_m": dict(F=328, depth=2, Cin=(48, 120, 352), B=16, sizes=(80, 40, 20))}


def torch_neck(F, depth, cins):
    """the reference's laterals, smooth blocks and top-down pass in torch (model_v2.py:15-22, 115-127, 194-203)"""
    import torch.nn.functional as TF
    from torch import nn

    def conv_block():
        layers = []
        for _ in range(depth):
            layers += [nn.Conv2d(F, F, 3, padding=1, bias=False), nn.BatchNorm2d(F), nn.SiLU(inplace=True)]
        return nn.Sequential(*layers)

    class Neck(nn.Module):
        def __init__(self):
            super().__init__()
            for i, ci in enumerate(cins):
                setattr(self, f"lateral{3 + i}", nn.Conv2d(ci, F, 1))
            for i in range(len(cins)):
                setattr(self, f"smooth{3 + i}", conv_block())

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
    ours = ya.DetectNeckMS(cins, F, depth, precision=PRECISION).to(dev).train()
    cast = {"fp16": torch.float16, "bf16": torch.bfloat16}.get(PRECISION)
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
        elif cast is None:
            torch.autograd.backward(m(feats_cl), gps_cl)
        else:
            with torch.autocast("cuda", dtype=cast):
                ps = m(feats_cl)
            torch.autograd.backward(ps, [g.to(p.dtype) for g, p in zip(gps_cl, ps)])

    plan = neckops.plan_ms(cins, F, depth, B, sizes)
    rows = [lp["rows"] for lp in plan["levels"]]
    res = {"model": name, "device_precision": PRECISION, "torch_autocast": PRECISION if cast is not None else "off", "F": F, "depth": depth, "in_channels": list(cins), "batch": B, "sizes": list(sizes),
           "steps_per_block": steps, "saved_bytes": plan["saved_bytes"], "nosave_bytes": plan["nosave_bytes"],
           "workspace_bytes": plan["workspace_bytes"], "table_bytes": plan["table_bytes"],
           "w3grad_splits": [lp["w3grad_splits"] for lp in plan["levels"]],
           # three passes (forward, input gradient, weight gradient) of 2 * 9 * F * F flops per row and block
           "conv3x3_flop_per_step": 3 * depth * sum(2 * 9 * F * F * M for M in rows)}
    launches = lambda: sum(ours.last_launches().values())    # noqa: E731
    if not tt.time_sides(res, lambda: step(ours), lambda: step(ref), launches, blocks, steps, trace):
        return res
    ref64 = torch_neck(F, depth, cins).to(dev).double().train()
    ref64.load_state_dict(ours.state_dict())
    torch.autograd.backward(ref64([f.double() for f in feats_cl]), [g.double() for g in gps_cl])
    res.update(tt.grad_errors(ours, ref, ref64, between=True))
    return res


if __name__ == "__main__":
    import argparse
    ap = argparse.ArgumentParser(add_help=False)
    ap.add_argument("--precision", choices=("fp32", "fp16", "bf16"), default="fp32")
    known, rest = ap.parse_known_args()
    PRECISION = known.precision
    sys.argv = sys.argv[:1] + rest
    tt.main("dense_neck_train_time.py", "yololite_n,yololite_m", run_model, header={"precision": PRECISION})
