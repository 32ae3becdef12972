#!/usr/bin/env python3
"""Time the backbone tail's forward + backward (yololite_amd.BackboneTail, csrc/yl_stage.hip) against the same module in
torch -- the stages behind the C4 tap of oracle/backbones.py's FeatureBackbone (UniversalInvertedResidual, ConvBnAct),
channels-last fp32 input, same weights -- in one process on one device.

Shapes: edge_n (mobilenetv4_conv_small_050: C4 [64,40,40,48] -> C5 [64,20,20,480]) and edge_m (mobilenetv4_conv_small:
C4 [32,40,40,96] -> C5 [32,20,20,960]).  --model yololite_n | yololite_m times the EfficientNet-Lite tail instead
(yololite_amd.EfficientNetLiteTail: InvertedResidual blocks under ReLU6 and TF-SAME; tf_efficientnet_lite0: C4
[64,40,40,112] -> C5 [64,20,20,320], tf_efficientnet_lite2: C4 [32,40,40,120] -> C5 [32,20,20,352]) against the oracle's
blocks of the same stages.  One step = train-mode forward of the tail on a fixed C4 that does not require
grad, backward from a fixed gradient of C5 into every parameter.

Block protocol: --blocks times, alternating the two sides, each block = synchronise, --steps steps, synchronise, host
clock around it.  Per side: median and minimum over the blocks of the time per step.  Prints one JSON line, with the
launches per step of the device side, what yl_stage_plan says the handle holds, and both sides' gradient errors against a
float64 run of the torch module.  Gradients whose float64 value stays below 1e-6 of the tail's largest gradient are left
out of those relative figures and counted in "grads_left_out": a per-channel shift in front of a convolution that a
train-mode BatchNorm follows has a gradient that is zero in exact arithmetic (dw_start's BatchNorm bias, for one), and an
error relative to rounding noise says nothing.

With --trace only --steps steps per side are run once (for `rocprofv3 --kernel-trace --stats -- python
tools/tail_train_time.py --trace ...`).

    python tools/tail_train_time.py [--models edge_n,edge_m | --model yololite_n] [--blocks 7] [--steps 20] [--out F] [--trace]"""
import os
import sys

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tools import _train_time as tt  # noqa: E402

SHAPES = {"edge_n": dict(B=64, S=40), "edge_m": dict(B=32, S=40), "yololite_n": dict(B=64, S=40), "yololite_m": dict(B=32, S=40)}


def torch_tail(backbone):
    """the stages behind the C4 tap of the oracle's backbone, as one module"""
    from torch import nn
    from oracle.backbones import FeatureBackbone
    bb = FeatureBackbone(backbone)
    first = bb._taps[-2] + 1

    class Tail(nn.Module):
        def __init__(self):
            super().__init__()
            self.blocks = nn.ModuleDict({str(si): bb.blocks[si] for si in range(first, len(bb.blocks))})

        def forward(self, x):
            for st in self.blocks.values():
                x = st(x)
            return x

    return Tail()


class _Only:
    """the parameters of `m` at the positions `keep`, as grad_errors reads a module"""

    def __init__(self, m, keep):
        self.named = [np_ for i, np_ in enumerate(m.named_parameters()) if i in keep]

    def named_parameters(self):
        return iter(self.named)

    def parameters(self):
        return (p for _, p in self.named)


def run_model(name, blocks, steps, trace):
    import torch
    import yololite_amd as ya
    from yololite_amd import irops, stageops
    from yololite_amd.program import zoo_meta
    B, S = SHAPES[name]["B"], SHAPES[name]["S"]
    dev = "cuda:0"
    torch.manual_seed(3)
    meta = zoo_meta(name, num_classes=3, img_size=16 * S)
    lite = irops.is_lite(meta)
    ours = (ya.EfficientNetLiteTail if lite else ya.BackboneTail).from_meta(meta).to(dev).train()
    sd = {k[len("backbone."):]: v for k, v in ours.state_dict().items()}
    ref = torch_tail(meta["backbone"])
    ref.load_state_dict(sd)
    ref = ref.to(dev).to(memory_format=torch.channels_last).train()
    gen = torch.Generator().manual_seed(5)
    So = ours.out_size(S)
    x = torch.randn(B, S, S, ours.in_channels, generator=gen).to(dev)                             # NHWC
    x_cl = x.permute(0, 3, 1, 2)                                                                  # the same memory, NCHW shape
    gy = (1e-3 * torch.randn(B, So, So, ours.out_channels, generator=gen)).to(dev)
    gy_cl = gy.permute(0, 3, 1, 2)

    def step(m):
        for p in m.parameters():
            p.grad = None
        if m is ours:
            m(x, layout="nhwc").backward(gy)
        else:
            m(x_cl).backward(gy_cl)

    plan = (irops if lite else stageops).plan(ours.in_channels, ours.blocks_cfg, B, S, ours.eps)
    res = {"model": name, "backbone": meta["backbone"], "batch": B, "c4": [B, S, S, ours.in_channels],
           "c5": [B, So, So, ours.out_channels], "blocks_in_tail": len(ours.blocks_cfg), "steps_per_block": steps,
           "saved_bytes": plan["saved_bytes"], "workspace_bytes": plan["workspace_bytes"]}
    launches = lambda: sum(ours.last_launches.values())    # noqa: E731
    if not tt.time_sides(res, lambda: step(ours), lambda: step(ref), launches, blocks, steps, trace):
        return res
    ref64 = torch_tail(meta["backbone"])
    ref64.load_state_dict(sd)
    ref64 = ref64.to(dev).double().train()
    ref64(x_cl.double()).backward(gy_cl.double())
    top = max(float(p.grad.abs().max()) for p in ref64.parameters())
    keep = {i for i, p in enumerate(ref64.parameters()) if float(p.grad.abs().max()) >= 1e-6 * top}
    res["grads_left_out"] = len(list(ref64.parameters())) - len(keep)
    res.update(tt.grad_errors(_Only(ours, keep), _Only(ref, keep), _Only(ref64, keep)))
    return res


if __name__ == "__main__":
    sys.argv = ["--models" if v == "--model" else v.replace("--model=", "--models=", 1) for v in sys.argv]    # one model: the same list
    tt.main("tail_train_time.py", "edge_n,edge_m", run_model)
