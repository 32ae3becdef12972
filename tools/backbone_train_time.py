#!/usr/bin/env python3
"""Time the trainable backbone's forward + backward (yololite_amd.MobileNetV4Backbone: stemops.BackboneStem,
stageops.BackboneMid, stageops.BackboneTail; csrc/yl_stem.hip, csrc/yl_stage.hip) against the same module in torch --
oracle/backbones.py's FeatureBackbone, channels-last fp32 input, same weights -- in one process on one device.

Shapes: edge_n (mobilenetv4_conv_small_050) at batch 64, 640 px and edge_m (mobilenetv4_conv_small) at batch 32, 640 px.
Two measurements per shape: "stem_step" (image -> C3: conv_stem, stages 0 and 1; backward from a fixed gradient of C3 into
every parameter) and "backbone_step" (image -> [C3, C4, C5]; backward from fixed gradients of all three maps).  The image does
not require grad.

Block protocol: --blocks times, alternating the two sides, each block = synchronise, --steps steps, synchronise, host
clock around it.  Per side: median and minimum over the blocks of the time per step.  Prints one JSON line, with the
launches per step of the device side and what yl_stem_plan / yl_stage_plan say the handles hold.

With --trace only --steps steps per side are run once (for `rocprofv3 --kernel-trace --stats -- python
tools/backbone_train_time.py --trace ...`).

--precision fp16 | bf16: the device side is MobileNetV4Backbone(precision=...), i.e. every dense GEMM (the stem's 3x3, every
1x1) on 16-bit MFMA with depthwise convolutions and BatchNorm in fp32; the torch side is the same module under
torch.autocast of that dtype (its parameters stay fp32), which also runs the depthwise convolutions in 16 bits.  The line
names the mode on both sides.

    python tools/backbone_train_time.py [--models edge_n,edge_m] [--blocks 7] [--steps 20] [--out F] [--trace]
                                        [--precision fp32|fp16|bf16]"""
import contextlib
import os
import sys

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tools import _train_time as tt  # noqa: E402

SHAPES = {"edge_n": dict(B=64, S=640), "edge_m": dict(B=32, S=640)}
PRECISIONS = ("fp32", "fp16", "bf16")
PRECISION = "fp32"


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


def torch_backbone(backbone, upto=None):
    """the oracle's backbone giving [c3, c4, c5], or (upto = "c3") only its part up to the C3 tap"""
    from torch import nn
    from oracle.backbones import FeatureBackbone
    bb = FeatureBackbone(backbone)
    c3_stage = bb._taps[-3]

    class Part(nn.Module):
        def __init__(self):
            super().__init__()
            self.conv_stem, self.bn1 = bb.conv_stem, bb.bn1
            last = c3_stage if upto == "c3" else len(bb.blocks) - 1
            self.blocks = nn.ModuleDict({str(si): bb.blocks[si] for si in range(last + 1)})

        def forward(self, x):
            x = self.bn1(self.conv_stem(x))
            feats = []
            for si, st in self.blocks.items():
                x = st(x)
                if int(si) in bb._taps[-3:]:
                    feats.append(x)
            return feats

    return Part()


def run_model(name, blocks, steps, trace):
    import torch
    import yololite_amd as ya
    from yololite_amd import stageops, stemops
    from yololite_amd.program import zoo_meta
    B, S = SHAPES[name]["B"], SHAPES[name]["S"]
    dev = "cuda:0"
    torch.manual_seed(3)
    meta = zoo_meta(name, num_classes=3, img_size=S)
    ours = ya.MobileNetV4Backbone.from_meta(meta, precision=PRECISION).to(dev).train()
    cast = {"fp16": torch.float16, "bf16": torch.bfloat16}.get(PRECISION)
    autocast = (lambda: torch.autocast("cuda", dtype=cast)) if cast else contextlib.nullcontext
    sd = {k[len("backbone."):]: v for k, v in ours.state_dict().items()}
    gen = torch.Generator().manual_seed(5)
    x = torch.randn(B, 3, S, S, generator=gen).to(dev)
    x_cl = x.contiguous(memory_format=torch.channels_last)
    with torch.no_grad():
        shapes = [tuple(c.shape) for c in ours(x)]
    gs = [(1e-3 * torch.randn(*sh, generator=gen)).to(dev) for sh in shapes]                       # NHWC
    gs_cl = [g.permute(0, 3, 1, 2) for g in gs]                                                   # the same memory, NCHW shape
    stem = ours.stem
    splan = stemops.plan(3, stem.units_cfg, B, S, stem.eps, input_layout="nchw")
    mplan = stageops.plan(ours.mid.in_channels, ours.mid.blocks_cfg, B, shapes[0][1], ours.mid.eps)
    tplan = stageops.plan(ours.tail.in_channels, ours.tail.blocks_cfg, B, shapes[1][1], ours.tail.eps)
    res = {"model": name, "device_precision": PRECISION, "torch_autocast": PRECISION if cast else "off", "backbone": meta["backbone"], "batch": B, "image": [B, 3, S, S], "c3": list(shapes[0]),
           "c4": list(shapes[1]), "c5": list(shapes[2]), "steps_per_block": steps,
           "stem_saved_bytes": splan["saved_bytes"], "stem_workspace_bytes": splan["workspace_bytes"],
           "stem_stat_rows": [u["stat_rows"] for u in splan["units"]], "stem_stat_tiles": [u["stat_tiles"] for u in splan["units"]],
           "mid_saved_bytes": mplan["saved_bytes"], "tail_saved_bytes": tplan["saved_bytes"]}

    def grads_off(m):
        for p in m.parameters():
            p.grad = None

    for what in ("stem", "backbone"):
        ref = torch_backbone(meta["backbone"], "c3" if what == "stem" else None)
        ref.load_state_dict({k: v for k, v in sd.items() if k in ref.state_dict()})
        ref = ref.to(dev).to(memory_format=torch.channels_last).train()

        def ours_step():
            grads_off(ours)
            if what == "stem":
                stem(x).backward(gs[0])
            else:
                torch.autograd.backward(ours(x), gs)

        def ref_step():
            grads_off(ref)
            with autocast():
                feats = ref(x_cl)
            if what == "stem":                             # the maps come out in the autocast dtype: the gradients follow
                feats[0].backward(gs_cl[0].to(feats[0].dtype))
            else:
                torch.autograd.backward(feats, [g.to(f.dtype) for g, f in zip(gs_cl, feats)])

        parts = (stem,) if what == "stem" else (stem, ours.mid, ours.tail)
        launches = lambda: sum(sum(p.last_launches.values()) for p in parts)   # noqa: E731
        sub = {}
        tt.time_sides(sub, ours_step, ref_step, launches, blocks, steps, trace)
        res[what + "_step"] = sub
        del ref
        torch.cuda.empty_cache()
    return res


if __name__ == "__main__":
    PRECISION = take_precision(sys.argv)
    tt.main("backbone_train_time.py", "edge_n,edge_m", run_model, header={"precision": PRECISION})
