#!/usr/bin/env python3
"""Time one training-step tail (what runs between backward() and the next forward) for the tensor shapes of edge_n and
yololite_m: the fused path (yololite_amd.FusedTrainStep: three kernels) against the reference's sequence of torch
calls as tools/train.py:352-359 makes them -- GradScaler.unscale_, clip_grad_norm_, GradScaler.step(torch.optim.AdamW
with torch's defaults, as the reference constructs it), GradScaler.update, and ModelEMA.update's loop over the
state_dict -- in the same process on the same device.

Shapes come from synth_state_dict(zoo_meta(name)): every `weight` / `bias` is a parameter (groups: backbone, head, the
rest, as the reference splits them), `running_mean` / `running_var` are buffers, and every BatchNorm gets the int64
`num_batches_tracked` a real state_dict has.  Gradients are seeded random tensors that stay in place; both sides run
with a loss scale of 1 and a clip threshold far above the norm, so the torch side's in-place unscale and clip leave
them as they are from step to step.

Block protocol: --blocks times, alternating the two sides, each block = synchronise, --steps tails, synchronise, host
clock around it (a launch-bound sequence is bounded by the host, so the wall time per tail is the figure).  Per side:
median and minimum over the blocks of the time per tail.  Prints one JSON line.

With --parity F the cases of tests/_train_cases.py are run for the three optimizers and the device errors against the
CPU float64 yardstick, the bars and their ratios are written to F.  With --trace only --steps tails per side are run
once (for `rocprofv3 --kernel-trace --stats -- python tools/train_step_time.py --trace ...`: the launch count per
tail is Calls / steps).

    python tools/train_step_time.py [--models edge_n,yololite_m] [--blocks 7] [--steps 50] [--out F] [--parity F]
                                    [--trace]"""
import argparse
import copy
import json
import math
import os
import sys
import time

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

EMA_DECAY, TOTAL_UPDATES, CLIP = 0.995, 30000, 1e9


def make_bag(name, seed, device):
    """-> nn.Module with the model's parameters and buffers under their state_dict names (dots as underscores)"""
    import torch
    from yololite_amd.program import synth_state_dict, zoo_meta
    sd = synth_state_dict(zoo_meta(name, num_classes=80, img_size=640), seed=seed)
    bag = torch.nn.Module()
    for k, v in sd.items():
        n = k.replace(".", "_")
        t = torch.from_numpy(v).to(device)
        if k.endswith(("running_mean", "running_var")):
            bag.register_buffer(n, t)
            if k.endswith("running_mean"):
                bag.register_buffer(n[:-len("running_mean")] + "num_batches_tracked",
                                    torch.zeros((), dtype=torch.int64, device=device))
        else:
            bag.register_parameter(n, torch.nn.Parameter(t))
    return bag


def groups_of(bag):
    g = {"backbone": [], "neck": [], "head": []}
    for n, p in bag.named_parameters():
        g["backbone" if n.startswith("backbone") else "head" if n.startswith("head") else "neck"].append(p)
    return [{"params": g["backbone"], "lr": 2e-4, "weight_decay": 1e-2}, {"params": g["neck"], "lr": 1e-3, "weight_decay": 1e-2},
            {"params": g["head"], "lr": 1e-3, "weight_decay": 1e-2}]


class RefEMA:
    """tools/train.py:29-57, restated"""

    def __init__(self, model, total_updates, decay):
        self.ema = copy.deepcopy(model).eval()
        self.updates, self.decay = 0, decay
        self.warmup_limit = max(100, total_updates // 5)
        for p in self.ema.parameters():
            p.requires_grad_(False)

    def update(self, model):
        import torch
        with torch.no_grad():
            self.updates += 1
            d = self.decay * (1 - math.exp(-self.updates / self.warmup_limit))
            msd = model.state_dict()
            for k, v in self.ema.state_dict().items():
                if v.dtype.is_floating_point:
                    v.mul_(d).add_(msd[k].detach(), alpha=1 - d)
                else:
                    v.copy_(msd[k])


def set_grads(bag, seed):
    import torch
    gen = torch.Generator(device="cpu").manual_seed(seed)
    for p in bag.parameters():
        p.grad = (0.01 * torch.randn(p.shape, generator=gen)).to(p.device)


def run_model(name, blocks, steps, trace):
    import numpy as np
    import torch
    import yololite_amd as ya
    dev = "cuda:0"
    a, b = make_bag(name, 2, dev), make_bag(name, 2, dev)
    ema_a = copy.deepcopy(a).eval()
    fts = ya.FusedTrainStep(groups_of(a), optimizer="adamw", grad_clip=CLIP, amp=True,
                            scaler_kwargs={"init_scale": 1.0, "growth_interval": 10 ** 9}, ema_model=ema_a, model=a,
                            ema_decay=EMA_DECAY, total_updates=TOTAL_UPDATES)
    opt = torch.optim.AdamW(groups_of(b))
    scaler = torch.amp.GradScaler("cuda", init_scale=1.0, growth_interval=10 ** 9)
    scaler.scale(torch.zeros(1, device=dev))
    ema_b = RefEMA(b, TOTAL_UPDATES, EMA_DECAY)
    set_grads(a, 7); set_grads(b, 7)
    params_b = list(b.parameters())

    def fused():
        fts.step()

    def ref():
        scaler.unscale_(opt)
        torch.nn.utils.clip_grad_norm_(params_b, CLIP)
        scaler.step(opt)
        scaler.update()
        ema_b.update(b)

    def block(fn, n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / n

    nparam = sum(p.numel() for p in a.parameters())
    nbuf = sum(v.numel() for v in a.buffers() if v.dtype.is_floating_point)
    res = {"model": name, "tensors": len(a.state_dict()), "parameters": len(list(a.parameters())),
           "parameter_elements": nparam, "buffer_elements": nbuf, "steps_per_block": steps,
           # bytes the algorithm needs: gradient once; then p, g, m, v, ema read and p, m, v, ema written, buffers 3 x
           "stats_bytes": 4 * nparam, "apply_bytes": 4 * (9 * nparam + 3 * nbuf)}
    if trace:
        block(fused, steps); block(ref, steps)
        return res
    for _ in range(2):
        block(fused, 5); block(ref, 5)
    tf, tr = [], []
    for _ in range(blocks):
        tf.append(block(fused, steps)); tr.append(block(ref, steps))
    # the two sides saw the same gradients from the same start: the runs can be compared as well as timed
    worst = max(float((p.detach() - q.detach()).abs().max()) for p, q in zip(a.parameters(), b.parameters()))
    worst_ema = max(float((ema_a.state_dict()[k].float() - v.float()).abs().max()) for k, v in ema_b.ema.state_dict().items())
    res.update({"blocks": blocks, "fused_ms": round(float(np.median(tf)), 4), "fused_ms_min": round(float(np.min(tf)), 4),
                "torch_ms": round(float(np.median(tr)), 4), "torch_ms_min": round(float(np.min(tr)), 4),
                "ratio": round(float(np.median(tr)) / float(np.median(tf)), 2),
                "fused_ms_blocks": [round(v, 4) for v in tf], "torch_ms_blocks": [round(v, 4) for v in tr],
                "max_abs_param_difference": worst, "max_abs_ema_difference": worst_ema})
    return res


def parity(path):
    import torch
    import _train_cases as tc
    rows, worst = [], (0.0, "")
    for kind in tc.KINDS:
        for nsteps in (1, tc.NSTEPS):
            r = tc.parity_rows(kind, nsteps, tc.run_fused(kind, nsteps))
            rows.append({"optimizer": kind, "steps": nsteps, **r})
            for q, v in r.items():
                worst = max(worst, (v["ratio"], f"{kind}/{q}/{nsteps}"))
    with open(path, "w") as f:
        json.dump(rows, f, indent=1)
    return {"worst_ratio": round(worst[0], 4), "at": worst[1]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--models", default="edge_n,yololite_m")
    ap.add_argument("--blocks", type=int, default=7)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--out", default="")
    ap.add_argument("--parity", default="")
    ap.add_argument("--trace", action="store_true")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("train_step_time.py needs a HIP device")
    res = {"gpu": torch.cuda.get_device_name(0), "optimizer": "adamw", "runs": []}
    for name in [m for m in args.models.split(",") if m]:
        res["runs"].append(run_model(name, args.blocks, args.steps, args.trace))
    if args.parity:
        res["parity"] = parity(args.parity)
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
