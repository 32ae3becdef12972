"""What tools/head_train_time.py and tools/neck_train_time.py share: the reference's DWConvBlock in torch, the block
protocol (synchronise, --steps steps, synchronise, host clock around it; --blocks times, alternating the two sides after
two short warm-up rounds), the gradient errors of both sides against a float64 copy of the torch module, and the command
line with its one JSON line."""
import argparse
import json
import time


def torch_block(F, n):
    """the reference's DWConvBlock(F, F, n) in torch (model_v2.py:23-39)"""
    from torch import nn

    class Block(nn.Module):
        def __init__(self):
            super().__init__()
            layers = []
            for _ in range(n):
                layers += [nn.Conv2d(F, F, 3, padding=1, groups=F, bias=False), nn.Conv2d(F, F, 1, bias=False),
                           nn.BatchNorm2d(F), nn.ReLU(inplace=True)]
            self.block = nn.Sequential(*layers)

        def forward(self, x):
            return self.block(x)

    return Block()


def timed_block(step, n):
    """milliseconds per step of n steps"""
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        step()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / n


def time_sides(res, ours_step, ref_step, launches, blocks, steps, trace):
    """The timing fields of `res`.  With `trace` each side runs --steps steps once and only the launches are recorded.
    `launches`: -> the device side's launches of its last step.  -> whether the sides were timed"""
    import numpy as np
    if trace:
        timed_block(ours_step, steps); timed_block(ref_step, steps)
        res["launches_per_step"] = launches()
        return False
    for _ in range(2):
        timed_block(ours_step, 3); timed_block(ref_step, 3)
    to, tr = [], []
    for _ in range(blocks):
        to.append(timed_block(ours_step, steps)); tr.append(timed_block(ref_step, steps))
    res.update({"blocks": blocks, "launches_per_step": launches(),
                "device_ms": round(float(np.median(to)), 4), "device_ms_min": round(float(np.min(to)), 4),
                "torch_ms": round(float(np.median(tr)), 4), "torch_ms_min": round(float(np.min(tr)), 4),
                "ratio": round(float(np.median(tr)) / float(np.median(to)), 3),
                "device_ms_blocks": [round(v, 4) for v in to], "torch_ms_blocks": [round(v, 4) for v in tr]})
    return True


def grad_errors(ours, ref, ref64, between=False):
    """Same weights, same inputs, one step behind each: both sides against the torch module in float64.  The largest
    error over the parameter gradients, relative to the gradient's largest element, and the L2 error, which a flipped
    ReLU mask of a BatchNorm output within fp32 rounding of zero does not dominate.  `between`: also device against torch"""
    worst, worst_t, btw, l2, l2_t = (0.0, ""), (0.0, ""), (0.0, ""), 0.0, 0.0
    for (n, p), q, r in zip(ours.named_parameters(), ref.parameters(), ref64.parameters()):
        m = r.grad.abs().max().clamp_min(1e-300)
        worst = max(worst, (float((p.grad.double() - r.grad).abs().max() / m), n))
        worst_t = max(worst_t, (float((q.grad.double() - r.grad).abs().max() / m), n))
        btw = max(btw, (float((p.grad.double() - q.grad.double()).abs().max() / m), n))
        l2 = max(l2, float((p.grad.double() - r.grad).norm() / r.grad.norm().clamp_min(1e-300)))
        l2_t = max(l2_t, float((q.grad.double() - r.grad).norm() / r.grad.norm().clamp_min(1e-300)))
    out = {"device_max_rel_grad_error_vs_float64": worst[0], "device_max_rel_grad_error_at": worst[1],
           "torch_max_rel_grad_error_vs_float64": worst_t[0], "torch_max_rel_grad_error_at": worst_t[1]}
    if between:
        out.update({"device_vs_torch_max_rel_grad_difference": btw[0], "device_vs_torch_max_rel_grad_difference_at": btw[1]})
    out.update({"device_max_rel_l2_grad_error_vs_float64": l2, "torch_max_rel_l2_grad_error_vs_float64": l2_t})
    return out


def main(tool, models, run_model, header=None, parity=None):
    """`run_model(name, blocks, steps, trace)` -> one entry of "runs"; `header`: the tool's own fields of the line;
    `parity(path)`: behind --parity, if the tool has it"""
    ap = argparse.ArgumentParser()
    ap.add_argument("--models", default=models)
    ap.add_argument("--blocks", type=int, default=7)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--out", default="")
    if parity:
        ap.add_argument("--parity", default="")
    ap.add_argument("--trace", action="store_true")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit(f"{tool} needs a HIP device")
    res = {"gpu": torch.cuda.get_device_name(0), **(header or {}), "runs": []}
    for name in [m for m in args.models.split(",") if m]:
        res["runs"].append(run_model(name, args.blocks, args.steps, args.trace))
    if parity and args.parity:
        res["parity"] = parity(args.parity)
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
