"""What the dense-FPN-neck GPU tests share: a DetectNeckMS with a case's weights, one forward + backward of it (on the
case's inputs or on others), and the device error and bar of every fixture tensor."""
import torch

import yololite_amd as ya
import _train_dev
from _dense_neck_cases import case_inputs, fixture_tensors, level_names
from _train_dev import DEV


def neck_of(case, inputs, train=True):
    m = ya.DetectNeckMS(case["Cin"], case["F"], case["depth"], level_names=level_names(case))
    sd = {}
    for lv in inputs:
        sd.update(lv["params"]); sd.update(lv["buffers"])
    m.load_state_dict({k: torch.as_tensor(v) for k, v in sd.items()})
    return m.to(DEV).train(train)


def run(m, inputs, c_grad=True, layout="nhwc", cs=None, gps=None):
    """forward + backward with the case's gp -> per level {fixture tensor name: cpu tensor}.  c_grad: one bool, or one
    per level.  cs / gps: other NHWC inputs / output gradients than the case's (numpy, per level)"""
    m.zero_grad(set_to_none=True)
    want = [c_grad] * len(inputs) if isinstance(c_grad, bool) else list(c_grad)
    src = [lv["c"] for lv in inputs] if cs is None else cs
    gps = [lv["gp"] for lv in inputs] if gps is None else gps
    cs = []
    for a, w in zip(src, want):
        c = torch.from_numpy(a).to(DEV)
        if layout == "nchw":                               # contiguous NCHW memory
            c = c.permute(0, 3, 1, 2).contiguous()
        elif layout == "channels_last":                    # NCHW shape over NHWC memory
            c = c.permute(0, 3, 1, 2)
        cs.append(c.requires_grad_(w))
    ps = m(cs, layout="nhwc" if layout == "nhwc" else "nchw")
    if any(p.requires_grad for p in ps):
        torch.autograd.backward(ps, [torch.from_numpy(g).to(DEV) for g in gps])
    out = []
    sd = m.state_dict()
    for lv, c, p in zip(inputs, cs, ps):
        k = lv["k"]
        d = {"p": p.detach().cpu()}
        if c.grad is not None:
            g = c.grad if layout == "nhwc" else c.grad.permute(0, 2, 3, 1)
            d["dc"] = g.contiguous().cpu()
        for t in range(m.depth):
            for s in ("running_mean", "running_var", "num_batches_tracked"):
                d[f"{s}.{t}"] = sd[f"smooth{k}.{3 * t + 1}.{s}"].cpu().clone()
        for n, q in m.named_parameters():
            if n.startswith((f"lateral{k}.", f"smooth{k}.")) and q.grad is not None:
                d["g." + n] = q.grad.cpu().clone()
        out.append(d)
    return out


def parity_ratios(case, mode, z):
    """{(level, tensor): (error, bar)} of one case and mode"""
    return _train_dev.parity_ratios(case, mode, z, neck_of, run, case_inputs, fixture_tensors)
