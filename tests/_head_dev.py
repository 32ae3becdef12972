"""What the detection-head GPU tests and tools/head_train_time.py --parity share: a DetectHeads with a case's weights,
one forward + backward of it, and the device error and bar of every fixture tensor."""
import torch

import yololite_amd as ya
import _train_dev
from _head_cases import case_inputs, fixture_tensors, level_names
from _train_dev import DEV


def heads_of(case, inputs, train=True):
    m = ya.DetectHeads(case["F"], case["C"], case["A"], case["depth"], level_names=level_names(case))
    sd = {}
    for lv in inputs:
        sd.update(lv["params"]); sd.update(lv["buffers"])
    m.load_state_dict({k: torch.as_tensor(v) for k, v in sd.items()})
    return m.to(DEV).train(train)


def run(m, inputs, x_grad=True, layout="nhwc"):
    """forward + backward with the case's gy -> {level: {fixture tensor name: cpu tensor}}"""
    m.zero_grad(set_to_none=True)
    xs = []
    for lv in inputs:
        x = torch.from_numpy(lv["x"]).to(DEV)
        if layout == "nchw":                               # a strided NCHW tensor: contiguous NCHW memory
            x = x.permute(0, 3, 1, 2).contiguous()
        elif layout == "channels_last":                    # NCHW shape over NHWC memory
            x = x.permute(0, 3, 1, 2)
        xs.append(x.requires_grad_(x_grad))
    ys = m(xs)
    torch.autograd.backward(ys, [torch.from_numpy(lv["gy"]).to(DEV) for lv in inputs])
    out = []
    for lv, x, y in zip(inputs, xs, ys):
        k = lv["k"]
        d = {"y": y.detach().cpu()}
        if x.grad is not None:
            g = x.grad if layout == "nhwc" else x.grad.permute(0, 2, 3, 1)
            d["dx"] = g.contiguous().cpu()
        sd = m.state_dict()
        for t in range(m.head_depth):
            for s in ("running_mean", "running_var", "num_batches_tracked"):
                d[f"{s}.{t}"] = sd[f"head{k}.trunk.{t}.block.2.{s}"].cpu().clone()
        for n, p in m.named_parameters():
            if n.startswith(f"head{k}.") and p.grad is not None:
                d["g." + n] = p.grad.cpu().clone()
        out.append(d)
    return out


def parity_ratios(case, mode, z):
    """{(level, tensor): (error, bar)} of one case and mode"""
    return _train_dev.parity_ratios(case, mode, z, heads_of, run, case_inputs, fixture_tensors)
