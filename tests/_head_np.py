"""The detection head restated in torch at a chosen precision (float64 for references): the arithmetic of the
reference's make_head / _forward_head (model_v2.py:23-53,182-192) written out op by op -- depthwise 3x3, 1x1,
BatchNorm2d from its definition (batch or running statistics, momentum 0.1, eps 1e-5), ReLU, the three output
convolutions laid out anchor-major -- with autograd for the backward.  No nn.Module, no device."""
import numpy as np
import torch
import torch.nn.functional as TF

EPS, MOMENTUM = 1e-5, 0.1


def head_forward(params, buffers, x_nhwc, k, A, C, depth, train, dtype=torch.float64):
    """params / buffers: {reference name: array or tensor}; x_nhwc [B,S,S,F] (tensor: kept as is, so that it may carry
    requires_grad).  -> y [B,A,S,S,5+C], {running stat name: new value}, BN outputs (before the ReLU) per block"""
    P = {n: (v if torch.is_tensor(v) else torch.as_tensor(np.asarray(v))).to(dtype) for n, v in params.items()}
    x = x_nhwc if torch.is_tensor(x_nhwc) else torch.as_tensor(np.asarray(x_nhwc)).to(dtype)
    h = x.permute(0, 3, 1, 2)
    B, F, S, _ = h.shape
    M = B * S * S
    new, bn_out = {}, []
    for t in range(depth):
        p = f"head{k}.trunk.{t}.block."
        d = TF.conv2d(h, P[p + "0.weight"], None, 1, 1, 1, F)
        z = TF.conv2d(d, P[p + "1.weight"])
        rm = torch.as_tensor(np.asarray(buffers[p + "2.running_mean"])).to(dtype)
        rv = torch.as_tensor(np.asarray(buffers[p + "2.running_var"])).to(dtype)
        if train:
            mean = z.mean((0, 2, 3))
            var = ((z - mean[None, :, None, None]) ** 2).mean((0, 2, 3))
            new[p + "2.running_mean"] = ((1 - MOMENTUM) * rm + MOMENTUM * mean).detach()
            new[p + "2.running_var"] = ((1 - MOMENTUM) * rv + MOMENTUM * var * M / (M - 1)).detach()
            new[p + "2.num_batches_tracked"] = int(np.asarray(buffers[p + "2.num_batches_tracked"])) + 1
        else:
            mean, var = rm, rv
        zh = (z - mean[None, :, None, None]) / torch.sqrt(var[None, :, None, None] + EPS)
        bn = zh * P[p + "2.weight"][None, :, None, None] + P[p + "2.bias"][None, :, None, None]
        bn_out.append(bn)
        h = torch.relu(bn)
    o = f"head{k}.out."
    box = TF.conv2d(h, P[o + "box.weight"], P[o + "box.bias"]).view(B, A, 4, S, S)
    obj = TF.conv2d(h, P[o + "obj.weight"], P[o + "obj.bias"]).view(B, A, 1, S, S)
    cls = TF.conv2d(h, P[o + "cls.weight"], P[o + "cls.bias"]).view(B, A, C, S, S)
    y = torch.cat([box, obj, cls], 2).permute(0, 1, 3, 4, 2).contiguous()
    return y, new, bn_out


def head_all(params, buffers, x_nhwc, gy, k, A, C, depth, train, dtype=torch.float64):
    """forward and backward -> {fixture tensor name: numpy array}: y, dx, running_mean.t / running_var.t /
    num_batches_tracked.t (the values after the call) and g.<parameter name>"""
    P = {n: torch.as_tensor(np.asarray(v)).to(dtype).requires_grad_(True) for n, v in params.items()}
    x = torch.as_tensor(np.asarray(x_nhwc)).to(dtype).requires_grad_(True)
    y, new, _ = head_forward(P, buffers, x, k, A, C, depth, train, dtype)
    y.backward(torch.as_tensor(np.asarray(gy)).to(dtype))
    out = {"y": y.detach().numpy(), "dx": x.grad.numpy()}
    for t in range(depth):
        p = f"head{k}.trunk.{t}.block.2."
        for s in ("running_mean", "running_var", "num_batches_tracked"):
            v = new.get(p + s, buffers[p + s])
            out[f"{s}.{t}"] = v.numpy() if torch.is_tensor(v) else np.asarray(v)
    for n, v in P.items():
        out["g." + n] = v.grad.numpy()
    return out


def fit_reference(cfg, inputs, dtype=torch.float64):
    """The end-to-end fit on the CPU in float64: `steps` times (heads in train mode on the fixed features, LossAF
    through tests/_lossaf_np.py and its gradient through tests/_lossaf_grad_np.py, SGD with momentum).  `inputs`:
    _head_cases.case_inputs(cfg).  -> the loss before every step and after the last one, [steps + 1]"""
    from _lossaf_grad_np import loss_af_grad, split_levels
    from _lossaf_np import loss_af
    A, C, depth = cfg["A"], cfg["C"], cfg["depth"]
    gt = np.asarray(cfg["gt_xyxy"], np.float32)
    lab, off = np.asarray(cfg["gt_label"], np.int64), np.asarray(cfg["gt_off"], np.int32)
    P = [{n: torch.as_tensor(v).to(dtype).requires_grad_(True) for n, v in lv["params"].items()} for lv in inputs]
    bufs = [dict(lv["buffers"]) for lv in inputs]
    mom = [{n: None for n in p} for p in P]
    losses = []

    def loss_and_grads(backward):
        ys, news = [], []
        for lv, p, b in zip(inputs, P, bufs):
            y, new, _ = head_forward(p, b, lv["x"], lv["k"], A, C, depth, True, dtype)
            ys.append(y); news.append(new)
        levels = [y.detach().numpy() for y in ys]
        r = loss_af(levels, gt, lab, off, C, cfg["img_size"], dtype=np.float64)
        if backward:
            g = loss_af_grad(levels, gt, lab, off, C, cfg["img_size"], dtype=np.float64, assign=r["assign"])["grad"]
            for y, gl in zip(ys, split_levels(g, levels)):
                y.backward(torch.as_tensor(np.ascontiguousarray(gl)).to(dtype))
        return r["box"] + r["obj"] + r["cls"], news

    for _ in range(cfg["steps"]):
        loss, news = loss_and_grads(True)
        losses.append(loss)
        with torch.no_grad():
            for p, m, b, new in zip(P, mom, bufs, news):
                for n, v in p.items():
                    m[n] = v.grad.clone() if m[n] is None else cfg["momentum"] * m[n] + v.grad
                    v -= cfg["lr"] * m[n]
                    v.grad = None
                b.update({n: (w.numpy() if torch.is_tensor(w) else w) for n, w in new.items()})
    losses.append(loss_and_grads(False)[0])
    return np.asarray(losses, np.float64)
