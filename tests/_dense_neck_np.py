"""The dense FPN neck restated in torch at a chosen precision (float64 for references): the arithmetic of the reference's
YOLOLiteMS.forward (model_v2.py:15-22, 115-127, 194-203) written out op by op -- lateral 1x1 with bias, the nearest
upsample as an index map (tests/_neck_np.py nearest_src), the add, and per smooth block a dense 3x3 convolution,
BatchNorm2d from its definition and SiLU as y * sigmoid(y) -- with autograd for the backward.  No nn.Module, no device."""
import numpy as np
import torch
import torch.nn.functional as TF

from _neck_np import EPS, MOMENTUM, _t, nearest_src


def neck_forward(params, buffers, cs, ks, depth, train, dtype=torch.float64):
    """params / buffers: {reference name: array or tensor}; cs: NHWC maps, finest first (tensors are kept as they are, so
    that they may carry requires_grad); ks: the level numbers (3, 4, 5).
    -> ps NHWC finest first, {running stat name: new value}"""
    P = {n: _t(v, dtype) for n, v in params.items()}
    L = len(cs)
    ps, new = [None] * L, {}
    for li in range(L - 1, -1, -1):
        k = ks[li]
        c = _t(cs[li], dtype).permute(0, 3, 1, 2)
        t = TF.conv2d(c, P[f"lateral{k}.weight"], P[f"lateral{k}.bias"])
        if li + 1 < L:
            S = t.shape[-1]
            src = torch.as_tensor(nearest_src(S, ps[li + 1].shape[-1]))
            t = ps[li + 1][:, :, src][:, :, :, src] + t
        h = t
        B, F, S, _ = h.shape
        M = B * S * S
        for i in range(depth):
            bnp = f"smooth{k}.{3 * i + 1}."
            z = TF.conv2d(h, P[f"smooth{k}.{3 * i}.weight"], None, 1, 1)
            rm, rv = _t(buffers[bnp + "running_mean"], dtype), _t(buffers[bnp + "running_var"], dtype)
            if train:
                mean = z.mean((0, 2, 3))
                var = ((z - mean[None, :, None, None]) ** 2).mean((0, 2, 3))
                new[bnp + "running_mean"] = ((1 - MOMENTUM) * rm + MOMENTUM * mean).detach()
                new[bnp + "running_var"] = ((1 - MOMENTUM) * rv + MOMENTUM * var * M / (M - 1)).detach()
                new[bnp + "num_batches_tracked"] = int(np.asarray(buffers[bnp + "num_batches_tracked"])) + 1
            else:
                mean, var = rm, rv
            zh = (z - mean[None, :, None, None]) / torch.sqrt(var[None, :, None, None] + EPS)
            y = zh * P[bnp + "weight"][None, :, None, None] + P[bnp + "bias"][None, :, None, None]
            h = y * torch.sigmoid(y)
        ps[li] = h
    return [p.permute(0, 2, 3, 1) for p in ps], new


def neck_all(inputs, depth, train, dtype=torch.float64):
    """forward and backward of sum <p_k, gp_k> -> per level {fixture tensor name: numpy array}.  `inputs`:
    _dense_neck_cases.case_inputs(case)"""
    params, buffers = {}, {}
    for lv in inputs:
        params.update(lv["params"]); buffers.update(lv["buffers"])
    P = {n: torch.as_tensor(np.asarray(v)).to(dtype).requires_grad_(True) for n, v in params.items()}
    cs = [torch.as_tensor(lv["c"]).to(dtype).requires_grad_(True) for lv in inputs]
    ps, new = neck_forward(P, buffers, cs, [lv["k"] for lv in inputs], depth, train, dtype)
    torch.autograd.backward(ps, [torch.as_tensor(lv["gp"]).to(dtype) for lv in inputs])
    out = []
    for lv, c, p in zip(inputs, cs, ps):
        k = lv["k"]
        d = {"p": p.detach().contiguous().numpy(), "dc": c.grad.numpy()}
        for t in range(depth):
            b = f"smooth{k}.{3 * t + 1}."
            for s in ("running_mean", "running_var", "num_batches_tracked"):
                v = new.get(b + s, buffers[b + s])
                d[f"{s}.{t}"] = v.numpy() if torch.is_tensor(v) else np.asarray(v)
        for n in lv["params"]:
            d["g." + n] = P[n].grad.numpy()
        out.append(d)
    return out


def fit_reference(cfg, inputs, hinputs, dtype=torch.float64):
    """The end-to-end fit on the CPU in float64: `steps` times (neck and heads in train mode on the fixed feature maps,
    LossAF through tests/_lossaf_np.py and its gradient through tests/_lossaf_grad_np.py, SGD with momentum).
    -> the loss before every step and after the last one, [steps + 1]"""
    from _head_np import head_forward
    from _lossaf_grad_np import loss_af_grad, split_levels
    from _lossaf_np import loss_af
    A, C = cfg["A"], cfg["C"]
    gt = np.asarray(cfg["gt_xyxy"], np.float32)
    lab, off = np.asarray(cfg["gt_label"], np.int64), np.asarray(cfg["gt_off"], np.int32)
    P, bufs = {}, {}
    for lv in list(inputs) + list(hinputs):
        P.update({n: torch.as_tensor(v).to(dtype).requires_grad_(True) for n, v in lv["params"].items()})
        bufs.update(lv["buffers"])
    mom = {n: None for n in P}
    ks = [lv["k"] for lv in inputs]
    losses = []

    def loss_and_grads(backward):
        news = {}
        ps, new = neck_forward(P, bufs, [lv["c"] for lv in inputs], ks, cfg["depth"], True, dtype)
        news.update(new)
        ys = []
        for p, hv in zip(ps, hinputs):
            y, new, _ = head_forward(P, bufs, p, hv["k"], A, C, cfg["head_depth"], True, dtype)
            ys.append(y); news.update(new)
        levels = [y.detach().numpy() for y in ys]
        r = loss_af(levels, gt, lab, off, C, cfg["img_size"], dtype=np.float64)
        if backward:
            g = loss_af_grad(levels, gt, lab, off, C, cfg["img_size"], dtype=np.float64, assign=r["assign"])["grad"]
            torch.autograd.backward(ys, [torch.as_tensor(np.ascontiguousarray(gl)).to(dtype)
                                         for gl in split_levels(g, levels)])
        return r["box"] + r["obj"] + r["cls"], news

    for _ in range(cfg["steps"]):
        loss, news = loss_and_grads(True)
        losses.append(loss)
        with torch.no_grad():
            for n, v in P.items():
                mom[n] = v.grad.clone() if mom[n] is None else cfg["momentum"] * mom[n] + v.grad
                v -= cfg["lr"] * mom[n]
                v.grad = None
            bufs.update({n: (w.numpy() if torch.is_tensor(w) else w) for n, w in news.items()})
    losses.append(loss_and_grads(False)[0])
    return np.asarray(losses, np.float64)
