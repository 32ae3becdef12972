"""The dense FPN neck of tests/_dense_neck_np.py with the 3x3 convolution of every smooth block replaced by the
rounded-operand convolution of DetectNeckMS's precision "fp16" / "bf16": x and W are rounded (nearest even) on the way
in, dz on the way back, and the three products -- x (*) W, dz (*) W, x (*) dz -- are taken of the rounded values in the
restatement's own dtype (float64 for references).  Everything else is _dense_neck_np.neck_forward's arithmetic, op by op.

`jitter`: a torch.Generator; every value entering a rounding is first multiplied by 1 + s 2^-23, s in {-1, 0, 1} drawn
from it.  This is how the fixture measures what an ulp of difference in a COMPUTED operand (t, h, dz) does once a rounding
flips (tests/golden/make_dense_neck_amp_fixtures.py)."""
import numpy as np
import torch
import torch.nn.functional as TF

from _neck_np import EPS, MOMENTUM, _t, nearest_src

DTYPES = {"fp16": torch.float16, "bf16": torch.bfloat16}


def round_to(t, precision, jitter=None):
    if jitter is not None:
        s = torch.randint(-1, 2, t.shape, generator=jitter).to(t.dtype)
        t = t * (1 + s * 2.0 ** -23)
    return t.to(DTYPES[precision]).to(t.dtype)


class RoundedConv3x3(torch.autograd.Function):
    """z = conv3x3(r(x), r(W)), pad 1; dx = conv3x3^T(r(dz), r(W)); dW = r(x) (*) r(dz); r = round_to"""

    @staticmethod
    def forward(ctx, x, w, precision, jitter):
        xr, wr = round_to(x, precision, jitter), round_to(w, precision, jitter)
        ctx.save_for_backward(xr, wr)
        ctx.precision, ctx.jitter = precision, jitter
        return TF.conv2d(xr, wr, None, 1, 1)

    @staticmethod
    def backward(ctx, dz):
        xr, wr = ctx.saved_tensors
        dzr = round_to(dz, ctx.precision, ctx.jitter)
        dx = TF.conv_transpose2d(dzr, wr, None, 1, 1)
        dw = torch.nn.grad.conv2d_weight(xr, wr.shape, dzr, padding=1)
        return dx, dw, None, None


def neck_forward(params, buffers, cs, ks, depth, train, precision, dtype=torch.float64, jitter=None):
    """_dense_neck_np.neck_forward with RoundedConv3x3 -> ps NHWC finest first, {running stat name: new value}"""
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
            z = RoundedConv3x3.apply(h, P[f"smooth{k}.{3 * i}.weight"], precision, jitter)
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


def neck_all(inputs, depth, train, precision, dtype=torch.float64, jitter=None):
    """forward and backward of sum <p_k, gp_k> -> per level {fixture tensor name: numpy array}"""
    params, buffers = {}, {}
    for lv in inputs:
        params.update(lv["params"]); buffers.update(lv["buffers"])
    P = {n: torch.as_tensor(np.asarray(v)).to(dtype).requires_grad_(True) for n, v in params.items()}
    cs = [torch.as_tensor(lv["c"]).to(dtype).requires_grad_(True) for lv in inputs]
    ps, new = neck_forward(P, buffers, cs, [lv["k"] for lv in inputs], depth, train, precision, dtype, jitter)
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
