"""Inputs of the EfficientNet-Lite stage tests (yololite_amd.irops) as a function of a seed, the fixture's layout, and the
stack of `ir` blocks restated in numpy at a chosen precision (float64 for references), with TF-SAME padding and ReLU6
written out.

tests/golden/ir_train.npz and ir_train_wide.npz (made by tests/golden/make_ir_fixtures.py from oracle.backbones.
InvertedResidual with same=True, act="relu6", eps=1e-3, torch autograd, in float64 and in fp32 on the same fp32-valued
inputs) have the layout of the stage fixture (_stage_cases.py): per case and mode
    <case>/<mode>/r64     the float64 results, the tensors of tensor_shapes() flattened and concatenated
    <case>/<mode>/e32     per tensor: the fp32 run's own error max|r32 - r64| (over the WHOLE tensor)
    <case>/<mode>/max64   per tensor: max|r64| (over the whole tensor)
tensors: y, dx, b.<buffer name>, g.<parameter name> under timm's names; a tensor of more than SAMPLE_ABOVE elements is
stored at the SAMPLE flat indices of _head_cases.sample_indices() only.

A block:  conv_pw 1x1, bn1, ReLU6   conv_dw depthwise k x k stride s under TF-SAME, bn2, ReLU6   conv_pwl 1x1, bn3,
plus the block's input when cin == c and s == 1.
TF-SAME for odd k: So = ceil(S / s); total = max((So - 1) s + k - S, 0) zeros, of which total // 2 stand in front of the
first row and column and the rest behind the last.  ReLU6: min(max(y, 0), 6); its gradient passes where 0 < y < 6."""
import os

import numpy as np

from _stage_cases import GOLDEN, MOMENTUM, SAMPLE_ABOVE, bar, sample_indices, stored_indices  # noqa: F401  (re-exported)

FIXTURE = os.path.join(GOLDEN, "ir_train.npz")
FIXTURE_WIDE = os.path.join(GOLDEN, "ir_train_wide.npz")
EPS = 1e-3


def _ir(k, s, mid, c, name="0.0"):
    return dict(type="ir", k=k, s=s, mid=mid, c=c, name=name)


# the smallest shapes that reach each way of going wrong.  Seeds: the first of 101, 202, 303, ... that the generator admits
# (make_ir_fixtures.py --search prints them)
CASES = [
    dict(name="k3s2", B=2, S=8, cin=8, blocks=[_ir(3, 2, 48, 16)], seed=101),            # SAME differs from symmetric: pad begin 0
    dict(name="k5s2", B=2, S=6, cin=8, blocks=[_ir(5, 2, 48, 16)], seed=101),            # pad begin 1
    dict(name="k5s2odd", B=2, S=7, cin=8, blocks=[_ir(5, 2, 48, 16)], seed=101),         # odd S: SAME equals symmetric
    # one output row and column per image.  bn2 sees TWO values per channel, beta -+ gamma / sqrt(1 + eps / var): with beta
    # around 1 none of them reaches 6, so this case draws beta around 2.5 (above 6 where gamma > 3.5, below 0 where gamma > 2.5)
    dict(name="k3s2one", B=2, S=2, cin=8, blocks=[_ir(3, 2, 48, 16)], seed=101, beta=2.5),
    dict(name="k3res", B=2, S=4, cin=8, blocks=[_ir(3, 1, 48, 8)], seed=101),            # residual
    dict(name="ragged", B=2, S=4, cin=12, blocks=[_ir(5, 1, 72, 20)], seed=101),         # channels % 16 != 0
    dict(name="rows", B=3, S=10, cin=8, blocks=[_ir(3, 1, 48, 16)], seed=202),           # 300 rows: two statistics tiles, one ragged
    # a lite tail in small: a strided block, a residual block and a widening block under the checkpoint's names; also eval
    dict(name="lite_tiny_tail", B=2, S=4, cin=16, prefix="backbone.", seed=404,
         blocks=[_ir(5, 2, 96, 24, "5.0"), _ir(5, 1, 144, 24, "5.1"), _ir(3, 1, 144, 40, "6.0")]),
]
EVAL_CASE = "lite_tiny_tail"
# the widths the zoo's lite backbones run, few rows each: lite0's blocks 5.0 (mid 672, 5x5 stride 2) and 6.0 (mid 1152 -> 320),
# lite4's widest (stage 5: 272 -> 1632 -> 272).  Tens of thousands of values stand in front of a ReLU6 here and each has to keep
# 64 x the fp32 error (some 1e-5 at these widths) from both kinks, so few seeds are admitted: wide1152's is the 358th tried
WIDE = [
    dict(name="wide672", B=2, S=4, cin=112, blocks=[_ir(5, 2, 672, 192)], seed=202),
    dict(name="wide1152", B=2, S=3, cin=192, blocks=[_ir(3, 1, 1152, 320)], seed=36158),
    dict(name="wide1632", B=2, S=2, cin=272, blocks=[_ir(5, 1, 1632, 272)], seed=9494),
]


def fixture_path(case):
    return FIXTURE_WIDE if any(case["name"] == w["name"] for w in WIDE) else FIXTURE


def modes(case):
    return ("train", "eval") if case["name"] == EVAL_CASE else ("train",)


def out_size(S, s):
    """TF-SAME: ceil(S / s)"""
    return -(-S // s)


def pad_begin(k, s, S, same=True):
    """the zeros in front of the first row and column"""
    if not same:
        return (k - 1) // 2
    return max((out_size(S, s) - 1) * s + k - S, 0) // 2


def units(case):
    """the units in running order: dict(key (the block's path under the prefix), conv / bn (names of the two layers), dw,
    act, k, s, cin, cout, first, last, res)"""
    out, cin = [], case["cin"]
    pre = case.get("prefix", "")
    for b in case["blocks"]:
        assert b["type"] == "ir"
        key = f"{pre}blocks.{b['name']}."
        res = cin == b["c"] and b["s"] == 1
        us = [dict(key=key, conv="conv_pw", bn="bn1", dw=False, act=True, k=1, s=1, cin=cin, cout=b["mid"]),
              dict(key=key, conv="conv_dw", bn="bn2", dw=True, act=True, k=b["k"], s=b["s"], cin=b["mid"], cout=b["mid"]),
              dict(key=key, conv="conv_pwl", bn="bn3", dw=False, act=False, k=1, s=1, cin=b["mid"], cout=b["c"])]
        for i, u in enumerate(us):
            u.update(first=i == 0, last=i == 2, res=res)
        out += us
        cin = b["c"]
    return out


def param_shapes(case):
    """name -> shape of the parameters, unit by unit: conv weight, BatchNorm weight, BatchNorm bias"""
    out = {}
    for u in units(case):
        out[u["key"] + u["conv"] + ".weight"] = (u["cout"], 1 if u["dw"] else u["cin"], u["k"], u["k"])
        out[u["key"] + u["bn"] + ".weight"] = (u["cout"],)
        out[u["key"] + u["bn"] + ".bias"] = (u["cout"],)
    return out


def buffer_shapes(case):
    out = {}
    for u in units(case):
        p = u["key"] + u["bn"] + "."
        out.update({p + "running_mean": (u["cout"],), p + "running_var": (u["cout"],), p + "num_batches_tracked": ()})
    return out


def sizes(case):
    """S of x and of every unit's output"""
    S, out = case["S"], [case["S"]]
    for u in units(case):
        if u["dw"]:
            S = out_size(S, u["s"])
        out.append(S)
    return out


def case_inputs(case, seed=None):
    """-> dict(params {name: fp32}, buffers {name: array}, x [B,S,S,cin] fp32, gy [B,So,So,cout] fp32).  Weights
    ~ N(0, 1 / fan_in).  In front of a ReLU6 gamma is in [2, 4] and beta ~ beta0 + 0.2 N(0,1), beta0 = 1 unless the case says
    otherwise, so that the normalised values' tails reach both kinks (about 5 % above 6, a third below 0); bn3 has the stage cases' gamma in [0.5, 1.5], beta ~
    0.2 N(0,1).  The running statistics are not the initial ones."""
    rs = np.random.RandomState(case["seed"] if seed is None else seed)
    f32 = np.float32
    params, buffers = {}, {}
    for u in units(case):
        shape = (u["cout"], 1 if u["dw"] else u["cin"], u["k"], u["k"])
        params[u["key"] + u["conv"] + ".weight"] = np.ascontiguousarray(
            rs.standard_normal(shape) / np.sqrt(shape[1] * shape[2] * shape[3]), f32)
        if u["act"]:
            g, b = rs.uniform(2.0, 4.0, (u["cout"],)), case.get("beta", 1.0) + 0.2 * rs.standard_normal((u["cout"],))
        else:
            g, b = rs.uniform(0.5, 1.5, (u["cout"],)), 0.2 * rs.standard_normal((u["cout"],))
        params[u["key"] + u["bn"] + ".weight"], params[u["key"] + u["bn"] + ".bias"] = g.astype(f32), b.astype(f32)
    for i, u in enumerate(units(case)):
        p = u["key"] + u["bn"] + "."
        buffers[p + "running_mean"] = (0.3 * rs.standard_normal((u["cout"],))).astype(f32)
        buffers[p + "running_var"] = rs.uniform(0.5, 1.5, (u["cout"],)).astype(f32)
        buffers[p + "num_batches_tracked"] = np.asarray(3 + i, np.int64)
    B, So = case["B"], sizes(case)[-1]
    x = rs.standard_normal((B, case["S"], case["S"], case["cin"])).astype(f32)
    gy = rs.standard_normal((B, So, So, case["blocks"][-1]["c"])).astype(f32)
    return dict(params=params, buffers=buffers, x=x, gy=gy)


def tensor_shapes(case):
    """name -> shape of the tensors of one case in the fixture, in the archive's order"""
    B, So = case["B"], sizes(case)[-1]
    out = {"y": (B, So, So, case["blocks"][-1]["c"]), "dx": (B, case["S"], case["S"], case["cin"])}
    out.update({"b." + n: sh for n, sh in buffer_shapes(case).items()})
    out.update({"g." + n: sh for n, sh in param_shapes(case).items()})
    return out


def fixture_tensors(z, case, mode):
    """-> {tensor name: (r64 values [flat, at idx], idx or None (= every element), e32, max64)}"""
    key = f"{case['name']}/{mode}"
    r64, e32, m64 = z[key + "/r64"], z[key + "/e32"], z[key + "/max64"]
    out, o = {}, 0
    for i, (name, shape) in enumerate(tensor_shapes(case).items()):
        idx = stored_indices(key, name, shape)
        n = len(idx) if idx is not None else int(np.prod(shape, dtype=np.int64))
        out[name] = (r64[o:o + n], idx, float(e32[i]), float(m64[i]))
        o += n
    assert o == len(r64)
    return out


# ---- the restatement.  Every array is NHWC in `dtype`; sums of more than two terms run in the order written

def _padded(x, k, s, So, pb):
    """x with pb zeros in front of the first row and column and as many behind the last as the taps of So outputs reach"""
    B, S, _, C = x.shape
    E = max((So - 1) * s + k, pb + S)
    xp = np.zeros((B, E, E, C), x.dtype)
    xp[:, pb:pb + S, pb:pb + S] = x
    return xp


def dw_forward(x, w, s, same=True):
    """depthwise k x k of stride s; w [C,1,k,k]; output row i, tap ky reads input row i s + ky - pb.  acc = 0;
    acc += x[tap] * w[tap], ky then kx ascending"""
    B, S, _, C = x.shape
    k = w.shape[-1]
    So, pb = out_size(S, s), pad_begin(k, s, S, same)
    xp = _padded(x, k, s, So, pb)
    out = np.zeros((B, So, So, C), x.dtype)
    for ky in range(k):
        for kx in range(k):
            out = out + xp[:, ky:ky + (So - 1) * s + 1:s, kx:kx + (So - 1) * s + 1:s] * w[:, 0, ky, kx]
    return out


def dw_dgrad(dy, w, s, S, same=True):
    """the gradient of dw_forward's x as the kernel gathers it: input pixel (i, j) sums, ky then kx ascending, the taps
    with t = i + pb - ky >= 0, t % s == 0, t / s < So (and the same along x): dy[t / s] * w[ky, kx]"""
    B, So, _, C = dy.shape
    k = w.shape[-1]
    pb = pad_begin(k, s, S, same)
    dx = np.zeros((B, S, S, C), dy.dtype)
    idx = np.arange(S)
    for ky in range(k):
        ty = idx + pb - ky
        iy = idx[(ty >= 0) & (ty % s == 0) & (ty // s < So)]
        for kx in range(k):
            tx = idx + pb - kx
            ix = idx[(tx >= 0) & (tx % s == 0) & (tx // s < So)]
            if len(iy) == 0 or len(ix) == 0:
                continue
            oy, ox = (iy + pb - ky) // s, (ix + pb - kx) // s
            dx[:, iy[:, None], ix[None, :]] = dx[:, iy[:, None], ix[None, :]] + dy[:, oy[:, None], ox[None, :]] * w[:, 0, ky, kx]
    return dx


def dw_wgrad(x, dy, k, s, same=True):
    """the gradient of dw_forward's w: dW[c, 0, ky, kx] = sum over the output pixels of dy * x[tap]"""
    B, S, _, C = x.shape
    So, pb = dy.shape[1], pad_begin(k, s, S, same)
    xp = _padded(x, k, s, So, pb)
    dw = np.zeros((C, 1, k, k), x.dtype)
    for ky in range(k):
        for kx in range(k):
            dw[:, 0, ky, kx] = (xp[:, ky:ky + (So - 1) * s + 1:s, kx:kx + (So - 1) * s + 1:s] * dy).sum((0, 1, 2))
    return dw


def stack_all(case, inputs, train, dtype=np.float64, pre_act=None):
    """forward and backward of <y, gy> -> {fixture tensor name: numpy array}.  `pre_act`: a list that receives every
    BatchNorm output in front of a ReLU6, in running order"""
    dt = dtype
    P = {n: np.asarray(v).astype(dt) for n, v in inputs["params"].items()}
    buf = inputs["buffers"]
    us = units(case)
    h = inputs["x"].astype(dt)
    out, saved = {}, []
    for u in us:
        if u["first"]:
            bin_ = h
        w = P[u["key"] + u["conv"] + ".weight"]
        bnp = u["key"] + u["bn"] + "."
        z = dw_forward(h, w, u["s"]) if u["dw"] else h @ w[:, :, 0, 0].T
        M = z.shape[0] * z.shape[1] * z.shape[2]
        rm, rv = buf[bnp + "running_mean"].astype(dt), buf[bnp + "running_var"].astype(dt)
        nbt = np.asarray(buf[bnp + "num_batches_tracked"])
        if train:
            mean = z.mean((0, 1, 2), dtype=dt)
            var = ((z - mean) ** 2).mean((0, 1, 2), dtype=dt)
            rm = ((1 - MOMENTUM) * rm + MOMENTUM * mean).astype(dt)
            rv = ((1 - MOMENTUM) * rv + MOMENTUM * (var * M / (M - 1))).astype(dt)
            nbt = nbt + 1
        else:
            mean, var = rm, rv
        out["b." + bnp + "running_mean"], out["b." + bnp + "running_var"] = rm, rv
        out["b." + bnp + "num_batches_tracked"] = nbt
        invstd = (1.0 / np.sqrt(var + dt(EPS))).astype(dt)
        xhat = (z - mean) * invstd
        y = xhat * P[bnp + "weight"] + P[bnp + "bias"]
        o = y
        if u["act"]:
            if pre_act is not None:
                pre_act.append(y)
            o = np.minimum(np.maximum(y, 0), 6)                # ReLU6
        if u["last"] and u["res"]:
            o = bin_ + o
        saved.append((h, xhat, invstd, y))
        h = o
    out["y"] = h
    g = inputs["gy"].astype(dt)
    G = None
    for u, (xin, xhat, invstd, y) in zip(us[::-1], saved[::-1]):
        w = P[u["key"] + u["conv"] + ".weight"]
        bnp = u["key"] + u["bn"] + "."
        if u["last"] and u["res"]:
            G = g
        if u["act"]:
            g = g * ((y > 0) & (y < 6))                        # both strict: torch's hardtanh_backward
        M = g.shape[0] * g.shape[1] * g.shape[2]
        dbeta, dgamma = g.sum((0, 1, 2), dtype=dt), (g * xhat).sum((0, 1, 2), dtype=dt)
        out["g." + bnp + "bias"], out["g." + bnp + "weight"] = dbeta, dgamma
        scale = P[bnp + "weight"] * invstd
        dz = scale * (g - dbeta / M - xhat * (dgamma / M)) if train else scale * g
        dz = dz.astype(dt)
        if u["dw"]:
            out["g." + u["key"] + u["conv"] + ".weight"] = dw_wgrad(xin, dz, u["k"], u["s"])
            g = dw_dgrad(dz, w, u["s"], xin.shape[1])
        else:
            out["g." + u["key"] + u["conv"] + ".weight"] = (dz.reshape(M, -1).T @ xin.reshape(M, -1))[:, :, None, None]
            g = dz @ w[:, :, 0, 0]
        if u["first"] and u["res"]:
            g = g + G
    out["dx"] = g
    return {n: np.asarray(out[n]) for n in tensor_shapes(case)}


def as_uib(case):
    """the case with every ir block written as the uir block with a = 0 it is, unit for unit (UIBStack's form), and the map
    IRStack state-dict key -> UIBStack state-dict key"""
    blocks = [dict(type="uir", a=0, k=b["k"], s=b["s"], mid=b["mid"], c=b["c"], name=b["name"]) for b in case["blocks"]]
    ren = {"conv_pw.": "pw_exp.conv.", "bn1.": "pw_exp.bn.", "conv_dw.": "dw_mid.conv.", "bn2.": "dw_mid.bn.",
           "conv_pwl.": "pw_proj.conv.", "bn3.": "pw_proj.bn."}

    def key(k):
        for a, b in ren.items():
            if "." + a in k:
                return k.replace("." + a, "." + b)
        raise KeyError(k)
    return dict(case, blocks=blocks), key
