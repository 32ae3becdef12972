"""Inputs of the backbone-stage tests as a function of a seed (numpy's frozen RandomState), the fixture's layout, and the
stack restated in numpy at a chosen precision (float64 for references).

tests/golden/stage_train.npz (made by tests/golden/make_stage_fixtures.py from the oracle/backbones.py modules, torch
autograd, in float64 and in fp32 on the same fp32-valued inputs) holds, per case and mode ("train", and "eval" for the
first case)
    <case>/<mode>/r64     the float64 results, the tensors of tensor_shapes() flattened and concatenated
    <case>/<mode>/e32     per tensor: the fp32 run's own error max|r32 - r64| (over the WHOLE tensor)
    <case>/<mode>/max64   per tensor: max|r64| (over the whole tensor)
tensors: y, dx, b.<buffer name> for every BatchNorm buffer and g.<parameter name> for every parameter, under timm's
names.  A tensor of more than SAMPLE_ABOVE elements is stored at the SAMPLE flat indices of _head_cases.sample_indices()
only (the rule of the head fixture).

The restatement (stack_all) writes every operation out: the depthwise convolution and its two gradients tap by tap in
the kernels' documented order (ky, then kx, ascending; the input gradient as a gather over the taps whose
(i + p - ky) is a multiple of the stride), the 1x1 as a matrix product, BatchNorm and its backward from their definitions.
"""
import os

import numpy as np

from _head_cases import SAMPLE_ABOVE, bar, sample_indices  # noqa: F401  (re-exported)
from _launch_classes import cdiv, r16, split_plan

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIXTURE = os.path.join(GOLDEN, "stage_train.npz")
MOMENTUM = 0.1


def _uir(a, k, s, mid, c, name="0.0"):
    return dict(type="uir", a=a, k=k, s=s, mid=mid, c=c, name=name)


# the smallest shapes that reach each way of going wrong
CASES = [
    dict(name="a5k5s2", B=2, S=9, cin=8, blocks=[_uir(5, 5, 2, 24, 16)], seed=404),      # both depthwise, odd S under stride 2; also eval
    dict(name="a3k0s2", B=2, S=8, cin=8, blocks=[_uir(3, 0, 2, 16, 16)], seed=101),      # the stride taken by dw_start
    dict(name="a3k0res", B=2, S=5, cin=8, blocks=[_uir(3, 0, 1, 16, 8)], seed=101),      # residual with a BN-only dw_start
    dict(name="k3res", B=2, S=4, cin=8, blocks=[_uir(0, 3, 1, 16, 8)], seed=101),        # residual
    dict(name="ffn", B=2, S=3, cin=8, blocks=[_uir(0, 0, 1, 16, 12)], seed=101),         # no depthwise at all
    dict(name="ragged", B=2, S=4, cin=12, blocks=[_uir(0, 3, 1, 40, 20)], seed=101),     # channels % 16 != 0: ragged k step, p-tile
    dict(name="s2to1", B=2, S=2, cin=8, blocks=[_uir(5, 5, 2, 16, 8)], seed=101),        # two output rows in all
    dict(name="rows", B=3, S=10, cin=8, blocks=[_uir(0, 3, 1, 16, 8)], seed=101),        # 300 rows: two statistics tiles, one ragged
    # oracle_tiny's stage 3 + stage 4 (what BackboneTail makes of it): strided block, 5x5 residual block, the cn block
    dict(name="tiny_tail", B=2, S=4, cin=16, prefix="backbone.", seed=101,
         blocks=[_uir(3, 3, 2, 64, 24, "3.0"), _uir(0, 5, 1, 48, 24, "3.1"), dict(type="cn", k=1, s=1, c=32, name="4.0")]),
]
EVAL_CASE = "a5k5s2"
EPS = 1e-5
# seeds: the first of 101, 202, 303.., counting up, whose case passes the generator's admission rule
# (make_stage_fixtures.py --search prints them; a5k5s2: 101, 202 and 303 fail it in one of the two modes)

# the widths the zoo's backbones run (edge_n: mid 288 / 256, C5 480; edge_s / m / l: mid 576 / 512, C5 960), in
# tests/golden/stage_train_wide.npz.  Above 256 channels the row reductions and the depthwise weight gradient run a second
# channel group and the per-channel kernels a second workgroup; few rows, because every value in front of a ReLU has to
# pass the admission rule (the row-count classes are test_stage_depthwise_gpu.py's and test_head_gemm_fp32_gpu.py's)
WIDE = [
    # 72 quads: two groups, the last ragged; 5x5 stride 2 over two groups; pt 6 with three (NP 288) and five (NP 480) p-tiles
    dict(name="wide288", B=2, S=4, cin=48, blocks=[_uir(0, 5, 2, 288, 64), dict(type="cn", k=1, s=1, c=480, name="1.0")], seed=303),
    # two full groups; 3x3 stride 1 over two full groups; pt 4 with eight full p-tiles; a weight gradient with 8 q groups
    dict(name="wide512", B=2, S=3, cin=64, blocks=[_uir(3, 3, 1, 512, 64)], seed=1616),
]
FIXTURE_WIDE = os.path.join(GOLDEN, "stage_train_wide.npz")


def fixture_path(case):
    return FIXTURE_WIDE if any(case["name"] == w["name"] for w in WIDE) else FIXTURE

# the shapes of test_stage_depthwise_gpu.py, (B, S, C), each run for every (k, stride) of DW_OP_KS and every pass.  C 260 is
# 65 quads: a second channel group with one quad switched on; C 512 is two full groups; (2, 32, 4) gives 2048 / 512 output
# rows under stride 1 / 2: full row tiles; (3, 20, 4) gives 1200 / 300: a ragged last tile
DW_OP_KS = [(k, s) for k in (3, 5) for s in (1, 2)]
DW_OP_SHAPES = [(B, S, C) for S in (1, 2, 5, 8, 9) for C in (4, 20) for B in (1, 3)] + [(3, 10, 4), (3, 10, 20)]
DW_OP_WIDE = [(1, 5, 260), (1, 5, 512), (2, 32, 4), (3, 20, 4)]


def modes(case):
    return ("train", "eval") if case["name"] == EVAL_CASE else ("train",)


def out_size(S, k, s):
    return (S + 2 * ((k - 1) // 2) - k) // s + 1


def units(case):
    """the units in running order: dict(key (the module path under the prefix), dw, relu, k, s, cin, cout, first, last,
    res, conv / bn (names of the two layers))"""
    out, cin = [], case["cin"]
    pre = case.get("prefix", "")
    for b in case["blocks"]:
        base = f"{pre}blocks.{b['name']}."
        if b["type"] == "cn":
            us = [dict(key=base, conv="conv", bn="bn1", dw=False, relu=True, k=1, s=1, cin=cin, cout=b["c"])]
            res = False
        else:
            us = []
            if b["a"]:
                us.append(dict(key=base + "dw_start.", dw=True, relu=False, k=b["a"], s=b["s"] if not b["k"] else 1, cin=cin, cout=cin))
            us.append(dict(key=base + "pw_exp.", dw=False, relu=True, k=1, s=1, cin=cin, cout=b["mid"]))
            if b["k"]:
                us.append(dict(key=base + "dw_mid.", dw=True, relu=True, k=b["k"], s=b["s"], cin=b["mid"], cout=b["mid"]))
            us.append(dict(key=base + "pw_proj.", dw=False, relu=False, k=1, s=1, cin=b["mid"], cout=b["c"]))
            res = cin == b["c"] and b["s"] == 1
        for i, u in enumerate(us):
            u.setdefault("conv", "conv"); u.setdefault("bn", "bn")
            u.update(first=i == 0, last=i == len(us) - 1, res=res)
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
            S = out_size(S, u["k"], u["s"])
        out.append(S)
    return out


def case_inputs(case, seed=None):
    """-> dict(params {name: fp32}, buffers {name: array}, x [B,S,S,cin] fp32, gy [B,So,So,cout] fp32).  Weights
    ~ N(0, 1 / fan_in), gamma in [0.5, 1.5], beta ~ 0.2 N(0,1), running statistics are not the initial ones."""
    rs = np.random.RandomState(case["seed"] if seed is None else seed)
    f32 = np.float32
    params, buffers = {}, {}
    for name, shape in param_shapes(case).items():
        if len(shape) == 4:
            v = rs.standard_normal(shape) / np.sqrt(shape[1] * shape[2] * shape[3])
        elif name.endswith(".weight"):
            v = rs.uniform(0.5, 1.5, shape)
        else:
            v = 0.2 * rs.standard_normal(shape)
        params[name] = np.ascontiguousarray(v, f32)
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


def stored_indices(key, name, shape):
    n = int(np.prod(shape, dtype=np.int64))
    return sample_indices(key + "/" + name, n) if n > SAMPLE_ABOVE else None


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

def dw_forward(x, w, s):
    """depthwise k x k, pad (k - 1) / 2, stride s; w [C,1,k,k].  acc = 0; acc += x[tap] * w[tap], ky then kx ascending"""
    B, S, _, C = x.shape
    k = w.shape[-1]
    p, So = (k - 1) // 2, out_size(S, k, s)
    xp = np.zeros((B, S + 2 * p, S + 2 * p, C), x.dtype)
    xp[:, p:p + S, p:p + S] = x
    out = np.zeros((B, So, So, C), x.dtype)
    for ky in range(k):
        for kx in range(k):
            out = out + xp[:, ky:ky + (So - 1) * s + 1:s, kx:kx + (So - 1) * s + 1:s] * w[:, 0, ky, kx]
    return out


def dw_dgrad(dy, w, s, S):
    """the gradient of dw_forward's x as the kernel gathers it: input pixel (i, j) sums, ky then kx ascending, the taps
    with t = i + p - ky >= 0, t % s == 0, t / s < So (and the same along x): dy[t / s] * w[ky, kx]"""
    B, So, _, C = dy.shape
    k = w.shape[-1]
    p = (k - 1) // 2
    dx = np.zeros((B, S, S, C), dy.dtype)
    idx = np.arange(S)
    for ky in range(k):
        ty = idx + p - ky
        iy = idx[(ty >= 0) & (ty % s == 0) & (ty // s < So)]
        for kx in range(k):
            tx = idx + p - kx
            ix = idx[(tx >= 0) & (tx % s == 0) & (tx // s < So)]
            if len(iy) == 0 or len(ix) == 0:
                continue
            oy, ox = (iy + p - ky) // s, (ix + p - kx) // s
            dx[:, iy[:, None], ix[None, :]] = dx[:, iy[:, None], ix[None, :]] + dy[:, oy[:, None], ox[None, :]] * w[:, 0, ky, kx]
    return dx


def dw_wgrad(x, dy, k, s):
    """the gradient of dw_forward's w: dW[c, 0, ky, kx] = sum over the output pixels of dy * x[tap]"""
    B, S, _, C = x.shape
    p, So = (k - 1) // 2, dy.shape[1]
    xp = np.zeros((B, S + 2 * p, S + 2 * p, C), x.dtype)
    xp[:, p:p + S, p:p + S] = x
    dw = np.zeros((C, 1, k, k), x.dtype)
    for ky in range(k):
        for kx in range(k):
            dw[:, 0, ky, kx] = (xp[:, ky:ky + (So - 1) * s + 1:s, kx:kx + (So - 1) * s + 1:s] * dy).sum((0, 1, 2))
    return dw


def stack_all(case, inputs, train, dtype=np.float64):
    """forward and backward of <y, gy> -> {fixture tensor name: numpy array}"""
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
        o = xhat * P[bnp + "weight"] + P[bnp + "bias"]
        if u["relu"]:
            o = np.maximum(o, 0)
        if u["last"] and u["res"]:
            o = bin_ + o
        saved.append((h, xhat, invstd, o))
        h = o
    out["y"] = h
    g = inputs["gy"].astype(dt)
    G = None
    for u, (xin, xhat, invstd, o) in zip(us[::-1], saved[::-1]):
        w = P[u["key"] + u["conv"] + ".weight"]
        bnp = u["key"] + u["bn"] + "."
        if u["last"] and u["res"]:
            G = g
        if u["relu"]:
            g = g * (o > 0)
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


def plan_restated(case, B=None, S=None, stat_rows=256, gemm_rows=64):
    """the byte formulas of include/yololite_hip.h (yl_stage_plan_info) written again"""
    def splits(M, NP, NQ):
        return split_plan(M, NP, NQ, gemm_rows)[:2]

    B = case["B"] if B is None else B
    c = dict(case, S=case["S"] if S is None else S)
    szs = sizes(c)
    x0 = B * szs[0] ** 2 * case["cin"] * 4
    saved, amax, cmax, smax, wmax = x0, 0, 0, 0, 0
    per_block = []
    for u, So in zip(units(c), szs[1:]):
        M = B * So * So
        if u["first"]:
            per_block.append(0)
        per_block[-1] += 2 * M * u["cout"] * 4 + 2 * u["cout"] * 4
        amax, cmax = max(amax, M * u["cout"] * 4), max(cmax, u["cout"])
        smax = max(smax, r16(cdiv(M, stat_rows) * (u["k"] ** 2 if u["dw"] else 2) * u["cout"] * 8))
        if not u["dw"]:
            wmax = max(wmax, r16(splits(M, u["cin"], u["cout"])[1] * u["cin"] * u["cout"] * 4))
    return dict(blocks=per_block, saved_bytes=saved + sum(per_block), nosave_bytes=4 * amax + 2 * cmax * 4,
                workspace_bytes=3 * max(amax, x0) + smax + 2 * cmax * 4 + wmax)
