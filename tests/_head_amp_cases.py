"""Cases and references of the mixed-precision tests of DetectHeads' 1x1 GEMMs (precision "fp16" / "bf16": both operands
rounded to nearest even, products exact, fp32 accumulation).

Op level (headops.head_gemm over yl_head_gemm).  The shapes are those of _head_cases.py, every level of every case: they
are the smallest at which yl_head_gemm_kernel can go wrong (F 20: a ragged 16-wide k step; A 2: the anchor path of the
level layout; F 244: several k steps and pt = 4 against 6; NE 85 and the 96-wide p-tile; 1152 rows: several row tiles and
weight-gradient splits with a ragged last one; S = 2).  The weights are the case's own (random fp32 values no 16-bit type
holds), the activation operands are drawn here.  The reference of an op is the float64 product of the RNE-rounded operands
(torch's .to(float16 / bfloat16) is RNE; the bias of the outputs' forward is added unrounded), the bar is _head_cases.bar
with e32 = the error of torch's fp32 CPU product of the SAME rounded operands: no rounding can flip, the operands are
given.  `unrounded` is the float64 result of the operands as they are: it must lie outside the bar, or the case could
not see a missing rounding.

Whole module: tests/golden/head_amp.npz (made by tests/golden/make_head_amp_fixtures.py from the reference's own make_head
/ _forward_head with its 1x1 convolutions computing Rounded1x1 below), per case, mode, precision and level
    <case>/<mode>/<precision>/L<i>/r64     the rounded-operand float64 results, _head_cases.tensor_shapes() flattened and
                                           concatenated (large tensors at _head_cases.stored_indices() only)
    <case>/<mode>/<precision>/L<i>/flip    per tensor: the flip allowance, over the WHOLE tensor
    <case>/<mode>/<precision>/L<i>/max64   per tensor: max|r64| (over the whole tensor)
There the rounded operands d, h, dz are computed fp32 values: an ulp of difference flips some roundings and one flip shows
in the max norm.  The flip allowance is measured on the reference as tests/_dense_neck_amp_cases.py describes it: FLIP_RUNS
fp32 runs in which every value entering a rounding is first multiplied by 1 + s 2^-23, s in {-1, 0, 1} at random (seed
FLIP_SEED + run); flip = the largest max|r32_j - r64|.  Bar = max(4 flip, 2 fp32 ulps at max64)."""
import functools
import os

import numpy as np
import torch
import torch.nn.functional as TF

from _dense_neck_amp_np import DTYPES, round_to
from _head_cases import CASES, WIDE, bar, case_inputs, stored_indices, tensor_shapes  # noqa: F401  (bar is re-exported)
from _head_np import EPS, MOMENTUM

PRECISIONS = ("fp16", "bf16")
PASSES = ("forward", "dgrad", "wgrad")
SITES = (0, "out")
BY_NAME = {c["name"]: c for c in CASES + WIDE}          # the op level runs over the wide cases as well


def rounded(t: torch.Tensor, precision: str) -> torch.Tensor:
    """fp32 -> the nearest value of the 16-bit type (ties to even), as fp32"""
    return t.to(DTYPES[precision]).to(torch.float32)


# ---- the output convolutions as one matrix: column n = a * E + e of the level tensor <-> a row of box / obj / cls

def cat_rows(box, obj, cls, A, C):
    """[4A, ...], [A, ...], [A C, ...] -> [A (5 + C), ...] in the level tensor's channel order"""
    rows = []
    for a in range(A):
        rows += [box[4 * a:4 * a + 4], obj[a:a + 1], cls[C * a:C * (a + 1)]]
    return torch.cat(rows, 0)


def split_rows(m, A, C):
    """the inverse of cat_rows: [A (5 + C), ...] -> (box [4A, ...], obj [A, ...], cls [A C, ...])"""
    E = 5 + C
    blk = [m[a * E:(a + 1) * E] for a in range(A)]
    return torch.cat([b[:4] for b in blk], 0), torch.cat([b[4:5] for b in blk], 0), torch.cat([b[5:] for b in blk], 0)


def level_weights(case, li):
    """-> dict(W1 [F,F] of block 0, Wout [NE,F], bout [NE]) as fp32 tensors, from the case's own parameters"""
    lv = case_inputs(case)[li]
    k, A, C, F = lv["k"], case["A"], case["C"], case["F"]
    p = {n: torch.from_numpy(v) for n, v in lv["params"].items()}
    o = f"head{k}.out."
    return dict(W1=p[f"head{k}.trunk.0.block.1.weight"].reshape(F, F),
                Wout=cat_rows(p[o + "box.weight"], p[o + "obj.weight"], p[o + "cls.weight"], A, C).reshape(-1, F),
                bout=cat_rows(p[o + "box.bias"], p[o + "obj.bias"], p[o + "cls.bias"], A, C))


def to_rows(y):
    """level tensor [B,A,S,S,E] -> [M, A E]"""
    B, A, S, _, E = y.shape
    return y.permute(0, 2, 3, 1, 4).reshape(B * S * S, A * E)


def to_level(y2, B, A, S):
    return y2.reshape(B, S, S, A, -1).permute(0, 3, 1, 2, 4).contiguous()


def gemm_pass(site, pass_, a, b, W, bias, A):
    """the six GEMMs on operands of one dtype (see headops.head_gemm), on the CPU.  W: W1 [F,F] or Wout [NE,F]; the
    outputs' weight gradient comes back as ONE matrix [NE,F] in the level tensor's channel order"""
    out = site == "out"
    if pass_ == "forward":
        B, S, _, F = a.shape
        z = a.reshape(-1, F) @ W.t()
        return to_level(z + bias.to(z.dtype), B, A, S) if out else z.reshape(B, S, S, -1)
    if pass_ == "dgrad":
        if out:
            B, _, S, _, _ = a.shape
            return (to_rows(a) @ W).reshape(B, S, S, -1)
        return (a.reshape(-1, a.shape[3]) @ W).reshape(a.shape)
    F = a.shape[3]
    g = to_rows(b) if out else b.reshape(-1, F)
    dW = g.t() @ a.reshape(-1, F)
    return dW if out else dW.reshape(F, F, 1, 1)


def op_operands(case, li, site, pass_):
    """random fp32 activation operands that no 16-bit type holds -> (a, b or None)"""
    g = torch.Generator().manual_seed(case["seed"] + 1000 * li + 17 * PASSES.index(pass_) + (7 if site == "out" else 0))
    B, S, F, A, E = case["B"], case["sizes"][li], case["F"], case["A"], 5 + case["C"]
    rows, lvl = (B, S, S, F), (B, A, S, S, E)
    a = torch.randn(lvl if (site == "out" and pass_ == "dgrad") else rows, generator=g)
    b = torch.randn(lvl if site == "out" else rows, generator=g) if pass_ == "wgrad" else None
    return a, b


def reference(case, li, site, pass_, a, b, precision, W=None, bias=None):
    """-> dict(r64, e32, max64, bar, unrounded) of given fp32 operands (W, bias: the level's own unless given)"""
    w = level_weights(case, li)
    W = (w["Wout"] if site == "out" else w["W1"]) if W is None else W
    bias = w["bout"] if bias is None else bias
    A = case["A"]
    ra, rW = rounded(a, precision), rounded(W, precision)
    rb = rounded(b, precision) if b is not None else None
    d = lambda t: None if t is None else t.double()     # noqa: E731
    r64 = gemm_pass(site, pass_, d(ra), d(rb), d(rW), d(bias), A)
    r32 = gemm_pass(site, pass_, ra, rb, rW, bias, A)
    e32 = float((r32.double() - r64).abs().max())
    m64 = float(r64.abs().max())
    return dict(r64=r64, e32=e32, max64=m64, bar=bar(e32, m64), unrounded=gemm_pass(site, pass_, d(a), d(b), d(W), d(bias), A))


@functools.lru_cache(maxsize=None)
def op_reference(name, li, site, pass_, precision):
    """computed once per (case, level, site, pass, precision) and shared; callers do not write to it"""
    case = BY_NAME[name]
    a, b = op_operands(case, li, site, pass_)
    return dict(reference(case, li, site, pass_, a, b, precision), a=a, b=b)


# ---- ties: operands on rounding midpoints with small-integer partners; every product and sum is exact in fp32
TIE_EPS = {"fp16": 2.0 ** -11, "bf16": 2.0 ** -8}      # half an ulp of the 16-bit type at 1


def tie_operands(case, li, site, pass_, precision, seed=1401):
    """the first operand is 1 + eps or 1 + 3 eps (midpoints: ties-to-even gives 1 and 1 + 4 eps); the weights (forward,
    dgrad), the bias and the second operand (wgrad) are small integers -> (a, b or None, W, bias)"""
    rs = np.random.RandomState(seed + PASSES.index(pass_) + (3 if site == "out" else 0))
    eps = TIE_EPS[precision]
    a0, b0 = op_operands(case, li, site, pass_)
    a = torch.from_numpy((1.0 + eps * rs.choice([1.0, 3.0], tuple(a0.shape))).astype(np.float32))
    b = None if b0 is None else torch.from_numpy(rs.randint(-2, 3, tuple(b0.shape)).astype(np.float32))
    w = level_weights(case, li)
    W = w["Wout"] if site == "out" else w["W1"]
    W = torch.from_numpy(rs.randint(-2, 3, tuple(W.shape)).astype(np.float32))
    bias = torch.from_numpy(rs.randint(-2, 3, tuple(w["bout"].shape)).astype(np.float32))
    assert not torch.equal(rounded(a, precision), a)
    return a, b, W, bias


# ---- the whole module

AMP_FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "head_amp.npz")
FLIP_RUNS, FLIP_SEED = 8, 5200
AMP_EVAL_CASE = "base"


def _amp_cases():
    """a2c1, c80 and base with the shapes and input recipe of _head_cases.py.  Every (case, mode, precision, level) must pass
    the admission rule of make_head_amp_fixtures.py and must be able to tell the unrounded result from the rounded one in at
    least one of y, dx and block 0's 1x1 weight gradient (test_head_amp_cpu.py); a case whose inputs cannot gets another
    seed HERE, never another rule.  It must also pass the bf16 rule of make_head_amp_fixtures.py (a level whose jittered
    runs flipped no forward rounding has no value of d that the kernel's own summation order rounds the other way).
    `c80` did (404: fp16 level 0 cannot tell, all three tensors inside the bar, 6404 likewise; 1404 .. 4404, 7404 and 8404
    fail the admission rule at level 0; 5404 fails the bf16 rule at level 1; 9404 is the first of 404 + 1000 i that passes
    all three) and `base` did (101 fails the bf16 rule at level 0: its eight jittered runs flip nothing there and one element
    of d rounds the other way in the kernel's order; 1101 passes)."""
    seeds = {"c80": 9404, "base": 1101}
    return [dict(BY_NAME[n], seed=seeds.get(n, BY_NAME[n]["seed"])) for n in ("a2c1", "c80", "base")]


AMP_CASES = _amp_cases()


def amp_modes(case):
    return ("train", "eval") if case["name"] == AMP_EVAL_CASE else ("train",)


def amp_fixture_tensors(z, case, mode, precision, li):
    """-> {tensor name: (r64 values [flat, at idx], idx or None (= every element), flip, max64)}"""
    key = f"{case['name']}/{mode}/{precision}/L{li}"
    r64, flip, m64 = z[key + "/r64"], z[key + "/flip"], z[key + "/max64"]
    out, o = {}, 0
    for i, (name, shape) in enumerate(tensor_shapes(case, 3 + li, case["sizes"][li]).items()):
        idx = stored_indices(f"{case['name']}/{mode}/L{li}", name, shape)
        n = len(idx) if idx is not None else int(np.prod(shape, dtype=np.int64))
        out[name] = (r64[o:o + n], idx, float(flip[i]), float(m64[i]))
        o += n
    assert o == len(r64)
    return out


FORWARD_FLIPS = {"n": 0}       # activations whose rounding the jitter flipped, summed over Rounded1x1.forward calls


class Rounded1x1(torch.autograd.Function):
    """z = conv1x1(r(x), r(W)) + bias; dx = conv1x1^T(r(dz), r(W)); dW = r(dz)^T r(x); dbias = sum of the UNROUNDED dz;
    r = round_to (with `jitter`: see _dense_neck_amp_np.round_to)"""

    @staticmethod
    def forward(ctx, x, w, bias, precision, jitter):
        xr, wr = round_to(x, precision, jitter), round_to(w, precision, jitter)
        if jitter is not None:
            FORWARD_FLIPS["n"] += int((xr != round_to(x, precision)).sum())
        ctx.save_for_backward(xr, wr)
        ctx.precision, ctx.jitter, ctx.has_bias = precision, jitter, bias is not None
        return TF.conv2d(xr, wr, bias)

    @staticmethod
    def backward(ctx, dz):
        xr, wr = ctx.saved_tensors
        dzr = round_to(dz, ctx.precision, ctx.jitter)
        dx = TF.conv_transpose2d(dzr, wr)
        dw = torch.nn.grad.conv2d_weight(xr, wr.shape, dzr)
        return dx, dw, (dz.sum((0, 2, 3)) if ctx.has_bias else None), None, None


def device_order_d(lv):
    """block 0's d = dw3x3(x) as csrc/yl_block.h's yl_head_dw_kernel sums it: fp32, the nine taps in (ky, kx) order, one
    rounding per product and per sum (the unit is compiled without contraction), taps outside the image skipped"""
    x, w = lv["x"], lv["params"][f"head{lv['k']}.trunk.0.block.0.weight"]
    B, S, _, F = x.shape
    xp = np.zeros((B, S + 2, S + 2, F), np.float32)
    xp[:, 1:-1, 1:-1] = x
    acc = np.zeros((B, S, S, F), np.float32)
    for ky in range(3):
        for kx in range(3):
            acc = acc + xp[:, ky:ky + S, kx:kx + S] * w[None, None, None, :, 0, ky, kx]     # float32 arrays: two roundings
    return torch.from_numpy(acc)


def d_flips(lv, precision):
    """how many elements of device_order_d round to another 16-bit value than the float64 d"""
    x, w = torch.from_numpy(lv["x"]).double(), torch.from_numpy(lv["params"][f"head{lv['k']}.trunk.0.block.0.weight"]).double()
    d64 = TF.conv2d(x.permute(0, 3, 1, 2), w, None, 1, 1, 1, x.shape[3]).permute(0, 2, 3, 1)
    return int((d64.to(DTYPES[precision]).double() != device_order_d(lv).to(DTYPES[precision]).double()).sum())


def head_forward_amp(P, buffers, x, k, A, C, depth, train, precision, jitter=None):
    """_head_np.head_forward with Rounded1x1 in the place of every 1x1 convolution; P, x: tensors of the run's dtype"""
    dtype = x.dtype
    h = x.permute(0, 3, 1, 2)
    B, F, S, _ = h.shape
    M = B * S * S
    new, bn_out = {}, []
    for t in range(depth):
        p = f"head{k}.trunk.{t}.block."
        d = TF.conv2d(h, P[p + "0.weight"], None, 1, 1, 1, F)
        z = Rounded1x1.apply(d, P[p + "1.weight"], None, precision, jitter)
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
    box = Rounded1x1.apply(h, P[o + "box.weight"], P[o + "box.bias"], precision, jitter).view(B, A, 4, S, S)
    obj = Rounded1x1.apply(h, P[o + "obj.weight"], P[o + "obj.bias"], precision, jitter).view(B, A, 1, S, S)
    cls = Rounded1x1.apply(h, P[o + "cls.weight"], P[o + "cls.bias"], precision, jitter).view(B, A, C, S, S)
    return torch.cat([box, obj, cls], 2).permute(0, 1, 3, 4, 2).contiguous(), new, bn_out


def head_all_amp(case, lv, train, precision, dtype=torch.float64, jitter=None):
    """forward and backward of one level -> {fixture tensor name: numpy array} (the names of _head_np.head_all)"""
    k, A, C, depth = lv["k"], case["A"], case["C"], case["depth"]
    P = {n: torch.as_tensor(np.asarray(v)).to(dtype).requires_grad_(True) for n, v in lv["params"].items()}
    x = torch.as_tensor(np.asarray(lv["x"])).to(dtype).requires_grad_(True)
    y, new, _ = head_forward_amp(P, lv["buffers"], x, k, A, C, depth, train, precision, jitter)
    y.backward(torch.as_tensor(np.asarray(lv["gy"])).to(dtype))
    out = {"y": y.detach().numpy(), "dx": x.grad.numpy()}
    for t in range(depth):
        p = f"head{k}.trunk.{t}.block.2."
        for s in ("running_mean", "running_var", "num_batches_tracked"):
            v = new.get(p + s, lv["buffers"][p + s])
            out[f"{s}.{t}"] = v.numpy() if torch.is_tensor(v) else np.asarray(v)
    for n, v in P.items():
        out["g." + n] = v.grad.numpy()
    return out
