"""Inputs of the dense-stem tests as a function of a seed (numpy's frozen RandomState), the fixture's layout, and the
stack restated in numpy at a chosen precision (float64 for references).

tests/golden/stem_train.npz (made by tests/golden/make_stem_fixtures.py from the oracle/backbones.py modules, torch
autograd, in float64 and in fp32 on the same fp32-valued inputs) has the layout of stage_train.npz (_stage_cases.py):
per case and mode ("train", and "eval" for EVAL_CASE) <case>/<mode>/r64, /e32, /max64 over the tensors of
tensor_shapes(): y, dx (cases with an NHWC input only: the planar image has no gradient), b.<buffer name>, g.<parameter
name>; a tensor of more than SAMPLE_ABOVE elements is stored at the flat indices of _head_cases.sample_indices() only.
The composite case `tiny_backbone` (the whole oracle_tiny FeatureBackbone, image -> [c3, c4, c5], loss sum_k <c_k, g_k>
with independent g3, g4, g5) stores y.c3, y.c4, y.c5 in place of y and no dx.

The restatement writes every operation out: the dense convolution and its two gradients tap by tap in the kernels'
documented order ((ty, tx) ascending; the input gradient under stride 1 as a gather over the flipped taps, under stride 2
as four parity classes of input pixels, each gathering its 1, 2, 2 or 4 taps and dropping those whose output index is
>= S_out), the 1x1 as a matrix product over every s-th pixel, BatchNorm and its backward from their definitions.
"""
import os

import numpy as np

import _stage_cases as sc
from _head_cases import SAMPLE_ABOVE, bar, sample_indices  # noqa: F401  (re-exported)

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIXTURE = os.path.join(GOLDEN, "stem_train.npz")
MOMENTUM = 0.1
EPS = 1e-5


def _u(k, s, c, conv=None, bn=None):
    d = dict(k=k, s=s, c=c)
    if conv:
        d.update(conv=conv, bn=bn)
    return d


# the smallest shapes that reach each way of going wrong
CASES = [
    dict(name="planar3", B=2, S=9, cin=3, planar=True, units=[_u(3, 2, 8)], seed=101),      # odd S; K = 27 of 36
    dict(name="s2even", B=2, S=8, cin=8, planar=False, units=[_u(3, 2, 12)], seed=101),     # even S; ragged cout
    dict(name="s1", B=2, S=5, cin=12, planar=False, units=[_u(3, 1, 20)], seed=101),
    dict(name="pw", B=2, S=4, cin=8, planar=False, units=[_u(1, 1, 12)], seed=101),         # a 1x1 unit
    dict(name="s2to1", B=2, S=2, cin=8, planar=False, units=[_u(3, 2, 8)], seed=101),       # two output rows in all
    dict(name="rows", B=3, S=20, cin=8, planar=False, units=[_u(3, 2, 8)], seed=101),       # 300 output rows: two statistics
                                                                                           # tiles, one ragged; 3 x 3 spatial tiles
    # oracle_tiny's stem + stage 0 + stage 1 (what BackboneStem makes of it): four units, planar input; also eval
    dict(name="stem_to_c3", B=2, S=16, cin=3, planar=True, prefix="backbone.", seed=101,
         units=[_u(3, 2, 16, "conv_stem", "bn1"), _u(3, 2, 8, "blocks.0.0.conv", "blocks.0.0.bn1"),
                _u(3, 2, 16, "blocks.1.0.conv", "blocks.1.0.bn1"), _u(1, 1, 8, "blocks.1.1.conv", "blocks.1.1.bn1")]),
]
EVAL_CASE = "stem_to_c3"
# the widths the zoo's stems run (stage 1 of mobilenetv4_conv_small: 32 -> 96 channels, 3x3 stride 2), in
# tests/golden/stem_train_wide.npz: the convolution with 48 output channels per workgroup (PT 3) and two channel blocks,
# and its weight gradient with two 64-wide blocks of dz channels
WIDE = [
    dict(name="wide96", B=2, S=4, cin=32, planar=False, units=[_u(3, 2, 96)], seed=101),
]
FIXTURE_WIDE = os.path.join(GOLDEN, "stem_train_wide.npz")


def fixture_path(case):
    return FIXTURE_WIDE if any(case["name"] == w["name"] for w in WIDE) else FIXTURE


# the whole oracle_tiny backbone: the stem_to_c3 units, then stage 2 (C3 -> C4) and stages 3 + 4 (C4 -> C5) as _stage_cases cases
TINY = dict(name="tiny_backbone", B=2, S=64, seed=34037,
            stem=dict(CASES[-1], name="tiny_backbone.stem", S=64),
            mid=dict(name="tiny_backbone.mid", B=2, S=8, cin=8, prefix="backbone.",
                     blocks=[sc._uir(5, 5, 2, 24, 16, "2.0"), sc._uir(0, 3, 1, 32, 16, "2.1"), sc._uir(3, 0, 1, 64, 16, "2.2")]),
            tail=dict(name="tiny_backbone.tail", B=2, S=4, cin=16, prefix="backbone.",
                      blocks=[sc._uir(3, 3, 2, 64, 24, "3.0"), sc._uir(0, 5, 1, 48, 24, "3.1"), dict(type="cn", k=1, s=1, c=32, name="4.0")]))
# seeds: the first of 101, 202, 303.., counting up, whose case passes the generator's admission rule
# (make_stem_fixtures.py --search prints them; tiny_backbone has seventeen ReLUs behind one another over up to 32768 values
# and the fp32 run's error grows with depth: 101 .. 33936 each put a BatchNorm output within 64 fp32 errors of zero)


def modes(case):
    return ("train", "eval") if case["name"] == EVAL_CASE else ("train",)


out_size = sc.out_size


def units(case):
    """the units in running order: dict(conv, bn (full names of the two layers), k, s, cin, cout)"""
    out, cin = [], case["cin"]
    pre = case.get("prefix", "")
    for i, u in enumerate(case["units"]):
        out.append(dict(conv=pre + u.get("conv", f"units.{i}.conv"), bn=pre + u.get("bn", f"units.{i}.bn1"), k=u["k"], s=u["s"],
                        cin=cin, cout=u["c"]))
        cin = u["c"]
    return out


def param_shapes(case):
    out = {}
    for u in units(case):
        out[u["conv"] + ".weight"] = (u["cout"], u["cin"], u["k"], u["k"])
        out[u["bn"] + ".weight"] = (u["cout"],)
        out[u["bn"] + ".bias"] = (u["cout"],)
    return out


def buffer_shapes(case):
    out = {}
    for u in units(case):
        p = u["bn"] + "."
        out.update({p + "running_mean": (u["cout"],), p + "running_var": (u["cout"],), p + "num_batches_tracked": ()})
    return out


def sizes(case):
    S, out = case["S"], [case["S"]]
    for u in units(case):
        S = out_size(S, u["k"], u["s"])
        out.append(S)
    return out


def case_inputs(case, seed=None):
    """-> dict(params, buffers, x [B,S,S,cin] fp32 (NHWC whatever the case's layout), gy [B,So,So,cout] fp32)"""
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
        p = u["bn"] + "."
        buffers[p + "running_mean"] = (0.3 * rs.standard_normal((u["cout"],))).astype(f32)
        buffers[p + "running_var"] = rs.uniform(0.5, 1.5, (u["cout"],)).astype(f32)
        buffers[p + "num_batches_tracked"] = np.asarray(3 + i, np.int64)
    B, So = case["B"], sizes(case)[-1]
    x = rs.standard_normal((B, case["S"], case["S"], case["cin"])).astype(f32)
    gy = rs.standard_normal((B, So, So, case["units"][-1]["c"])).astype(f32)
    return dict(params=params, buffers=buffers, x=x, gy=gy)


def tensor_shapes(case):
    B, So = case["B"], sizes(case)[-1]
    out = {"y": (B, So, So, case["units"][-1]["c"])}
    if not case["planar"]:
        out["dx"] = (B, case["S"], case["S"], case["cin"])
    out.update({"b." + n: sh for n, sh in buffer_shapes(case).items()})
    out.update({"g." + n: sh for n, sh in param_shapes(case).items()})
    return out


def stored_indices(key, name, shape):
    n = int(np.prod(shape, dtype=np.int64))
    return sample_indices(key + "/" + name, n) if n > SAMPLE_ABOVE else None


def fixture_tensors(z, case, mode, shapes=None):
    """-> {tensor name: (r64 values [flat, at idx], idx or None (= every element), e32, max64)}"""
    key = f"{case['name']}/{mode}"
    r64, e32, m64 = z[key + "/r64"], z[key + "/e32"], z[key + "/max64"]
    out, o = {}, 0
    for i, (name, shape) in enumerate((shapes or tensor_shapes(case)).items()):
        idx = stored_indices(key, name, shape)
        n = len(idx) if idx is not None else int(np.prod(shape, dtype=np.int64))
        out[name] = (r64[o:o + n], idx, float(e32[i]), float(m64[i]))
        o += n
    assert o == len(r64)
    return out


# ---- the restatement.  Every array is NHWC in `dtype`; sums of more than two terms run in the order written

def conv_forward(x, w, s):
    """dense k x k, pad (k - 1) / 2, stride s; w [N,C,k,k].  acc = 0; acc += x[tap] . w[tap]^T, ty then tx ascending"""
    B, S, _, C = x.shape
    k = w.shape[-1]
    p, So = (k - 1) // 2, out_size(S, k, s)
    xp = np.zeros((B, S + 2 * p, S + 2 * p, C), x.dtype)
    xp[:, p:p + S, p:p + S] = x
    out = np.zeros((B, So, So, w.shape[0]), x.dtype)
    for ky in range(k):
        for kx in range(k):
            out = out + xp[:, ky:ky + (So - 1) * s + 1:s, kx:kx + (So - 1) * s + 1:s] @ w[:, :, ky, kx].T
    return out


def conv_dgrad(dy, w, s, S):
    """the gradient of conv_forward's x as the kernels gather it.  1x1: every s-th pixel gets dy . W, the others zero.
    3x3 stride 1: pixel (i, j) sums, (ty, tx) ascending, dy[i - 1 + ty][j - 1 + tx] . W[2 - ty][2 - tx].  3x3 stride 2:
    parity class (pi, pj) holds the pixels (2 a + pi, 2 b + pj); along y it has the taps ty = 0 .. pi reading dy row
    a + ty with ky = 1 (pi = 0) or 2 - 2 ty (pi = 1), and likewise along x; a row or column >= S_out is dropped."""
    B, So, _, N = dy.shape
    k, C = w.shape[-1], w.shape[1]
    dx = np.zeros((B, S, S, C), dy.dtype)
    if k == 1:
        dx[:, ::s, ::s] = dy @ w[:, :, 0, 0]
        return dx
    dp = np.zeros((B, So + 2, So + 2, N), dy.dtype)        # dy with a border of zeros: rows -1 .. So
    dp[:, 1:1 + So, 1:1 + So] = dy
    if s == 1:
        for ty in range(3):
            for tx in range(3):
                dx = dx + dp[:, ty:ty + S, tx:tx + S] @ w[:, :, 2 - ty, 2 - tx]
        return dx
    for pi in range(2):
        for pj in range(2):
            ny, nx = (S - pi + 1) // 2, (S - pj + 1) // 2  # the class's pixels along y and x
            if ny < 1 or nx < 1:
                continue
            acc = np.zeros((B, ny, nx, C), dy.dtype)
            for ty in range(1 + pi):
                ky = 2 - 2 * ty if pi else 1
                for tx in range(1 + pj):
                    kx = 2 - 2 * tx if pj else 1
                    rows = np.minimum(np.arange(ny) + ty, So) + 1          # row So of dp is the zero border
                    cols = np.minimum(np.arange(nx) + tx, So) + 1
                    acc = acc + dp[:, rows[:, None], cols[None, :]] @ w[:, :, ky, kx]
            dx[:, pi::2, pj::2] = acc
    return dx


def conv_wgrad(x, dy, k, s):
    """dW[n, c, ky, kx] = sum over the output pixels m of dy[m][n] * x[s m + tap - p][c]"""
    B, S, _, C = x.shape
    p, So, N = (k - 1) // 2, dy.shape[1], dy.shape[3]
    xp = np.zeros((B, S + 2 * p, S + 2 * p, C), x.dtype)
    xp[:, p:p + S, p:p + S] = x
    dw = np.zeros((N, C, k, k), x.dtype)
    g = dy.reshape(-1, N)
    for ky in range(k):
        for kx in range(k):
            dw[:, :, ky, kx] = g.T @ xp[:, ky:ky + (So - 1) * s + 1:s, kx:kx + (So - 1) * s + 1:s].reshape(-1, C)
    return dw


def stack_all(case, inputs, train, dtype=np.float64):
    """forward and backward of <y, gy> -> {fixture tensor name: numpy array} (dx as well, whatever the case's layout)"""
    dt = dtype
    P = {n: np.asarray(v).astype(dt) for n, v in inputs["params"].items()}
    buf = inputs["buffers"]
    us = units(case)
    h = inputs["x"].astype(dt)
    out, saved = {}, []
    for u in us:
        w = P[u["conv"] + ".weight"]
        bnp = u["bn"] + "."
        z = conv_forward(h, w, u["s"])
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
        o = np.maximum(xhat * P[bnp + "weight"] + P[bnp + "bias"], 0)
        saved.append((h, xhat, invstd, o))
        h = o
    out["y"] = h
    g = inputs["gy"].astype(dt)
    for u, (xin, xhat, invstd, o) in zip(us[::-1], saved[::-1]):
        w = P[u["conv"] + ".weight"]
        bnp = u["bn"] + "."
        g = g * (o > 0)
        M = g.shape[0] * g.shape[1] * g.shape[2]
        dbeta, dgamma = g.sum((0, 1, 2), dtype=dt), (g * xhat).sum((0, 1, 2), dtype=dt)
        out["g." + bnp + "bias"], out["g." + bnp + "weight"] = dbeta, dgamma
        scale = P[bnp + "weight"] * invstd
        dz = (scale * (g - dbeta / M - xhat * (dgamma / M)) if train else scale * g).astype(dt)
        out["g." + u["conv"] + ".weight"] = conv_wgrad(xin, dz, u["k"], u["s"])
        g = conv_dgrad(dz, w, u["s"], xin.shape[1])
    out["dx"] = g
    return {n: np.asarray(out[n]) for n in list(tensor_shapes(case)) + (["dx"] if case["planar"] else [])}


# ---- the composite case: image -> [c3, c4, c5]

def tiny_parts():
    return TINY["stem"], TINY["mid"], TINY["tail"]


def tiny_inputs(seed=None):
    """-> dict(params, buffers, x [B,S,S,3], g3, g4, g5): the three parts' inputs under seeds of their own, merged"""
    seed = TINY["seed"] if seed is None else seed
    stem, mid, tail = tiny_parts()
    a, b, c = case_inputs(stem, seed), sc.case_inputs(dict(mid, seed=seed + 1)), sc.case_inputs(dict(tail, seed=seed + 2))
    rs = np.random.RandomState(seed + 3)
    g3, g4 = rs.standard_normal(a["gy"].shape).astype(np.float32), rs.standard_normal(b["gy"].shape).astype(np.float32)
    return dict(params={**a["params"], **b["params"], **c["params"]}, buffers={**a["buffers"], **b["buffers"], **c["buffers"]},
                x=a["x"], g3=g3, g4=g4, g5=c["gy"])


def tiny_tensor_shapes():
    stem, mid, tail = tiny_parts()
    B = TINY["B"]
    S3, S4, S5 = sizes(stem)[-1], sc.sizes(mid)[-1], sc.sizes(tail)[-1]
    out = {"y.c3": (B, S3, S3, stem["units"][-1]["c"]), "y.c4": (B, S4, S4, mid["blocks"][-1]["c"]),
           "y.c5": (B, S5, S5, tail["blocks"][-1]["c"])}
    for shapes in (buffer_shapes(stem), sc.buffer_shapes(mid), sc.buffer_shapes(tail)):
        out.update({"b." + n: sh for n, sh in shapes.items()})
    for shapes in (param_shapes(stem), sc.param_shapes(mid), sc.param_shapes(tail)):
        out.update({"g." + n: sh for n, sh in shapes.items()})
    return out


def tiny_all(inputs, train=True, dtype=np.float64):
    """forward of the three parts, then backward with the gradient joins: C4 receives g4 + the tail's dx, C3 receives
    g3 + the mid stage's dx"""
    stem, mid, tail = tiny_parts()
    sub = lambda x, gy: dict(params=inputs["params"], buffers=inputs["buffers"], x=x, gy=gy)   # noqa: E731
    zeros = lambda a: np.zeros_like(a)                     # noqa: E731
    c3 = stack_all(stem, sub(inputs["x"], zeros(inputs["g3"])), train, dtype)["y"]
    c4 = sc.stack_all(mid, sub(c3, zeros(inputs["g4"])), train, dtype)["y"]
    rt = sc.stack_all(tail, sub(c4, inputs["g5"]), train, dtype)
    rm = sc.stack_all(mid, sub(c3, inputs["g4"].astype(dtype) + rt["dx"]), train, dtype)
    rsm = stack_all(stem, sub(inputs["x"], inputs["g3"].astype(dtype) + rm["dx"]), train, dtype)
    out = {"y.c3": c3, "y.c4": c4, "y.c5": rt["y"]}
    for r in (rsm, rm, rt):
        out.update({n: v for n, v in r.items() if n[:2] in ("b.", "g.")})
    return {n: np.asarray(out[n]) for n in tiny_tensor_shapes()}


# ---- the plan, restated

def plan_restated(case, B=None, S=None, stat_rows=256, gemm_rows=64, conv_tile=8, stat_tiles_max=1024):
    """the formulas of include/yololite_hip.h (yl_stem_plan_info, yl_stem_unit_plan) written again"""
    def cdiv(a, b):
        return -(-a // b)

    def r16(v):
        return (v + 15) // 16 * 16

    def r4(v):
        return (v + 3) // 4 * 4

    def pick_pt(NP):
        return 6 if cdiv(NP, 96) * 96 < cdiv(NP, 64) * 64 else 4

    def splits1(M, NP, NQ):
        tiles = cdiv(NP, 16 * pick_pt(NP)) * cdiv(NQ, gemm_rows)
        want = min(max(1024 // tiles, 8), 128)
        want = min(want, cdiv(M, 64))
        rows = cdiv(cdiv(M, want), 16) * 16
        return rows, cdiv(M, rows)

    def splits3(B, So, cin, cout):
        tiles = B * cdiv(So, conv_tile) ** 2
        want = min(max(1024 // (cdiv(r4(cin), 32) * cdiv(cout, 64)), 1), tiles)
        rows = cdiv(tiles, want)
        return rows, cdiv(tiles, rows)

    def conv_block(cout):
        return 16 * min((4, 3, 2), key=lambda pt: (cdiv(cout, 16 * pt) * pt, -pt))

    B = case["B"] if B is None else B
    c = dict(case, S=case["S"] if S is None else S)
    szs = sizes(c)
    x0 = B * szs[0] ** 2 * case["cin"] * 4
    amax = cmax = smax = pmax = wmax = 0
    per_unit = []
    for u, Si, So in zip(units(c), szs[:-1], szs[1:]):
        M = B * So * So
        srows = stat_rows * cdiv(cdiv(M, stat_rows), stat_tiles_max)
        tiles = cdiv(M, srows)
        rows, sp = splits1(M, u["cin"], u["cout"]) if u["k"] == 1 else splits3(B, So, u["cin"], u["cout"])
        W = u["cin"] * u["cout"] if u["k"] == 1 else 9 * u["cout"] * r4(u["cin"])
        per_unit.append(dict(size_in=Si, size_out=So, rows_out=M, stat_rows=srows, stat_tiles=tiles, wgrad_rows=rows,
                             wgrad_splits=sp, conv_block=conv_block(u["cout"]) if u["k"] == 3 else 0,
                             saved_bytes=2 * M * u["cout"] * 4 + 2 * u["cout"] * 4))
        amax, cmax = max(amax, M * u["cout"] * 4), max(cmax, u["cout"])
        smax = max(smax, r16(tiles * 2 * u["cout"] * 8))
        wmax = max(wmax, r16(sp * W * 4))
        if u["k"] == 3:
            pmax = max(pmax, r16(W * 4))
    return dict(units=per_unit, saved_bytes=r16(x0) + sum(p["saved_bytes"] for p in per_unit),
                nosave_bytes=3 * amax + 2 * cmax * 4, workspace_bytes=2 * amax + smax + 2 * cmax * 4 + pmax + wmax)


def forward_launches(case, train):
    """the header's count for yl_stem_forward"""
    return sum((2 if u["k"] == 3 else 1) + (1 if train else 0) + 2 for u in units(case))


def backward_launches(case, train, want_dx, wanted=None):
    """the header's count for yl_stem_backward; `wanted`: per unit, are its parameter gradients wanted (default: all)"""
    us, szs = units(case), sizes(case)
    wanted = [True] * len(us) if wanted is None else list(wanted)
    first = 0 if want_dx else min([i for i, w in enumerate(wanted) if w], default=len(us))
    n = 0
    for i in range(len(us) - 1, first - 1, -1):
        u, g = us[i], wanted[i]
        n += (1 if (train or g) else 0) + 1
        need_dx = i > first or (i == 0 and want_dx)
        if not need_dx and not g:
            break
        n += 1 + (2 if g else 0)
        if not need_dx:
            break
        n += 1 if u["k"] == 1 else (2 if u["s"] == 1 else 1 + (4 if szs[i] >= 2 else 1))
    return n
