"""Inputs of the FPN-neck tests as a function of a seed (numpy's frozen RandomState), and the fixture's layout.

tests/golden/neck_train.npz (made by tests/golden/make_neck_fixtures.py from the reference's own YOLOLiteMS_CPU.forward)
holds, per case, mode ("train", and "eval" for the first case), level and tensor
    <case>/<mode>/L<i>/r64     the reference's float64 results, the tensors of tensor_shapes() flattened and concatenated
    <case>/<mode>/L<i>/e32     per tensor: the reference's own fp32 error max|r32 - r64| (over the WHOLE tensor)
    <case>/<mode>/L<i>/max64   per tensor: max|r64| (over the whole tensor)
tensors: p, dc, running_mean.<t>, running_var.<t>, num_batches_tracked.<t> and g.<parameter name> for every parameter.
A tensor of more than SAMPLE_ABOVE elements is stored at the SAMPLE flat indices of _head_cases.sample_indices() only
(the rule of the head fixture).  Also stored: `keys` (name, shape, dtype of the reference's lateral* / smooth3..5
state_dict entries for the KEYS configuration) and `e2e/losses`, the float64 CPU loop of the end-to-end test.

Level L<i> is the i-th level, finest first.  A case of three levels is p3, p4, p5; of four, p2..p5 (use_p2); of two,
p4, p5 (the generator runs the reference with a dummy p3 whose gradient is zero, which leaves p4 / p5 as they are).
"""
import math
import os

import numpy as np

from _head_cases import SAMPLE_ABOVE, bar, sample_indices  # noqa: F401  (re-exported)

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIXTURE = os.path.join(GOLDEN, "neck_train.npz")

# the smallest shapes that reach each way of going wrong
CASES = [
    dict(name="base", B=2, F=16, Cin=(8, 12, 20), depth=1, sizes=(8, 4, 2), seed=102),     # exact 2x; also eval mode
    dict(name="odd", B=3, F=20, Cin=(4, 24, 36), depth=2, sizes=(5, 3, 2), seed=202),      # maps 3->5, 2->3; F % 16 != 0
    dict(name="wide", B=1, F=96, Cin=(64, 480), depth=1, sizes=(6, 3), seed=303),          # many k-tiles, Cin > F, B = 1
    dict(name="ragged", B=2, F=16, Cin=(40, 40), depth=1, sizes=(6, 3), seed=404),         # Cin % 16 != 0
    dict(name="rows", B=2, F=16, Cin=(8, 8), depth=1, sizes=(24, 12), seed=506),           # 1152 rows: several row tiles
    dict(name="l4", B=2, F=16, Cin=(8, 8, 8, 8), depth=1, sizes=(16, 8, 4, 2), seed=606),  # four levels (use_p2)
]
EVAL_CASE = "base"
# seeds: the first of 101, 202, 303.., counting up, whose case passes the generator's admission rule (base: 101 puts an
# eval-mode BatchNorm output of p4 within 64 fp32 errors of zero; rows: 505 fails the rule likewise)

# the widths the zoo's depthwise necks run (F = 160 .. 320, Cin up to 960), in tests/golden/neck_train_wide.npz; few rows,
# because every value in front of a ReLU has to pass the admission rule.  Seeds: the rule of CASES (f288: 101, 202 and 303
# fail it; f320: 101 .. 707 do)
WIDE = [
    dict(name="f288", B=1, F=288, Cin=(96, 960), depth=1, sizes=(4, 2), seed=404),     # 72 quads: a ragged second group; pt 6, three p-tiles; K = 960
    dict(name="f320", B=2, F=320, Cin=(64, 128), depth=1, sizes=(4, 2), seed=808),     # 80 quads; pt 4, five full p-tiles
]
FIXTURE_WIDE = os.path.join(GOLDEN, "neck_train_wide.npz")


def fixture_path(case):
    return FIXTURE_WIDE if any(case["name"] == w["name"] for w in WIDE) else FIXTURE


# the configuration whose reference key list DetectNeck is held to
KEYS = dict(B=1, F=16, Cin=(8, 12, 20), depth=2, sizes=(8, 4, 2))

# the 20-step fit of the end-to-end test (neck + heads on one fixed batch of feature maps; SGD with momentum, amp off)
E2E = dict(name="e2e", B=2, F=16, Cin=(8, 12, 20), depth=1, sizes=(8, 4, 2), seed=707, C=3, A=1, head_depth=1,
           img_size=64, lr=0.02, momentum=0.9, steps=20,
           gt_xyxy=[[6.0, 8.0, 30.0, 34.0], [36.0, 30.0, 60.0, 58.0], [10.0, 12.0, 50.0, 44.0]], gt_label=[0, 2, 1],
           gt_off=[0, 2, 3])


def level_names(case):
    L = len(case["sizes"])
    return {2: ("p4", "p5"), 3: ("p3", "p4", "p5"), 4: ("p2", "p3", "p4", "p5")}[L]


def param_shapes(F, Cin, depth, k):
    """name -> shape of one level's parameters, in the reference's naming"""
    out = {f"lateral{k}.weight": (F, Cin, 1, 1), f"lateral{k}.bias": (F,)}
    for i in range(depth):
        p = f"smooth{k}.block."
        out[f"{p}{4 * i}.weight"] = (F, 1, 3, 3)
        out[f"{p}{4 * i + 1}.weight"] = (F, F, 1, 1)
        out[f"{p}{4 * i + 2}.weight"] = (F,)
        out[f"{p}{4 * i + 2}.bias"] = (F,)
    return out


def case_inputs(case):
    """-> per level dict(k, S, Cin, params {name: fp32}, buffers {name: array}, c [B,S,S,Cin] fp32, gp [B,S,S,F] fp32).
    Weights ~ N(0, 1 / fan_in), lateral bias ~ 0.1 N(0,1), gamma in [0.5, 1.5], beta ~ 0.2 N(0,1), running statistics
    are not the initial ones."""
    rs = np.random.RandomState(case["seed"])
    F, depth, B = case["F"], case["depth"], case["B"]
    f32 = np.float32
    out = []
    for n, S, Cin in zip(level_names(case), case["sizes"], case["Cin"]):
        k = int(n[1:])
        params, buffers = {}, {}
        for name, shape in param_shapes(F, Cin, depth, k).items():
            if name.startswith("lateral") and name.endswith(".bias"):
                v = 0.1 * rs.standard_normal(shape)
            elif len(shape) == 1 and name.endswith(".weight"):
                v = rs.uniform(0.5, 1.5, shape)
            elif len(shape) == 1:
                v = 0.2 * rs.standard_normal(shape)
            else:
                v = rs.standard_normal(shape) / math.sqrt(shape[1] * shape[2] * shape[3])
            params[name] = np.ascontiguousarray(v, f32)
        for i in range(depth):
            p = f"smooth{k}.block.{4 * i + 2}."
            buffers[p + "running_mean"] = (0.3 * rs.standard_normal((F,))).astype(f32)
            buffers[p + "running_var"] = rs.uniform(0.5, 1.5, (F,)).astype(f32)
            buffers[p + "num_batches_tracked"] = np.asarray(3 + i, np.int64)
        c = rs.standard_normal((B, S, S, Cin)).astype(f32)
        gp = rs.standard_normal((B, S, S, F)).astype(f32)
        out.append(dict(k=k, S=S, Cin=Cin, params=params, buffers=buffers, c=c, gp=gp))
    return out


def head_inputs(cfg):
    """the heads of the end-to-end fit: _head_cases.case_inputs of the same F / sizes (their x is not used)"""
    from _head_cases import case_inputs as head_case_inputs
    return head_case_inputs(dict(F=cfg["F"], C=cfg["C"], A=cfg["A"], depth=cfg["head_depth"], B=cfg["B"],
                                 sizes=cfg["sizes"], seed=cfg["seed"] + 1))


def tensor_shapes(case, k, S, Cin):
    """name -> shape of the tensors of one level in the fixture, in the archive's order"""
    F, depth, B = case["F"], case["depth"], case["B"]
    out = {"p": (B, S, S, F), "dc": (B, S, S, Cin)}
    for t in range(depth):
        out.update({f"running_mean.{t}": (F,), f"running_var.{t}": (F,), f"num_batches_tracked.{t}": ()})
    out.update({"g." + n: sh for n, sh in param_shapes(F, Cin, depth, k).items()})
    return out


def stored_indices(key, name, shape):
    n = int(np.prod(shape, dtype=np.int64))
    return sample_indices(key + "/" + name, n) if n > SAMPLE_ABOVE else None


def fixture_tensors(z, case, mode, li):
    """-> {tensor name: (r64 values [flat, at idx], idx or None (= every element), e32, max64)}"""
    key = f"{case['name']}/{mode}/L{li}"
    r64, e32, m64 = z[key + "/r64"], z[key + "/e32"], z[key + "/max64"]
    k = int(level_names(case)[li][1:])
    out, o = {}, 0
    for i, (name, shape) in enumerate(tensor_shapes(case, k, case["sizes"][li], case["Cin"][li]).items()):
        idx = stored_indices(key, name, shape)
        n = len(idx) if idx is not None else int(np.prod(shape, dtype=np.int64))
        out[name] = (r64[o:o + n], idx, float(e32[i]), float(m64[i]))
        o += n
    assert o == len(r64)
    return out


def modes(case):
    return ("train", "eval") if case["name"] == EVAL_CASE else ("train",)
