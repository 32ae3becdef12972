"""Inputs of the dense-FPN-neck tests (DetectNeckMS) as a function of a seed (numpy's frozen RandomState), and the
fixture's layout.

tests/golden/dense_neck_train.npz (made by tests/golden/make_dense_neck_fixtures.py from the reference's own
YOLOLiteMS.forward) has the layout of neck_train.npz (tests/_neck_cases.py): per case, mode ("train", and "eval" for
the first case) and level
    <case>/<mode>/L<i>/r64     the reference's float64 results, the tensors of tensor_shapes() flattened and concatenated
    <case>/<mode>/L<i>/e32     per tensor: the reference's own fp32 error max|r32 - r64| (over the WHOLE tensor)
    <case>/<mode>/L<i>/max64   per tensor: max|r64| (over the whole tensor)
tensors: p, dc, running_mean.<t>, running_var.<t>, num_batches_tracked.<t> and g.<parameter name> for every parameter.
A tensor of more than SAMPLE_ABOVE elements is stored at the SAMPLE flat indices of _head_cases.sample_indices() only.
Also stored: `keys` (name, shape, dtype of the reference's lateral* / smooth3..5 state_dict entries for the KEYS
configuration) and `e2e/losses`, the float64 CPU loop of the end-to-end test.  SiLU has no ties: there is no admission
rule, and the seeds are simply 111, 212, ...

Names are the reference's for conv_block, a plain nn.Sequential: smooth{k}.{3i}.weight [F,F,3,3] and
smooth{k}.{3i+1}.{weight, bias, running_mean, running_var, num_batches_tracked}.
"""
import math
import os

import numpy as np

from _head_cases import SAMPLE_ABOVE, bar, sample_indices  # noqa: F401  (re-exported)
from _neck_cases import head_inputs, level_names, stored_indices  # noqa: F401  (re-exported)

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIXTURE = os.path.join(GOLDEN, "dense_neck_train.npz")

# the smallest shapes that reach each way of going wrong (spatial tile 8 x 8, 64 output channels per workgroup,
# k-blocks of 16 input channels; the weight gradient works on 64 x 64 channel blocks and runs of spatial tiles)
CASES = [
    dict(name="base", B=2, F=16, Cin=(8, 12, 20), depth=1, sizes=(8, 4, 2), seed=111),     # exact 2x; also eval mode
    dict(name="odd", B=3, F=20, Cin=(4, 24, 36), depth=2, sizes=(5, 3, 2), seed=212),      # F % 16 != 0, odd sizes, ragged tiles, two blocks
    dict(name="wide", B=1, F=100, Cin=(64, 480), depth=1, sizes=(6, 3), seed=313),         # two channel blocks, 7 k-blocks (ragged last), B = 1
    dict(name="rows", B=2, F=16, Cin=(8, 8), depth=1, sizes=(24, 12), seed=414),           # 9 tiles per image: interior seams, 18 wgrad splits
    dict(name="tiny", B=4, F=8, Cin=(8, 8), depth=2, sizes=(2, 1), seed=515),              # S = 1: only the centre tap is inside; F < 16
    dict(name="l4", B=2, F=16, Cin=(8, 8, 8, 8), depth=1, sizes=(16, 8, 4, 2), seed=616),  # four levels (use_p2)
]
EVAL_CASE = "base"

# the widths the zoo's dense necks run (F = 196 .. 512), in tests/golden/dense_neck_train_wide.npz.  Seeds: the series goes on
# (717 is E2E's)
WIDE = [
    dict(name="f328", B=1, F=328, Cin=(48, 320), depth=1, sizes=(4, 2), seed=818),     # six channel blocks and 21 k-blocks, the last ragged; two groups
    dict(name="f512", B=1, F=512, Cin=(64, 64), depth=1, sizes=(3, 2), seed=919),      # eight full channel blocks, two full groups
]
FIXTURE_WIDE = os.path.join(GOLDEN, "dense_neck_train_wide.npz")


def fixture_path(case):
    return FIXTURE_WIDE if any(case["name"] == w["name"] for w in WIDE) else FIXTURE


# the configuration whose reference key list DetectNeckMS is held to
KEYS = dict(B=1, F=16, Cin=(8, 12, 20), depth=2, sizes=(8, 4, 2))

# the 20-step fit of the end-to-end test (neck + heads on one fixed batch of feature maps; SGD with momentum, amp off)
E2E = dict(name="e2e", B=2, F=16, Cin=(8, 12, 20), depth=1, sizes=(8, 4, 2), seed=717, C=3, A=1, head_depth=1,
           img_size=64, lr=0.02, momentum=0.9, steps=20,
           gt_xyxy=[[6.0, 8.0, 30.0, 34.0], [36.0, 30.0, 60.0, 58.0], [10.0, 12.0, 50.0, 44.0]], gt_label=[0, 2, 1],
           gt_off=[0, 2, 3])


def param_shapes(F, Cin, depth, k):
    """name -> shape of one level's parameters, in the reference's naming"""
    out = {f"lateral{k}.weight": (F, Cin, 1, 1), f"lateral{k}.bias": (F,)}
    for i in range(depth):
        out[f"smooth{k}.{3 * i}.weight"] = (F, F, 3, 3)
        out[f"smooth{k}.{3 * i + 1}.weight"] = (F,)
        out[f"smooth{k}.{3 * i + 1}.bias"] = (F,)
    return out


def case_inputs(case):
    """-> per level dict(k, S, Cin, params {name: fp32}, buffers {name: array}, c [B,S,S,Cin] fp32, gp [B,S,S,F] fp32).
    The recipe of _neck_cases.case_inputs: weights ~ N(0, 1 / fan_in), lateral bias ~ 0.1 N(0,1), gamma in [0.5, 1.5],
    beta ~ 0.2 N(0,1), running statistics that are not the initial ones."""
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
            p = f"smooth{k}.{3 * i + 1}."
            buffers[p + "running_mean"] = (0.3 * rs.standard_normal((F,))).astype(f32)
            buffers[p + "running_var"] = rs.uniform(0.5, 1.5, (F,)).astype(f32)
            buffers[p + "num_batches_tracked"] = np.asarray(3 + i, np.int64)
        c = rs.standard_normal((B, S, S, Cin)).astype(f32)
        gp = rs.standard_normal((B, S, S, F)).astype(f32)
        out.append(dict(k=k, S=S, Cin=Cin, params=params, buffers=buffers, c=c, gp=gp))
    return out


def tensor_shapes(case, k, S, Cin):
    """name -> shape of the tensors of one level in the fixture, in the archive's order"""
    F, depth, B = case["F"], case["depth"], case["B"]
    out = {"p": (B, S, S, F), "dc": (B, S, S, Cin)}
    for t in range(depth):
        out.update({f"running_mean.{t}": (F,), f"running_var.{t}": (F,), f"num_batches_tracked.{t}": ()})
    out.update({"g." + n: sh for n, sh in param_shapes(F, Cin, depth, k).items()})
    return out


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
