"""Inputs of the detection-head tests as a function of a seed (numpy's frozen RandomState), and the fixture's layout.

tests/golden/head_train.npz (made by tests/golden/make_head_fixtures.py from the reference's own make_head /
_forward_head) holds, per case, mode ("train", and "eval" for the first case), level and tensor
    <case>/<mode>/L<i>/r64     the reference's float64 results, the tensors of tensor_shapes() flattened and concatenated
    <case>/<mode>/L<i>/e32     per tensor: the reference's own fp32 error max|r32 - r64| (over the WHOLE tensor)
    <case>/<mode>/L<i>/max64   per tensor: max|r64| (over the whole tensor)
tensors: y, dx, running_mean.<t>, running_var.<t>, num_batches_tracked.<t> and g.<parameter name> for every parameter.
A tensor of more than SAMPLE_ABOVE elements is stored at the SAMPLE flat indices of sample_indices() only: a committed
file may not exceed 1 MiB, and the 1x1 weight gradients of the F = 244 case alone are 1.9 MB in float64.
fixture_tensors() takes the archive apart again.
"""
import math
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIXTURE = os.path.join(GOLDEN, "head_train.npz")
SAMPLE_ABOVE = 8192
SAMPLE = 4096

# the smallest shapes that reach each way of going wrong
CASES = [
    dict(name="base", F=16, C=3, A=1, depth=1, B=2, sizes=(8, 4, 2), seed=101),      # three levels; S = 2: mostly padding
    dict(name="a2c1", F=20, C=1, A=2, depth=2, B=3, sizes=(5, 3), seed=202),         # F % 16 != 0, anchors, two blocks, odd S
    dict(name="f244", F=244, C=4, A=1, depth=2, B=1, sizes=(6, 3), seed=306),        # several k-tiles, a ragged last one; B = 1
    dict(name="c80", F=96, C=80, A=1, depth=1, B=2, sizes=(6, 3), seed=404),         # E = 85
    dict(name="rows", F=16, C=1, A=1, depth=1, B=2, sizes=(24,), seed=505),          # 1152 rows: row tiles, multi-partial sums
]
EVAL_CASE = "base"
# seeds: the first of 101, 202, 303.., counting up, whose case passes the generator's admission rule (f244: 303-305 put
# a BatchNorm output within 64 fp32 errors of zero)

# the widths the zoo's heads run (F = 160 .. 512), in tests/golden/head_train_wide.npz.  Above 256 channels the row
# reductions and the depthwise weight gradient run a second channel group and the per-channel kernels a second workgroup;
# few rows, because every value in front of a ReLU has to pass the admission rule.  Seeds: the rule of CASES (101 is
# admitted for all of them)
WIDE = [
    dict(name="f328", F=328, C=2, A=1, depth=1, B=2, sizes=(3,), seed=101),    # 82 quads: a ragged second group; six p-tiles, the last ragged
    dict(name="f512", F=512, C=2, A=1, depth=2, B=2, sizes=(2,), seed=101),    # two full groups, two blocks
]
FIXTURE_WIDE = os.path.join(GOLDEN, "head_train_wide.npz")


def fixture_path(case):
    return FIXTURE_WIDE if any(case["name"] == w["name"] for w in WIDE) else FIXTURE


# the shapes of test_head_gemm_fp32_gpu.py: where split_plan's other bounds decide.  cap128: 10 368 rows, want 128 against
# most 162: 108 splits of 96 rows.  free: 4 608 rows, 16 tiles, want 64 against most 72: 58 splits of 80 rows; three
# anchors of 85 columns are 255 columns, four q groups, so the outputs' weight gradient has 16 tiles and is cut the same way
GEMM_OP_SHAPES = [
    dict(name="cap128", F=16, C=3, A=1, depth=1, B=2, sizes=(72,), seed=1501, wgrad=(96, 108, "cap128")),
    dict(name="free", F=256, C=80, A=3, depth=1, B=2, sizes=(48,), seed=1502, wgrad=(80, 58, "free")),
]

# the 20-step fit of the end-to-end test: one fixed batch, SGD with momentum (no nesterov, no weight decay), amp off
E2E = dict(F=16, C=3, A=1, depth=1, B=2, sizes=(8, 4, 2), seed=707, img_size=64, lr=0.02, momentum=0.9, steps=20,
           gt_xyxy=[[6.0, 8.0, 30.0, 34.0], [36.0, 30.0, 60.0, 58.0], [10.0, 12.0, 50.0, 44.0]], gt_label=[0, 2, 1],
           gt_off=[0, 2, 3])


def level_names(case):
    return tuple("p%d" % (3 + i) for i in range(len(case["sizes"])))


def param_shapes(F, C, A, depth, k):
    """name -> shape of one head's parameters, in the reference's state_dict order"""
    out = {}
    for t in range(depth):
        p = f"head{k}.trunk.{t}.block."
        out[p + "0.weight"] = (F, 1, 3, 3)
        out[p + "1.weight"] = (F, F, 1, 1)
        out[p + "2.weight"] = (F,)
        out[p + "2.bias"] = (F,)
    for n, r in (("box", 4 * A), ("obj", A), ("cls", A * C)):
        out[f"head{k}.out.{n}.weight"] = (r, F, 1, 1)
        out[f"head{k}.out.{n}.bias"] = (r,)
    return out


def case_inputs(case):
    """-> per level dict(k, S, params {name: fp32}, buffers {name: array}, x [B,S,S,F] fp32, gy [B,A,S,S,5+C] fp32).
    Weights ~ N(0, 1 / fan_in), gamma in [0.5, 1.5], beta ~ 0.2 N(0,1), the output biases are the reference's initial
    values plus 0.1 N(0,1), running statistics are not the initial ones."""
    rs = np.random.RandomState(case["seed"])
    F, C, A, depth, B = (case[k] for k in ("F", "C", "A", "depth", "B"))
    f32 = np.float32
    init = {"box": 0.0, "obj": -math.log(99.0), "cls": -math.log(C) if C > 1 else 0.0}
    out = []
    for li, S in enumerate(case["sizes"]):
        k = 3 + li
        params, buffers = {}, {}
        for name, shape in param_shapes(F, C, A, depth, k).items():
            if ".out." in name and name.endswith(".bias"):
                v = init[name.split(".")[2]] + 0.1 * rs.standard_normal(shape)
            elif name.endswith("2.weight"):
                v = rs.uniform(0.5, 1.5, shape)
            elif name.endswith("2.bias"):
                v = 0.2 * rs.standard_normal(shape)
            else:
                v = rs.standard_normal(shape) / math.sqrt(shape[1] * shape[2] * shape[3])
            params[name] = np.ascontiguousarray(v, f32)
        for t in range(depth):
            p = f"head{k}.trunk.{t}.block.2."
            buffers[p + "running_mean"] = (0.3 * rs.standard_normal((F,))).astype(f32)
            buffers[p + "running_var"] = rs.uniform(0.5, 1.5, (F,)).astype(f32)
            buffers[p + "num_batches_tracked"] = np.asarray(3 + t, np.int64)
        x = rs.standard_normal((B, S, S, F)).astype(f32)
        gy = rs.standard_normal((B, A, S, S, 5 + C)).astype(f32)
        out.append(dict(k=k, S=S, params=params, buffers=buffers, x=x, gy=gy))
    return out


def sample_indices(name, n):
    """the flat indices a tensor of n > SAMPLE_ABOVE elements is stored at: a seeded choice without repetition, sorted"""
    seed = sum((i + 1) * ord(c) for i, c in enumerate(name)) % (2 ** 31)
    return np.sort(np.random.RandomState(seed).choice(n, SAMPLE, replace=False)).astype(np.int64)


def tensor_shapes(case, k, S):
    """name -> shape of the tensors of one level in the fixture, in the archive's order"""
    F, C, A, depth, B = (case[n] for n in ("F", "C", "A", "depth", "B"))
    out = {"y": (B, A, S, S, 5 + C), "dx": (B, S, S, F)}
    for t in range(depth):
        out.update({f"running_mean.{t}": (F,), f"running_var.{t}": (F,), f"num_batches_tracked.{t}": ()})
    out.update({"g." + n: sh for n, sh in param_shapes(F, C, A, depth, k).items()})
    return out


def stored_indices(key, name, shape):
    n = int(np.prod(shape, dtype=np.int64))
    return sample_indices(key + "/" + name, n) if n > SAMPLE_ABOVE else None


def fixture_tensors(z, case, mode, li):
    """-> {tensor name: (r64 values [flat, at idx], idx or None (= every element), e32, max64)}"""
    key = f"{case['name']}/{mode}/L{li}"
    r64, e32, m64 = z[key + "/r64"], z[key + "/e32"], z[key + "/max64"]
    out, o = {}, 0
    for i, (name, shape) in enumerate(tensor_shapes(case, 3 + li, case["sizes"][li]).items()):
        idx = stored_indices(key, name, shape)
        n = len(idx) if idx is not None else int(np.prod(shape, dtype=np.int64))
        out[name] = (r64[o:o + n], idx, float(e32[i]), float(m64[i]))
        o += n
    assert o == len(r64)
    return out


def modes(case):
    return ("train", "eval") if case["name"] == EVAL_CASE else ("train",)


def bar(e32, max64):
    """max(4 x the reference's own fp32 error, 2 fp32 ulps at the tensor's largest magnitude)"""
    ulp = float(np.spacing(np.float32(max64))) if max64 > 0 else 0.0
    return max(4.0 * float(e32), 2.0 * ulp)
