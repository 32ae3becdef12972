"""Cases and references of the mixed-precision tests of DetectNeckMS's three 3x3 GEMMs (precision "fp16" / "bf16": both
operands rounded to nearest even, products exact, fp32 accumulation).

OP_CASES are the smallest shapes that reach each way of going wrong in csrc/yl_dneck.hip as it stands: spatial tile 8 x 8,
64 output channels per workgroup, k-blocks of 16 input channels in the convolution (one v_mfma_f32_16x16x16 per tap and 16
outputs; a 32-channel k-block of the 16x16x32 forms would be ragged at the same F, so the shapes hold for it too); 64 x 64
channel blocks and runs of spatial tiles in the weight gradient, whose k index is the pixel (four 16-pixel steps per tile).
Re-derive them if the tile or the k-block changes.

The reference of an op is the float64 convolution of the RNE-rounded operands (torch's .to(float16 / bfloat16) is RNE),
the bar is _head_cases.bar with e32 = the error of torch's fp32 CPU convolution of the SAME rounded operands: no rounding
can flip, the operands are given.  `unrounded` is the float64 result of the operands as they are: it must lie outside
the bar, or the case could not see a missing rounding."""
import functools

import numpy as np
import torch
import torch.nn.functional as Fn

from _head_cases import bar  # noqa: F401  (re-exported)

DTYPES = {"fp16": torch.float16, "bf16": torch.bfloat16}
PASSES = ("forward", "dgrad", "wgrad")

OP_CASES = [
    dict(name="ragged", F=20, S=5, B=3, seed=1201),     # F % 8 and % 16 != 0, ragged tile
    dict(name="wide", F=100, S=6, B=1, seed=1202),      # two channel blocks, ragged last k-block at both 16 and 32
    dict(name="rows", F=16, S=24, B=2, seed=1203),      # nine tiles per image, 18 weight-gradient splits
    dict(name="centre", F=8, S=1, B=4, seed=1204),      # centre tap only
    dict(name="k32", F=40, S=3, B=1, seed=1205),        # one full 32-block plus a ragged one
]
# the first level of the wide cases of _dense_neck_cases.py: six channel blocks and 21 k-blocks of 16 with a ragged last
# (F 328), eight full channel blocks (F 512)
OP_WIDE = [
    dict(name="f328", F=328, S=4, B=1, seed=1206),
    dict(name="f512", F=512, S=3, B=1, seed=1207),
]
OP_BY_NAME = {c["name"]: c for c in OP_CASES + OP_WIDE}


def rounded(t: torch.Tensor, precision: str) -> torch.Tensor:
    """fp32 -> the nearest value of the 16-bit type (ties to even), as fp32"""
    return t.to(DTYPES[precision]).to(torch.float32)


def conv_pass(a: torch.Tensor, b: torch.Tensor, pass_: str) -> torch.Tensor:
    """the three passes on NHWC operands of one dtype (see neckops.conv3x3), on the CPU"""
    an = a.permute(0, 3, 1, 2)
    if pass_ == "forward":
        return Fn.conv2d(an, b, padding=1).permute(0, 2, 3, 1).contiguous()
    if pass_ == "dgrad":
        return Fn.conv_transpose2d(an, b, padding=1).permute(0, 2, 3, 1).contiguous()
    F = a.shape[3]
    return torch.nn.grad.conv2d_weight(an, (F, F, 3, 3), b.permute(0, 3, 1, 2), padding=1).contiguous()


def op_operands(case, pass_):
    """random fp32 operands that no 16-bit type holds: (x or dz [B,S,S,F], W [F,F,3,3] or dz [B,S,S,F])"""
    g = torch.Generator().manual_seed(case["seed"] + 17 * PASSES.index(pass_))
    B, S, F = case["B"], case["S"], case["F"]
    a = torch.randn((B, S, S, F), generator=g)
    b = torch.randn((B, S, S, F), generator=g) if pass_ == "wgrad" else torch.randn((F, F, 3, 3), generator=g) / (9 * F) ** 0.5
    return a, b


def reference(a, b, pass_, precision):
    """-> dict(r64, e32, max64, bar, unrounded) of given fp32 operands"""
    ra, rb = rounded(a, precision), rounded(b, precision)
    r64 = conv_pass(ra.double(), rb.double(), pass_)
    r32 = conv_pass(ra, rb, pass_)
    e32 = float((r32.double() - r64).abs().max())
    m64 = float(r64.abs().max())
    return dict(r64=r64, e32=e32, max64=m64, bar=bar(e32, m64), unrounded=conv_pass(a.double(), b.double(), pass_))


@functools.lru_cache(maxsize=None)
def op_reference(name, pass_, precision):
    """computed once per (case, pass, precision) and shared; callers do not write to it"""
    a, b = op_operands(OP_BY_NAME[name], pass_)
    return dict(reference(a, b, pass_, precision), a=a, b=b)


# ---- ties: operands on rounding midpoints with small-integer partners; every product and sum is exact in fp32
TIE_EPS = {"fp16": 2.0 ** -11, "bf16": 2.0 ** -8}      # half an ulp of the 16-bit type at 1


def tie_operands(pass_, precision, F=20, S=5, B=3, seed=1301):
    """the first operand is 1 + eps or 1 + 3 eps (midpoints: ties-to-even gives 1 and 1 + 4 eps), the second small integers"""
    rs = np.random.RandomState(seed + PASSES.index(pass_))
    eps = TIE_EPS[precision]
    a = torch.from_numpy((1.0 + eps * rs.choice([1.0, 3.0], (B, S, S, F))).astype(np.float32))
    shape = (B, S, S, F) if pass_ == "wgrad" else (F, F, 3, 3)
    b = torch.from_numpy(rs.randint(-2, 3, shape).astype(np.float32))
    assert not torch.equal(rounded(a, precision), a)
    return a, b


# ---- the whole module: tests/golden/dense_neck_amp.npz (made by tests/golden/make_dense_neck_amp_fixtures.py from the
# reference's own YOLOLiteMS.forward with its smooth convolutions wrapped in _dense_neck_amp_np.RoundedConv3x3), the six
# CASES of _dense_neck_cases.py and their inputs, per case, mode, precision and level
#     <case>/<mode>/<precision>/L<i>/r64     the rounded-operand float64 results, tensor_shapes() flattened and concatenated
#     <case>/<mode>/<precision>/L<i>/flip    per tensor: the flip allowance (below), over the WHOLE tensor
#     <case>/<mode>/<precision>/L<i>/max64   per tensor: max|r64| (over the whole tensor)
# Two precisions of every case: to stay under the size limit of a committed file, a tensor of more than AMP_SAMPLE_ABOVE
# elements is stored at the AMP_SAMPLE flat indices of amp_stored_indices() only (flip and max64 are of the whole tensor).
# When an operand of a rounded GEMM is itself a computed fp32 value (t, h, dz), an ulp of difference flips some roundings
# and one flip shows in the max norm, so the reference's plain fp32 error is no bar for a device with other ulps.  The flip
# allowance is measured on the reference: FLIP_RUNS fp32 runs of the same rounded model in which every value entering a
# rounding is first multiplied by 1 + s 2^-23, s in {-1, 0, 1} at random (seed FLIP_SEED + run); flip = the largest
# max|r32_j - r64|.  Bar = max(4 flip, 2 fp32 ulps at max64): _head_cases.bar with flip in the place of e32.
import os  # noqa: E402

AMP_FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "dense_neck_amp.npz")
AMP_PRECISIONS = ("fp16", "bf16")
FLIP_RUNS, FLIP_SEED = 8, 4100
AMP_SAMPLE_ABOVE, AMP_SAMPLE = 2048, 1024


def _amp_cases():
    """the six dense-neck cases (shapes and input recipe of _dense_neck_cases.py).  Every (case, mode, precision, level)
    must be able to tell the unrounded result from the rounded one in at least one of p, dc and the first block's weight
    gradient (test_dense_neck_amp_cpu.py); a case whose inputs cannot gets another seed here, never another rule: `odd`
    (212: fp16 levels 0 and 1 inside the bar) and `l4` (616) did; the new ones are the first found with a margin of nearly 2."""
    from _dense_neck_cases import CASES
    seeds = {"odd": 81212, "l4": 5616}
    return [dict(c, seed=seeds.get(c["name"], c["seed"])) for c in CASES]


AMP_CASES = _amp_cases()


def amp_stored_indices(key, name, shape):
    """the flat indices a tensor is stored at (sorted, a seeded choice without repetition), or None: every element"""
    n = int(np.prod(shape, dtype=np.int64))
    if n <= AMP_SAMPLE_ABOVE:
        return None
    seed = sum((i + 1) * ord(c) for i, c in enumerate(key + "/" + name)) % (2 ** 31)
    return np.sort(np.random.RandomState(seed).choice(n, AMP_SAMPLE, replace=False)).astype(np.int64)


def amp_fixture_tensors(z, case, mode, precision, li):
    """-> {tensor name: (r64 values [flat, at idx], idx or None (= every element), flip, max64)}"""
    from _dense_neck_cases import level_names, tensor_shapes
    key = f"{case['name']}/{mode}/{precision}/L{li}"
    r64, flip, m64 = z[key + "/r64"], z[key + "/flip"], z[key + "/max64"]
    k = int(level_names(case)[li][1:])
    out, o = {}, 0
    for i, (name, shape) in enumerate(tensor_shapes(case, k, case["sizes"][li], case["Cin"][li]).items()):
        idx = amp_stored_indices(f"{case['name']}/{mode}/L{li}", name, shape)
        n = len(idx) if idx is not None else int(np.prod(shape, dtype=np.int64))
        out[name] = (r64[o:o + n], idx, float(flip[i]), float(m64[i]))
        o += n
    assert o == len(r64)
    return out
