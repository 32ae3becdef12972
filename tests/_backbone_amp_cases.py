"""Cases and float64 references of the backbone's 16-bit modes (precision "fp16" / "bf16" of stemops / stageops), shared
by test_stem_conv_amp_gpu.py, test_backbone_amp_cpu.py and test_backbone_amp_gpu.py.  No device here.

Op level: one dense convolution on GIVEN operands.  The reference is torch's CPU conv2d in float64 on the operands rounded
to nearest even (ties to even) to the 16-bit type; the bar is the project's rule (_head_cases.bar) with e32 the error of
torch's fp32 CPU convolution on the SAME rounded operands.  A cell must also hold the UNROUNDED float64 result outside
that bar in every pass it is used for, or a kernel that forgets a rounding would pass: a cell whose first seed cannot
takes the next one (SEEDS_TRIED), never another rule."""
import contextlib
import functools
import json
import os

import numpy as np
import torch
import torch.nn.functional as TF

from _head_amp_cases import PRECISIONS, TIE_EPS, rounded
from _head_cases import bar

T = 8                                                      # yl_stem_plan's conv_tile
KS = [(k, s) for k in (1, 3) for s in (1, 2)]
PASSES = ("forward", "dgrad", "wgrad")
CHANNELS = [(4, 4), (8, 12), (20, 36)]
SIZES = (1, 2, T - 1, T, T + 1, 2 * T + 1)
# (B, S, cin, cout, planar)
SHAPES = [(B, S, ci, co, False) for S in SIZES for ci, co in CHANNELS for B in (1, 3)]
SHAPES += [(1, T + 1, 28, 60, False), (1, T + 1, 36, 68, False)]   # around the weight gradient's 32 / 64 channel blocks
PLANAR = [(B, S, 3, co, True) for S in SIZES for co in (8, 32) for B in (1, 3)]
SEEDS_TRIED = 20
PARITY = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "backbone_amp_parity.json")


def record(section, key, value):
    """the figures of a GPU run into profiles/backbone_amp_parity.json, beside the others' (best effort)"""
    try:
        table = json.load(open(PARITY)) if os.path.exists(PARITY) else {}
        table.setdefault(section, {})[key] = value
        with open(PARITY, "w") as f:
            json.dump(table, f, indent=1, sort_keys=True)
            f.write("\n")
    except OSError:
        pass


def out_size(S, k, s):
    return (S + 2 * ((k - 1) // 2) - k) // s + 1


def conv_all(x, w, dy, k, s, dtype):
    """x NHWC, w [O][I][k][k], dy NHWC -> {"forward", "dgrad", "wgrad"} of torch's CPU conv2d in `dtype`, NHWC"""
    xt = x.to(dtype).permute(0, 3, 1, 2).requires_grad_(True)
    wt = w.to(dtype).requires_grad_(True)
    y = TF.conv2d(xt, wt, None, s, (k - 1) // 2)
    y.backward(dy.to(dtype).permute(0, 3, 1, 2))
    return {"forward": y.detach().permute(0, 2, 3, 1).contiguous(), "dgrad": xt.grad.permute(0, 2, 3, 1).contiguous(),
            "wgrad": wt.grad.contiguous()}


def operands(k, s, B, S, cin, cout, seed):
    rs = np.random.RandomState(100000 * k + 10000 * s + 100 * S + 7 * cin + cout + B + 1000003 * seed)
    So = out_size(S, k, s)
    x = torch.from_numpy(rs.standard_normal((B, S, S, cin)).astype(np.float32))
    w = torch.from_numpy((rs.standard_normal((cout, cin, k, k)) / np.sqrt(cin * k * k)).astype(np.float32))
    dy = torch.from_numpy(rs.standard_normal((B, So, So, cout)).astype(np.float32))
    return x, w, dy


def reference(x, w, dy, k, s, precision):
    """-> {pass: {"r64", "unrounded", "bar"}} for the given fp32 operands"""
    xr, wr, dyr = (rounded(t, precision) for t in (x, w, dy))
    r64, r32, un = conv_all(xr, wr, dyr, k, s, torch.float64), conv_all(xr, wr, dyr, k, s, torch.float32), conv_all(x, w, dy, k, s, torch.float64)
    out = {}
    for p in PASSES:
        b = bar(float((r32[p].double() - r64[p]).abs().max()), float(r64[p].abs().max()))
        out[p] = {"r64": r64[p], "unrounded": un[p], "bar": b}
    return out


def passes_of(planar):
    return ("forward", "wgrad") if planar else PASSES


@functools.lru_cache(maxsize=None)
def cell(k, s, B, S, cin, cout, planar, precision):
    """-> (x, w, dy, reference, seed): the first seed at which every pass of the cell tells the rounded result from the
    unrounded one; None for the seed if none of the first SEEDS_TRIED does.  Computed once, shared, never written to"""
    for seed in range(SEEDS_TRIED):
        x, w, dy = operands(k, s, B, S, cin, cout, seed)
        ref = reference(x, w, dy, k, s, precision)
        if all(float((ref[p]["unrounded"] - ref[p]["r64"]).abs().max()) > ref[p]["bar"] for p in passes_of(planar)):
            return x, w, dy, ref, seed
    return x, w, dy, ref, None


def tie_operands(k, s, B, S, cin, cout, precision, which, seed=1501):
    """operands whose 16-bit rounding is all ties: `which` ("x" or "dy") holds 1 + eps and 1 + 3 eps (eps half an ulp of
    the type at 1: RNE gives 1 and 1 + 4 eps), the other two tensors small integers.  Every product and every sum of the
    rounded operands is then exact in fp32, whatever the order"""
    g = torch.Generator().manual_seed(seed + 10 * k + s)
    eps = TIE_EPS[precision]
    So = out_size(S, k, s)
    ties = lambda shape: 1.0 + eps * (1.0 + 2.0 * torch.randint(0, 2, shape, generator=g).float())      # noqa: E731
    ints = lambda shape: torch.randint(-2, 3, shape, generator=g).float()                                 # noqa: E731
    x = ties((B, S, S, cin)) if which == "x" else ints((B, S, S, cin))
    dy = ties((B, So, So, cout)) if which == "dy" else ints((B, So, So, cout))
    return x, ints((cout, cin, k, k)), dy


# ---- module level: tests/golden/backbone_amp.npz (made by tests/golden/make_backbone_amp_fixtures.py from the
# oracle/backbones.py modules under torch autograd with every DENSE convolution computing RoundedConv below).
# Layout, as head_amp.npz and dense_neck_amp.npz: per case, mode and precision <case>/<mode>/<precision>/r64, /flip, /max64
# over the tensors of the case's tensor_shapes() (y, dx, b.<buffer>, g.<parameter>; large tensors at stored_indices()).
# flip = the largest max|r32_j - r64| over FLIP_RUNS fp32 runs whose rounding inputs are jittered by +-1 fp32 ulp
# (generator seeded FLIP_SEED + j): what a correct fp32 implementation that rounds at the same places may differ by.
# Bar = max(4 x flip, 2 fp32 ulps at max64).
# Admission rule, asserted by the generator for every case, mode, precision and ReLU: the ReLU masks of the float64 run and
# of EVERY fp32 run (plain and jittered) of the rounded model are identical, and the smallest |BatchNorm output| in front
# of the ReLU in the float64 run is at least 1e-5 and at least 64 x the largest deviation of that tensor in any of those
# fp32 runs -- the margin is thereby scaled to the precision's perturbation: a flipped rounding moves a BatchNorm output by
# an ulp of the 16-bit type, not of fp32.
# Midpoint rule (the bf16 rule of make_head_amp_fixtures.py, stated on the reference alone): a rounding flips once per 2^15
# (bf16) or 2^12 (fp16) values and fp32 ulp of difference, so the eight jittered runs of a small case often flip none, and
# the allowance is then a plain fp32 error that ONE flip on another correct fp32 implementation exceeds sixtyfold.  So a
# (case, mode, precision) whose jittered runs flipped no rounding at all must have no activation or gradient in front of a
# rounding (ROUND_LOG) that lies within 4 x its fp32 error of a rounding midpoint: round(t + 4 e) == round(t - 4 e) for every
# element, e the larger of the element's own error (plain fp32 run against float64) and |t| x the tensor's relative error
# (largest error / largest magnitude).  (The weights and the case's x are given: they cannot flip.)
# A case that fails gets the next seed of its list (seed + 101 j, j < 20), never
# another rule; AMP_SEEDS records the first admitted seed and thereby the seeds tried before it.
# Cap, checked in test_backbone_amp_cpu.py: every (case, mode, precision) kept tells the rounded result from the unrounded
# one (the plain fixtures' float64 model on the same seed) in at least one of y, dx and the first dense weight gradient.
import _stage_cases as _sc
import _stem_cases as _st
from _dense_neck_amp_np import round_to
from _head_amp_cases import FLIP_RUNS, FLIP_SEED  # noqa: F401  (re-exported)

AMP_FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "backbone_amp.npz")
_STEM = {c["name"]: c for c in _st.CASES}
_STAGE = {c["name"]: c for c in _sc.CASES}
# a dz is rounded at the join between two units
CHAIN = dict(name="chain", B=2, S=8, cin=8, planar=False, units=[dict(k=3, s=2, c=12), dict(k=1, s=1, c=8)], seed=101)
AMP_STEM = [_STEM[n] for n in ("planar3", "s2even", "s1", "pw")] + [CHAIN]
AMP_STAGE = [_STAGE[n] for n in ("ffn", "k3res", "a3k0s2", "ragged")]
AMP_EVAL_CASE = "chain"
SEED_STEP, SEEDS_PER_CASE = 101, 20
# (case, precision) -> the first admitted seed of case["seed"] + 101 j (every j below it was tried and refused); a pair
# that is absent admitted none of the twenty and is dropped for that precision.  make_backbone_amp_fixtures.py --search
# prints this table
AMP_SEEDS = {
    ("planar3", "fp16"): 808,
    ("planar3", "bf16"): 101,
    ("s2even", "fp16"): 101,
    ("s2even", "bf16"): 202,
    ("s1", "fp16"): 505,
    ("s1", "bf16"): 101,
    ("pw", "fp16"): 505,
    ("pw", "bf16"): 101,
    ("chain", "fp16"): 303,
    ("chain", "bf16"): 101,
    ("ffn", "fp16"): 101,
    ("ffn", "bf16"): 101,
    ("k3res", "fp16"): 101,
    ("k3res", "bf16"): 202,
    ("a3k0s2", "fp16"): 101,
    ("a3k0s2", "bf16"): 202,
    ("ragged", "fp16"): 101,
    ("ragged", "bf16"): 101,
}


def amp_kind(case):
    return "stem" if "units" in case else "stage"


def amp_mod(case):
    return _st if amp_kind(case) == "stem" else _sc


def amp_modes(case):
    return ("train", "eval") if case["name"] == AMP_EVAL_CASE else ("train",)


def amp_cases():
    """[(case with the admitted seed, precision)]"""
    return [(dict(c, seed=AMP_SEEDS[(c["name"], p)]), p) for c in AMP_STEM + AMP_STAGE for p in PRECISIONS
            if (c["name"], p) in AMP_SEEDS]


def amp_fixture_tensors(z, case, mode, precision):
    """-> {tensor name: (r64 values [flat, at idx], idx or None, flip, max64)}: _stem_cases.fixture_tensors' form"""
    m = amp_mod(case)
    key = f"{case['name']}/{mode}/{precision}"
    r64, flip, m64 = z[key + "/r64"], z[key + "/flip"], z[key + "/max64"]
    out, o = {}, 0
    for i, (name, shape) in enumerate(m.tensor_shapes(case).items()):
        idx = m.stored_indices(key, name, shape)
        n = len(idx) if idx is not None else int(np.prod(shape, dtype=np.int64))
        out[name] = (r64[o:o + n], idx, float(flip[i]), float(m64[i]))
        o += n
    assert o == len(r64)
    return out


def first_dense_weight(case):
    """the fixture name of the first dense convolution's weight gradient"""
    m = amp_mod(case)
    for u in m.units(case):
        if amp_kind(case) == "stem":
            return "g." + u["conv"] + ".weight"
        if not u["dw"]:
            return "g." + u["key"] + u["conv"] + ".weight"
    raise AssertionError(case["name"])


# what the generator reads off a run: every activation / gradient tensor in front of a rounding, in running order, and how
# many of their elements a jittered run rounded to another 16-bit value than the unjittered rounding of the same tensor
ROUND_LOG = {"inputs": None, "flips": 0}


def _log_rounding(t, precision, jitter, tr):
    if ROUND_LOG["inputs"] is not None:
        ROUND_LOG["inputs"].append(t.detach().clone())
    if jitter is not None:
        ROUND_LOG["flips"] += int((tr != round_to(t, precision)).sum())


class RoundedConv(torch.autograd.Function):
    """z = conv(r(x), r(W)); dx = conv^T(r(dz), r(W)); dW = r(x) (*) r(dz); r = round_to (nearest even; with `jitter` the
    value moves by -1, 0 or +1 fp32 ulp first).  Rounded1x1 of _head_amp_cases.py for any kernel size, stride and padding"""

    @staticmethod
    def forward(ctx, x, w, stride, padding, precision, jitter):
        xr, wr = round_to(x, precision, jitter), round_to(w, precision, jitter)
        _log_rounding(x, precision, jitter, xr)
        ctx.save_for_backward(xr, wr)
        ctx.conf = (stride, padding, precision, jitter)
        return TF.conv2d(xr, wr, None, stride, padding)

    @staticmethod
    def backward(ctx, dz):
        xr, wr = ctx.saved_tensors
        stride, padding, precision, jitter = ctx.conf
        dzr = round_to(dz, precision, jitter)
        _log_rounding(dz, precision, jitter, dzr)
        dx = torch.nn.grad.conv2d_input(xr.shape, wr, dzr, stride=stride, padding=padding)
        dw = torch.nn.grad.conv2d_weight(xr, wr.shape, dzr, stride=stride, padding=padding)
        return dx, dw, None, None, None, None


@contextlib.contextmanager
def rounded_dense_convs(precision, jitter=None):
    """while active, every bias-free nn.Conv2d with groups == 1 computes RoundedConv; depthwise convolutions, BatchNorm,
    ReLU and the residual add stay what they are"""
    plain = torch.nn.Conv2d.forward

    def forward(self, x):
        if self.groups != 1:
            return plain(self, x)
        assert self.bias is None and self.dilation == (1, 1) and self.padding_mode == "zeros"
        return RoundedConv.apply(x, self.weight, self.stride, self.padding, precision, jitter)

    torch.nn.Conv2d.forward = forward
    try:
        yield
    finally:
        torch.nn.Conv2d.forward = plain
