"""The three 3x3 GEMMs of DetectNeckMS in precision "fp16" / "bf16" (yololite_amd.neckops.conv3x3 over yl_dneck_conv3x3,
csrc/yl_dneck.hip) on given operands, against the float64 convolution of the RNE-rounded operands.

The operands are given, so no rounding can flip: the bar is the project's rule, max(4 x e32, 2 fp32 ulps at the tensor's
maximum), e32 = the error of torch's fp32 CPU convolution of the same rounded operands.  Every case also holds the
UNROUNDED float64 result outside that bar: a kernel that forgets to round cannot pass.  The worst error / bar of every
(case, pass, precision) is written to profiles/dense_neck_amp_parity.json under "op"."""
import json
import os

import numpy as np
import pytest
import torch

from yololite_amd import neckops
from _dense_neck_amp_cases import (OP_BY_NAME, OP_CASES, OP_WIDE, PASSES, conv_pass, op_reference, reference, rounded, tie_operands)
from _train_dev import DEV

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARITY = os.path.join(ROOT, "profiles", "dense_neck_amp_parity.json")
PRECISIONS = ("fp16", "bf16")


def _dev(a, b, pass_, precision):
    return neckops.conv3x3(a.to(DEV), b.to(DEV), pass_, precision).cpu()


def _record(section, key, value):
    try:                                                   # the figures of this run, beside the others' (best effort)
        table = json.load(open(PARITY)) if os.path.exists(PARITY) else {}
        table.setdefault(section, {})[key] = value
        with open(PARITY, "w") as f:
            json.dump(table, f, indent=1, sort_keys=True)
            f.write("\n")
    except OSError:
        pass


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("case", OP_CASES + OP_WIDE, ids=[c["name"] for c in OP_CASES + OP_WIDE])
def test_op_parity_with_the_rounded_operand_reference(case, precision):
    bad, worst = [], {}
    for pass_ in PASSES:
        ref = op_reference(case["name"], pass_, precision)
        got = _dev(ref["a"], ref["b"], pass_, precision)
        assert got.shape == ref["r64"].shape and got.dtype == torch.float32
        err = float((got.double() - ref["r64"]).abs().max())
        miss = float((ref["unrounded"] - ref["r64"]).abs().max())
        print(f"{case['name']:7s} {precision} {pass_:8s} err {err:.3e}  bar {ref['bar']:.3e}  ratio {err / ref['bar']:.3f}  "
              f"unrounded {miss / ref['bar']:.1f} bars away")
        worst[pass_] = round(err / ref["bar"], 4)
        assert miss > ref["bar"], (pass_, "the case cannot see a missing rounding: take the next seed")
        if not err <= ref["bar"]:
            bad.append((pass_, err, ref["bar"]))
        again = _dev(ref["a"], ref["b"], pass_, precision)
        assert torch.equal(got, again), (pass_, "two calls differ")
    _record("op", f"{case['name']}/{precision}", worst)
    assert not bad, bad


@pytest.mark.parametrize("precision", PRECISIONS)
def test_fp32_precision_is_the_unrounded_convolution(precision):
    """the same entry in "fp32" sums the operands as they are: inside the bar of the UNROUNDED reference, and outside
    the rounded one's (the modes are told apart from both sides)"""
    for pass_ in PASSES:
        ref = op_reference("ragged", pass_, precision)
        got = _dev(ref["a"], ref["b"], pass_, "fp32").double()
        r32 = conv_pass(ref["a"], ref["b"], pass_).double()
        b = max(4.0 * float((r32 - ref["unrounded"]).abs().max()),
                2.0 * float(np.spacing(np.float32(ref["unrounded"].abs().max()))))
        assert float((got - ref["unrounded"]).abs().max()) <= b, pass_
        assert float((got - ref["r64"]).abs().max()) > ref["bar"], pass_


@pytest.mark.parametrize("precision", PRECISIONS)
def test_ties_round_to_even_bit_for_bit(precision):
    for pass_ in PASSES:
        a, b = tie_operands(pass_, precision)
        exact = conv_pass(rounded(a, precision).double(), b.double(), pass_)
        assert torch.equal(exact.float().double(), exact)                # representable: the sums are exact in fp32
        got = _dev(a, b, pass_, precision)
        assert torch.equal(got, exact.float()), (pass_, float((got.double() - exact).abs().max()))
        away = conv_pass(a.double(), b.double(), pass_)                   # what no rounding at all would give
        assert not torch.equal(away, exact)


def test_an_operand_beyond_fp16_overflows_to_inf_and_bf16_holds_it():
    """weight-gradient pass, dz with one entry 1e5: RNE to fp16 is +inf, nothing is clamped, and that output channel's dW
    is not finite (what FusedTrainStep's found-inf looks for); bf16 has fp32's range and stays inside its bar"""
    case = OP_BY_NAME["ragged"]
    ref = op_reference(case["name"], "wgrad", "bf16")
    x, dz = ref["a"], ref["b"].clone()
    n = 7
    dz[1, 2, 3, n] = 1e5
    got = _dev(x, dz, "wgrad", "fp16")
    assert not torch.isfinite(got[n]).any(), "the overflowing channel must not be finite anywhere"
    rest = torch.cat([got[:n], got[n + 1:]])
    assert torch.isfinite(rest).all()
    r = reference(x, dz, "wgrad", "bf16")
    got = _dev(x, dz, "wgrad", "bf16")
    assert torch.isfinite(got).all()
    err = float((got.double() - r["r64"]).abs().max())
    print(f"bf16 with 1e5: err {err:.3e} bar {r['bar']:.3e}")
    assert err <= r["bar"], (err, r["bar"])


@pytest.mark.parametrize("precision", PRECISIONS)
def test_image_0_does_not_change_by_a_bit_when_image_1_does(precision):
    """S = 24: nine spatial tiles per image, so windows meet image seams and row ends"""
    for pass_ in ("forward", "dgrad"):
        ref = op_reference("rows", pass_, precision)
        a2 = ref["a"].clone()
        a2[1] = 100.0 * torch.randn(a2[1].shape, generator=torch.Generator().manual_seed(5))
        one, two = _dev(ref["a"], ref["b"], pass_, precision), _dev(a2, ref["b"], pass_, precision)
        assert torch.equal(one[0], two[0]), pass_
        assert not torch.equal(one[1], two[1]), pass_


def test_conv3x3_refuses_what_it_cannot_run():
    x = torch.zeros((1, 2, 2, 8), device=DEV)
    w = torch.zeros((8, 8, 3, 3), device=DEV)
    with pytest.raises(ValueError, match="precision"):
        neckops.conv3x3(x, w, "forward", "fp8")
    with pytest.raises(ValueError, match="pass_"):
        neckops.conv3x3(x, w, "backward", "fp16")
    with pytest.raises(ValueError, match="second operand"):
        neckops.conv3x3(x, w, "wgrad", "fp16")
    with pytest.raises(neckops._lib.YoloLiteHipError):
        neckops.conv3x3(x.cpu(), w.cpu(), "forward", "fp16")
