"""The dense convolution passes of the trainable stem in precision "fp16" / "bf16" (yololite_amd.stemops.conv(...,
precision=) -> yl_amp_stem_conv, csrc/yl_stem.hip) on given operands, against torch's CPU conv2d in float64 on the
RNE-rounded operands.

The cells are those of test_stem_conv_gpu.py: k in {1, 3} x stride in {1, 2} x {forward, dgrad, wgrad} x S in {1, 2, 7, 8,
9, 17} (T - 1, T, T + 1 and 2 T + 1 for the tile edge T = 8) x (cin, cout) in {(4, 4), (8, 12), (20, 36)} x B in {1, 3},
the planar cin 3 image with cout {8, 32} for forward and wgrad, and (28, 60), (36, 68) at S 9 around the weight gradient's
32 / 64 channel blocks.  The operands are given, so no rounding can flip: the bar is the project's rule, max(4 x e32, 2 fp32
ulps at the tensor's maximum), e32 the error of torch's fp32 CPU convolution on the same rounded operands.  Every cell also
holds the UNROUNDED float64 result outside that bar (_backbone_amp_cases.cell; checked without a device in
test_backbone_amp_cpu.py).  The worst error / bar per (k, s, pass, precision) goes to profiles/backbone_amp_parity.json
under "op"."""
import ctypes as C

import pytest
import torch

from yololite_amd import _lib, stemops
from _backbone_amp_cases import (KS, PASSES, PLANAR, PRECISIONS, SHAPES, cell, conv_all, out_size, record, reference, rounded,
                                 tie_operands)
from _head_cases import bar
from _train_dev import DEV

pytestmark = pytest.mark.gpu

YL_ERR_INVALID = -1                                        # include/yololite_hip.h, yl_status


def device_pass(pass_, k, s, x, w, dy, precision, planar=False):
    """x, dy NHWC and w on the CPU -> the pass's result on the CPU"""
    xd = x.permute(0, 3, 1, 2).contiguous().to(DEV) if planar else x.to(DEV)
    layout = "nchw" if planar else "nhwc"
    if pass_ == "forward":
        out = stemops.conv(xd, w.to(DEV), "forward", k, s, layout=layout, precision=precision)
    elif pass_ == "dgrad":
        out = stemops.conv(dy.to(DEV), w.to(DEV), "dgrad", k, s, size=x.shape[1], precision=precision)
    else:
        out = stemops.conv(xd, dy.to(DEV), "wgrad", k, s, layout=layout, precision=precision)
    return out.cpu()


def held(k, s, pass_, precision, shapes):
    bad, worst = [], (0.0, "")
    for B, S, cin, cout, planar in shapes:
        x, w, dy, ref, seed = cell(k, s, B, S, cin, cout, planar, precision)
        assert seed is not None, (B, S, cin, cout, "no seed tells the rounded result from the unrounded one")
        r = ref[pass_]
        got = device_pass(pass_, k, s, x, w, dy, precision, planar)
        assert got.shape == r["r64"].shape and got.dtype == torch.float32
        err = float((got.double() - r["r64"]).abs().max())
        miss = float((r["unrounded"] - r["r64"]).abs().max())
        at = f"B{B} S{S} {cin}->{cout}{' planar' if planar else ''}"
        print(f"k{k} s{s} {pass_:7s} {precision} {at:22s} seed {seed}  err {err:.3e}  bar {r['bar']:.3e}  "
              f"ratio {err / r['bar']:.3f}  unrounded {miss / r['bar']:.1f} bars away")
        worst = max(worst, (round(err / r["bar"], 4), at))
        assert miss > r["bar"], at
        if not err <= r["bar"]:
            bad.append((at, err, r["bar"]))
    return bad, worst


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("pass_", PASSES)
@pytest.mark.parametrize("k,s", KS)
def test_every_cell_against_the_rounded_operand_convolution(k, s, pass_, precision):
    bad, worst = held(k, s, pass_, precision, SHAPES)
    record("op", f"k{k}/s{s}/{pass_}/{precision}", {"worst_ratio": worst[0], "at": worst[1]})
    assert not bad, bad


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("pass_", ("forward", "wgrad"))
@pytest.mark.parametrize("k,s", KS)
def test_the_planar_image_against_the_rounded_operand_convolution(k, s, pass_, precision):
    bad, worst = held(k, s, pass_, precision, PLANAR)
    record("op", f"k{k}/s{s}/{pass_}/{precision}/planar", {"worst_ratio": worst[0], "at": worst[1]})
    assert not bad, bad


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("s", (1, 2))
def test_ties_round_to_even_bit_for_bit(s, precision):
    """3x3, all three passes: 1 + 2^-11 and 1 + 3 2^-11 (fp16; 2^-8 for bf16) against small integers.  RNE gives 1 and
    1 + 4 eps, every product and sum is exact in fp32, so the device must give the exact value"""
    k = 3
    for B, S, cin, cout, planar in ((3, 9, 20, 36, False), (1, 17, 8, 12, False), (3, 9, 3, 8, True)):
        for which, passes in (("x", ("forward", "wgrad")), ("dy", ("dgrad", "wgrad"))):
            x, w, dy = tie_operands(k, s, B, S, cin, cout, precision, which)
            exact = conv_all(rounded(x, precision), w, rounded(dy, precision), k, s, torch.float64)
            away = conv_all(x, w, dy, k, s, torch.float64)
            for pass_ in passes:
                if planar and pass_ == "dgrad":
                    continue
                assert torch.equal(exact[pass_].float().double(), exact[pass_])     # representable: the sums are exact in fp32
                assert not torch.equal(away[pass_], exact[pass_])                  # what no rounding at all would give
                got = device_pass(pass_, k, s, x, w, dy, precision, planar)
                assert torch.equal(got, exact[pass_].float()), (S, cin, cout, planar, which, pass_,
                                                                float((got.double() - exact[pass_]).abs().max()))


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("k,s", KS)
def test_a_one_hot_centre_tap_reproduces_x_bit_for_bit(k, s, precision):
    """x on the 16-bit grid, W[n][c] = delta_nc at the centre tap: forward is x[:, ::s, ::s] and dgrad puts it back"""
    for B, S, Cn in ((1, 1, 4), (3, 7, 20), (1, 8, 4), (3, 9, 12), (1, 2, 20), (1, 17, 36)):
        x = rounded(cell(k, s, B, S, Cn, Cn, False, precision)[0], precision).to(DEV)
        w = torch.zeros(Cn, Cn, k, k, device=DEV)
        w[torch.arange(Cn), torch.arange(Cn), k // 2, k // 2] = 1.0
        y = stemops.conv(x, w, "forward", k, s, precision=precision)
        assert torch.equal(y, x[:, ::s, ::s].contiguous()), (B, S, Cn)
        dx = stemops.conv(y, w, "dgrad", k, s, size=S, precision=precision)
        want = torch.zeros_like(x)
        want[:, ::s, ::s] = x[:, ::s, ::s]
        assert torch.equal(dx, want), (B, S, Cn)


@pytest.mark.parametrize("k,s", KS)
def test_an_operand_beyond_fp16_overflows_to_inf_and_bf16_holds_it(k, s):
    """x with one entry 1e5: RNE to fp16 is +inf and nothing is clamped, so exactly the outputs whose window holds that
    pixel are not finite (what FusedTrainStep's found-inf looks for); bf16 has fp32's range and stays inside its bar"""
    B, S, cin, cout = 3, 9, 20, 36
    x, w, dy, _, _ = cell(k, s, B, S, cin, cout, False, "bf16")
    x = x.clone()
    iy, ix = 4, 6
    x[1, iy, ix, 5] = 1e5
    So, pad = out_size(S, k, s), (k - 1) // 2
    touched = torch.zeros(B, So, So, dtype=torch.bool)
    for oy in range(So):
        for ox in range(So):
            if 0 <= iy - (oy * s - pad) < k and 0 <= ix - (ox * s - pad) < k:
                touched[1, oy, ox] = True
    assert touched.any()
    got = device_pass("forward", k, s, x, w, dy, "fp16")
    assert not torch.isfinite(got[touched]).any(), "every output the operand reaches must be non-finite"
    assert torch.isfinite(got[~touched]).all()
    # the weight gradient: input channel 5 of every tap that pairs the pixel with an output pixel
    gw = device_pass("wgrad", k, s, x, w, dy, "fp16")
    assert not torch.isfinite(gw[:, 5]).all() and torch.isfinite(gw[:, :5]).all() and torch.isfinite(gw[:, 6:]).all()
    ref = reference(x, w, dy, k, s, "bf16")
    for pass_ in ("forward", "wgrad"):
        got = device_pass(pass_, k, s, x, w, dy, "bf16")
        assert torch.isfinite(got).all()
        err = float((got.double() - ref[pass_]["r64"]).abs().max())
        print(f"k{k} s{s} {pass_} bf16 with 1e5: err {err:.3e} bar {ref[pass_]['bar']:.3e}")
        assert err <= ref[pass_]["bar"], (pass_, err, ref[pass_]["bar"])


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("pass_", PASSES)
def test_two_calls_give_equal_bits(pass_, precision):
    for k, s in KS:
        for B, S, cin, cout in ((3, 9, 20, 36), (3, 17, 8, 12)):
            x, w, dy, _, _ = cell(k, s, B, S, cin, cout, False, precision)
            assert torch.equal(device_pass(pass_, k, s, x, w, dy, precision), device_pass(pass_, k, s, x, w, dy, precision))


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("k,s", KS)
def test_image_0_does_not_change_by_a_bit_when_image_1_does(k, s, precision):
    x, w, dy, _, _ = cell(k, s, 3, 9, 20, 36, False, precision)
    x2, dy2 = x.clone(), dy.clone()
    x2[1:] = x2[1:] * 3 + 1
    dy2[1:] = dy2[1:] * 3 + 1
    for pass_ in ("forward", "dgrad"):
        a, b = device_pass(pass_, k, s, x, w, dy, precision), device_pass(pass_, k, s, x2, w, dy2, precision)
        assert torch.equal(a[0], b[0]) and not torch.equal(a[1], b[1])


def _shifted(t):
    """a contiguous copy of t on the device that starts 4 bytes past a 16-byte boundary"""
    buf = torch.zeros(t.numel() + 5, device=DEV)
    o = 1 + (-(buf.data_ptr() // 4) % 4)
    view = buf[o:o + t.numel()].view(t.shape)
    view.copy_(t)
    assert view.data_ptr() % 16 == 4 and view.is_contiguous()
    return view


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("k,s", KS)
def test_a_weight_and_a_planar_image_four_bytes_past_a_16_byte_boundary_give_the_bits_of_aligned_ones(k, s, precision):
    x, w, dy, _, _ = cell(k, s, 3, 9, 20, 36, False, precision)
    xd, wd, dyd = x.to(DEV), w.to(DEV), dy.to(DEV)
    off = _shifted(wd)
    assert torch.equal(stemops.conv(xd, off, "forward", k, s, precision=precision),
                       stemops.conv(xd, wd, "forward", k, s, precision=precision))
    assert torch.equal(stemops.conv(dyd, off, "dgrad", k, s, size=9, precision=precision),
                       stemops.conv(dyd, wd, "dgrad", k, s, size=9, precision=precision))
    x, w, dy, _, _ = cell(k, s, 3, 9, 3, 8, True, precision)
    img, wd, dyd = x.permute(0, 3, 1, 2).contiguous().to(DEV), w.to(DEV), dy.to(DEV)
    assert img.data_ptr() % 16 == 0
    ioff = _shifted(img)
    assert torch.equal(stemops.conv(ioff, _shifted(wd), "forward", k, s, layout="nchw", precision=precision),
                       stemops.conv(img, wd, "forward", k, s, layout="nchw", precision=precision))
    assert torch.equal(stemops.conv(ioff, dyd, "wgrad", k, s, layout="nchw", precision=precision),
                       stemops.conv(img, dyd, "wgrad", k, s, layout="nchw", precision=precision))


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("k,s", KS)
def test_fp32_precision_is_the_unrounded_convolution(k, s, precision):
    """precision="fp32" sums the operands as they are: inside the bar of the UNROUNDED reference and outside the rounded
    one's, and it is yl_stem_conv bit for bit (the modes are told apart from both sides)"""
    B, S, cin, cout = 3, 9, 20, 36
    x, w, dy, ref, _ = cell(k, s, B, S, cin, cout, False, precision)
    r32 = conv_all(x, w, dy, k, s, torch.float32)
    for pass_ in PASSES:
        got = device_pass(pass_, k, s, x, w, dy, "fp32")
        un = ref[pass_]["unrounded"]
        b = bar(float((r32[pass_].double() - un).abs().max()), float(un.abs().max()))
        assert float((got.double() - un).abs().max()) <= b, pass_
        assert float((got.double() - ref[pass_]["r64"]).abs().max()) > ref[pass_]["bar"], pass_
        assert torch.equal(got, device_pass(pass_, k, s, x, w, dy, None)), pass_


def test_launch_counts_do_not_depend_on_the_precision():
    for k, s in KS:
        x, w, dy, _, _ = cell(k, s, 3, 9, 20, 36, False, "fp16")
        for pass_ in PASSES:
            counts = []
            for precision in (None, "fp32", "fp16", "bf16"):
                device_pass(pass_, k, s, x, w, dy, precision)
                counts.append(stemops.conv.last_launches)
            assert len(set(counts)) == 1 and counts[0] >= 1, (k, s, pass_, counts)


def test_yl_amp_stem_conv_refuses_what_is_not_a_mode():
    x = torch.zeros((1, 8, 8, 4), device=DEV)
    w = torch.zeros((4, 4, 3, 3), device=DEV)
    y = torch.zeros((1, 8, 8, 4), device=DEV)
    lib = _lib.load()
    n = C.c_int32()
    for mode in (_lib.YL_HEAD_F16 | _lib.YL_HEAD_BF16, 0x400, 1):
        st = lib.yl_amp_stem_conv(x.data_ptr(), w.data_ptr(), y.data_ptr(), _lib.YL_STAGE_PASS_FORWARD, 3, 1, 1, 8, 4, 4, 0,
                                  mode, None, C.byref(n))
        assert st == YL_ERR_INVALID, mode
    for mode in (0, _lib.YL_HEAD_F16, _lib.YL_HEAD_BF16):
        st = lib.yl_amp_stem_conv(x.data_ptr(), w.data_ptr(), y.data_ptr(), _lib.YL_STAGE_PASS_FORWARD, 3, 1, 1, 8, 4, 4, 0,
                                  mode, None, C.byref(n))
        assert st == 0 and n.value == 2, mode
    with pytest.raises(ValueError, match="precision"):
        stemops.conv(x, w, "forward", 3, 1, precision="fp8")
